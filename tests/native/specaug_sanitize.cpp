// specaug_sanitize.cpp -- SpecAugment's host code under ASan + UBSan
// (go-mp3_amd/csrc/Makefile target asan-specaug; run by
// tests/test_specaug_cpu.py).  Host buffers of exactly the sizes the contract
// names: mp3g_specaug_host in both layouts, with and without the warp and the mean
// fill, in and out of place, over descriptors at every edge (warps at and outside
// the row's ends, masks clipped, past the end and with an end above 2^32, counts
// above the maxima), and the argument refusals of the host and the device calls.
// No device call is made.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mp3g.h"

// (the library's error-text sink lives in mp3g_abi.cpp, which is not linked)
namespace mp3g {
int abi_fail(int status, const char*) { return status; }
}  // namespace mp3g

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

static uint32_t g_seed = 12345;
static uint32_t rnd32() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}
static float rnd() { return (float)rnd32() / 16777216.0f; }

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT;
  const uint32_t rows = 8, planes = 2, big = 0xffffffffu;
  for (uint32_t F : {1u, 2u, 3u, 33u, 97u})
    for (uint32_t bins : {1u, 5u, 13u}) {
      const uint32_t lengths[rows] = {0, 1, 2, F / 2, F, F + 7, big, 3};
      std::vector<mp3g_specaug_row> desc(rows);
      for (uint32_t pass = 0; pass < 6; pass++) {
        std::memset(desc.data(), 0, rows * sizeof(mp3g_specaug_row));
        for (uint32_t r = 0; r < rows; r++) {
          const uint32_t n = lengths[r] < F ? lengths[r] : F;
          mp3g_specaug_row& d = desc[r];
          const uint32_t edge[8] = {0, 1, n ? n - 1 : 0, n, n + 1, n / 2, big, 2};
          d.warp_center = edge[(r + pass) % 8];
          d.warp_to = edge[(r + 3 * pass + 1) % 8];
          d.n_time = pass == 5 ? big : rnd32() % 18;
          d.n_freq = pass == 5 ? 1000 : rnd32() % 6;
          for (uint32_t k = 0; k < MP3G_SPECAUG_MAX_TIME_MASKS; k++) {
            d.time[k][0] = k % 4 == 3 ? big - (rnd32() % 3) : rnd32() % (n + 3);
            d.time[k][1] = k % 5 == 4 ? big : rnd32() % (n + 2);
          }
          for (uint32_t k = 0; k < MP3G_SPECAUG_MAX_FREQ_MASKS; k++) {
            d.freq[k][0] = k == 3 ? big : rnd32() % (bins + 2);
            d.freq[k][1] = k == 2 ? big : rnd32() % 3;
          }
        }
        for (uint32_t flags = 0; flags < 8; flags++) {
          const bool fm = flags & MP3G_SPECAUG_FREQ_MAJOR;
          const uint32_t live = fm ? F : bins, stride = live + (pass % 2 ? 3 : 0), outer = fm ? bins : F;
          const size_t words = (size_t)rows * planes * outer * stride;
          std::vector<float> x(words), y(words, -1.0f), fills(rows * planes, -1.0f);
          for (float& v : x) v = 20.0f * rnd() - 5.0f;
          CHECK(mp3g_specaug_host(x.data(), y.data(), rows, planes, F, bins, stride, lengths, desc.data(), flags, 0.5f,
                                  fills.data()) == MP3G_OK);
          for (size_t i = 0; i < words; i++) {
            if (i % stride >= live) CHECK(y[i] == -1.0f);  // the stride's tail: never written
            else CHECK(std::isfinite(y[i]));
          }
          for (size_t i = 0; i < (size_t)planes * outer * stride; i++)
            if (i % stride < live) CHECK(y[i] == x[i]);  // row 0 has no frames: a copy
          if (flags & MP3G_SPECAUG_FILL_MEAN) {
            CHECK(fills[0] == 0.0f && !std::signbit(fills[0]));
            for (float f : fills) CHECK(f >= -5.0f && f <= 15.0f);
          } else {
            for (float f : fills) CHECK(f == -1.0f);
          }
          if (!(flags & MP3G_SPECAUG_WARP)) {  // in place: the same words as out of place
            std::vector<float> z(x);
            CHECK(mp3g_specaug_host(z.data(), z.data(), rows, planes, F, bins, stride, lengths, desc.data(), flags,
                                    0.5f, fills.data()) == MP3G_OK);
            for (size_t i = 0; i < words; i++)
              if (i % stride < live) CHECK(std::memcmp(&z[i], &y[i], 4) == 0);
              else CHECK(z[i] == x[i]);
          }
        }
      }
    }
  // ---- refusals, the same for the host and the device call (before any device call)
  {
    std::vector<float> x(2 * 6 * 8 + 8), y(2 * 6 * 8), f(2);
    const uint32_t lengths[2] = {6, 3};
    std::vector<mp3g_specaug_row> d(2);
    std::memset(d.data(), 0, 2 * sizeof(mp3g_specaug_row));
    const uint32_t W = MP3G_SPECAUG_WARP, FM = MP3G_SPECAUG_FREQ_MAJOR, MEAN = MP3G_SPECAUG_FILL_MEAN;
    auto both = [&](const float* in, float* out, uint32_t nr, uint32_t np, uint32_t F, uint32_t nb, uint32_t stride,
                    const uint32_t* len, const mp3g_specaug_row* dd, uint32_t flags, float* fills, int want) {
      CHECK(mp3g_specaug_host(in, out, nr, np, F, nb, stride, len, dd, flags, 0.f, fills) == want);
      if (want != MP3G_OK || !nr || !np || !F || !nb)  // (an accepted call with work would reach the device)
        CHECK(mp3g_specaug_rows(0, in, out, nr, np, F, nb, stride, len, dd, flags, 0.f, fills, nullptr) == want);
    };
    both(x.data(), y.data(), 2, 1, 6, 8, 8, lengths, d.data(), W, nullptr, MP3G_OK);
    both(x.data(), y.data(), 2, 1, 6, 8, 8, lengths, d.data(), 8, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 6, 8, 7, lengths, d.data(), 0, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 9, 6, 8, lengths, d.data(), FM, nullptr, inv);
    both(nullptr, y.data(), 2, 1, 6, 8, 8, lengths, d.data(), 0, nullptr, inv);
    both(x.data(), nullptr, 2, 1, 6, 8, 8, lengths, d.data(), 0, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 6, 8, 8, nullptr, d.data(), 0, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 6, 8, 8, lengths, nullptr, 0, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 6, 8, 8, lengths, d.data(), MEAN, nullptr, inv);
    both(x.data(), y.data(), 2, 1, 6, 8, 8, lengths, d.data(), MEAN, f.data(), MP3G_OK);
    both(x.data(), x.data(), 2, 1, 6, 8, 8, lengths, d.data(), W, nullptr, inv);
    both(x.data(), x.data(), 2, 1, 6, 8, 8, lengths, d.data(), 0, nullptr, MP3G_OK);
    both(x.data(), x.data() + 8, 2, 1, 6, 8, 8, lengths, d.data(), 0, nullptr, inv);
    both(x.data() + 8, x.data(), 2, 1, 6, 8, 8, lengths, d.data(), 0, nullptr, inv);
    both(nullptr, nullptr, 1, 1, (1u << 22) + 1, 1, 1, lengths, d.data(), W, nullptr, MP3G_ERR_UNSUPPORTED);
    both(nullptr, nullptr, 0, 1, 6, 8, 8, nullptr, nullptr, W, nullptr, MP3G_OK);
    both(nullptr, nullptr, 2, 0, 6, 8, 8, nullptr, nullptr, W, nullptr, MP3G_OK);
    both(nullptr, nullptr, 2, 1, 0, 8, 8, nullptr, nullptr, W, nullptr, MP3G_OK);
    both(nullptr, nullptr, 2, 1, 6, 0, 8, nullptr, nullptr, W, nullptr, MP3G_OK);
    CHECK(mp3g_specaug_rows(-1, x.data(), y.data(), 2, 1, 6, 8, 8, lengths, d.data(), 0, 0.f, nullptr, nullptr) == inv);
  }
  if (g_failed) {
    std::fprintf(stderr, "specaug_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("specaug_sanitize ok\n");
  return 0;
}
