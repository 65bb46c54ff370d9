// frameops_sanitize.cpp -- the sliding CMN's, the energy VAD's and the frame
// selection's host code under ASan + UBSan (go-mp3_amd/csrc/Makefile target
// asan-frameops; run by tests/test_vad_select_cpu.py).  Host buffers of exactly
// the sizes the contract names: mp3g_sliding_cmn_host, mp3g_vad_energy_host and
// mp3g_select_frames_host over every length and window edge, and the argument
// refusals of the host and the device calls.  No device call is made.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
static float rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) / 16777216.0f;
}

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT;
  const uint32_t rows = 6, planes = 2, stride = 5, cols = 4;
  for (uint32_t F : {1u, 31u, 32u, 33u, 97u}) {
    const uint32_t lengths[rows] = {0, 1, F / 2, F, F + 7, 0xffffffffu};
    const size_t words = (size_t)rows * planes * F * stride;
    std::vector<float> x(words), y(words);
    for (float& v : x) v = 20.0f * rnd() - 5.0f;
    // ---- sliding CMN: every flag, windows below, at and above the row
    for (uint32_t flags = 0; flags < 4; flags++)
      for (uint32_t W : {1u, 2u, 3u, 32u, 64u, 600u, 0xffffffffu})
        for (uint32_t mw : {1u, 100u, F + 5, 0xffffffffu}) {
          std::fill(y.begin(), y.end(), -1.0f);
          CHECK(mp3g_sliding_cmn_host(x.data(), y.data(), rows, planes, F, stride, cols, lengths, W, mw, flags) ==
                MP3G_OK);
          for (size_t i = 0; i < words; i++) {
            if (i % stride >= cols) CHECK(y[i] == -1.0f);  // the stride's tail: never written
            else CHECK(std::isfinite(y[i]));
          }
          for (size_t i = 0; i < (size_t)planes * F * stride; i++)
            if (i % stride < cols) CHECK(y[i] == x[i]);  // row 0 has no frames: a copy
        }
    // ---- VAD: contexts below and above the row, both threshold forms
    std::vector<uint8_t> v((size_t)rows * planes * F);
    std::vector<uint32_t> counts(rows * planes), m(rows * planes);
    for (uint32_t ctx : {0u, 2u, F + 3, 0xffffffffu})
      for (float scale : {0.0f, 0.5f}) {
        std::fill(v.begin(), v.end(), (uint8_t)7);
        CHECK(mp3g_vad_energy_host(x.data(), rows, planes, F, stride, cols, cols - 1, lengths, 5.5f, scale, 0.12f, ctx,
                                   v.data(), counts.data()) == MP3G_OK);
        for (uint32_t p = 0; p < rows * planes; p++) {
          uint32_t ones = 0;
          for (uint32_t f = 0; f < F; f++) {
            CHECK(v[(size_t)p * F + f] <= 1);
            ones += v[(size_t)p * F + f];
          }
          CHECK(ones == counts[p]);
          CHECK(counts[p] <= (lengths[p / planes] < F ? lengths[p / planes] : F));
        }
        // ---- selection: fewer, as many and more output frames than voiced ones
        for (uint32_t Fo : {0u, 1u, F / 2, F, F + 3}) {
          const uint32_t so = cols + 2;
          std::vector<float> o((size_t)rows * planes * Fo * so, -1.0f);
          CHECK(mp3g_select_frames_host(x.data(), rows, planes, F, stride, cols, v.data(), lengths, o.data(), Fo, so,
                                        m.data()) == MP3G_OK);
          for (uint32_t p = 0; p < rows * planes; p++) {
            CHECK(m[p] == (counts[p] < Fo ? counts[p] : Fo));
            for (uint32_t j = 0; j < Fo; j++)
              for (uint32_t c = 0; c < so; c++) {
                const float w = o[((size_t)p * Fo + j) * so + c];
                if (c >= cols) CHECK(w == -1.0f);
                else if (j >= m[p]) CHECK(w == 0.0f && !std::signbit(w));
              }
          }
        }
      }
  }
  // ---- refusals (host, then the device calls: before any device call)
  {
    const uint32_t F = 4;
    std::vector<float> x((size_t)2 * F * 6), y(x.size());
    std::vector<uint8_t> v(2 * F);
    uint32_t n[2] = {4, 4}, cnt[2], m[2];
    float* px = x.data();
    float* py = y.data();
    CHECK(mp3g_sliding_cmn_host(px, py, 2, 1, F, 6, 7, n, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, py, 2, 1, F, 6, 6, n, 300, 100, 4) == inv);
    CHECK(mp3g_sliding_cmn_host(px, py, 2, 1, F, 6, 6, n, 0, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, py, 2, 1, F, 6, 6, n, 300, 0, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, px, 2, 1, F, 6, 6, n, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, px + 6, 1, 1, F - 1, 6, 6, n, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(nullptr, py, 2, 1, F, 6, 6, n, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, nullptr, 2, 1, F, 6, 6, n, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(px, py, 2, 1, F, 6, 6, nullptr, 300, 100, 0) == inv);
    CHECK(mp3g_sliding_cmn_host(nullptr, nullptr, 0, 1, F, 6, 6, nullptr, 300, 100, 0) == MP3G_OK);
    CHECK(mp3g_sliding_cmn_host(nullptr, nullptr, 2, 1, 0, 6, 6, nullptr, 300, 100, 0) == MP3G_OK);
    CHECK(mp3g_sliding_cmn_host(nullptr, nullptr, 2, 1, F, 6, 0, nullptr, 300, 100, 0) == MP3G_OK);
    CHECK(mp3g_sliding_cmn_rows(0, px, py, 2, 1, F, 6, 7, n, 300, 100, 0, nullptr) == inv);
    CHECK(mp3g_sliding_cmn_rows(0, px, px, 2, 1, F, 6, 6, n, 300, 100, 0, nullptr) == inv);
    CHECK(mp3g_sliding_cmn_rows(-1, px, py, 2, 1, F, 6, 6, n, 300, 100, 0, nullptr) == inv);
    CHECK(mp3g_sliding_cmn_rows(0, nullptr, nullptr, 0, 1, F, 6, 6, nullptr, 300, 100, 0, nullptr) == MP3G_OK);

    CHECK(mp3g_vad_energy_host(px, 2, 1, F, 6, 6, 6, n, 5, .5f, .6f, 0, v.data(), cnt) == inv);
    CHECK(mp3g_vad_energy_host(px, 2, 1, F, 6, 7, 0, n, 5, .5f, .6f, 0, v.data(), cnt) == inv);
    CHECK(mp3g_vad_energy_host(nullptr, 2, 1, F, 6, 6, 0, n, 5, .5f, .6f, 0, v.data(), cnt) == inv);
    CHECK(mp3g_vad_energy_host(px, 2, 1, F, 6, 6, 0, nullptr, 5, .5f, .6f, 0, v.data(), cnt) == inv);
    CHECK(mp3g_vad_energy_host(px, 2, 1, F, 6, 6, 0, n, 5, .5f, .6f, 0, nullptr, cnt) == inv);
    CHECK(mp3g_vad_energy_host(px, 2, 1, F, 6, 6, 0, n, 5, .5f, .6f, 0, v.data(), nullptr) == inv);
    CHECK(mp3g_vad_energy_host(nullptr, 0, 1, F, 6, 6, 0, nullptr, 5, .5f, .6f, 0, nullptr, nullptr) == MP3G_OK);
    cnt[0] = cnt[1] = 9;
    CHECK(mp3g_vad_energy_host(nullptr, 2, 1, 0, 6, 6, 0, n, 5, .5f, .6f, 0, nullptr, cnt) == MP3G_OK);
    CHECK(cnt[0] == 0 && cnt[1] == 0);
    CHECK(mp3g_vad_energy_rows(0, px, 2, 1, F, 6, 6, 6, n, 5, .5f, .6f, 0, v.data(), cnt, nullptr) == inv);
    CHECK(mp3g_vad_energy_rows(-1, px, 2, 1, F, 6, 6, 0, n, 5, .5f, .6f, 0, v.data(), cnt, nullptr) == inv);
    CHECK(mp3g_vad_energy_rows(0, nullptr, 2, 1, F, 6, 6, 0, n, 5, .5f, .6f, 0, v.data(), cnt, nullptr) == inv);

    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 7, v.data(), n, py, F, 7, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, v.data(), n, py, F, 5, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, v.data(), n, px, F, 6, m) == inv);
    CHECK(mp3g_select_frames_host(nullptr, 2, 1, F, 6, 6, v.data(), n, py, F, 6, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, nullptr, n, py, F, 6, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, v.data(), nullptr, py, F, 6, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, v.data(), n, nullptr, F, 6, m) == inv);
    CHECK(mp3g_select_frames_host(px, 2, 1, F, 6, 6, v.data(), n, py, F, 6, nullptr) == inv);
    CHECK(mp3g_select_frames_host(nullptr, 0, 1, F, 6, 6, nullptr, nullptr, nullptr, F, 6, nullptr) == MP3G_OK);
    CHECK(mp3g_select_frames_rows(0, px, 2, 1, F, 6, 6, v.data(), n, px, F, 6, m, nullptr) == inv);
    CHECK(mp3g_select_frames_rows(-1, px, 2, 1, F, 6, 6, v.data(), n, py, F, 6, m, nullptr) == inv);
    CHECK(mp3g_select_frames_rows(0, px, 2, 1, F, 6, 7, v.data(), n, py, F, 7, m, nullptr) == inv);
  }
  if (g_failed) {
    std::fprintf(stderr, "frameops_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("frameops_sanitize ok\n");
  return 0;
}
