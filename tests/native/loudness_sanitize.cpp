// loudness_sanitize.cpp -- the BS.1770 loudness measure's and the gain stage's
// host code under ASan + UBSan (go-mp3_amd/csrc/Makefile target asan-loudness;
// run by tests/test_loudness_cpu.py).  Host-only objects (device = -1): the
// K-weighting design and the segment tables at the rates' edges,
// mp3g_loudness_host on exactly sized buffers at every length around a segment
// and a block, mp3g_gain_host and the argument refusals.  No device call is made.
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

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  const double inf = std::numeric_limits<double>::infinity();
  // ---- refusals, before anything is built
  mp3g_loudness* ld = reinterpret_cast<mp3g_loudness*>(1);
  CHECK(mp3g_loudness_create(-1, 0, &ld) == inv && !ld);
  CHECK(mp3g_loudness_create(-1, -5, &ld) == inv && !ld);
  CHECK(mp3g_loudness_create(-1, 7999, &ld) == uns && !ld);
  CHECK(mp3g_loudness_create(-1, 192001, &ld) == uns && !ld);
  CHECK(mp3g_loudness_create(-3, 48000, &ld) == inv && !ld);
  CHECK(mp3g_loudness_create(-1, 48000, nullptr) == inv);
  CHECK(mp3g_loudness_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
  CHECK(mp3g_loudness_blocks(nullptr, 1000) == 0);
  CHECK(mp3g_loudness_scratch_bytes(nullptr, 1, 1, 1000) == 0);
  mp3g_loudness_free(nullptr);

  // ---- tables: walked to their last entry at the rates' edges and the odd segment
  for (int rate : {8000, 11025, 44100, 48000, 192000}) {
    CHECK(mp3g_loudness_create(-1, rate, &ld) == MP3G_OK);
    if (!ld) std::exit(2);
    uint32_t H = 0;
    const double *shelf = nullptr, *hp = nullptr, *V = nullptr, *AH = nullptr, *G = nullptr;
    CHECK(mp3g_loudness_info(ld, &H, &shelf, &hp, &V, &AH, &G) == MP3G_OK);
    CHECK(H == (uint32_t)((rate + 5) / 10));
    CHECK(hp[0] == 1.0 && hp[1] == -2.0 && hp[2] == 1.0 && shelf[0] > 1.0);
    double g00 = 0.0;
    for (uint32_t n = 0; n < H; n++) {
      for (uint32_t k = 0; k < 4; k++) CHECK(std::isfinite(V[4 * (size_t)n + k]));
      g00 += V[4 * (size_t)n] * V[4 * (size_t)n];
    }
    CHECK(g00 == G[0]);
    for (int k = 0; k < 16; k++) CHECK(std::isfinite(AH[k]) && std::isfinite(G[k]));
    CHECK(mp3g_loudness_blocks(ld, 4ull * H - 1) == 0 && mp3g_loudness_blocks(ld, 4ull * H) == 1);
    CHECK(mp3g_loudness_scratch_bytes(ld, 2, 2, 5 * H + 1) == 2ull * 2 * 6 * 76);
    CHECK(mp3g_loudness_scratch_bytes(ld, 1, 3, 100) == 0);
    mp3g_loudness_free(ld);
    ld = nullptr;
  }

  // ---- mp3g_loudness_host: exactly sized buffers at every length around a segment and a block
  CHECK(mp3g_loudness_create(-1, 8000, &ld) == MP3G_OK);
  if (!ld) std::exit(2);
  const uint32_t H = 800;
  const double target = mp3g_loudness_target_energy(-23.0);
  CHECK(std::fabs(target - std::pow(10.0, -2.2309)) < 1e-15);
  for (uint32_t planes = 1; planes <= 2; planes++)
    for (uint32_t T : {0u, 1u, H - 1, H, H + 1, 4 * H - 1, 4 * H, 4 * H + 1, 5 * H + 17, 9 * H}) {
      const uint32_t rows = 3;
      std::vector<float> x((size_t)rows * planes * T);  // (exactly sized: a read past either end is caught)
      for (size_t i = 0; i < x.size(); i++) x[i] = 0.2f * std::sin(0.37f * (float)i) + (i % 7 == 0 ? 0.1f : 0.f);
      std::vector<mp3g_loudness_stats> st(rows), st2(rows);
      std::memset(st.data(), 0x5a, rows * sizeof(st[0]));
      CHECK(mp3g_loudness_host(ld, T ? x.data() : nullptr, rows, planes, T, nullptr, st.data()) == MP3G_OK);
      const uint32_t nb = T / H >= 4 ? T / H - 3 : 0;
      for (uint32_t r = 0; r < rows; r++) {
        CHECK(st[r].n_blocks == nb && st[r].n_abs == nb && st[r].n_gated == nb && st[r].zero == 0);
        CHECK(nb ? (st[r].energy > 0.0 && std::isfinite(st[r].lufs)) : (st[r].energy == 0.0 && std::isinf(st[r].lufs)));
        CHECK(T ? st[r].peak > 0.f : st[r].peak == 0.f);
      }
      // lengths: zero, over the end, one short
      const uint32_t lengths[rows] = {0, T + 9, T ? T - 1 : 0};
      CHECK(mp3g_loudness_host(ld, T ? x.data() : nullptr, rows, planes, T, lengths, st2.data()) == MP3G_OK);
      CHECK(st2[0].energy == 0.0 && st2[0].peak == 0.f && st2[0].n_blocks == 0);
      CHECK(std::memcmp(&st2[1], &st[1], sizeof(st[1])) == 0);
      // the gain: in place, nothing past a row's length
      std::vector<float> y = x, gains(rows, -1.f);
      CHECK(mp3g_gain_host(T ? y.data() : nullptr, rows, planes, T, lengths, st2.data(), target, 0.5f, gains.data()) ==
            MP3G_OK);
      CHECK(gains[0] == 1.0f && gains[1] > 0.f && gains[2] > 0.f);
      for (uint32_t p = 0; p < planes; p++) {
        for (uint32_t n = 0; n < T; n++) CHECK(y[(size_t)p * T + n] == x[(size_t)p * T + n]);  // (row 0: length 0)
        if (T) CHECK(std::memcmp(&y[((size_t)2 * planes + p) * T + T - 1], &x[((size_t)2 * planes + p) * T + T - 1], 4) == 0);
      }
      if (st2[1].energy > 0.0 && T)
        CHECK(y[(size_t)planes * T] == x[(size_t)planes * T] * gains[1]);
    }
  {
    float x[8] = {};
    mp3g_loudness_stats st = {};
    CHECK(mp3g_loudness_host(nullptr, x, 1, 1, 8, nullptr, &st) == inv);
    CHECK(mp3g_loudness_host(ld, x, 1, 0, 8, nullptr, &st) == inv);
    CHECK(mp3g_loudness_host(ld, x, 1, 3, 2, nullptr, &st) == inv);
    CHECK(mp3g_loudness_host(ld, nullptr, 1, 1, 8, nullptr, &st) == inv);
    CHECK(mp3g_loudness_host(ld, x, 1, 1, 8, nullptr, nullptr) == inv);
    CHECK(mp3g_loudness_host(ld, x, 1, 1, 1u << 31, nullptr, &st) == uns);
    CHECK(mp3g_loudness_host(ld, nullptr, 0, 1, 8, nullptr, nullptr) == MP3G_OK);
    CHECK(mp3g_gain_host(x, 1, 3, 8, nullptr, &st, target, 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, &st, 0.0, 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, &st, inf, 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, &st, std::nan(""), 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, &st, target, -1.f, nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, &st, target, std::nanf(""), nullptr) == inv);
    CHECK(mp3g_gain_host(x, 1, 1, 8, nullptr, nullptr, target, 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(nullptr, 1, 1, 8, nullptr, &st, target, 0.f, nullptr) == inv);
    CHECK(mp3g_gain_host(nullptr, 0, 1, 8, nullptr, nullptr, target, 0.f, nullptr) == MP3G_OK);
    // the device calls' refusals come before any device call
    CHECK(mp3g_loudness_rows(ld, x, 1, 1, 8, nullptr, nullptr, 0, x, &st, nullptr) == inv);  // (a host-only object)
    CHECK(mp3g_loudness_rows(nullptr, x, 1, 1, 8, nullptr, nullptr, 0, x, &st, nullptr) == inv);
    CHECK(mp3g_loudness_rows(ld, x, 1, 3, 2, nullptr, nullptr, 0, x, &st, nullptr) == inv);
    CHECK(mp3g_gain_rows(-1, x, 1, 1, 8, nullptr, &st, target, 0.f, nullptr, nullptr) == inv);
    CHECK(mp3g_gain_rows(0, x, 1, 3, 8, nullptr, &st, target, 0.f, nullptr, nullptr) == inv);
    CHECK(mp3g_gain_rows(0, x, 1, 1, 8, nullptr, &st, -1.0, 0.f, nullptr, nullptr) == inv);
    CHECK(mp3g_gain_rows(0, nullptr, 0, 1, 8, nullptr, nullptr, target, 0.f, nullptr, nullptr) == MP3G_OK);
  }
  mp3g_loudness_free(ld);

  if (g_failed) {
    std::fprintf(stderr, "loudness_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("loudness_sanitize ok\n");
  return 0;
}
