// mfcc_sanitize.cpp -- the Kaldi MFCC features' and the per-row normalisation's
// host code under ASan + UBSan (go-mp3_amd/csrc/Makefile target asan-mfcc; run
// by tests/test_mfcc_cpu.py).  Host-only objects (device = -1): the DCT and
// lifter tables, mp3g_mfcc_host's edge cases in both framing modes and both
// energies, mp3g_cmvn_host and the argument refusals.  No device call is made.
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

static int create(int N, int hop, int n_mels, int n_ceps, double Q, double floor, uint32_t flags, mp3g_mfcc** out) {
  return mp3g_mfcc_create(-1, 16000, N, hop, n_mels, n_ceps, 20.0, 0.0, 0.97, 32768.0, Q, floor, 0, flags, out);
}

int main() {
  const uint32_t front = MP3G_FBANK_REMOVE_DC | MP3G_FBANK_SNIP_EDGES;
  const uint32_t all = front | MP3G_MFCC_USE_ENERGY | MP3G_MFCC_RAW_ENERGY;
  const double inf = std::numeric_limits<double>::infinity();
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  // ---- refusals, before anything is built
  mp3g_mfcc* mf = nullptr;
  CHECK(create(400, 160, 23, 0, 22, 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 24, 22, 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, -1, 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, std::nan(""), 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, inf, 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, -1, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, 1e-40, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, inf, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, 1e39, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, std::nan(""), all, &mf) == inv && !mf);
  CHECK(create(400, 160, 23, 13, 22, 0, 16, &mf) == inv && !mf);
  CHECK(create(400, 401, 23, 13, 22, 0, all, &mf) == inv && !mf);
  CHECK(create(400, 160, 0, 13, 22, 0, all, &mf) == inv && !mf);
  CHECK(create(15, 4, 4, 4, 22, 0, all, &mf) == uns && !mf);
  CHECK(create(1025, 160, 23, 13, 22, 0, all, &mf) == uns && !mf);
  CHECK(create(400, 160, 129, 13, 22, 0, all, &mf) == uns && !mf);
  CHECK(create(400, 160, 23, 13, 22, 0, all, nullptr) == inv);
  CHECK(mp3g_mfcc_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
  CHECK(mp3g_mfcc_frames(nullptr, 100) == 0);
  mp3g_mfcc_free(nullptr);

  // ---- tables: every configuration's sizes are walked to their last entry
  const int cfg[][4] = {{400, 160, 23, 13}, {400, 160, 40, 40}, {551, 220, 80, 20}, {1024, 1024, 128, 128},
                        {16, 4, 4, 4},      {400, 160, 23, 1},  {17, 1, 128, 1}};
  for (const auto& c : cfg)
    for (double Q : {22.0, 0.0}) {
      CHECK(create(c[0], c[1], c[2], c[3], Q, 0.0, all, &mf) == MP3G_OK);
      if (!mf) std::exit(2);
      const mp3g_fbank* fb = nullptr;
      uint32_t nc = 0, in_lds = 9, K = 0;
      const float *D = nullptr, *lift = nullptr, *w = nullptr;
      float lef = 1.f;
      CHECK(mp3g_mfcc_info(mf, &fb, &nc, &D, &lift, &lef, &in_lds) == MP3G_OK);
      CHECK(fb && nc == (uint32_t)c[3] && lef == 0.f && in_lds == 0);
      CHECK(mp3g_fbank_info(fb, nullptr, &K, nullptr, nullptr, nullptr, nullptr, &w, nullptr) == MP3G_OK && K >= 8);
      for (int i = 0; i < c[3]; i++) {
        double dot = 0;
        for (int m = 0; m < c[2]; m++) dot += (double)D[(size_t)i * c[2] + m] * D[(size_t)i * c[2] + m];
        CHECK(std::fabs(dot - 1.0) < 1e-5);
        CHECK(Q == 0.0 ? lift[i] == 1.0f : (lift[i] >= 1.0f - 11.0f && lift[i] <= 1.0f + 11.0f));
      }
      CHECK(w[c[0] - 1] >= 0.f);
      mp3g_mfcc_free(mf);
      mf = nullptr;
    }

  // ---- mp3g_mfcc_host: the shortest row, every frame count, strides, the refusals
  for (uint32_t flags = 0; flags < 16; flags++) {
    CHECK(create(61, 16, 10, 7, 22.0, flags & 4 ? 1.0 : 0.0, flags, &mf) == MP3G_OK);  // (an odd window: P = 64)
    if (!mf) std::exit(2);
    const bool snip = flags & MP3G_FBANK_SNIP_EDGES;
    const uint64_t Ts[] = {61, 76, 100, 257};
    for (uint64_t T : Ts) {
      std::vector<float> x(T);  // (exactly T samples: a read past either end is caught)
      for (uint64_t i = 0; i < T; i++) x[i] = std::sin(0.3f * (float)i) + (i % 5 == 0 ? 0.25f : 0.f);
      const uint64_t nf = mp3g_mfcc_frames(mf, T);
      CHECK(nf == (snip ? (T - 61) / 16 + 1 : (T + 8) / 16));
      std::vector<float> full(7 * nf, -1.f);
      CHECK(mp3g_mfcc_host(mf, x.data(), T, nf, full.data(), 7) == MP3G_OK);
      for (float v : full) CHECK(std::isfinite(v));
      // fewer frames, a wider stride: the same features, nothing else written
      std::vector<float> part(9 * nf, -7.f);
      CHECK(mp3g_mfcc_host(mf, x.data(), T, 1, part.data(), 9) == MP3G_OK);
      for (uint64_t i = 0; i < 9 * nf; i++) CHECK(part[i] == (i < 7 ? full[i] : -7.f));
      float y[16] = {};
      CHECK(mp3g_mfcc_host(mf, x.data(), T, nf + 1, full.data(), 7) == inv);
      CHECK(mp3g_mfcc_host(mf, x.data(), T, 1, y, 6) == inv);
      CHECK(mp3g_mfcc_host(mf, nullptr, T, 1, y, 7) == inv);
      CHECK(mp3g_mfcc_host(mf, x.data(), T, 1, nullptr, 7) == inv);
      CHECK(mp3g_mfcc_host(mf, x.data(), T, 0, nullptr, 7) == MP3G_OK);
    }
    CHECK(mp3g_mfcc_frames(mf, 60) == 0);
    CHECK(mp3g_mfcc_frames(mf, 1ull << 62) == 0);
    float y[16] = {}, z = 0;
    CHECK(mp3g_mfcc_host(mf, &z, 1, 1, y, 7) == inv);
    CHECK(mp3g_mfcc_host(mf, &z, 1ull << 62, 1, y, 7) == inv);
    CHECK(mp3g_mfcc_host(nullptr, &z, 1, 1, y, 7) == inv);
    // an all-zero row: the energy at its floor
    std::vector<float> zeros(200, 0.f), out(7 * 5, 1.f);
    CHECK(mp3g_mfcc_host(mf, zeros.data(), 200, 5, out.data(), 7) == MP3G_OK);
    if (flags & MP3G_MFCC_USE_ENERGY)
      for (int f = 0; f < 5; f++) CHECK(out[7 * f] == (flags & 4 ? 0.f : (float)(-23.0 * std::log(2.0))));
    // the device call refuses a host-only object before any device call
    CHECK(mp3g_mfcc_execute(mf, nullptr, 1, 1, 200, nullptr, 1, 7, nullptr) == inv);
    CHECK(mp3g_mfcc_execute(mf, nullptr, 1, 3, 200, nullptr, 1, 7, nullptr) == inv);
    mp3g_mfcc_free(mf);
    mf = nullptr;
  }

  // ---- mp3g_cmvn_host: exactly sized buffers, every length, the refusals
  for (uint32_t flags : {0u, (uint32_t)MP3G_CMVN_NORM_VARS}) {
    const uint32_t rows = 5, planes = 2, F = 7, stride = 6, cols = 5;
    const uint32_t lengths[rows] = {0, 1, 2, F, F + 5};
    std::vector<float> x((size_t)rows * planes * F * stride);
    for (size_t i = 0; i < x.size(); i++) x[i] = std::cos(0.7f * (float)i) * 100.f + (float)(i % stride);
    const std::vector<float> before = x;
    CHECK(mp3g_cmvn_host(x.data(), rows, planes, F, stride, cols, lengths, flags) == MP3G_OK);
    for (uint32_t r = 0; r < rows; r++)
      for (uint32_t p = 0; p < planes; p++)
        for (uint32_t f = 0; f < F; f++)
          for (uint32_t c = 0; c < stride; c++) {
            const size_t i = (((size_t)r * planes + p) * F + f) * stride + c;
            CHECK(std::isfinite(x[i]));
            if (c >= cols || f >= lengths[r]) CHECK(std::memcmp(&x[i], &before[i], 4) == 0);
            if (c < cols && f == 0 && lengths[r] == 1) CHECK(x[i] == 0.f);
          }
    CHECK(mp3g_cmvn_host(x.data(), rows, planes, F, 4, cols, lengths, flags) == inv);
    CHECK(mp3g_cmvn_host(nullptr, rows, planes, F, stride, cols, lengths, flags) == inv);
    CHECK(mp3g_cmvn_host(x.data(), rows, planes, F, stride, cols, nullptr, flags) == inv);
    CHECK(mp3g_cmvn_host(x.data(), rows, planes, F, stride, cols, lengths, 2) == inv);
    CHECK(mp3g_cmvn_host(nullptr, 0, planes, F, stride, cols, nullptr, flags) == MP3G_OK);
    CHECK(mp3g_cmvn_host(nullptr, rows, planes, 0, stride, cols, nullptr, flags) == MP3G_OK);
    CHECK(mp3g_cmvn_host(nullptr, rows, planes, F, stride, 0, nullptr, flags) == MP3G_OK);
    // the device call's refusals come before any device call
    CHECK(mp3g_cmvn_rows(0, x.data(), rows, planes, F, 4, cols, lengths, flags, nullptr) == inv);
    CHECK(mp3g_cmvn_rows(0, nullptr, rows, planes, F, stride, cols, lengths, flags, nullptr) == inv);
    CHECK(mp3g_cmvn_rows(-1, x.data(), rows, planes, F, stride, cols, lengths, flags, nullptr) == inv);
    CHECK(mp3g_cmvn_rows(0, nullptr, 0, planes, F, stride, cols, nullptr, flags, nullptr) == MP3G_OK);
  }

  if (g_failed) {
    std::fprintf(stderr, "mfcc_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("mfcc_sanitize ok\n");
  return 0;
}
