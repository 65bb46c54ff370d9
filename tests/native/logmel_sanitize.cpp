// logmel_sanitize.cpp -- the log-mel features' host code under ASan + UBSan
// (go-mp3_amd/csrc/Makefile target asan-logmel; run by
// tests/test_logmel_cpu.py).  Host-only objects (device = -1): the table
// design, mp3g_logmel_host's edge cases, mp3g_log10f and the argument
// refusals.  No device call is made.
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

struct Info {
  uint32_t K = 0, tile = 0;
  const float *cw = nullptr, *sw = nullptr, *wm = nullptr;
  const uint32_t* support = nullptr;
};

static mp3g_logmel* make(int rate, int n_fft, int hop, int n_mels, uint32_t flags, Info* in) {
  mp3g_logmel* lm = nullptr;
  CHECK(mp3g_logmel_create(-1, rate, n_fft, hop, n_mels, 0.0, 0.0, flags, &lm) == MP3G_OK);
  if (!lm) std::exit(2);
  CHECK(mp3g_logmel_info(lm, &in->K, &in->cw, &in->sw, &in->wm, &in->support, &in->tile) == MP3G_OK);
  return lm;
}

int main() {
  const uint32_t both = MP3G_LOGMEL_CENTER | MP3G_LOGMEL_CLAMP;
  // ---- refusals, before anything is built
  mp3g_logmel* lm = nullptr;
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  CHECK(mp3g_logmel_create(-1, 0, 400, 160, 80, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 0, 160, 80, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 0, 80, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 401, 80, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 0, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, -1.0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, 0, 8000.5, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, 4000, 4000, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, std::nan(""), 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, 0, 0, 4, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-2, 16000, 400, 160, 80, 0, 0, both, &lm) == inv && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 12, 4, 4, 0, 0, both, &lm) == uns && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 402, 160, 80, 0, 0, both, &lm) == uns && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 1028, 160, 80, 0, 0, both, &lm) == uns && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 129, 0, 0, both, &lm) == uns && !lm);
  CHECK(mp3g_logmel_create(-1, 16000, 400, 160, 80, 0, 0, both, nullptr) == inv);
  CHECK(mp3g_logmel_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
  CHECK(mp3g_logmel_frames(nullptr, 100) == 0);
  mp3g_logmel_free(nullptr);

  // ---- tables: every configuration's sizes are walked to their last entry
  const int cfg[][4] = {{16000, 400, 160, 80}, {16000, 400, 160, 128}, {44100, 1024, 256, 128},
                        {16000, 16, 4, 4},     {16000, 1024, 1024, 1}, {8000, 16, 1, 128}};
  for (const auto& c : cfg) {
    Info in;
    lm = make(c[0], c[1], c[2], c[3], both, &in);
    CHECK(in.K == (uint32_t)c[1] / 2 + 1 && in.tile >= 8 && in.tile <= 32);
    double s = 0;
    for (size_t i = 0; i < (size_t)in.K * c[1]; i++) s += std::fabs(in.cw[i]) + std::fabs(in.sw[i]);
    CHECK(s > 0 && std::isfinite(s));
    for (int m = 0; m < c[3]; m++) {
      const uint32_t lo = in.support[2 * m], hi = in.support[2 * m + 1];
      CHECK(lo > hi || hi < in.K);
      for (uint32_t k = 0; k < in.K; k++) {
        const float w = in.wm[(size_t)m * in.K + k];
        CHECK(w >= 0.f && ((w != 0.f) <= (lo <= k && k <= hi)));
      }
    }
    mp3g_logmel_free(lm);
  }

  // ---- mp3g_logmel_host: the shortest row, every frame count, strides, the refusals
  for (uint32_t flags : {0u, (uint32_t)MP3G_LOGMEL_CENTER, (uint32_t)MP3G_LOGMEL_CLAMP, both}) {
    Info in;
    lm = make(16000, 64, 16, 10, flags, &in);
    const bool center = flags & MP3G_LOGMEL_CENTER;
    const uint64_t Ts[] = {center ? 33u : 64u, 100, 257};
    for (uint64_t T : Ts) {
      std::vector<float> x(T);  // (exactly T samples: a read past either end is caught)
      for (uint64_t i = 0; i < T; i++) x[i] = std::sin(0.3f * (float)i) + (i % 5 == 0 ? 0.25f : 0.f);
      const uint64_t nf = mp3g_logmel_frames(lm, T);
      CHECK(nf == (center ? T / 16 + 1 : (T - 64) / 16 + 1));
      std::vector<float> all(10 * nf, -1.f);
      CHECK(mp3g_logmel_host(lm, x.data(), T, nf, all.data(), nf) == MP3G_OK);
      for (float v : all) CHECK(std::isfinite(v));
      if (!(flags & MP3G_LOGMEL_CLAMP)) {  // fewer frames, a wider stride: the same features, nothing else written
        std::vector<float> part(10 * (nf + 3), -7.f);
        CHECK(mp3g_logmel_host(lm, x.data(), T, 1, part.data(), nf + 3) == MP3G_OK);
        for (int m = 0; m < 10; m++) {
          CHECK(part[m * (nf + 3)] == all[m * nf]);
          for (uint64_t f = 1; f < nf + 3; f++) CHECK(part[m * (nf + 3) + f] == -7.f);
        }
      }
      float y = 0;
      CHECK(mp3g_logmel_host(lm, x.data(), T, nf + 1, all.data(), nf + 1) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_logmel_host(lm, x.data(), T, 2, all.data(), 1) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_logmel_host(lm, nullptr, T, 1, &y, 1) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_logmel_host(lm, x.data(), T, 1, nullptr, 1) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_logmel_host(lm, x.data(), T, 0, nullptr, 0) == MP3G_OK);
    }
    CHECK(mp3g_logmel_frames(lm, center ? 32 : 63) == 0);
    CHECK(mp3g_logmel_frames(lm, 1ull << 62) == 0);
    float y = 0, z = 0;
    CHECK(mp3g_logmel_host(lm, &z, 1, 1, &y, 1) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_logmel_host(lm, &z, 1ull << 62, 1, &y, 1) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_logmel_host(nullptr, &z, 1, 1, &y, 1) == MP3G_ERR_INVALID_ARGUMENT);
    // an all-zero row: the floor, log10(1e-10f) = -10, clamped to (-10 + 4) / 4
    std::vector<float> zeros(200, 0.f), out(10 * 5, 1.f);
    CHECK(mp3g_logmel_host(lm, zeros.data(), 200, 5, out.data(), 5) == MP3G_OK);
    for (float v : out) CHECK(v == (flags & MP3G_LOGMEL_CLAMP ? -1.5f : -10.f));
    // the device call refuses a host-only object before any device call
    CHECK(mp3g_logmel_execute(lm, nullptr, 1, 1, 200, nullptr, 1, 1, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_logmel_execute(lm, nullptr, 1, 3, 200, nullptr, 1, 1, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
    mp3g_logmel_free(lm);
  }

  // ---- mp3g_log10f: powers of ten are exact, the extremes of the domain
  {
    const float x[] = {1e-10f, 1.f, 10.f, 1e10f, 1.1754944e-38f, 3.4028235e38f, 0.70710677f, 0.70710683f};
    float y[8];
    mp3g_logmel_log10f(x, 8, y);
    CHECK(y[0] == -10.f && y[1] == 0.f && y[2] == 1.f && y[3] == 10.f);
    for (int i = 0; i < 8; i++) CHECK(std::fabs((double)y[i] - std::log10((double)x[i])) < 3e-6);
  }

  if (g_failed) {
    std::fprintf(stderr, "logmel_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("logmel_sanitize ok\n");
  return 0;
}
