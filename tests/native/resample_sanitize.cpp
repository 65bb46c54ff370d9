// resample_sanitize.cpp -- the resampler's host code under ASan + UBSan
// (go-mp3_amd/csrc/Makefile target asan-resample; run by
// tests/test_resample_cpu.py).  Host-only resamplers (device = -1): the filter
// design, mp3g_resample_host's edge cases and the argument refusals.  No
// device call is made.
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
  uint32_t L = 0, M = 0, W = 0, tile = 0;
  const float* taps = nullptr;
};

static mp3g_resampler* make(int fi, int fo, int zeros, double rolloff, double beta, Info* info) {
  mp3g_resampler* r = nullptr;
  CHECK(mp3g_resampler_create(-1, fi, fo, zeros, rolloff, beta, &r) == MP3G_OK);
  if (!r) std::exit(2);
  CHECK(mp3g_resampler_info(r, &info->L, &info->M, &info->W, &info->taps, &info->tile) == MP3G_OK);
  return r;
}

// y[n] over the whole zero-extended signal, one output per call
static float one(const mp3g_resampler* r, const std::vector<float>& x, uint64_t origin, uint64_t n) {
  float y = -1.f;
  CHECK(mp3g_resample_host(r, x.data(), origin, x.size(), n, 1, &y) == MP3G_OK);
  return y;
}

int main() {
  const double fz = MP3G_RESAMPLE_FAST_ROLLOFF, fb = MP3G_RESAMPLE_FAST_BETA;
  // ---- refusals, before anything is built
  mp3g_resampler* r = nullptr;
  CHECK(mp3g_resampler_create(-1, 0, 16000, 16, fz, fb, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_resampler_create(-1, 44100, -1, 16, fz, fb, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16000, 0, fz, fb, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16000, 65, fz, fb, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16000, 16, 0.0, fb, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16000, 16, std::nan(""), fb, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16001, 16, fz, fb, &r) == MP3G_ERR_UNSUPPORTED && !r);  // L 2W > 2^18
  CHECK(mp3g_resampler_create(-1, 2147483647, 1, 16, fz, fb, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_resampler_create(-1, 44100, 16000, 16, fz, fb, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_resampler_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
  mp3g_resampler_free(nullptr);

  // ---- filter design: the sizes, a DC gain near 1 in every phase
  struct Case { int fi, fo, zeros; double rolloff, beta; uint32_t L, M, W; };
  const Case cases[] = {
      {44100, 16000, 16, fz, fb, 160, 441, 52},
      {44100, 16000, 64, MP3G_RESAMPLE_BEST_ROLLOFF, MP3G_RESAMPLE_BEST_BETA, 160, 441, 187},
      {32000, 44100, 64, MP3G_RESAMPLE_BEST_ROLLOFF, MP3G_RESAMPLE_BEST_BETA, 441, 320, 68},
      {48000, 16000, 16, fz, fb, 1, 3, 57},
      {24000, 16000, 4, fz, fb, 2, 3, 8},
  };
  for (const Case& c : cases) {
    Info in;
    r = make(c.fi, c.fo, c.zeros, c.rolloff, c.beta, &in);
    CHECK(in.L == c.L && in.M == c.M && in.W == c.W && in.tile > 0 && in.taps);
    if (c.zeros >= 16) {
      for (uint32_t ph = 0; ph < in.L; ph++) {
        double s = 0;
        for (uint32_t k = 0; k < 2 * in.W; k++) s += in.taps[(size_t)ph * 2 * in.W + k];
        CHECK(std::fabs(s - 1.0) < 3e-5);
      }
    }
    mp3g_resampler_free(r);
  }

  // ---- mp3g_resample_host: windows before, over and after the source range
  Info in;
  r = make(44100, 16000, 4, fz, fb, &in);
  const uint64_t N = 1000;
  std::vector<float> x(N);
  for (uint64_t i = 0; i < N; i++) x[i] = std::sin(0.01f * (float)i) + (i % 7 == 0 ? 0.5f : 0.f);
  const uint64_t n_y = (N * in.L + in.M - 1) / in.M;
  std::vector<float> y(n_y + 64, -1.f);
  CHECK(mp3g_resample_host(r, x.data(), 0, N, 0, n_y + 64, y.data()) == MP3G_OK);
  // a window equals the same outputs of the whole, wherever it lies
  const uint64_t starts[] = {0, 1, in.L - 1, in.L, n_y - 3, n_y, n_y + 40};
  for (uint64_t s : starts) {
    std::vector<float> w(20, -2.f);
    CHECK(mp3g_resample_host(r, x.data(), 0, N, s, 20, w.data()) == MP3G_OK);
    CHECK(std::memcmp(w.data(), y.data() + s, 20 * sizeof(float)) == 0);
  }
  // far past the source: zeros
  for (uint64_t i = n_y + 30; i < n_y + 64; i++) CHECK(y[i] == 0.f);
  // empty calls touch nothing
  CHECK(mp3g_resample_host(r, nullptr, 0, 0, 0, 0, nullptr) == MP3G_OK);
  float z[4] = {-3.f, -3.f, -3.f, -3.f};
  CHECK(mp3g_resample_host(r, nullptr, 0, 0, 5, 4, z) == MP3G_OK);  // an empty source: all zero
  CHECK(z[0] == 0.f && z[3] == 0.f);
  CHECK(mp3g_resample_host(r, x.data(), 0, N, 0, 0, nullptr) == MP3G_OK);
  CHECK(mp3g_resample_host(nullptr, x.data(), 0, N, 0, 1, z) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_resample_host(r, nullptr, 0, N, 0, 1, z) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_resample_host(r, x.data(), 0, N, 0, 1, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
  // a source part with its origin: the part [200, 600) alone, outputs inside it
  {
    std::vector<float> part(x.begin() + 200, x.begin() + 600), px(N, 0.f);
    std::copy(part.begin(), part.end(), px.begin() + 200);
    for (uint64_t n = 60; n < 230; n += 13) CHECK(one(r, part, 200, n) == one(r, px, 0, n));
  }
  // a large out_start with the source at the matching origin: same bits as
  // the same phase near zero (out_start a multiple of L moves q by a multiple of M)
  {
    const uint64_t shift = ((1ull << 33) / in.L + 1) * in.L, q_shift = shift / in.L * in.M;
    for (uint64_t n = 0; n < n_y; n += 17) CHECK(one(r, x, q_shift, shift + n) == y[n]);
    // the largest indices accepted, and the first refused
    const uint64_t big = (1ull << 62) / in.M * in.L - 4 * (uint64_t)in.L;
    float yb = -1.f;
    CHECK(mp3g_resample_host(r, x.data(), (1ull << 62) - 1 - N, N, big - 8, 8, &y[0]) == MP3G_OK);
    CHECK(mp3g_resample_host(r, x.data(), 0, N, 1ull << 62, 1, &yb) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_resample_host(r, x.data(), 1ull << 62, N, 0, 1, &yb) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_resample_host(r, x.data(), 0, N, ~0ull, 2, &yb) == MP3G_ERR_INVALID_ARGUMENT);
  }
  mp3g_resampler_free(r);

  // ---- equal rates: a copy, zero outside the source
  r = make(16000, 16000, 16, fz, fb, &in);
  CHECK(in.L == 1 && in.M == 1 && in.W == 0 && !in.taps);
  {
    std::vector<float> w(N + 10, -1.f);
    CHECK(mp3g_resample_host(r, x.data(), 5, N, 0, N + 10, w.data()) == MP3G_OK);
    CHECK(w[0] == 0.f && w[4] == 0.f && w[N + 5] == 0.f && std::memcmp(&w[5], x.data(), N * sizeof(float)) == 0);
  }
  mp3g_resampler_free(r);

  if (g_failed) {
    std::fprintf(stderr, "resample_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("resample_sanitize ok\n");
  return 0;
}
