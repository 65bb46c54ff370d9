// varresample_sanitize.cpp -- the variable-ratio resampler's host code under
// ASan + UBSan (go-mp3_amd/csrc/Makefile target asan-varresample; run by
// tests/test_varresample_cpu.py).  Host-only objects (device = -1): the
// prototype table, mp3g_varresample_host's edge cases over every kind of ratio
// and the argument refusals.  No device call is made.
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
  uint32_t P = 0, Z = 0, R = 0, tile = 0, stage = 0;
  const float* table = nullptr;
};

static mp3g_varresampler* make(int zeros, double rolloff, double beta, int precision, Info* info) {
  mp3g_varresampler* r = nullptr;
  CHECK(mp3g_varresampler_create(-1, zeros, rolloff, beta, precision, &r) == MP3G_OK);
  if (!r) std::exit(2);
  CHECK(mp3g_varresampler_info(r, &info->P, &info->Z, &info->R, &info->table, &info->tile, &info->stage) == MP3G_OK);
  return r;
}

int main() {
  const double fz = MP3G_RESAMPLE_FAST_ROLLOFF, fb = MP3G_RESAMPLE_FAST_BETA;
  // ---- refusals, before anything is built
  mp3g_varresampler* r = nullptr;
  CHECK(mp3g_varresampler_create(-1, 0, fz, fb, 9, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_varresampler_create(-1, 65, fz, fb, 9, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_varresampler_create(-1, 16, fz, fb, 4, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_varresampler_create(-1, 16, fz, fb, 10, &r) == MP3G_ERR_UNSUPPORTED && !r);
  CHECK(mp3g_varresampler_create(-1, 16, 0.0, fb, 9, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_varresampler_create(-1, 16, 1.0001, fb, 9, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_varresampler_create(-1, 16, std::nan(""), fb, 9, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);
  CHECK(mp3g_varresampler_create(-1, 16, 0.03, fb, 5, &r) == MP3G_ERR_INVALID_ARGUMENT && !r);  // R == 0
  CHECK(mp3g_varresampler_create(-1, 16, fz, fb, 9, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresampler_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
        MP3G_ERR_INVALID_ARGUMENT);
  mp3g_varresampler_free(nullptr);

  // ---- the table: sizes, its ends, F + D = the next F to float32 rounding
  struct Case { int zeros, P; double rolloff, beta; uint32_t R; };
  const Case cases[] = {{16, 9, fz, fb, 435},
                        {64, 9, MP3G_RESAMPLE_BEST_ROLLOFF, MP3G_RESAMPLE_BEST_BETA, 485},
                        {4, 7, fz, fb, 108},
                        {1, 5, 1.0, 0.0, 32},
                        {64, 5, fz, fb, 27}};
  for (const Case& c : cases) {
    Info in;
    r = make(c.zeros, c.rolloff, c.beta, c.P, &in);
    CHECK(in.P == (uint32_t)c.P && in.Z == (uint32_t)c.zeros << c.P && in.R == c.R && in.tile > 0 && in.stage > 0);
    CHECK(in.table && in.table[0] == 1.f && in.table[2 * in.Z] == 0.f && in.table[2 * in.Z + 1] == 0.f);
    for (uint32_t i = 0; i + 1 <= in.Z; i++)
      CHECK(std::fabs((double)in.table[2 * i] + (double)in.table[2 * i + 1] - (double)in.table[2 * i + 2]) < 2e-7);
    mp3g_varresampler_free(r);
  }

  // ---- mp3g_varresample_host: windows before, over and after the source range, every kind of ratio
  Info in;
  r = make(4, fz, fb, 9, &in);
  const uint64_t N = 1000;
  std::vector<float> x(N);
  for (uint64_t i = 0; i < N; i++) x[i] = std::sin(0.01f * (float)i) + (i % 7 == 0 ? 0.5f : 0.f);
  struct Ratio { uint32_t num, den; };
  const Ratio ratios[] = {{441, 160}, {4851, 1600}, {10, 11}, {1, 435}, {435, 1}, {457317, 160000},
                          {2147483647u, 2147483000u}, {2147483000u, 2147483647u}, {48, 1}, {1, 48}};
  for (const Ratio& q : ratios) {
    const uint64_t n_y = (N * q.den + q.num - 1) / q.num;
    const uint64_t n_all = n_y + 64;
    std::vector<float> y(n_all, -1.f);
    CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, n_all, y.data(), q.num, q.den, 1.f) == MP3G_OK);
    // a window equals the same outputs of the whole, wherever it lies
    const uint64_t starts[] = {0, 1, n_y / 2, n_y > 3 ? n_y - 3 : 0, n_y, n_y + 40};
    for (uint64_t s : starts) {
      std::vector<float> w(20, -2.f);
      CHECK(mp3g_varresample_host(r, x.data(), 0, N, s, 20, w.data(), q.num, q.den, 1.f) == MP3G_OK);
      CHECK(std::memcmp(w.data(), y.data() + s, 20 * sizeof(float)) == 0);
    }
    // a part of the source at its origin = the whole with the rest zeroed
    {
      std::vector<float> part(x.begin() + 200, x.begin() + 600), px(N, 0.f);
      std::copy(part.begin(), part.end(), px.begin() + 200);
      std::vector<float> a(n_all), b(n_all);
      CHECK(mp3g_varresample_host(r, part.data(), 200, 400, 0, n_all, a.data(), q.num, q.den, 0.5f) == MP3G_OK);
      CHECK(mp3g_varresample_host(r, px.data(), 0, N, 0, n_all, b.data(), q.num, q.den, 0.5f) == MP3G_OK);
      CHECK(std::memcmp(a.data(), b.data(), n_all * sizeof(float)) == 0);
    }
    // a large out_start with the source far from the origin: the same bits as near zero when out_start moves by
    // a multiple of den (q moves by the same multiple of num)
    {
      const uint64_t k = ((1ull << 33) + 7) / q.den + 1, shift = k * q.den, q_shift = k * q.num;
      if (q_shift < (1ull << 61)) {
        std::vector<float> w(32, -2.f);
        const uint64_t s = n_y / 3;
        CHECK(mp3g_varresample_host(r, x.data(), q_shift, N, shift + s, 32, w.data(), q.num, q.den, 1.f) == MP3G_OK);
        CHECK(std::memcmp(w.data(), y.data() + s, 32 * sizeof(float)) == 0);
      }
    }
  }
  // empty calls touch nothing; an empty source gives zeros
  CHECK(mp3g_varresample_host(r, nullptr, 0, 0, 0, 0, nullptr, 3, 2, 1.f) == MP3G_OK);
  float z[4] = {-3.f, -3.f, -3.f, -3.f};
  CHECK(mp3g_varresample_host(r, nullptr, 0, 0, 5, 4, z, 3, 2, 1.f) == MP3G_OK);
  CHECK(z[0] == 0.f && z[3] == 0.f);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 0, nullptr, 3, 2, 1.f) == MP3G_OK);
  // refusals
  CHECK(mp3g_varresample_host(nullptr, x.data(), 0, N, 0, 1, z, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, nullptr, 0, N, 0, 1, z, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, nullptr, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, z, 0, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, z, 3, 0, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, z, 1u << 31, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, z, 3, 1u << 31, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 1, z, 436, 1, 1.f) == MP3G_ERR_INVALID_ARGUMENT);  // I == 0
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, 1ull << 62, 1, z, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 1ull << 62, N, 0, 1, z, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  CHECK(mp3g_varresample_host(r, x.data(), 0, N, ~0ull, 2, z, 3, 2, 1.f) == MP3G_ERR_INVALID_ARGUMENT);
  // the largest indices accepted
  {
    const uint64_t big = (1ull << 62) / 4851 * 1600 - 4 * 1600ull;
    float yb[8];
    CHECK(mp3g_varresample_host(r, x.data(), (1ull << 62) - 1 - N, N, big - 8, 8, yb, 4851, 1600, 1.f) == MP3G_OK);
    CHECK(mp3g_varresample_host(r, x.data(), 5, N, (1ull << 62) - 9, 8, yb, 1, 435, 1.f) == MP3G_OK);
  }
  // num == den: a copy times gain, zero outside the source, -0 kept
  {
    std::vector<float> w(N + 10, -1.f);
    x[3] = -0.f;
    CHECK(mp3g_varresample_host(r, x.data(), 5, N, 0, N + 10, w.data(), 77, 77, 1.f) == MP3G_OK);
    CHECK(w[0] == 0.f && w[4] == 0.f && w[N + 5] == 0.f && std::memcmp(&w[5], x.data(), N * sizeof(float)) == 0);
    CHECK(mp3g_varresample_host(r, x.data(), 5, N, 3, 4, w.data(), 1, 1, 2.f) == MP3G_OK);
    CHECK(w[0] == 0.f && w[2] == 2.f * x[0] && w[3] == 2.f * x[1]);
  }
  mp3g_varresampler_free(r);

  // ---- the long filter at its narrowest and widest cutoffs
  r = make(64, MP3G_RESAMPLE_BEST_ROLLOFF, MP3G_RESAMPLE_BEST_BETA, 9, &in);
  {
    std::vector<float> y(40);
    CHECK(mp3g_varresample_host(r, x.data(), 0, N, 0, 3, y.data(), 485, 1, 1.f) == MP3G_OK);  // I == 1: Wr = Z
    CHECK(mp3g_varresample_host(r, x.data(), 0, N, 10, 40, y.data(), 48, 1, 1.f) == MP3G_OK);
    CHECK(mp3g_varresample_host(r, x.data(), 0, N, 500, 40, y.data(), 10, 11, 1.f) == MP3G_OK);
  }
  mp3g_varresampler_free(r);

  if (g_failed) {
    std::fprintf(stderr, "varresample_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("varresample_sanitize ok\n");
  return 0;
}
