// stft_sanitize.cpp -- the STFT features' host code under ASan + UBSan
// (go-mp3_amd/csrc/Makefile target asan-stft; run by tests/test_stft_cpu.py).
// Host-only objects (device = -1): the table design, mp3g_stft_host's edge cases
// in both framing modes and every output, the shared transform of stft_fft.h at
// all five sizes and the argument refusals.  No device call is made.
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

struct Info {
  uint32_t K = 0, tile = 0;
  const float *window = nullptr, *tw = nullptr, *wm = nullptr;
  const uint32_t* support = nullptr;
};

static const uint32_t kDefault = MP3G_STFT_CENTER | MP3G_STFT_MEL_NORM;

static mp3g_stft* make(int rate, int P, int win, int hop, int output, int n_mels, int log, float floor, uint32_t flags,
                       Info* in) {
  mp3g_stft* st = nullptr;
  CHECK(mp3g_stft_create(-1, rate, P, win, hop, output, n_mels, 0.0, 0.0, log, floor, flags, &st) == MP3G_OK);
  if (!st) std::exit(2);
  CHECK(mp3g_stft_info(st, &in->K, &in->window, &in->tw, &in->wm, &in->support, &in->tile) == MP3G_OK);
  return st;
}

// create with one argument list; the status
static int create(int rate, int P, int win, int hop, int output, int n_mels, double fmin, double fmax, int log,
                  float floor, uint32_t flags, int device = -1) {
  mp3g_stft* st = reinterpret_cast<mp3g_stft*>(&g_failed);  // (must come back NULL)
  const int status = mp3g_stft_create(device, rate, P, win, hop, output, n_mels, fmin, fmax, log, floor, flags, &st);
  CHECK(st == nullptr);
  return status;
}

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  const int PW = MP3G_STFT_POWER, CX = MP3G_STFT_COMPLEX, MG = MP3G_STFT_MAGNITUDE;
  const float inf = std::numeric_limits<float>::infinity();
  // ---- refusals, before anything is built
  CHECK(create(0, 2048, 2048, 512, PW, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 0, 512, PW, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2049, 512, PW, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 0, PW, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 2049, PW, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, 3, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, -1, 0, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 0, 0, 0, 3, 1.f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 0, 0, 0, -1, 1.f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, CX, 80, 0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, CX, 0, 0, 0, MP3G_STFT_LOG_LN, 1e-5f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, MP3G_STFT_LOG_LN, 0.f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, MP3G_STFT_LOG_LN, -1.f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, MP3G_STFT_LOG_LOG10, 1e-40f, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, MP3G_STFT_LOG_LOG10, inf, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, MP3G_STFT_LOG_LOG10, std::nanf(""), kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, -1.0, 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 22050.5, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 4000, 4000, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, std::nan(""), 0, 0, 0, kDefault) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, 0, 0, 8u) == inv);
  CHECK(create(44100, 2048, 2048, 512, PW, 80, 0, 0, 0, 0, kDefault, -2) == inv);
  for (int P : {0, -2048, 128, 400, 1000, 2047, 3072, 8192})
    CHECK(create(44100, P, P > 0 ? P : 1, 1, PW, 0, 0, 0, 0, 0, kDefault) == uns);
  CHECK(create(44100, 2048, 2048, 512, PW, 129, 0, 0, 0, 0, kDefault) == uns);
  CHECK(create(44100, 2048, 2048, 512, PW, -1, 0, 0, 0, 0, kDefault) == uns);
  CHECK(mp3g_stft_create(-1, 44100, 2048, 2048, 512, PW, 0, 0, 0, 0, 0, kDefault, nullptr) == inv);
  CHECK(mp3g_stft_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
  CHECK(mp3g_stft_frames(nullptr, 100) == 0);
  mp3g_stft_free(nullptr);
  CHECK(create(44100, 2048, 2048, 512, PW, 0, 0, 0, 0, 0, 8u | kDefault) == inv);
  {  // (the floor is ignored without a logarithm)
    Info in;
    mp3g_stft* st = make(44100, 256, 256, 64, PW, 0, 0, -1.f, kDefault, &in);
    CHECK(in.wm == nullptr && in.support == nullptr);
    mp3g_stft_free(st);
  }

  // ---- tables: every size's are walked to their last entry
  for (int P : {256, 512, 1024, 2048, 4096})
    for (uint32_t flags : {0u, 2u, 4u, 6u}) {
      Info in;
      const int wins[] = {1, P - 1, P};
      for (int win : wins) {
        mp3g_stft* st = make(44100, P, win, P / 4, PW, 128, 0, 0.f, flags, &in);
        CHECK(in.K == (uint32_t)P / 2 + 1 && (in.tile == 8 || in.tile == 16));
        double s = 0;
        int nz = 0;
        for (int n = 0; n < P; n++) {
          s += in.window[n] + in.tw[2 * n] * in.tw[2 * n] + in.tw[2 * n + 1] * in.tw[2 * n + 1];
          nz += in.window[n] != 0.f;
        }
        CHECK(std::fabs(s - (win == 1 ? 1.0 : 0.5 * win) - P) < 1e-3 * P);
        CHECK(nz == (win == 1 ? 1 : win - 1));
        for (int m = 0; m < 128; m++) {
          const uint32_t lo = in.support[2 * m], hi = in.support[2 * m + 1];
          CHECK(lo > hi || hi < in.K);
          for (uint32_t k = 0; k < in.K; k++) {
            const float w = in.wm[(size_t)m * in.K + k];
            CHECK(w >= 0.f && w <= 1.f && ((w != 0.f) <= (lo <= k && k <= hi)));
          }
        }
        mp3g_stft_free(st);
      }
    }

  // ---- mp3g_stft_host: the shortest rows, every frame count, strides, the refusals
  for (int P : {256, 512, 1024, 2048, 4096})
    for (uint32_t center : {0u, 1u})
      for (int output : {CX, PW, MG}) {
        Info in;
        const int hop = output == PW ? P : (output == MG ? 1 : P / 4);
        const int n_mels = output == CX || P == 512 ? 0 : 40;
        const int log = output == CX ? 0 : (output == PW ? MP3G_STFT_LOG_LN : MP3G_STFT_LOG_LOG10);
        mp3g_stft* st = make(44100, P, P - (output == MG), hop, output, n_mels, log, 1e-7f, center | 4u, &in);
        const uint32_t bins = n_mels ? (uint32_t)n_mels : in.K, w = output == CX ? 2 : 1;
        const uint64_t pad = center ? P / 2 : 0;
        const uint64_t Ts[] = {center ? pad + 1 : (uint64_t)P, (uint64_t)P + 3, (uint64_t)(2 * P + 37)};
        for (uint64_t T : Ts) {
          std::vector<float> x(T);  // (exactly T samples: a read past either end is caught)
          for (uint64_t i = 0; i < T; i++) x[i] = std::sin(0.3f * (float)i) + (i % 5 == 0 ? 0.25f : 0.f);
          uint64_t nf = mp3g_stft_frames(st, T);
          CHECK(nf == (center ? T / hop + 1 : (T - P) / hop + 1));
          if (nf > 40) nf = 40;  // (hop = 1)
          std::vector<float> all(bins * nf * w, -1.f);
          CHECK(mp3g_stft_host(st, x.data(), T, nf, all.data(), nf) == MP3G_OK);
          for (float v : all) CHECK(std::isfinite(v));
          if (output == CX)
            for (uint64_t f = 0; f < nf; f++) {
              CHECK(all[f * 2 + 1] == 0.f && !std::signbit(all[f * 2 + 1]));
              CHECK(all[((bins - 1) * nf + f) * 2 + 1] == 0.f && !std::signbit(all[((bins - 1) * nf + f) * 2 + 1]));
            }
          // fewer frames, a wider stride: the same values, nothing else written
          const uint64_t stride = nf + 3;
          std::vector<float> part(bins * stride * w, -7.f);
          CHECK(mp3g_stft_host(st, x.data(), T, 1, part.data(), stride) == MP3G_OK);
          for (uint32_t b = 0; b < bins; b++)
            for (uint64_t f = 0; f < stride; f++)
              for (uint32_t c = 0; c < w; c++) {
                const float got = part[(b * stride + f) * w + c];
                CHECK(f == 0 ? std::memcmp(&got, &all[(b * nf + f) * w + c], 4) == 0 : got == -7.f);
              }
          float y[2] = {};
          CHECK(mp3g_stft_host(st, x.data(), T, mp3g_stft_frames(st, T) + 1, all.data(), 1u << 20) == inv);
          CHECK(mp3g_stft_host(st, x.data(), T, 2, all.data(), 1) == inv);
          CHECK(mp3g_stft_host(st, nullptr, T, 1, y, 1) == inv);
          CHECK(mp3g_stft_host(st, x.data(), T, 1, nullptr, 1) == inv);
          CHECK(mp3g_stft_host(st, x.data(), T, 0, nullptr, 0) == MP3G_OK);
        }
        CHECK(mp3g_stft_frames(st, center ? pad : (uint64_t)P - 1) == 0);
        CHECK(mp3g_stft_frames(st, 1ull << 62) == 0);
        float y[2] = {}, z = 0;
        CHECK(mp3g_stft_host(st, &z, 1, 1, y, 1) == inv);
        CHECK(mp3g_stft_host(st, &z, 1ull << 62, 1, y, 1) == inv);
        CHECK(mp3g_stft_host(nullptr, &z, 1, 1, y, 1) == inv);
        // the device call refuses a host-only object before any device call
        CHECK(mp3g_stft_execute(st, nullptr, 1, 1, 3 * P, nullptr, 1, 10, nullptr) == inv);
        CHECK(mp3g_stft_execute(st, nullptr, 1, 3, 3 * P, nullptr, 1, 10, nullptr) == inv);
        mp3g_stft_free(st);
      }

  // an all-zero row: the floor's logarithm
  {
    Info in;
    mp3g_stft* st = make(22050, 1024, 1024, 256, PW, 80, MP3G_STFT_LOG_LOG10, 1e-10f, kDefault, &in);
    std::vector<float> zeros(3000, 0.f), out(80 * 5, 1.f);
    CHECK(mp3g_stft_host(st, zeros.data(), 3000, 5, out.data(), 5) == MP3G_OK);
    for (float v : out) CHECK(v == -10.f);
    mp3g_stft_free(st);
  }

  if (g_failed) {
    std::fprintf(stderr, "stft_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("stft_sanitize ok\n");
  return 0;
}
