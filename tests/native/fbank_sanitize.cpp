// fbank_sanitize.cpp -- the Kaldi filter-bank features' host code under ASan +
// UBSan (go-mp3_amd/csrc/Makefile target asan-fbank; run by
// tests/test_fbank_cpu.py).  Host-only objects (device = -1): the table design,
// mp3g_fbank_host's edge cases in both framing modes, mp3g_logf and the
// argument refusals.  No device call is made.
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
  uint32_t P = 0, K = 0, tile = 0;
  const float *cw = nullptr, *sw = nullptr, *wm = nullptr, *w = nullptr;
  const uint32_t* support = nullptr;
};

static mp3g_fbank* make(int rate, int N, int hop, int n_mels, int window, uint32_t flags, Info* in) {
  mp3g_fbank* fb = nullptr;
  CHECK(mp3g_fbank_create(-1, rate, N, hop, n_mels, 20.0, 0.0, 0.97, 32768.0, window, flags, &fb) == MP3G_OK);
  if (!fb) std::exit(2);
  CHECK(mp3g_fbank_info(fb, &in->P, &in->K, &in->cw, &in->sw, &in->wm, &in->support, &in->w, &in->tile) == MP3G_OK);
  return fb;
}

int main() {
  const uint32_t both = MP3G_FBANK_REMOVE_DC | MP3G_FBANK_SNIP_EDGES;
  const double inf = std::numeric_limits<double>::infinity();
  // ---- refusals, before anything is built
  mp3g_fbank* fb = nullptr;
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  CHECK(mp3g_fbank_create(-1, 0, 400, 160, 80, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 0, 160, 80, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 0, 80, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 401, 80, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 0, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, -1.0, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 8000.5, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 4000, 4000, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, -8000, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, std::nan(""), 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, inf, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, -0.5, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 1.5, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, std::nan(""), 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 0, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, inf, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 1e39, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, std::nan(""), 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 32768, 4, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 32768, -1, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 32768, 0, 4, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-2, 16000, 400, 160, 80, 20, 0, 0.97, 32768, 0, both, &fb) == inv && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 15, 4, 4, 20, 0, 0.97, 32768, 0, both, &fb) == uns && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 1025, 160, 80, 20, 0, 0.97, 32768, 0, both, &fb) == uns && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 129, 20, 0, 0.97, 32768, 0, both, &fb) == uns && !fb);
  CHECK(mp3g_fbank_create(-1, 16000, 400, 160, 80, 20, 0, 0.97, 32768, 0, both, nullptr) == inv);
  CHECK(mp3g_fbank_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
  CHECK(mp3g_fbank_frames(nullptr, 100) == 0);
  mp3g_fbank_free(nullptr);

  // ---- tables: every configuration's sizes are walked to their last entry
  const int cfg[][5] = {{16000, 400, 160, 80, 0},  {16000, 400, 160, 128, 1}, {8000, 200, 80, 23, 2},
                        {22050, 551, 220, 80, 3},  {16000, 16, 4, 4, 0},      {16000, 1024, 1024, 1, 0},
                        {8000, 17, 1, 128, 0},     {44100, 1023, 441, 128, 0}};
  for (const auto& c : cfg) {
    Info in;
    fb = make(c[0], c[1], c[2], c[3], c[4], both, &in);
    uint32_t P = 16;
    while (P < (uint32_t)c[1]) P *= 2;
    CHECK(in.P == P && in.K == P / 2 && in.tile >= 8 && in.tile <= 32);
    double s = 0;
    for (size_t i = 0; i < (size_t)in.K * c[1]; i++) s += std::fabs(in.cw[i]) + std::fabs(in.sw[i]);
    for (int n = 0; n < c[1]; n++) s += in.w[n];
    CHECK(s > 0 && std::isfinite(s));
    for (int m = 0; m < c[3]; m++) {
      const uint32_t lo = in.support[2 * m], hi = in.support[2 * m + 1];
      CHECK(lo > hi || hi < in.K);
      for (uint32_t k = 0; k < in.K; k++) {
        const float w = in.wm[(size_t)m * in.K + k];
        CHECK(w >= 0.f && w <= 1.f && ((w != 0.f) <= (lo <= k && k <= hi)));
      }
    }
    mp3g_fbank_free(fb);
  }

  // ---- mp3g_fbank_host: the shortest row, every frame count, strides, the refusals
  for (uint32_t flags : {0u, (uint32_t)MP3G_FBANK_REMOVE_DC, (uint32_t)MP3G_FBANK_SNIP_EDGES, both}) {
    Info in;
    fb = make(16000, 61, 16, 10, 0, flags, &in);  // (an odd window: P = 64)
    const bool snip = flags & MP3G_FBANK_SNIP_EDGES;
    const uint64_t Ts[] = {61, 76, 100, 257};
    for (uint64_t T : Ts) {
      std::vector<float> x(T);  // (exactly T samples: a read past either end is caught)
      for (uint64_t i = 0; i < T; i++) x[i] = std::sin(0.3f * (float)i) + (i % 5 == 0 ? 0.25f : 0.f);
      const uint64_t nf = mp3g_fbank_frames(fb, T);
      CHECK(nf == (snip ? (T - 61) / 16 + 1 : (T + 8) / 16));
      std::vector<float> all(10 * nf, -1.f);
      CHECK(mp3g_fbank_host(fb, x.data(), T, nf, all.data(), 10) == MP3G_OK);
      for (float v : all) CHECK(std::isfinite(v));
      // fewer frames, a wider stride: the same features, nothing else written
      std::vector<float> part(13 * nf, -7.f);
      CHECK(mp3g_fbank_host(fb, x.data(), T, 1, part.data(), 13) == MP3G_OK);
      for (uint64_t i = 0; i < 13 * nf; i++) CHECK(part[i] == (i < 10 ? all[i] : -7.f));
      float y[16] = {};
      CHECK(mp3g_fbank_host(fb, x.data(), T, nf + 1, all.data(), 10) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_fbank_host(fb, x.data(), T, 1, y, 9) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_fbank_host(fb, nullptr, T, 1, y, 10) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_fbank_host(fb, x.data(), T, 1, nullptr, 10) == MP3G_ERR_INVALID_ARGUMENT);
      CHECK(mp3g_fbank_host(fb, x.data(), T, 0, nullptr, 10) == MP3G_OK);
    }
    CHECK(mp3g_fbank_frames(fb, 60) == 0);
    CHECK(mp3g_fbank_frames(fb, 1ull << 62) == 0);
    float y[16] = {}, z = 0;
    CHECK(mp3g_fbank_host(fb, &z, 1, 1, y, 10) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_fbank_host(fb, &z, 1ull << 62, 1, y, 10) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_fbank_host(nullptr, &z, 1, 1, y, 10) == MP3G_ERR_INVALID_ARGUMENT);
    // an all-zero row: the floor, ln(2^-23)
    std::vector<float> zeros(200, 0.f), out(10 * 5, 1.f);
    CHECK(mp3g_fbank_host(fb, zeros.data(), 200, 5, out.data(), 10) == MP3G_OK);
    for (float v : out) CHECK(v == (float)(-23.0 * std::log(2.0)));
    // the device call refuses a host-only object before any device call
    CHECK(mp3g_fbank_execute(fb, nullptr, 1, 1, 200, nullptr, 1, 10, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
    CHECK(mp3g_fbank_execute(fb, nullptr, 1, 3, 200, nullptr, 1, 10, nullptr) == MP3G_ERR_INVALID_ARGUMENT);
    mp3g_fbank_free(fb);
  }

  // ---- mp3g_logf: the exact values, the extremes of the domain
  {
    const float x[] = {0x1p-23f, 1.f, 2.f, 1e10f, 1.1754944e-38f, 3.4028235e38f, 0.70710677f, 0.70710683f};
    float y[8];
    mp3g_fbank_logf(x, 8, y);
    CHECK(y[0] == (float)(-23.0 * std::log(2.0)) && y[1] == 0.f && !std::signbit(y[1]) && y[2] == (float)std::log(2.0));
    for (int i = 0; i < 8; i++) CHECK(std::fabs((double)y[i] - std::log((double)x[i])) < 6e-6);
  }

  if (g_failed) {
    std::fprintf(stderr, "fbank_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("fbank_sanitize ok\n");
  return 0;
}
