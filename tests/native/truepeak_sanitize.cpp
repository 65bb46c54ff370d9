// truepeak_sanitize.cpp -- the true peak's, the loudness range's and the
// gain-with-peak's host code under ASan + UBSan (go-mp3_amd/csrc/Makefile target
// asan-truepeak; run by tests/test_truepeak_cpu.py).  Host-only objects
// (device = -1): mp3g_true_peak_host on exactly sized buffers at every length
// around the interpolator's 12 taps and a tile, mp3g_loudness_range_host at
// every segment count around a short-term block, mp3g_gain_host_peak and the
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

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  // ---- the coefficients: walked to their last entry
  const float* c = nullptr;
  CHECK(mp3g_true_peak_coefs(nullptr) == inv);
  CHECK(mp3g_true_peak_coefs(&c) == MP3G_OK && c);
  if (!c) std::exit(2);
  for (int t = 0; t < 12; t++) {
    CHECK(c[t] == c[2 * 12 + 11 - t] && c[12 + t] == c[12 + 11 - t]);
    for (int f = 0; f < 3; f++) CHECK(std::fabs(c[12 * f + t]) > 1e-6f && std::fabs(c[12 * f + t]) < 1.0f);
  }
  const uint32_t tile = mp3g_true_peak_tile();
  CHECK(tile >= 12);

  // ---- mp3g_true_peak_host: exactly sized buffers at every length around the taps and a tile
  for (uint32_t planes = 1; planes <= 2; planes++)
    for (uint32_t T : {0u, 1u, 3u, 11u, 12u, 13u, 100u, tile - 1, tile, tile + 1}) {
      const uint32_t rows = 3;
      std::vector<float> x((size_t)rows * planes * T);  // (exactly sized: a read past either end is caught)
      for (size_t i = 0; i < x.size(); i++) x[i] = 0.4f * std::sin(0.37f * (float)i) + (i % 7 == 0 ? 0.1f : 0.f);
      std::vector<float> tp(rows, -1.f), tp2(rows, -1.f);
      CHECK(mp3g_true_peak_host(T ? x.data() : nullptr, rows, planes, T, nullptr, tp.data()) == MP3G_OK);
      for (uint32_t r = 0; r < rows; r++) {
        float peak = 0.f;
        for (size_t i = (size_t)r * planes * T; i < (size_t)(r + 1) * planes * T; i++)
          peak = std::fmax(peak, std::fabs(x[i]));
        CHECK(tp[r] >= peak && tp[r] <= 1.8642f * peak * (1.f + 0x1p-20f));
        CHECK(T ? tp[r] > 0.f : (tp[r] == 0.f && !std::signbit(tp[r])));
      }
      // lengths: zero, over the end, one short
      const uint32_t lengths[rows] = {0, T + 9, T ? T - 1 : 0};
      CHECK(mp3g_true_peak_host(T ? x.data() : nullptr, rows, planes, T, lengths, tp2.data()) == MP3G_OK);
      CHECK(tp2[0] == 0.f && tp2[1] == tp[1] && tp2[2] <= tp[2]);
    }
  {
    float x[8] = {}, tp = 7.f;
    CHECK(mp3g_true_peak_host(x, 1, 0, 8, nullptr, &tp) == inv);
    CHECK(mp3g_true_peak_host(x, 1, 3, 2, nullptr, &tp) == inv);
    CHECK(mp3g_true_peak_host(nullptr, 1, 1, 8, nullptr, &tp) == inv);
    CHECK(mp3g_true_peak_host(x, 1, 1, 8, nullptr, nullptr) == inv);
    CHECK(mp3g_true_peak_host(x, 1, 1, 1u << 31, nullptr, &tp) == uns);
    CHECK(mp3g_true_peak_host(nullptr, 0, 1, 8, nullptr, nullptr) == MP3G_OK);
    CHECK(tp == 7.f);
    CHECK(mp3g_true_peak_scratch_bytes(1, 3, 8) == 0);
    // the device call's refusals come before any device call
    CHECK(mp3g_true_peak_rows(-1, x, 1, 1, 8, nullptr, nullptr, 0, x, &tp, nullptr) == inv);
    CHECK(mp3g_true_peak_rows(0, x, 1, 3, 2, nullptr, nullptr, 0, x, &tp, nullptr) == inv);
    CHECK(mp3g_true_peak_rows(0, x, 1, 1, 8, nullptr, nullptr, 0, x, nullptr, nullptr) == inv);
    CHECK(mp3g_true_peak_rows(0, nullptr, 0, 1, 8, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == MP3G_OK);
    CHECK(tp == 7.f);
  }

  // ---- mp3g_loudness_range_host: every segment count around a short-term block
  mp3g_loudness* ld = nullptr;
  CHECK(mp3g_loudness_create(-1, 8000, &ld) == MP3G_OK);
  if (!ld) std::exit(2);
  const uint32_t H = 800;
  const double target = mp3g_loudness_target_energy(-23.0);
  for (uint32_t planes = 1; planes <= 2; planes++)
    for (uint32_t T : {0u, 1u, 4 * H, 29 * H + H - 1, 30 * H, 30 * H + 1, 31 * H, 45 * H + 17}) {
      const uint32_t rows = 3;
      std::vector<float> x((size_t)rows * planes * T);  // (exactly sized)
      for (size_t i = 0; i < x.size(); i++)
        x[i] = (0.2f + 0.15f * std::sin(2e-4f * (float)i)) * std::sin(0.37f * (float)i) + (i % 7 == 0 ? 0.1f : 0.f);
      std::vector<mp3g_loudness_range> out(rows), out2(rows);
      std::memset(out.data(), 0x5a, rows * sizeof(out[0]));
      CHECK(mp3g_loudness_range_host(ld, T ? x.data() : nullptr, rows, planes, T, nullptr, out.data()) == MP3G_OK);
      const uint32_t nseg = T / H, ns = nseg >= 30 ? nseg - 29 : 0;
      for (uint32_t r = 0; r < rows; r++) {
        CHECK(out[r].n_short == ns && out[r].n_range == ns && out[r].zero == 0);
        CHECK(nseg >= 4 ? std::isfinite(out[r].momentary_max) : std::isinf(out[r].momentary_max));
        CHECK(ns ? (std::isfinite(out[r].shortterm_max) && out[r].range_lo <= out[r].range_hi && out[r].lra >= 0.f)
                 : (std::isinf(out[r].shortterm_max) && std::isinf(out[r].range_lo) && out[r].lra == 0.f));
      }
      const uint32_t lengths[rows] = {0, T + 9, T ? T - 1 : 0};
      CHECK(mp3g_loudness_range_host(ld, T ? x.data() : nullptr, rows, planes, T, lengths, out2.data()) == MP3G_OK);
      CHECK(out2[0].n_short == 0 && std::isinf(out2[0].momentary_max) && out2[0].lra == 0.f);
      CHECK(std::memcmp(&out2[1], &out[1], sizeof(out[1])) == 0);
      // the gain against a supplied peak: in place, nothing past a row's length
      std::vector<mp3g_loudness_stats> st(rows);
      std::vector<float> tp(rows), y = x, y2 = x, gains(rows, -1.f), gains2(rows, -1.f);
      CHECK(mp3g_loudness_host(ld, T ? x.data() : nullptr, rows, planes, T, lengths, st.data()) == MP3G_OK);
      CHECK(mp3g_true_peak_host(T ? x.data() : nullptr, rows, planes, T, lengths, tp.data()) == MP3G_OK);
      float* yp = T ? y.data() : nullptr;
      float* y2p = T ? y2.data() : nullptr;
      CHECK(mp3g_gain_host_peak(yp, rows, planes, T, lengths, st.data(), target, 0.25f, gains.data(), tp.data()) ==
            MP3G_OK);
      CHECK(mp3g_gain_host(y2p, rows, planes, T, lengths, st.data(), target, 0.25f, gains2.data()) == MP3G_OK);
      for (uint32_t r = 0; r < rows; r++) CHECK(gains[r] <= gains2[r] && gains[r] > 0.f);
      CHECK(gains[0] == 1.0f);
      for (uint32_t p = 0; p < planes; p++) {
        for (uint32_t n = 0; n < T; n++) CHECK(y[(size_t)p * T + n] == x[(size_t)p * T + n]);  // (row 0: length 0)
        const size_t end = ((size_t)2 * planes + p) * T + T - 1;  // (row 2 is one short: its last sample stays)
        if (T) CHECK(std::memcmp(&y[end], &x[end], 4) == 0);
      }
      // a null peak array is mp3g_gain_host
      std::vector<float> y3 = x, gains3(rows, -1.f);
      CHECK(mp3g_gain_host_peak(T ? y3.data() : nullptr, rows, planes, T, lengths, st.data(), target, 0.25f,
                                gains3.data(), nullptr) == MP3G_OK);
      CHECK(y3.size() == y2.size() && (y3.empty() || std::memcmp(y3.data(), y2.data(), y3.size() * 4) == 0));
      CHECK(std::memcmp(gains3.data(), gains2.data(), rows * 4) == 0);
    }
  {
    float x[8] = {};
    mp3g_loudness_range out;
    std::memset(&out, 0x5a, sizeof(out));
    const mp3g_loudness_range before = out;
    mp3g_loudness_stats st = {};
    CHECK(mp3g_loudness_range_host(nullptr, x, 1, 1, 8, nullptr, &out) == inv);
    CHECK(mp3g_loudness_range_host(ld, x, 1, 0, 8, nullptr, &out) == inv);
    CHECK(mp3g_loudness_range_host(ld, x, 1, 3, 2, nullptr, &out) == inv);
    CHECK(mp3g_loudness_range_host(ld, nullptr, 1, 1, 8, nullptr, &out) == inv);
    CHECK(mp3g_loudness_range_host(ld, x, 1, 1, 8, nullptr, nullptr) == inv);
    CHECK(mp3g_loudness_range_host(ld, x, 1, 1, 1u << 31, nullptr, &out) == uns);
    CHECK(mp3g_loudness_range_host(ld, nullptr, 0, 1, 8, nullptr, nullptr) == MP3G_OK);
    CHECK(mp3g_loudness_range_scratch_bytes(nullptr, 1, 1, 8) == 0);
    CHECK(mp3g_loudness_range_scratch_bytes(ld, 2, 2, 5 * H + 1) == 2ull * 6 * 8);
    // (a host-only object, then none)
    CHECK(mp3g_loudness_range_rows(ld, 1, 1, 8, nullptr, nullptr, 0, x, x, &out, nullptr) == inv);
    CHECK(mp3g_loudness_range_rows(nullptr, 1, 1, 8, nullptr, nullptr, 0, x, x, &out, nullptr) == inv);
    CHECK(std::memcmp(&out, &before, sizeof(out)) == 0);
    CHECK(mp3g_gain_host_peak(x, 1, 3, 8, nullptr, &st, target, 0.f, nullptr, x) == inv);
    CHECK(mp3g_gain_host_peak(x, 1, 1, 8, nullptr, &st, 0.0, 0.f, nullptr, x) == inv);
    CHECK(mp3g_gain_host_peak(x, 1, 1, 8, nullptr, &st, target, -1.f, nullptr, x) == inv);
    CHECK(mp3g_gain_host_peak(x, 1, 1, 8, nullptr, nullptr, target, 0.f, nullptr, x) == inv);
    CHECK(mp3g_gain_host_peak(nullptr, 1, 1, 8, nullptr, &st, target, 0.f, nullptr, x) == inv);
    CHECK(mp3g_gain_host_peak(nullptr, 0, 1, 8, nullptr, nullptr, target, 0.f, nullptr, nullptr) == MP3G_OK);
    CHECK(mp3g_gain_rows_peak(-1, x, 1, 1, 8, nullptr, &st, target, 0.f, nullptr, nullptr, x) == inv);
    CHECK(mp3g_gain_rows_peak(0, x, 1, 3, 8, nullptr, &st, target, 0.f, nullptr, nullptr, x) == inv);
    CHECK(mp3g_gain_rows_peak(0, nullptr, 0, 1, 8, nullptr, nullptr, target, 0.f, nullptr, nullptr, x) == MP3G_OK);
  }
  mp3g_loudness_free(ld);

  if (g_failed) {
    std::fprintf(stderr, "truepeak_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("truepeak_sanitize ok\n");
  return 0;
}
