// framectx_sanitize.cpp -- the delta features' and the frame context's host code
// under ASan + UBSan (go-mp3_amd/csrc/Makefile target asan-framectx; run by
// tests/test_framectx_cpu.py).  Host buffers of exactly the sizes the contract
// names: mp3g_delta_scales, mp3g_add_deltas_host and mp3g_stack_frames_host over
// every limit of their parameters (orders 0..4, halos up to 32 on rows shorter
// than the halo, contexts up to 64, steps and firsts past the row, lengths per
// row and per plane, 0 and 2^32 - 1 among them), and the argument refusals of the
// host and the device calls.  No device call is made.
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

static uint32_t g_seed = 2468;
static uint32_t rnd32() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}
static float rnd() { return (float)rnd32() / 16777216.0f; }

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT, uns = MP3G_ERR_UNSUPPORTED;
  const uint32_t rows = 8, big = 0xffffffffu;
  // ---- scales
  for (uint32_t O = 0; O <= 4; O++)
    for (uint32_t W : {1u, 2u, 8u, 16u, 32u}) {
      if (O * W > 32) {
        float one;
        CHECK(mp3g_delta_scales(O, W, &one) == uns);
        continue;
      }
      std::vector<float> s((O + 1) + W * O * (O + 1));
      CHECK(mp3g_delta_scales(O, W, s.data()) == MP3G_OK);
      CHECK(s[0] == 1.0f);
      for (float v : s) CHECK(std::isfinite(v));
    }
  // ---- deltas and stacks of every shape
  for (uint32_t planes : {1u, 2u})
    for (uint32_t F : {1u, 2u, 5u, 33u, 70u})
      for (uint32_t cols : {1u, 4u, 13u}) {
        const uint32_t stride = cols + (F % 2 ? 3 : 0);
        const uint32_t per_row[rows] = {0, 1, 2, F / 2, F, F + 7, big, 3};
        std::vector<uint32_t> per_plane(rows * planes);
        for (uint32_t i = 0; i < rows * planes; i++) per_plane[i] = per_row[(i * 3 + 1) % rows];
        std::vector<float> x((size_t)rows * planes * F * stride);
        for (float& v : x) v = 20.0f * rnd() - 5.0f;
        for (uint32_t lp : {1u, planes}) {
          const uint32_t* lengths = lp == 1 ? per_row : per_plane.data();
          const uint32_t ow[][2] = {{0, 1}, {0, 900}, {1, 2}, {2, 2}, {3, 1}, {1, 32}, {4, 8}, {2, 16}};
          for (const auto& p : ow) {
            const uint32_t O = p[0], W = p[1], live = (O + 1) * cols, so = live + (cols % 2 ? 2 : 0);
            std::vector<float> y((size_t)rows * planes * F * so, -1.0f);
            CHECK(mp3g_add_deltas_host(x.data(), y.data(), rows, planes, F, stride, cols, so, lengths, lp, O, W) ==
                  MP3G_OK);
            for (size_t i = 0; i < y.size(); i++) {
              if (i % so >= live) CHECK(y[i] == -1.0f);  // the stride's tail: never written
              else CHECK(std::isfinite(y[i]));
            }
            for (uint32_t r = 0; r < rows; r++)
              for (uint32_t pl = 0; pl < planes; pl++) {
                const uint32_t len = lengths[lp == 1 ? r : r * planes + pl], n = len < F ? len : F;
                const size_t plane = (size_t)r * planes + pl;
                for (uint32_t t = 0; t < F; t++)
                  for (uint32_t c = 0; c < cols; c++) {
                    const float got = y[(plane * F + t) * so + c];
                    CHECK(t < n ? got == x[(plane * F + t) * stride + c] : (got == 0.0f && !std::signbit(got)));
                  }
              }
          }
          const uint32_t lrsf[][4] = {{0, 0, 1, 0}, {3, 3, 1, 0}, {3, 3, 6, 0}, {0, 0, 3, 2},   {64, 64, 1, 0},
                                      {64, 0, 7, 5}, {0, 64, big, 0}, {1, 1, 1, big}, {2, 1, 2, F}, {1, 2, 3, F - 1}};
          for (const auto& p : lrsf) {
            const uint32_t left = p[0], right = p[1], step = p[2], first = p[3], ctx = left + right + 1;
            const uint32_t full = mp3g_stack_frames_count(F, step, first);
            for (uint32_t Fo : {0u, full / 2, full, full + 3}) {
              const uint32_t live = ctx * cols, so = live + (cols % 2 ? 1 : 0);
              std::vector<float> y((size_t)rows * planes * Fo * so, -1.0f);
              std::vector<uint32_t> m(rows * planes, 77u);
              CHECK(mp3g_stack_frames_host(x.data(), rows, planes, F, stride, cols, lengths, lp, left, right, step,
                                           first, y.data(), Fo, so, m.data()) == MP3G_OK);
              for (size_t i = 0; i < y.size(); i++) {
                if (i % so >= live) CHECK(y[i] == -1.0f);
                else CHECK(std::isfinite(y[i]));
              }
              for (uint32_t r = 0; r < rows; r++)
                for (uint32_t pl = 0; pl < planes; pl++) {
                  const uint32_t len = lengths[lp == 1 ? r : r * planes + pl], n = len < F ? len : F;
                  const uint32_t want = mp3g_stack_frames_count(n, step, first);
                  CHECK(m[r * planes + pl] == (want < Fo ? want : Fo));
                }
            }
          }
        }
      }
  // ---- refusals, the same for the host and the device call (before any device call)
  {
    std::vector<float> x(2 * 6 * 8 + 8), y(2 * 6 * 40);
    const uint32_t lengths[2] = {6, 3};
    uint32_t m[2];
    auto deltas = [&](const float* in, float* out, uint32_t nr, uint32_t np, uint32_t F, uint32_t stride, uint32_t nc,
                      uint32_t so, const uint32_t* len, uint32_t lp, uint32_t O, uint32_t W, int want) {
      CHECK(mp3g_add_deltas_host(in, out, nr, np, F, stride, nc, so, len, lp, O, W) == want);
      if (want != MP3G_OK || !nr || !np || !F || !nc)  // (an accepted call with work would reach the device)
        CHECK(mp3g_add_deltas_rows(0, in, out, nr, np, F, stride, nc, so, len, lp, O, W, nullptr) == want);
    };
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, MP3G_OK);
    deltas(x.data(), y.data(), 2, 1, 6, 7, 8, 24, lengths, 1, 2, 2, inv);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 23, lengths, 1, 2, 2, inv);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 0, inv);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 24, lengths, 2, 2, 2, inv);
    deltas(x.data(), x.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, inv);
    deltas(nullptr, y.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, inv);
    deltas(x.data(), nullptr, 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, inv);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 24, nullptr, 1, 2, 2, inv);
    deltas(x.data(), x.data() + 8, 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, inv);
    deltas(x.data() + 8, x.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, inv);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 48, lengths, 1, 5, 1, uns);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 17, uns);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 40, lengths, 1, 4, 9, uns);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 40, lengths, 1, 4, 8, MP3G_OK);
    deltas(x.data(), y.data(), 2, 1, 6, 8, 8, 8, lengths, 1, 0, big, MP3G_OK);
    deltas(nullptr, nullptr, 0, 1, 6, 8, 8, 24, nullptr, 1, 2, 2, MP3G_OK);
    deltas(nullptr, nullptr, 2, 0, 6, 8, 8, 24, nullptr, 1, 2, 2, MP3G_OK);
    deltas(nullptr, nullptr, 2, 1, 0, 8, 8, 24, nullptr, 1, 2, 2, MP3G_OK);
    deltas(nullptr, nullptr, 2, 1, 6, 8, 0, 24, nullptr, 1, 2, 2, MP3G_OK);
    CHECK(mp3g_add_deltas_rows(-1, x.data(), y.data(), 2, 1, 6, 8, 8, 24, lengths, 1, 2, 2, nullptr) == inv);
    float one;
    CHECK(mp3g_delta_scales(1, 0, &one) == inv);
    CHECK(mp3g_delta_scales(1, 2, nullptr) == inv);
    CHECK(mp3g_delta_scales(5, 1, &one) == uns);

    auto stack = [&](const float* in, uint32_t nr, uint32_t np, uint32_t F, uint32_t stride, uint32_t nc,
                     const uint32_t* len, uint32_t lp, uint32_t left, uint32_t right, uint32_t step, float* out,
                     uint32_t Fo, uint32_t so, uint32_t* lo, int want) {
      CHECK(mp3g_stack_frames_host(in, nr, np, F, stride, nc, len, lp, left, right, step, 0, out, Fo, so, lo) == want);
      if (want != MP3G_OK || !nr || !np)
        CHECK(mp3g_stack_frames_rows(0, in, nr, np, F, stride, nc, len, lp, left, right, step, 0, out, Fo, so, lo,
                                     nullptr) == want);
    };
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, y.data(), 6, 24, m, MP3G_OK);
    stack(x.data(), 2, 1, 6, 7, 8, lengths, 1, 1, 1, 1, y.data(), 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, y.data(), 6, 23, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 0, y.data(), 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 2, 1, 1, 1, y.data(), 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, x.data(), 6, 24, m, inv);
    stack(nullptr, 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, y.data(), 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, nullptr, 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, nullptr, 1, 1, 1, 1, y.data(), 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, y.data(), 6, 24, nullptr, inv);
    stack(x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, x.data() + 8, 6, 24, m, inv);
    stack(x.data(), 2, 1, 6, 1, 1, lengths, 1, 65, 0, 1, y.data(), 6, 66, m, uns);
    stack(x.data(), 2, 1, 6, 1, 1, lengths, 1, 0, 65, 1, y.data(), 6, 66, m, uns);
    stack(nullptr, 0, 1, 6, 8, 8, nullptr, 1, 1, 1, 1, nullptr, 6, 24, nullptr, MP3G_OK);
    stack(nullptr, 2, 0, 6, 8, 8, nullptr, 1, 1, 1, 1, nullptr, 6, 24, nullptr, MP3G_OK);
    m[0] = m[1] = 9;
    stack(nullptr, 2, 1, 6, 8, 0, lengths, 1, 1, 1, 1, nullptr, 6, 24, m, MP3G_OK);  // no word, but the counts
    CHECK(m[0] == 6 && m[1] == 3);
    stack(nullptr, 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, nullptr, 0, 24, m, MP3G_OK);
    CHECK(m[0] == 0 && m[1] == 0);
    stack(nullptr, 2, 1, 0, 8, 8, lengths, 1, 1, 1, 1, y.data(), 6, 24, m, MP3G_OK);  // no frames: zeros
    CHECK(y[0] == 0.0f && m[0] == 0);
    CHECK(mp3g_stack_frames_rows(-1, x.data(), 2, 1, 6, 8, 8, lengths, 1, 1, 1, 1, 0, y.data(), 6, 24, m, nullptr) ==
          inv);
  }
  if (g_failed) {
    std::fprintf(stderr, "framectx_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("framectx_sanitize ok\n");
  return 0;
}
