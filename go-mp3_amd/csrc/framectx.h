// framectx.h -- what the host references and the kernels of framectx.hip share
// (include/mp3g.h "Delta features and frame context"): the recurrence that makes
// Kaldi's delta scales, the clamp of a source frame to its row, the tap chain of
// one delta word and the number of frames a stack leaves.  Both sides compile
// THESE functions, so a scale, a source frame or a count cannot differ between
// them.
#pragma once
#include <cstdint>

#include "../../include/mp3g.h"

#if defined(__HIPCC__)
#define MP3G_FC_HD __host__ __device__
#else
#define MP3G_FC_HD
#endif

namespace mp3g {

constexpr uint32_t kDeltaMaxOrder = 4;  // O <= 4
constexpr uint32_t kDeltaMaxHalo = 32;  // O * W <= 32: the frames a word reads on either side
constexpr uint32_t kStackMaxContext = 64;  // left, right <= 64

// The scales of orders 1..O, as the kernel takes them: s[i - 1][j + i * W] is the
// tap of order i at offset j, -i W <= j <= i W.
struct DeltaTaps {
  float s[kDeltaMaxOrder][2 * kDeltaMaxHalo + 1];
};

// Kaldi's DeltaFeatures scales in float32: scales[0] = {1}; order i from the
// already rounded order i - 1, a float32 product then a float32 add per term (the
// translation units are built with -ffp-contract=off), then every entry times
// (float)(1 / sum of j^2).  Needs order <= kDeltaMaxOrder, order * window <=
// kDeltaMaxHalo, window >= 1.
MP3G_FC_HD inline void framectx_delta_taps(uint32_t order, uint32_t window, DeltaTaps* taps) {
  const int32_t W = (int32_t)window;
  float prev[2 * kDeltaMaxHalo + 1], cur[2 * kDeltaMaxHalo + 1];
  int32_t prev_len = 1;
  prev[0] = 1.0f;
  uint64_t norm = 0;
  for (int32_t j = -W; j <= W; j++) norm += (uint64_t)((int64_t)j * j);
  const float normalizer = (float)(1.0 / (double)norm);
  for (uint32_t i = 1; i <= order; i++) {
    const int32_t cur_len = prev_len + 2 * W, prev_offset = (prev_len - 1) / 2, cur_offset = prev_offset + W;
    for (int32_t k = 0; k < cur_len; k++) cur[k] = 0.0f;
    for (int32_t j = -W; j <= W; j++)
      for (int32_t k = -prev_offset; k <= prev_offset; k++) {
        const float term = (float)j * prev[k + prev_offset];
        cur[j + k + cur_offset] = cur[j + k + cur_offset] + term;
      }
    for (int32_t k = 0; k < cur_len; k++) {
      cur[k] = cur[k] * normalizer;
      taps->s[i - 1][k] = prev[k] = cur[k];
    }
    prev_len = cur_len;
  }
}

// Source frame t of a row of n >= 1 frames, clamped to [0, n - 1].
MP3G_FC_HD inline uint32_t framectx_clamp(int64_t t, uint32_t n) {
  return t < 0 ? 0u : (t > (int64_t)n - 1 ? n - 1 : (uint32_t)t);
}

// One tap of a delta word: a scale of exactly 0 is skipped (Kaldi's test; it
// keeps 0 * Inf out), every other one is an explicit fused multiply-add.
MP3G_FC_HD inline float framectx_tap(float scale, float x, float y) {
  return scale == 0.0f ? y : __builtin_fmaf(scale, x, y);
}

// The frames a stack with (step >= 1, first) leaves of a row of n.
MP3G_FC_HD inline uint32_t framectx_n_out(uint32_t n, uint32_t step, uint32_t first) {
  if (n <= first || step == 0) return 0;
  return (uint32_t)(((uint64_t)(n - first) + step - 1) / step);
}

}  // namespace mp3g
