// specaug.h -- what the host reference and the kernels of specaug.hip share
// (include/mp3g.h "SpecAugment"): the descriptor's reading (which warp is a warp,
// how a mask is clipped), the integer source position of a warped frame with its
// four cubic weights, the tap chain and the end of the mean fill.  Both sides
// compile THESE functions, so a position, a weight or a clip cannot differ
// between them.
#pragma once
#include <cstdint>

#include "../../include/mp3g.h"

#if defined(__HIPCC__)
#define MP3G_SA_HD __host__ __device__
#else
#define MP3G_SA_HD
#endif

namespace mp3g {

constexpr uint32_t kSpecaugMaxWarpFrames = 1u << 22;  // (float)r and (float)(2 n_out) stay exact

// Whether (c, w) warps a row of n frames: both inside [1, n - 1].
MP3G_SA_HD inline bool specaug_warps(uint32_t c, uint32_t w, uint32_t n) {
  return n >= 2 && c >= 1 && c <= n - 1 && w >= 1 && w <= n - 1;
}

// A mask [start, start + width) clipped to [0, extent): *lo <= *hi, equal when
// nothing is masked.  The end is formed in 64 bits.
MP3G_SA_HD inline void specaug_clip(uint32_t start, uint32_t width, uint32_t extent, uint32_t* lo, uint32_t* hi) {
  const uint64_t end = (uint64_t)start + (uint64_t)width;
  const uint32_t h = end < (uint64_t)extent ? (uint32_t)end : extent;
  const uint32_t l = start < h ? start : h;
  *lo = l;
  *hi = h;
}

MP3G_SA_HD inline uint32_t specaug_count(uint32_t n, uint32_t max) { return n < max ? n : max; }

// Keys' cubic convolution kernel with A = -0.75, in the header's operation order.
MP3G_SA_HD inline float specaug_c1(float x) {
  return __builtin_fmaf(__builtin_fmaf(1.25f, x, -2.25f), x * x, 1.0f);
}
MP3G_SA_HD inline float specaug_c2(float x) {
  return __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(-0.75f, x, 3.75f), x, -6.0f), x, 3.0f);
}

// One warped destination frame: the four source frames src[0..3] (frames of the
// row, clamped to the frame's own segment) and their weights.
struct SpecaugTap {
  uint32_t src[4];
  float w[4];
};

// Destination frame j < n of a row warped by (c, w), specaug_warps(c, w, n).
MP3G_SA_HD inline void specaug_tap(uint32_t j, uint32_t c, uint32_t w, uint32_t n, SpecaugTap* tap) {
  uint32_t jj, n_in, n_out, base;
  if (j < w) {
    jj = j, n_in = c, n_out = w, base = 0;
  } else {
    jj = j - w, n_in = n - c, n_out = n - w, base = c;
  }
  const int64_t two_out = 2 * (int64_t)n_out;
  const int64_t p = (2 * (int64_t)jj + 1) * (int64_t)n_in - (int64_t)n_out;  // >= 1 - n_out
  const int64_t i = p >= 0 ? p / two_out : -1;
  const int64_t r = p - i * two_out;  // [0, 2 n_out)
  const float t = (float)(uint32_t)r / (float)(uint32_t)two_out;
  tap->w[0] = specaug_c2(t + 1.0f);
  tap->w[1] = specaug_c1(t);
  tap->w[2] = specaug_c1(1.0f - t);
  tap->w[3] = specaug_c2(2.0f - t);
  const int64_t last = (int64_t)n_in - 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 4; k++) {
    int64_t s = i - 1 + k;
    s = s < 0 ? 0 : (s > last ? last : s);
    tap->src[k] = base + (uint32_t)s;
  }
}

// The tap chain, in ascending source order.
MP3G_SA_HD inline float specaug_interp(const float w[4], float x0, float x1, float x2, float x3) {
  return __builtin_fmaf(w[3], x3, __builtin_fmaf(w[2], x2, __builtin_fmaf(w[1], x1, w[0] * x0)));
}

// The blocked sum of the per-frame sums s[0..n), as frameops.h defines P[n] with
// K = 32: one frame at a time.
constexpr uint32_t kSpecaugBlock = 32;
struct SpecaugTotal {
  double bp = 0.0, part = 0.0;
  uint32_t pos = 0;
  MP3G_SA_HD inline void add(double s) {
    part += s;
    pos++;
    if (pos % kSpecaugBlock == 0) {
      bp += part;
      part = 0.0;
    }
  }
  MP3G_SA_HD inline double total() const { return bp + part; }
};

// The fill of a plane from its total; n = 0 (or no bins) gives +0.0.
MP3G_SA_HD inline float specaug_mean(double total, uint32_t n, uint32_t n_bins) {
  if (n == 0 || n_bins == 0) return 0.0f;
  return (float)(total / ((double)n * (double)n_bins));
}

}  // namespace mp3g
