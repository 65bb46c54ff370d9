// frameops.h -- what the host references and the kernels of frameops.hip share
// (include/mp3g.h "Sliding-window CMN, energy VAD and voiced-frame selection"):
// the window rule of the sliding mean and the blocked order of its sums.  Both
// sides compile THESE functions, so a window or a sum cannot differ between them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MP3G_FO_HD __host__ __device__
#else
#define MP3G_FO_HD
#endif

namespace mp3g {

// The sums' block: frames are cut into blocks of kFrameBlock.  b[j] is the
// float64 sum of (double)x[f] over block j, f ascending from +0.0; Bp[j] the
// float64 sum of b[0..j), ascending from +0.0; P[f] = Bp[f / K] + (block f / K's
// partial sum up to but excluding f, ascending from +0.0).
constexpr uint32_t kFrameBlock = 32;

// The window [s, e) of frame t in a row of n frames (t < n): Kaldi's
// SlidingWindowCmnInternal, in the words of include/mp3g.h.  0 <= s <= t < e
// <= n; s and e never decrease in t and grow by at most one per frame.
MP3G_FO_HD inline void scmn_window(uint32_t t, uint32_t n, uint32_t W, uint32_t min_window, bool center, uint32_t* s_out,
                                   uint32_t* e_out) {
  int64_t s, e;
  if (center) {
    s = (int64_t)t - (int64_t)(W / 2);
    e = s + (int64_t)W;
  } else {
    s = (int64_t)t - (int64_t)W;
    e = (int64_t)t + 1;
  }
  if (s < 0) {
    e -= s;
    s = 0;
  }
  if (!center && e > (int64_t)t) {
    const int64_t a = (int64_t)t + 1, b = (int64_t)min_window;
    e = a > b ? a : b;
  }
  if (e > (int64_t)n) {
    s -= e - (int64_t)n;
    e = (int64_t)n;
    if (s < 0) s = 0;
  }
  *s_out = (uint32_t)s;
  *e_out = (uint32_t)e;
}

// One prefix chain: P[pos] = Bp[pos / K] + part (and the same over the squares),
// walked forward one frame at a time; the partial sums restart at each block
// boundary, where the block prefix takes over.
struct PrefixChain {
  uint32_t pos;
  double part, part2;
  MP3G_FO_HD inline void start(uint32_t block_first) {
    pos = block_first;
    part = 0.0;
    part2 = 0.0;
  }
  MP3G_FO_HD inline void add(float x) {
    const double v = (double)x;
    part += v;
    part2 += v * v;
    pos++;
    if (pos % kFrameBlock == 0) {
      part = 0.0;
      part2 = 0.0;
    }
  }
};

// y of one frame from the two window ends' prefixes.
MP3G_FO_HD inline float scmn_value(float x, double Ps, double Pe, double P2s, double P2e, uint32_t len, bool norm_vars) {
  const double mean = (Pe - Ps) / (double)len;
  float y = (float)((double)x - mean);
  if (norm_vars) {
    const double var = (P2e - P2s) / (double)len - mean * mean;
    const float v32 = (float)var;
    const float vf = v32 > 1e-10f ? v32 : 1e-10f;  // fmaxf(v32, 1e-10f), a NaN included
    const float scale = 1.0f / __builtin_sqrtf(vf);
    y = y * scale;
  }
  return y;
}

// The energy VAD's threshold from the column's blocked sum Pn = P[n].
MP3G_FO_HD inline float vad_threshold(float energy_threshold, float energy_mean_scale, double Pn, uint32_t n) {
  return (float)((double)energy_threshold + (double)energy_mean_scale * (Pn / (double)n));
}

// The decision from the window's counts: a float32 product, rounded once.
MP3G_FO_HD inline bool vad_decision(uint32_t num, uint32_t den, float proportion_threshold) {
  const float rhs = (float)den * proportion_threshold;
  return (float)num >= rhs;
}

}  // namespace mp3g
