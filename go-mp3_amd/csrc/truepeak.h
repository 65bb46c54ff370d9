// truepeak.h -- the arithmetic of the true-peak measure that the host reference
// (truepeak_tables.cpp) and the kernel (truepeak.hip) both compile
// (include/mp3g.h "True peak of decoded rows"), and the constants both share.
// The interpolator is libebur128's: 49 taps at factor 4, a Hann-windowed sinc;
// phase 0 is the sample itself, phases 1..3 have 12 taps each
// (truepeak_coefs.inc, tools/gen_truepeak.py).  Everything is float32 with
// explicit fmaf in ONE written-down order; the library is built with
// -ffp-contract=off, so nothing else is fused on either side.
#pragma once
#include <cstdint>

#include "../../include/mp3g.h"
#include "truepeak_coefs.inc"

#if defined(__HIPCC__)
#define MP3G_TP_HD __host__ __device__
#else
#define MP3G_TP_HD
#endif

namespace mp3g {

constexpr uint32_t kTpPhases = 3, kTpTaps = 12, kTpHalo = kTpTaps - 1;
// the kernel: outputs a thread forms, threads of a block, samples of a tile
constexpr uint32_t kTpPer = 16, kTpBlock = 256, kTpTile = kTpPer * kTpBlock;
// the row kernel's block: one wave folds a row's partial maxima
constexpr uint32_t kTpRowBlock = 64;

// tiles a plane of T samples has
inline uint32_t tp_tiles(uint32_t T) { return (uint32_t)(((uint64_t)T + kTpTile - 1) / kTpTile); }

// v > tp ? v : tp -- a NaN never enters, and the maximum is order-free
MP3G_TP_HD inline float tp_max(float tp, float v) { return v > tp ? v : tp; }
// The same for a v that an fmaf produced: tp is never a NaN or -0 and such a v
// is never a signalling NaN, so fmaxf(tp, v) has tp_max's bits for every input
// (one v_max_f32 on the device instead of a compare and a select).
MP3G_TP_HD inline float tp_max_of_fma(float tp, float v) { return __builtin_fmaxf(tp, v); }

// The interpolated values between x[n - 1] and x[n] and the sample itself:
// xn points at x[n] and xn[-t] = x[n - t], t = 0..11, is read (zero before the
// plane's first sample: the caller's).  Returns the largest magnitude folded
// into tp.
MP3G_TP_HD inline float tp_sample(const float* xn, float tp) {
  static constexpr float kTpCoef[kTpPhases][kTpTaps] = {MP3G_TRUE_PEAK_COEFS};
  tp = tp_max(tp, __builtin_fabsf(xn[0]));
  for (uint32_t f = 0; f < kTpPhases; f++) {
    float y = 0.f;
    for (uint32_t t = 0; t < kTpTaps; t++) y = __builtin_fmaf(kTpCoef[f][t], xn[-(int)t], y);
    tp = tp_max_of_fma(tp, __builtin_fabsf(y));
  }
  return tp;
}

// truepeak_tables.cpp: the argument check both forms of the call share; *tiles
// is the tile count of a plane.
int true_peak_check(uint32_t n_rows, uint32_t n_planes, uint32_t T, uint32_t* tiles);

}  // namespace mp3g
