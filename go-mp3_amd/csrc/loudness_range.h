// loudness_range.h -- the arithmetic of the momentary and short-term maxima and
// the loudness range (EBU Tech 3342) that the host reference
// (truepeak_tables.cpp) and the kernel (truepeak.hip) both compile
// (include/mp3g.h "Momentary and short-term maxima, loudness range").  It works
// on the scratch of the loudness measure as loudness_filter.h leaves it: the
// scanned segment energies E_j in the items' first doubles, the momentary block
// energies z_i in the second doubles of plane 0's items.  Everything is float64
// in ONE written-down order, without contraction.
#pragma once
#include <cstdint>

#include "loudness_filter.h"

namespace mp3g {

// segments of a short-term block (3 s); its step is one segment
constexpr uint32_t kRangeWin = 30;
// the range kernel's block: one block per row
constexpr uint32_t kRangeBlock = 256;

MP3G_LOUD_HD inline uint32_t range_short_count(uint32_t nseg) { return nseg >= kRangeWin ? nseg - (kRangeWin - 1) : 0; }

// S_k: the short-term block energy from the planes' scanned items (plane p's at
// items + p * S1 * 9), u ascending within a plane, plane 0 first.
MP3G_LOUD_HD inline double range_short_energy(const double* items, uint32_t n_planes, uint32_t S1, uint32_t k,
                                              uint32_t H) {
  constexpr uint32_t kD = kLoudItemDoubles;
  double s = 0.0;
  for (uint32_t p = 0; p < n_planes; p++) {
    const double* e = items + ((size_t)p * S1 + k) * kD;
    double P = e[0];
    for (uint32_t u = 1; u < kRangeWin; u++) P = P + e[(size_t)u * kD];
    s = p ? s + P : P;
  }
  return s / (double)((uint64_t)kRangeWin * H);
}

// An energy as LUFS, the way the integrated loudness is formed; -inf for none.
MP3G_LOUD_HD inline float range_lufs(double v) {
  if (!(v > 0.0)) return -__builtin_inff();
  const float t = 10.0f * mp3g_log10f((float)v);
  return -0.691f + t;
}

// The relative gate of the range: 0.01 of the mean of the S_k at or above the
// absolute gate (-20 LU), k ascending; 0 when there is none.  (Eight values are
// read ahead of their sums.)
MP3G_LOUD_HD inline double range_rel_gate(const double* S, uint32_t ns, uint32_t* n_abs_out) {
  constexpr uint32_t kGroup = 8;
  double sum_abs = 0.0;
  uint32_t n_abs = 0;
  for (uint32_t k0 = 0; k0 < ns; k0 += kGroup) {
    double v[kGroup];
    for (uint32_t u = 0; u < kGroup; u++) v[u] = k0 + u < ns ? S[k0 + u] : 0.0;
    for (uint32_t u = 0; u < kGroup; u++)
      if (v[u] >= kLoudAbsGate) {  // (a padding 0 is below the gate)
        sum_abs += v[u];
        n_abs++;
      }
  }
  *n_abs_out = n_abs;
  return n_abs ? 0.01 * (sum_abs / (double)n_abs) : 0.0;
}

MP3G_LOUD_HD inline bool range_gated(double s, double rel) { return s >= kLoudAbsGate && s >= rel; }

// nearest ranks of the 10th and the 95th percentile among n gated values (n >= 1)
MP3G_LOUD_HD inline uint32_t range_rank_lo(uint32_t n) { return (uint32_t)(((uint64_t)(n - 1) * 10 + 50) / 100); }
MP3G_LOUD_HD inline uint32_t range_rank_hi(uint32_t n) { return (uint32_t)(((uint64_t)(n - 1) * 95 + 50) / 100); }

// Selection by counting.  A gated value is a positive double, so values order as
// their bit patterns do.  The value of rank r (0-based, ascending) is the
// largest pattern t with #{gated x : bits(x) < t} <= r; t is built from its top
// bit down, one count per bit (63 counts, whatever the ties).  range_trial gives
// the pattern a step tries, range_keep whether the step keeps it.
MP3G_LOUD_HD inline uint64_t range_trial(uint64_t prefix, uint32_t bit) { return prefix | (1ull << bit); }
MP3G_LOUD_HD inline bool range_below(double s, double rel, uint64_t trial) {
  return range_gated(s, rel) && __builtin_bit_cast(uint64_t, s) < trial;
}
MP3G_LOUD_HD inline double range_select(const double* S, uint32_t ns, double rel, uint32_t rank) {
  uint64_t prefix = 0;
  for (uint32_t b = 63; b-- > 0;) {
    const uint64_t trial = range_trial(prefix, b);
    uint32_t below = 0;
    for (uint32_t k = 0; k < ns; k++) below += range_below(S[k], rel, trial) ? 1u : 0u;
    if (below <= rank) prefix = trial;
  }
  return __builtin_bit_cast(double, prefix);
}

// The record from the maxima, the counts and the two selected energies.
MP3G_LOUD_HD inline void range_record(double M, double Smax, uint32_t n_short, uint32_t n_range, double vlo, double vhi,
                                      mp3g_loudness_range* out) {
  out->momentary_max = range_lufs(M);
  out->shortterm_max = range_lufs(Smax);
  if (n_range) {
    out->range_lo = range_lufs(vlo);
    out->range_hi = range_lufs(vhi);
    out->lra = out->range_hi - out->range_lo;
  } else {
    out->range_lo = out->range_hi = -__builtin_inff();
    out->lra = 0.f;
  }
  out->n_short = n_short;
  out->n_range = n_range;
  out->zero = 0;
}

}  // namespace mp3g
