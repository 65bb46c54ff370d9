// loudness_filter.h -- the arithmetic of the BS.1770 loudness measure that the
// host reference (loudness_tables.cpp) and the kernels (loudness.hip) both
// compile (include/mp3g.h "Integrated loudness of decoded rows"): the K-weighting
// step, a segment's energy under a carried-in state, the state's advance over a
// segment, and a row's blocks, gates and record.  Everything is float64 in ONE
// written-down order; the library is built with -ffp-contract=off, so no
// product is fused into a sum on either side and both give the same bits.
#pragma once
#include <cstdint>

#include "../../include/mp3g.h"
#include "logmel_log10.h"

#if defined(__HIPCC__)
#define MP3G_LOUD_HD __host__ __device__
#else
#define MP3G_LOUD_HD
#endif

namespace mp3g {

// The two biquads of the K-weighting, a0 = 1: the shelf b0 b1 b2 a1 a2, then
// the high-pass a1 a2 (its numerator is 1 -2 1, not normalised).
struct LoudCoef {
  double b0, b1, b2, a1, a2, ha1, ha2;
};

// doubles a segment leaves in the scratch: Ezs, g[4], send[4]
constexpr uint32_t kLoudItemDoubles = 9;
// -70 LUFS as an energy: the double nearest 10^(-6.9309)
constexpr double kLoudAbsGate = MP3G_LOUDNESS_ABS_GATE;

// One sample through both sections, transposed direct form II; s[0..1] the
// shelf's state, s[2..3] the high-pass's.  Returns the K-weighted sample.
MP3G_LOUD_HD inline double loud_step(const LoudCoef& c, double* s, double x) {
  const double y = c.b0 * x + s[0];
  s[0] = (c.b1 * x - c.a1 * y) + s[1];
  s[1] = c.b2 * x - c.a2 * y;
  const double w = y + s[2];
  s[2] = (-2.0 * y - c.ha1 * w) + s[3];
  s[3] = y - c.ha2 * w;
  return w;
}

// The energy of a segment whose filter started from state s0, from what the
// segment left when run from zero state (it[0] = Ezs, it[1..4] = g) and
// G = sum V^T V:  Ezs + 2 g.s0 + s0^T G s0, floored at 0.
MP3G_LOUD_HD inline double loud_segment_energy(const double* it, const double* G, const double* s0) {
  const double gs = ((it[1] * s0[0] + it[2] * s0[1]) + it[3] * s0[2]) + it[4] * s0[3];
  double q = 0.0;
  for (uint32_t a = 0; a < 4; a++) {
    const double* Ga = G + 4 * a;
    const double t = ((Ga[0] * s0[0] + Ga[1] * s0[1]) + Ga[2] * s0[2]) + Ga[3] * s0[3];
    q = a ? q + s0[a] * t : s0[a] * t;
  }
  const double e = (it[0] + 2.0 * gs) + q;
  return e > 0.0 ? e : 0.0;
}

// s0 = AH s0 + send (it[5..8]): the state at the end of the segment.
MP3G_LOUD_HD inline void loud_advance(const double* it, const double* AH, double* s0) {
  double t[4];
  for (uint32_t m = 0; m < 4; m++) {
    const double* Am = AH + 4 * m;
    t[m] = ((((Am[0] * s0[0] + Am[1] * s0[1]) + Am[2] * s0[2]) + Am[3] * s0[3])) + it[5 + m];
  }
  for (uint32_t m = 0; m < 4; m++) s0[m] = t[m];
}

// The scan of one plane: its items' first doubles become the energies E_j.
// Items are read four ahead of the one being scanned, so that the recurrence
// does not wait for memory at every step (the arithmetic is per item, in order).
MP3G_LOUD_HD inline void loud_scan_plane(double* items, uint32_t nseg, const double* G, const double* AH) {
  constexpr uint32_t kAhead = 4, kD = kLoudItemDoubles;
  double s0[4] = {0.0, 0.0, 0.0, 0.0};
  double cur[kAhead][kD], nxt[kAhead][kD];
  for (uint32_t u = 0; u < kAhead; u++)
    for (uint32_t d = 0; d < kD; d++) cur[u][d] = u < nseg ? items[(size_t)u * kD + d] : 0.0;
  for (uint32_t j0 = 0; j0 < nseg; j0 += kAhead) {
    for (uint32_t u = 0; u < kAhead; u++)
      for (uint32_t d = 0; d < kD; d++)
        nxt[u][d] = j0 + kAhead + u < nseg ? items[(size_t)(j0 + kAhead + u) * kD + d] : 0.0;
    for (uint32_t u = 0; u < kAhead; u++) {
      if (j0 + u < nseg) {
        items[(size_t)(j0 + u) * kD] = loud_segment_energy(cur[u], G, s0);
        loud_advance(cur[u], AH, s0);
      }
      for (uint32_t d = 0; d < kD; d++) cur[u][d] = nxt[u][d];
    }
  }
}

// A row's blocks, gates and record from its planes' scanned items (plane p's at
// items + p * S1 * 9; the second double of plane 0's item i is overwritten with
// z_i) and the items' peaks (peaks + p * S1, entries 0 .. nseg).
MP3G_LOUD_HD inline void loud_row_record(double* items, const float* peaks, uint32_t n_planes, uint32_t S1,
                                         uint32_t nseg, uint32_t H, mp3g_loudness_stats* out) {
  const uint32_t nb = nseg >= 4 ? nseg - 3 : 0;
  const double den = (double)(4ull * H);
  double sum_abs = 0.0;
  uint32_t n_abs = 0;
  // (eight blocks' energies are read before the first of their z is stored, so
  // that the loop does not wait for memory at every block; the sums are per block)
  constexpr uint32_t kGroup = 8, kD = kLoudItemDoubles;
  double win[2][3 + kGroup];
  for (uint32_t p = 0; p < 2; p++)
    for (uint32_t u = 0; u < 3; u++) win[p][u] = (p < n_planes && nb) ? items[((size_t)p * S1 + u) * kD] : 0.0;
  for (uint32_t i0 = 0; i0 < nb; i0 += kGroup) {
    for (uint32_t p = 0; p < 2; p++)
      for (uint32_t u = 0; u < kGroup; u++)
        win[p][3 + u] = (p < n_planes && i0 + u < nb) ? items[((size_t)p * S1 + i0 + u + 3) * kD] : 0.0;
    for (uint32_t u = 0; u < kGroup; u++) {
      if (i0 + u >= nb) break;
      double z = ((win[0][u] + win[0][u + 1]) + win[0][u + 2]) + win[0][u + 3];
      if (n_planes == 2) z = z + (((win[1][u] + win[1][u + 1]) + win[1][u + 2]) + win[1][u + 3]);
      z = z / den;
      items[(size_t)(i0 + u) * kD + 1] = z;
      if (z >= kLoudAbsGate) {
        sum_abs += z;
        n_abs++;
      }
    }
    for (uint32_t p = 0; p < 2; p++)
      for (uint32_t u = 0; u < 3; u++) win[p][u] = win[p][kGroup + u];
  }
  double sum = 0.0;
  uint32_t n_gated = 0;
  if (n_abs) {
    const double rel = 0.1 * (sum_abs / (double)n_abs);
    for (uint32_t i0 = 0; i0 < nb; i0 += kGroup) {
      double zs[kGroup];
      for (uint32_t u = 0; u < kGroup; u++) zs[u] = i0 + u < nb ? items[(size_t)(i0 + u) * kD + 1] : 0.0;
      for (uint32_t u = 0; u < kGroup; u++) {
        const double z = zs[u];  // (a padding 0 is below the absolute gate)
        if (z >= kLoudAbsGate && z >= rel) {
          sum += z;
          n_gated++;
        }
      }
    }
  }
  float peak = 0.f;
  for (uint32_t p = 0; p < n_planes; p++)
    for (uint32_t j0 = 0; j0 <= nseg; j0 += kGroup) {
      float v[kGroup];
      for (uint32_t u = 0; u < kGroup; u++) v[u] = j0 + u <= nseg ? peaks[(size_t)p * S1 + j0 + u] : 0.f;
      for (uint32_t u = 0; u < kGroup; u++) peak = v[u] > peak ? v[u] : peak;
    }
  const double energy = n_gated ? sum / (double)n_gated : 0.0;
  float lufs = -__builtin_inff();
  if (n_gated) {
    const float t = 10.0f * mp3g_log10f((float)energy);
    lufs = -0.691f + t;
  }
  out->energy = energy;
  out->lufs = lufs;
  out->peak = peak;
  out->n_blocks = nb;
  out->n_abs = n_abs;
  out->n_gated = n_gated;
  out->zero = 0;
}

// The gain of a row (include/mp3g.h "The gain stage").
MP3G_LOUD_HD inline float loud_gain(double energy, float peak, double target_energy, float peak_ceiling) {
  if (!(energy > 0.0)) return 1.0f;
  float g = (float)__builtin_sqrt(target_energy / energy);
  if (peak_ceiling > 0.f && peak > 0.f) {
    const float c = peak_ceiling / peak;
    g = c < g ? c : g;
  }
  return g;
}

}  // namespace mp3g
