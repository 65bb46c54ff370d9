// varresample.h -- the variable-ratio resampler (include/mp3g.h "variable-ratio
// resampling of decoded rows"): its object, and the per-output arithmetic that
// the host reference (varresample_tables.cpp) and the kernel (varresample.hip)
// both compile -- the divmods, the interpolation fractions, the weight, the
// chain and the final scale.  Integer arithmetic is exact on both sides, the
// two float64 divisions are correctly rounded on both sides, every float32
// operation is written down in ONE order with explicit fused multiply-adds
// (the library is built with -ffp-contract=off), so both give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"

#if defined(__HIPCC__)
#define MP3G_VR_HD __host__ __device__
#else
#define MP3G_VR_HD
#endif

struct mp3g_varresampler {
  int device = -1;
  uint32_t zeros = 0, P = 0, Z = 0, R = 0;
  std::vector<float> table;   // [Z + 1][2]: (F[i], D[i])
  float* d_table = nullptr;   // device: the same pairs
  bool table_lds = false;     // the device call keeps the table in LDS
};

namespace mp3g {

// How the device call tiles a row (varresample.hip): a workgroup makes
// kVarTile consecutive outputs of one row, both planes; a tile's source span
// is staged in LDS when a plane's share of kVarStageFloats holds it.  A table
// of at most kVarTableLdsPairs (F, D) pairs can live in LDS beside the stage.
constexpr uint32_t kVarTile = 512;
constexpr uint32_t kVarStageFloats = 4096;      // 16 KB
constexpr uint32_t kVarTableLdsPairs = 8192;    // 64 KB: zeros = 16 at P = 9
constexpr int64_t kVarFar = (int64_t)1 << 44;   // |q - src_origin| beyond any tap

// (q, r) = divmod(n num, den) without forming n num -- resample.h's
// resample_divmod, for both sides: exact for every n with n num / den < 2^64.
MP3G_VR_HD inline void var_divmod(uint64_t n, uint32_t num, uint32_t den, uint64_t* q, uint32_t* r) {
  const uint64_t t = (n % den) * num;
  *q = (n / den) * num + t / den;
  *r = (uint32_t)(t % den);
}

// The row's cutoff index step I: R for num <= den, else floor(R den / num).
MP3G_VR_HD inline uint32_t var_step(uint32_t R, uint32_t num, uint32_t den) {
  return num <= den ? R : (uint32_t)(((uint64_t)R * den) / num);
}

// What one output needs besides the table: its integer source position q, the
// two wings' first table indices and tap counts, and their fractions.
struct VarTaps {
  uint64_t q;
  uint32_t oL, oR, nL, nR;
  float etaL, etaR;
};

// (o, eta) of a wing: (o, rem) = divmod(I a, den), eta = (float)((double)rem /
// (double)den).  a <= den < 2^31 and I <= 2^9, so the product is formed in 32
// bits when den allows and in 64 otherwise -- the same integers either way.
MP3G_VR_HD inline void var_wing(uint32_t I, uint32_t a, uint32_t den, uint32_t* o, float* eta) {
  uint32_t rem;
  if (den <= (1u << 22)) {
    const uint32_t p = I * a;
    *o = p / den;
    rem = p - *o * den;
  } else {
    const uint64_t p = (uint64_t)I * a;
    const uint64_t d = p / den;
    *o = (uint32_t)d;
    rem = (uint32_t)(p - d * den);
  }
  *eta = (float)((double)rem / (double)den);
}

// Output whose position is (q, r) = divmod(n num, den), 0 <= r < den; I >= 1.
MP3G_VR_HD inline VarTaps var_taps(uint64_t q, uint32_t r, uint32_t den, uint32_t I, uint32_t Z) {
  VarTaps t;
  t.q = q;
  var_wing(I, r, den, &t.oL, &t.etaL);
  var_wing(I, den - r, den, &t.oR, &t.etaR);
  // a tap exists while its index o + I k is < Z  (oL < I <= Z, oR <= I <= Z)
  t.nL = (Z - t.oL + I - 1) / I;
  t.nR = (Z - t.oR + I - 1) / I;
  return t;
}

// q - src_origin as a signed distance, held within +-kVarFar: farther than any
// tap reaches either way, so the clamp changes no result.
MP3G_VR_HD inline int64_t var_rel(uint64_t q, uint64_t src_origin) {
  const int64_t d = (int64_t)(q - src_origin);
  return d > kVarFar ? kVarFar : (d < -kVarFar ? -kVarFar : d);
}

MP3G_VR_HD inline float var_weight(const float* __restrict__ tab, uint32_t i, float eta) {
  return fmaf(eta, tab[2 * i + 1], tab[2 * i]);
}

// n taps of one wing in ascending j: table indices i, i + step, ... (step = -I
// on the left wing, in wrapping unsigned arithmetic), samples p, p + 1, ...
// Four taps' loads are issued before their FMAs, which keep their order: the
// same bits as one tap at a time, with the loads' latency paid once in four.
template <int C, class Src>
MP3G_VR_HD inline void var_run(const float* __restrict__ tab, uint32_t i, uint32_t step, float eta, int64_t p,
                               int32_t n, Src x, float* acc) {
  for (; n >= 4; n -= 4) {
    float f[4], dd[4], xv[4][C];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t iu = i + (uint32_t)u * step;
      f[u] = tab[2 * iu];
      dd[u] = tab[2 * iu + 1];
      for (int c = 0; c < C; c++) xv[u][c] = x(c, p + u);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const float w = fmaf(eta, dd[u], f[u]);
      for (int c = 0; c < C; c++) acc[c] = fmaf(w, xv[u][c], acc[c]);
    }
    i += 4u * step;
    p += 4;
  }
  for (; n > 0; n--) {
    const float w = var_weight(tab, i, eta);
    for (int c = 0; c < C; c++) acc[c] = fmaf(w, x(c, p), acc[c]);
    i += step;
    p++;
  }
}

// The chain: acc[c] = +0, then acc[c] = fmaf(w, x_c[j], acc[c]) over the
// existing taps in ascending j -- the left wing (j = q - k) from its farthest
// tap inwards, then the right wing (j = q + 1 + k) outwards.  d = var_rel(q,
// src_origin); x(c, p) is the sample of plane c at p = j - src_origin, asked
// only for 0 <= p < n (taps elsewhere are skipped).  One weight feeds all
// C chains.
template <int C, class Src>
MP3G_VR_HD inline void var_chain(const float* __restrict__ tab, const VarTaps& t, uint32_t I, int64_t d,
                                 int64_t n, Src x, float* acc) {
  for (int c = 0; c < C; c++) acc[c] = 0.f;
  {
    // 0 <= d - k < n
    const int64_t hi = d < (int64_t)t.nL - 1 ? d : (int64_t)t.nL - 1;
    const int64_t lo = d - n + 1 > 0 ? d - n + 1 : 0;
    if (hi >= lo) var_run<C>(tab, t.oL + I * (uint32_t)hi, 0u - I, t.etaL, d - hi, (int32_t)(hi - lo) + 1, x, acc);
  }
  {
    // 0 <= d + 1 + k < n
    const int64_t lo = -d - 1 > 0 ? -d - 1 : 0;
    const int64_t hi = n - d - 1 < (int64_t)t.nR ? n - d - 1 : (int64_t)t.nR;  // exclusive
    if (hi > lo) var_run<C>(tab, t.oR + I * (uint32_t)lo, I, t.etaR, d + 1 + lo, (int32_t)(hi - lo), x, acc);
  }
}

// y = (c acc) gain, c = I / 2^P (exact in float32): two multiplications.
MP3G_VR_HD inline float var_cutoff(uint32_t I, uint32_t P) { return (float)I / (float)(1u << P); }
MP3G_VR_HD inline float var_scale(float c, float acc, float gain) { return (c * acc) * gain; }

// varresample.hip: the table uploaded to r->device (synchronous), and its
// release.  Return an mp3g_status.
int varresample_device_upload(mp3g_varresampler* r);
void varresample_device_free(mp3g_varresampler* r);

}  // namespace mp3g
