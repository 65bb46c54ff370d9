// fbank_log.h -- mp3g_logf, the Kaldi filter-bank features' natural logarithm
// (include/mp3g.h "Kaldi filter-bank features of decoded rows").  The host
// reference (fbank_tables.cpp) and the kernel (fbank.hip) both compile THIS
// function: integer operations and explicit fused multiply-adds only (an
// addition is fmaf(a, 1, b): the l10_* helpers of logmel_log10.h), no libm and
// no device intrinsic, so both give the same bits.
//
// The construction is mp3g_log10f's.  x = 2^e m with m in [sqrt(1/2), sqrt(2)),
// split off by bit operations.  Entry i = the top 6 bits of m's offset in that
// interval gives inv_i ~ 1 / m and -ln(inv_i) as a hi/lo pair; r = m inv_i - 1
// is formed exactly as rh + rl (|r| < 2^-6.9) and
//   ln x = e ln(2) - ln(inv_i) + r - r^2 / 2 + r^3 (c3 + .. + c6 r^3)
// is summed in hi/lo float32 pairs: ln(2) in three parts (e times the first is
// exact), r itself and -r^2 / 2 as exact pairs (the coefficients 1 and -1/2 need
// no rounding, which is what the natural logarithm saves over log10), the high
// parts through error-free two-sums in ascending magnitude, the low parts in
// plain float32.  The result is the float32 nearest to a sum that is within
// about 2^-44 of ln x (DESIGN.md 9e has the measured figures).
// Domain: normal positive finite x; the features only call it with x >= 2^-23.
#pragma once
#include <cstdint>

#include "fbank_log_consts.inc"
#include "logmel_log10.h"

namespace mp3g {

MP3G_L10_HD inline float mp3g_logf(float x) {
  static constexpr float kTab[64][3] = {MP3G_LN_TABLE};
  constexpr uint32_t kLo = 0x3f3504f3u;  // sqrt(1/2)
  const uint32_t ix = __builtin_bit_cast(uint32_t, x) + (0x3f800000u - kLo);
  const float fe = (float)((int32_t)(ix >> 23) - 127);
  const uint32_t off = ix & 0x007fffffu;
  const float m = __builtin_bit_cast(float, off + kLo);
  const float inv = kTab[off >> 17][0], th = kTab[off >> 17][1], tl = kTab[off >> 17][2];
  // r = m inv - 1 = rh + rl exactly: the product as a pair, ph - 1 exact (Sterbenz)
  const float ph = l10_fma(m, inv, 0.0f);
  const float rl = l10_fma(m, inv, -ph);
  const float rh = l10_sub(ph, 1.0f);
  // s = r^2, w = -s / 2 (exact halving)
  const float sh = l10_fma(rh, rh, 0.0f);
  float sl = l10_fma(rh, rh, -sh);
  sl = l10_fma(l10_add(rh, rh), rl, sl);
  const float wh = l10_fma(-0.5f, sh, 0.0f);
  const float wl = l10_fma(-0.5f, sl, 0.0f);
  // rl, and its share of the cubic term (3 c3 rh^2 rl = rh^2 rl: 2^-39, the last that matters)
  const float ul = l10_fma(sh, rl, rl);
  // q = r^3 (c3 + c4 r + c5 r^2 + c6 r^3)
  float q = l10_fma(MP3G_LN_C6, rh, MP3G_LN_C5);
  q = l10_fma(q, rh, MP3G_LN_C4);
  q = l10_fma(q, rh, MP3G_LN_C3);
  q = l10_fma(q, l10_fma(sh, rh, 0.0f), 0.0f);
  // v = e ln(2): a exact, the rest a pair
  const float a = l10_fma(fe, MP3G_LN_L2A, 0.0f);
  const float vh = l10_fma(fe, MP3G_LN_L2B, 0.0f);
  float vl = l10_fma(fe, MP3G_LN_L2B, -vh);
  vl = l10_fma(fe, MP3G_LN_L2C, vl);
  // the low parts, then the high parts' two-sum errors, smallest first
  float lo = l10_add(l10_add(l10_add(l10_add(vl, wl), ul), tl), q);
  float e1, e2, e3, e4;
  float s = l10_two_sum(wh, vh, &e1);
  s = l10_two_sum(s, rh, &e2);
  s = l10_two_sum(s, th, &e3);
  s = l10_two_sum(s, a, &e4);
  lo = l10_add(l10_add(l10_add(l10_add(lo, e1), e2), e3), e4);
  return l10_add(s, lo);
}

// The features' floor and logarithm: Kaldi floors the mel energy at float32 epsilon.
constexpr float kFbankFloor = 0x1p-23f;
MP3G_L10_HD inline float fbank_log(float mel) { return mp3g_logf(mel > kFbankFloor ? mel : kFbankFloor); }

}  // namespace mp3g
