// logmel_log10.h -- mp3g_log10f, the log-mel features' base-10 logarithm
// (include/mp3g.h "log-mel features of decoded rows").  The host reference
// (logmel_tables.cpp) and the kernel (logmel.hip) both compile THIS function:
// integer operations and explicit fused multiply-adds only (an addition is
// fmaf(a, 1, b)), no libm and no device intrinsic, so both give the same bits.
//
// x = 2^e m with m in [sqrt(1/2), sqrt(2)), split off by bit operations.  Entry
// i = the top 6 bits of m's offset in that interval gives inv_i ~ 1 / m and
// -log10(inv_i) as a hi/lo pair; r = m inv_i - 1 is formed exactly as rh + rl
// (|r| < 2^-6.9) and
//   log10 x = e log10(2) - log10(inv_i) + c1 r + c2 r^2 + r^3 (c3 + .. + c6 r^3)
// is summed in hi/lo float32 pairs: log10(2) in three parts (e times the first
// is exact), c1 and c2 as pairs, the high parts through error-free two-sums in
// ascending magnitude, the low parts in plain float32 (each below 2^-20, so a
// rounding of at most 2^-45).  The result is the float32 nearest to a sum that
// is within about 2^-45 of log10 x: |error| <= half an ulp of the result +
// 2^-45, which is below 2^-20 for |log10 x| < 16 and rounds one float32 of
// [1e16, 2^60) the other way (DESIGN.md 9d has the exhaustive figures).
// Domain: normal positive finite x; the features only call it with x >= 1e-10.
#pragma once
#include <cstdint>

#include "logmel_log10_consts.inc"

#if defined(__HIPCC__)
#define MP3G_L10_HD __host__ __device__
#else
#define MP3G_L10_HD
#endif

namespace mp3g {

MP3G_L10_HD inline float l10_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
MP3G_L10_HD inline float l10_add(float a, float b) { return __builtin_fmaf(a, 1.0f, b); }
MP3G_L10_HD inline float l10_sub(float a, float b) { return __builtin_fmaf(b, -1.0f, a); }
// s = fl(a + b) and *e = a + b - s exactly (Knuth's two-sum)
MP3G_L10_HD inline float l10_two_sum(float a, float b, float* e) {
  const float s = l10_add(a, b);
  const float bb = l10_sub(s, a);
  *e = l10_add(l10_sub(a, l10_sub(s, bb)), l10_sub(b, bb));
  return s;
}

MP3G_L10_HD inline float mp3g_log10f(float x) {
  static constexpr float kTab[64][3] = {MP3G_L10_TABLE};
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
  // u = c1 r
  const float uh = l10_fma(MP3G_L10_C1H, rh, 0.0f);
  float ul = l10_fma(MP3G_L10_C1H, rh, -uh);
  ul = l10_fma(MP3G_L10_C1L, rh, ul);
  ul = l10_fma(MP3G_L10_C1H, rl, ul);
  // s = r^2, w = c2 s
  const float sh = l10_fma(rh, rh, 0.0f);
  float sl = l10_fma(rh, rh, -sh);
  sl = l10_fma(l10_add(rh, rh), rl, sl);
  const float wh = l10_fma(MP3G_L10_C2H, sh, 0.0f);
  float wl = l10_fma(MP3G_L10_C2H, sh, -wh);
  wl = l10_fma(MP3G_L10_C2H, sl, wl);
  wl = l10_fma(MP3G_L10_C2L, sh, wl);
  // (rl's share of the cubic term, 3 c3 rh^2 rl with 3 c3 = c1: 2^-40, the last that matters)
  ul = l10_fma(l10_fma(MP3G_L10_C1H, sh, 0.0f), rl, ul);
  // q = r^3 (c3 + c4 r + c5 r^2 + c6 r^3)
  float q = l10_fma(MP3G_L10_C6, rh, MP3G_L10_C5);
  q = l10_fma(q, rh, MP3G_L10_C4);
  q = l10_fma(q, rh, MP3G_L10_C3);
  q = l10_fma(q, l10_fma(sh, rh, 0.0f), 0.0f);
  // v = e log10(2): a exact, the rest a pair
  const float a = l10_fma(fe, MP3G_L10_L2A, 0.0f);
  const float vh = l10_fma(fe, MP3G_L10_L2B, 0.0f);
  float vl = l10_fma(fe, MP3G_L10_L2B, -vh);
  vl = l10_fma(fe, MP3G_L10_L2C, vl);
  // the low parts, then the high parts' two-sum errors, smallest first
  float lo = l10_add(l10_add(l10_add(l10_add(vl, wl), ul), tl), q);
  float e1, e2, e3, e4;
  float s = l10_two_sum(wh, vh, &e1);
  s = l10_two_sum(s, uh, &e2);
  s = l10_two_sum(s, th, &e3);
  s = l10_two_sum(s, a, &e4);
  lo = l10_add(l10_add(l10_add(l10_add(lo, e1), e2), e3), e4);
  return l10_add(s, lo);
}

// The features' floor and logarithm, and Whisper's clamp: shared statements.
constexpr float kLogmelFloor = 1e-10f;
MP3G_L10_HD inline float logmel_log(float mel) { return mp3g_log10f(mel > kLogmelFloor ? mel : kLogmelFloor); }
MP3G_L10_HD inline float logmel_clamp(float y, float mx) {
  const float t = mx - 8.0f;
  return ((y > t ? y : t) + 4.0f) * 0.25f;
}

}  // namespace mp3g
