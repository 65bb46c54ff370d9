// stft_fft.h -- the transform of the STFT features (include/mp3g.h "STFT and mel
// spectrograms of decoded rows"), written once.  The host reference
// (stft_tables.cpp) and the kernel (stft.hip) both compile THESE functions: the
// host walks the butterflies in plain loops, the kernel deals them to lanes, and
// because a butterfly's operands and operations are the same either way, so are
// its bits (every TU is built with -ffp-contract=off: an addition stays an
// addition, a fused multiply-add is one only where it is spelled).
//
// The network.  A frame's P real samples v[0 .. P) are read as N = P / 2 complex
// values z[n] = v[2 n] + i v[2 n + 1].  Z = FFT_N(z) is a decimation-in-frequency
// network in place: radix-4 passes over blocks of len = N, N / 4, .. (>= 4), then
// one radix-2 pass if a block of 2 is left (N = 128, 512, 2048).  A radix-4
// butterfly of the block at `base`, n < q = len / 4, takes x_r = z[base + n + r q]:
//   t0 = x0 + x2, t1 = x0 - x2, t2 = x1 + x3, t3 = -i (x1 - x3)
//   z[base + n]       =  t0 + t2
//   z[base + n + q]   = (t1 + t3) W_len^n
//   z[base + n + 2 q] = (t0 - t2) W_len^2n
//   z[base + n + 3 q] = (t1 - t3) W_len^3n
// with W_len^j = tw[j P / len], tw[k] = exp(-2 pi i k / P) computed in float64 and
// rounded once (k a multiple of P / 4: exactly 1, -i, -1, i).  Z[k] ends at slot
// stft_slot(k): the digits of k (base 4, then the radix-2 bit) reversed.  The
// real transform's bins come from pairs of slots:
//   E = Z[k] + conj(Z[N - k]), O = Z[k] - conj(Z[N - k]), T = tw[k] O
//   X[k]     = ((E.re + T.im) / 2,  (E.im - T.re) / 2)
//   X[N - k] = ((E.re - T.im) / 2, (-E.im - T.re) / 2)        0 < k <= N / 2
//   X[0] = (Z[0].re + Z[0].im, +0), X[N] = (Z[0].re - Z[0].im, +0)
// A complex product (a + i b)(c + i d) is t = b d, re = fmaf(a, c, -t), u = b c,
// im = fmaf(a, d, u); by 1, -i, -1, i it is moves and negations.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/mp3g.h"
#include "fbank_log.h"  // mp3g_logf; through it logmel_log10.h: mp3g_log10f, MP3G_L10_HD

namespace mp3g {

struct StftC {
  float re, im;
};

// (host only) tw[k] = exp(-2 pi i k / P), k < P: float64, rounded once
inline StftC stft_twiddle(uint32_t k, uint32_t P) {
  const uint32_t quarter = P / 4;
  if (k % quarter == 0) {
    const StftC unit[4] = {{1.f, 0.f}, {0.f, -1.f}, {-1.f, 0.f}, {0.f, 1.f}};
    return unit[(k / quarter) & 3];
  }
  const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)P;
  return StftC{(float)std::cos(a), (float)-std::sin(a)};
}

// the slot of Z[k] after the passes (k < N = 2^log2n)
MP3G_L10_HD inline uint32_t stft_slot(uint32_t k, uint32_t log2n) {
  // the low log2n & ~1 bits as base-4 digits, reversed: the bits reversed, then
  // each pair swapped back; an odd log2n leaves k's top bit, which goes last
  const uint32_t even = log2n & ~1u;
  const uint32_t r = __builtin_bitreverse32(k << (32 - even));  // (even >= 6)
  const uint32_t digits = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
  return (log2n & 1u) ? (digits << 1) | (k >> even) : digits;
}

MP3G_L10_HD inline StftC stft_add(StftC a, StftC b) { return StftC{a.re + b.re, a.im + b.im}; }
MP3G_L10_HD inline StftC stft_sub(StftC a, StftC b) { return StftC{a.re - b.re, a.im - b.im}; }

// x tw[idx]
MP3G_L10_HD inline StftC stft_mul_tw(StftC x, const StftC* tw, uint32_t idx, uint32_t P) {
  const uint32_t quarter = P >> 2;
  if ((idx & (quarter - 1)) == 0) {
    switch ((idx / quarter) & 3u) {
      case 0: return x;
      case 1: return StftC{x.im, -x.re};
      case 2: return StftC{-x.re, -x.im};
      default: return StftC{-x.im, x.re};
    }
  }
  const float c = tw[idx].re, d = tw[idx].im;
  const float t = x.im * d;
  const float re = __builtin_fmaf(x.re, c, -t);
  const float u = x.im * c;
  const float im = __builtin_fmaf(x.re, d, u);
  return StftC{re, im};
}

// one radix-4 butterfly; idx = n P / len, the index of W_len^n in tw
MP3G_L10_HD inline void stft_bfly4(StftC* x0, StftC* x1, StftC* x2, StftC* x3, const StftC* tw, uint32_t idx,
                                   uint32_t P) {
  const StftC t0 = stft_add(*x0, *x2), t1 = stft_sub(*x0, *x2), t2 = stft_add(*x1, *x3), d = stft_sub(*x1, *x3);
  const StftC t3 = StftC{d.im, -d.re};
  *x0 = stft_add(t0, t2);
  *x1 = stft_mul_tw(stft_add(t1, t3), tw, idx, P);
  *x2 = stft_mul_tw(stft_sub(t0, t2), tw, 2 * idx, P);
  *x3 = stft_mul_tw(stft_sub(t1, t3), tw, 3 * idx, P);
}

MP3G_L10_HD inline void stft_bfly2(StftC* x0, StftC* x1) {
  const StftC a = *x0, b = *x1;
  *x0 = stft_add(a, b);
  *x1 = stft_sub(a, b);
}

// X[k] and X[N - k] from zk = Z[k] and zn = Z[N - k], 0 < k <= N / 2
MP3G_L10_HD inline void stft_split(StftC zk, StftC zn, const StftC* tw, uint32_t k, uint32_t P, StftC* xk, StftC* xn) {
  const StftC e = StftC{zk.re + zn.re, zk.im - zn.im}, o = StftC{zk.re - zn.re, zk.im + zn.im};
  const StftC t = stft_mul_tw(o, tw, k, P);
  *xk = StftC{(e.re + t.im) * 0.5f, (e.im - t.re) * 0.5f};
  *xn = StftC{(e.re - t.im) * 0.5f, (-e.im - t.re) * 0.5f};
}
// X[0] and X[N] from Z[0]
MP3G_L10_HD inline void stft_split0(StftC z0, StftC* x0, StftC* xn) {
  *x0 = StftC{z0.re + z0.im, 0.f};
  *xn = StftC{z0.re - z0.im, 0.f};
}

// what a bin stores beside the complex value: the power, or the magnitude
MP3G_L10_HD inline float stft_power(StftC x) { return __builtin_fmaf(x.re, x.re, x.im * x.im); }
MP3G_L10_HD inline float stft_scalar(StftC x, uint32_t output) {
  const float p = stft_power(x);
  return output == MP3G_STFT_MAGNITUDE ? __builtin_sqrtf(p) : p;
}
// the logarithm stage
MP3G_L10_HD inline float stft_log(float s, uint32_t log, float floor) {
  if (log == MP3G_STFT_LOG_NONE) return s;
  const float t = s > floor ? s : floor;
  return log == MP3G_STFT_LOG_LN ? mp3g_logf(t) : mp3g_log10f(t);
}

}  // namespace mp3g
