// reverb_fft.h -- the transforms and the spectral product of the reverberation
// (include/mp3g.h "Room reverberation and noise at an SNR"), written once.  The
// host reference (reverb_tables.cpp) and the kernels (reverb.hip) both compile
// THESE functions: the host walks the butterflies in plain loops, the kernels
// deal them to lanes, and because a butterfly's operands and operations are the
// same either way, so are its bits (every TU is built with -ffp-contract=off).
//
// N = 2048 complex points.  The forward transform is stft_fft.h's
// decimation-in-frequency network with P = 4096, tw[k] = exp(-2 pi i k / 4096):
// radix-4 passes over blocks of len = 2048, 512, 128, 32, 8 and one radix-2
// pass; Z[k] ends at slot stft_slot(k, 11).  The spectra are multiplied slot by
// slot, so the bins are never brought into natural order.  The inverse is the
// TRANSPOSED network with conjugated twiddles: it reads slot order and writes
// natural order.  Its passes run the other way round -- the radix-2 pass, then
// radix-4 over len = 8, 32, 128, 512, 2048 -- and a butterfly of the block at
// `base`, n < q = len / 4, takes x_r = z[base + n + r q]:
//   a1 = x1 conj(W_len^n), a2 = x2 conj(W_len^2n), a3 = x3 conj(W_len^3n)
//   t0 = x0 + a2, t1 = x0 - a2, t2 = a1 + a3, t3 = +i (a1 - a3)
//   z[base + n] = t0 + t2, z[.. + q] = t1 + t3, z[.. + 2 q] = t0 - t2, z[.. + 3 q] = t1 - t3
// which is N times the inverse DFT; the caller multiplies by 2^-11 (exact).
#pragma once
#include <cstdint>

#include "stft_fft.h"

namespace mp3g {

constexpr uint32_t kRvN = 2048, kRvLog2N = 11, kRvS = 1024, kRvTw = 4096;
constexpr float kRvInvN = 0x1p-11f;

// x conj(tw[idx]): stft_mul_tw with the twiddle's imaginary part negated (a
// negation is exact); by 1, +i, -1, -i it is moves and negations
MP3G_L10_HD inline StftC rv_mul_twc(StftC x, const StftC* tw, uint32_t idx) {
  constexpr uint32_t quarter = kRvTw >> 2;
  if ((idx & (quarter - 1)) == 0) {
    switch ((idx / quarter) & 3u) {
      case 0: return x;
      case 1: return StftC{-x.im, x.re};
      case 2: return StftC{-x.re, -x.im};
      default: return StftC{x.im, -x.re};
    }
  }
  const float c = tw[idx].re, d = -tw[idx].im;
  const float t = x.im * d;
  const float re = __builtin_fmaf(x.re, c, -t);
  const float u = x.im * c;
  const float im = __builtin_fmaf(x.re, d, u);
  return StftC{re, im};
}

// one butterfly of the inverse network; idx = n 4096 / len
MP3G_L10_HD inline void rv_ibfly4(StftC* x0, StftC* x1, StftC* x2, StftC* x3, const StftC* tw, uint32_t idx) {
  const StftC a1 = rv_mul_twc(*x1, tw, idx), a2 = rv_mul_twc(*x2, tw, 2 * idx), a3 = rv_mul_twc(*x3, tw, 3 * idx);
  const StftC t0 = stft_add(*x0, a2), t1 = stft_sub(*x0, a2), t2 = stft_add(a1, a3), d = stft_sub(a1, a3);
  const StftC t3 = StftC{-d.im, d.re};
  *x0 = stft_add(t0, t2);
  *x1 = stft_add(t1, t3);
  *x2 = stft_sub(t0, t2);
  *x3 = stft_sub(t1, t3);
}

// acc + x g: the product as stft_mul_tw's general case spells it (two
// multiplies, two fmaf), then one float32 addition per part
MP3G_L10_HD inline StftC rv_mac(StftC acc, StftC x, StftC g) {
  const float t = x.im * g.im;
  const float re = __builtin_fmaf(x.re, g.re, -t);
  const float u = x.im * g.re;
  const float im = __builtin_fmaf(x.re, g.im, u);
  return StftC{acc.re + re, acc.im + im};
}

// (host) the forward network in place: natural order in, slot order out
inline void rv_fft_forward(StftC* z, const StftC* tw) {
  uint32_t len = kRvN;
  for (; len >= 4; len >>= 2) {
    const uint32_t q = len >> 2, step = kRvTw / len;
    for (uint32_t base = 0; base < kRvN; base += len)
      for (uint32_t n = 0; n < q; n++)
        stft_bfly4(z + base + n, z + base + n + q, z + base + n + 2 * q, z + base + n + 3 * q, tw, n * step, kRvTw);
  }
  for (uint32_t j = 0; j < kRvN; j += 2) stft_bfly2(z + j, z + j + 1);  // (len == 2 is left at N = 2048)
}

// (host) the inverse network in place: slot order in, natural order out, times N
inline void rv_fft_inverse(StftC* z, const StftC* tw) {
  for (uint32_t j = 0; j < kRvN; j += 2) stft_bfly2(z + j, z + j + 1);
  for (uint32_t len = 8; len <= kRvN; len <<= 2) {
    const uint32_t q = len >> 2, step = kRvTw / len;
    for (uint32_t base = 0; base < kRvN; base += len)
      for (uint32_t n = 0; n < q; n++)
        rv_ibfly4(z + base + n, z + base + n + q, z + base + n + 2 * q, z + base + n + 3 * q, tw, n * step);
  }
}

}  // namespace mp3g
