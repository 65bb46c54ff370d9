// reverb.h -- the reverberation object and the arithmetic of the augmentation
// that the host reference (reverb_tables.cpp) and the kernels (reverb.hip) both
// compile (include/mp3g.h "Room reverberation and noise at an SNR"; the
// transforms are reverb_fft.h's).  Every power is a float64 sum of exact
// products in ONE order -- blocks of 1,024 samples, each ascending from +0.0,
// then the block sums ascending from +0.0 -- and the divide and the square root
// are IEEE on both sides, so the records are the host's bit for bit.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"
#include "reverb_fft.h"

namespace mp3g {

constexpr uint32_t kRvMaxTaps = 65536, kRvMaxSlots = 8;
// the kernels: a transform is one workgroup of kRvFftLanes (16 values to a lane);
// the mixing and scaling kernels take kRvTileBlocks blocks of 1,024 samples
constexpr uint32_t kRvFftLanes = 128, kRvTileBlocks = 4, kRvTile = kRvTileBlocks * kRvS, kRvMixLanes = 256;
// a working set in LDS: value i at float2 slot i + (i >> 5), as the STFT's
MP3G_L10_HD inline uint32_t rv_skew(uint32_t i) { return i + (i >> 5); }
constexpr uint32_t kRvSlots = kRvN + (kRvN >> 5);

struct RvRir {
  uint32_t L, peak, es, ee, P, zero;
  uint64_t goff;  // of G_0 in the bank's spectra, in complex values
};

// blocks of 1,024 that n samples have
MP3G_L10_HD inline uint32_t rv_blocks(uint32_t n) { return (n + kRvS - 1) / kRvS; }
// the output blocks of the full timeline that a row of n samples needs with the
// response r: [k0, k1] covers [es, n + ee - 1), n >= 1 (ee > peak >= es: the object
// refuses rates below 20 Hz, so ee >= 1 and the kept samples [peak, peak + n) lie inside)
MP3G_L10_HD inline uint32_t rv_k0(const RvRir& r) { return r.es / kRvS; }
MP3G_L10_HD inline uint32_t rv_k1(const RvRir& r, uint32_t n) { return (n + r.ee - 2) / kRvS; }

// the sum of squares of v[0 .. cnt), ascending from +0.0
MP3G_L10_HD inline double rv_sumsq(const float* v, uint32_t cnt) {
  double s = 0.0;
  for (uint32_t j = 0; j < cnt; j++) {
    const double a = (double)v[j];
    s += a * a;
  }
  return s;
}
// block sums ascending from +0.0
MP3G_L10_HD inline double rv_sum(const double* part, uint32_t cnt) {
  double s = 0.0;
  for (uint32_t j = 0; j < cnt; j++) s += part[j];
  return s;
}
MP3G_L10_HD inline double rv_mean(double sum, uint64_t count) { return count ? sum / (double)count : 0.0; }
MP3G_L10_HD inline float rv_gain(double snr_ratio, double signal_power, double noise_power) {
  return (float)__builtin_sqrt(snr_ratio * signal_power / noise_power);
}
MP3G_L10_HD inline double rv_scale(double power_before, double power_after, uint32_t n) {
  return (n == 0 || power_after == 0.0) ? 1.0 : __builtin_sqrt(power_before / power_after);
}

// One sample of the mix: v = fmaf(g_a, noise, v) over the slots in ascending
// order.  g[a] is the slot's gain; live[a] whether it takes part at all.
struct RvMix {
  const float* noise[kRvMaxSlots];  // the slot's noise row
  uint32_t len[kRvMaxSlots], start[kRvMaxSlots], offset[kRvMaxSlots], wrap[kRvMaxSlots];
  float g[kRvMaxSlots];
  bool live[kRvMaxSlots];
};
MP3G_L10_HD inline float rv_mix_sample(const RvMix& m, uint32_t A, uint32_t j, float v) {
  for (uint32_t a = 0; a < A; a++) {
    if (!m.live[a] || j < m.start[a]) continue;
    const uint32_t d = j - m.start[a];  // (offset < len < 2^31, d < 2^31)
    uint32_t at = m.offset[a] + d;
    if (m.wrap[a])
      at %= m.len[a];
    else if (at >= m.len[a])
      continue;
    v = __builtin_fmaf(m.g[a], m.noise[a][at], v);
  }
  return v;
}

// the scratch of one augment call: doubles first, then the spectra
struct RvLayout {
  uint32_t TB, KB, MB;  // per plane: blocks of x and of v; output blocks; input spectra
  uint64_t pb, pv, pe;  // offsets in doubles: the partial sums of x^2, v^2 and y_e^2
  uint64_t spectra;     // offset in bytes
  uint64_t bytes;
};
inline RvLayout rv_layout(uint32_t Lmax, uint64_t planes, uint32_t T) {
  RvLayout l = {};
  l.TB = rv_blocks(T);
  l.KB = Lmax && T ? (uint32_t)(((uint64_t)T + Lmax - 2) / kRvS) + 1 : 0;
  l.MB = Lmax && T ? l.TB + 1 : 0;
  l.pb = 0;
  l.pv = planes * l.TB;
  l.pe = l.pv + planes * l.TB;
  l.spectra = (l.pe + planes * l.KB) * sizeof(double);
  l.bytes = l.spectra + planes * l.MB * kRvN * sizeof(StftC);
  return l;
}

}  // namespace mp3g

struct mp3g_reverb {
  int device = -1;
  uint32_t rate = 0, R = 0, Lmax = 0;
  std::vector<mp3g::RvRir> rirs;
  std::vector<mp3g::StftC> tw;  // [4096]
  std::vector<mp3g::StftC> G;   // per response P partitions of 2,048 slots
  // device (reverb.hip)
  mp3g::RvRir* d_rirs = nullptr;
  mp3g::StftC* d_tw = nullptr;
  mp3g::StftC* d_G = nullptr;
};

namespace mp3g {

// reverb_tables.cpp: the checks both forms of the calls share.  *work: whether
// anything is to be done.
int augment_shape_check(const mp3g_reverb* rv, uint32_t n_rows, uint32_t n_planes, uint32_t T);
int augment_check(const mp3g_reverb* rv, const mp3g_augment_args* a, bool* work);
// what the rows refer to, from the host copies of rir_index, the noise lengths and the slots
int augment_check_refs(const mp3g_reverb* rv, const mp3g_augment_args* a, const int32_t* rir_index,
                       const uint32_t* noise_lengths, const mp3g_augment_slot* slots);
int row_power_check(uint32_t n_rows, uint32_t T);
// reverb.hip: the tables uploaded to rv->device (synchronous), and their release
int reverb_device_upload(mp3g_reverb* rv);
void reverb_device_free(mp3g_reverb* rv);

}  // namespace mp3g
