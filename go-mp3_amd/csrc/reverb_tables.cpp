// reverb_tables.cpp -- host side of the reverberation and noise mixing
// (include/mp3g.h "Room reverberation and noise at an SNR"): the object (the
// responses' peaks, early windows and partition spectra), the argument checks,
// mp3g_row_power_host and mp3g_augment_host -- the plain-C++ statements that the
// device calls (reverb.hip) equal bit for bit.  No HIP call is made here.
#include <cstring>
#include <new>

#include "abi_util.h"
#include "reverb.h"

using namespace mp3g;

namespace {

bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

// one (row, plane) of mp3g_augment_host; X and part are the caller's buffers
void augment_plane(const mp3g_reverb* rv, const mp3g_augment_args& a, uint32_t row, uint32_t plane,
                   std::vector<StftC>& X, std::vector<double>& part) {
  const uint32_t T = a.T, n = a.lengths && a.lengths[row] < T ? a.lengths[row] : T;
  const size_t rp = (size_t)row * a.n_planes + plane;
  const float* xp = a.x + rp * T;
  float* op = a.out + rp * T;
  double* st = a.stats + rp * 4;
  const uint32_t nb = rv_blocks(n);
  part.resize(nb);
  for (uint32_t b = 0; b < nb; b++) part[b] = rv_sumsq(xp + (size_t)b * kRvS, std::min(kRvS, n - b * kRvS));
  const double power_before = rv_mean(rv_sum(part.data(), nb), n);
  double signal_power = power_before;
  const int32_t ri = a.rir_index ? a.rir_index[row] : -1;
  if (ri >= 0 && n) {
    const RvRir& r = rv->rirs[(size_t)ri];
    const StftC* tw = rv->tw.data();
    X.resize((size_t)(nb + 1) * kRvN);
    for (uint32_t m = 0; m <= nb; m++) {  // X_m: blocks m - 1 and m of x
      StftC* z = X.data() + (size_t)m * kRvN;
      for (uint32_t i = 0; i < kRvN; i++) {
        const int64_t t = ((int64_t)m - 1) * kRvS + i;
        z[i] = StftC{t >= 0 && t < (int64_t)n ? xp[t] : 0.f, 0.f};
      }
      rv_fft_forward(z, tw);
    }
    const uint32_t k0 = rv_k0(r), k1 = rv_k1(r, n);
    const uint64_t e_end = (uint64_t)n + r.ee - 1;  // the early response's output ends here
    std::vector<StftC> z(kRvN);
    std::vector<float> e(kRvS);
    std::vector<double> pe(k1 - k0 + 1);
    for (uint32_t k = k0; k <= k1; k++) {
      for (uint32_t s = 0; s < kRvN; s++) z[s] = StftC{0.f, 0.f};
      const uint32_t plo = k > nb ? k - nb : 0, phi = std::min(r.P - 1, k);
      for (uint32_t p = plo; p <= phi; p++) {
        const StftC* xs = X.data() + (size_t)(k - p) * kRvN;
        const StftC* gs = rv->G.data() + r.goff + (size_t)p * kRvN;
        for (uint32_t s = 0; s < kRvN; s++) z[s] = rv_mac(z[s], xs[s], gs[s]);
      }
      rv_fft_inverse(z.data(), tw);
      const uint64_t t0 = (uint64_t)k * kRvS;  // of z[1024]
      for (uint32_t i = 0; i < kRvS; i++) {
        const uint64_t t = t0 + i;
        if (t >= r.peak && t < (uint64_t)r.peak + n) op[t - r.peak] = z[kRvS + i].re * kRvInvN;
        e[i] = z[kRvS + i].im * kRvInvN;
      }
      const uint64_t lo = std::max<uint64_t>(t0, r.es), hi = std::min<uint64_t>(t0 + kRvS, e_end);
      pe[k - k0] = hi > lo ? rv_sumsq(e.data() + (lo - t0), (uint32_t)(hi - lo)) : 0.0;
    }
    signal_power = rv_mean(rv_sum(pe.data(), k1 - k0 + 1), (uint64_t)n + (r.ee - r.es) - 1);
  } else if (n) {
    std::memcpy(op, xp, (size_t)n * sizeof(float));
  }
  RvMix mix = {};
  for (uint32_t s = 0; s < a.A; s++) {
    const mp3g_augment_slot& sl = a.slots[(size_t)row * a.A + s];
    mix.live[s] = false;
    if (sl.noise_index < 0) continue;
    const double pn = a.noise_power[sl.noise_index];
    if (pn == 0.0) continue;
    mix.live[s] = true;
    mix.noise[s] = a.noise + (size_t)sl.noise_index * a.Tn;
    mix.len[s] = std::min(a.noise_lengths[sl.noise_index], a.Tn);
    mix.start[s] = sl.start;
    mix.offset[s] = sl.offset;
    mix.wrap[s] = sl.wrap;
    mix.g[s] = rv_gain(sl.snr_ratio, signal_power, pn);
  }
  for (uint32_t j = 0; j < n; j++) op[j] = rv_mix_sample(mix, a.A, j, op[j]);
  for (uint32_t j = n; j < T; j++) op[j] = 0.f;
  for (uint32_t b = 0; b < nb; b++) part[b] = rv_sumsq(op + (size_t)b * kRvS, std::min(kRvS, n - b * kRvS));
  const double power_after = rv_mean(rv_sum(part.data(), nb), n);
  double scale = 1.0;
  if (a.flags & MP3G_AUGMENT_NORMALIZE) {
    scale = rv_scale(power_before, power_after, n);
    for (uint32_t j = 0; j < n; j++) op[j] = (float)((double)op[j] * scale);
  }
  st[0] = power_before;
  st[1] = signal_power;
  st[2] = power_after;
  st[3] = scale;
}

}  // namespace

namespace mp3g {

int row_power_check(uint32_t n_rows, uint32_t T) {
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "row power: rows of 2^31 samples or more");
  if ((uint64_t)n_rows * rv_blocks(T) >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "row power: 2^31 blocks or more");
  return MP3G_OK;
}

int augment_shape_check(const mp3g_reverb* rv, uint32_t n_rows, uint32_t n_planes, uint32_t T) {
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: 1 or 2 planes");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "augment: rows of 2^31 samples or more");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes * (rv_layout(rv ? rv->Lmax : 0, 1, T).KB + rv_blocks(T) + 2) >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "augment: 2^31 blocks or more");
  return MP3G_OK;
}

int augment_check(const mp3g_reverb* rv, const mp3g_augment_args* a, bool* work) {
  *work = false;
  if (!a) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: null arguments");
  const int st = augment_shape_check(rv, a->n_rows, a->n_planes, a->T);
  if (st != MP3G_OK) return st;
  if (a->flags & ~MP3G_AUGMENT_NORMALIZE) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: unknown flag");
  if (a->A > kRvMaxSlots) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: more than 8 additive slots");
  if (a->Tn >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "augment: noise rows of 2^31 samples or more");
  const uint64_t planes = (uint64_t)a->n_rows * a->n_planes;
  if (a->x && a->x == a->out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: out is x (the call is out of place)");
  if (!a->n_rows || !a->T) return MP3G_OK;
  if (!a->x || !a->out || !a->stats) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: null buffer");
  const uint64_t bytes = planes * a->T * sizeof(float);
  if (overlap(a->x, bytes, a->out, bytes)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: out overlaps x");
  if (a->A && !a->slots) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: slots without their table");
  *work = true;
  return MP3G_OK;
}

// the checks of what the rows refer to: the host copies of rir_index, of the
// noise lengths and of the slots
int augment_check_refs(const mp3g_reverb* rv, const mp3g_augment_args* a, const int32_t* rir_index,
                       const uint32_t* noise_lengths, const mp3g_augment_slot* slots) {
  for (uint32_t r = 0; r < a->n_rows; r++) {
    if (rir_index && rir_index[r] >= 0 && (!rv || (uint32_t)rir_index[r] >= rv->R))
      return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: rir_index past the bank");
    for (uint32_t s = 0; s < a->A; s++) {
      const mp3g_augment_slot& sl = slots[(size_t)r * a->A + s];
      if (sl.noise_index < 0) continue;
      if (!a->noise || !noise_lengths || !a->noise_power || (uint32_t)sl.noise_index >= a->n_noise)
        return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: noise_index past the bank");
      const uint32_t len = std::min(noise_lengths[sl.noise_index], a->Tn);
      if (sl.offset >= len) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: noise_offset at or past the noise's length");
      if (sl.start >= (1u << 31)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: start of 2^31 or more");
    }
  }
  return MP3G_OK;
}

}  // namespace mp3g

extern "C" {

int mp3g_reverb_create(int device, int rate, const float* rirs, uint32_t n_rirs, uint32_t stride,
                       const uint32_t* rir_lengths, mp3g_reverb** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (rate <= 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "reverb: rate not positive");
  // (below 20 Hz the early window [peak - rate / 1000, peak + rate / 20) is empty and does not hold the peak)
  if (rate < 20 || rate > 384000) return abi_fail(MP3G_ERR_UNSUPPORTED, "reverb: rate below 20 or above 384000");
  if (n_rirs == 0 || !rirs || !rir_lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "reverb: no responses");
  if (n_rirs >= (1u << 20)) return abi_fail(MP3G_ERR_UNSUPPORTED, "reverb: 2^20 responses or more");
  for (uint32_t i = 0; i < n_rirs; i++)
    if (rir_lengths[i] < 1 || rir_lengths[i] > kRvMaxTaps || rir_lengths[i] > stride)
      return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "reverb: a response of no taps, of more than 65,536 or of more than its row");
  mp3g_reverb* rv = new (std::nothrow) mp3g_reverb;
  if (!rv) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "reverb");
  try {
    rv->device = device;
    rv->rate = (uint32_t)rate;
    rv->R = n_rirs;
    rv->tw.resize(kRvTw);
    for (uint32_t k = 0; k < kRvTw; k++) rv->tw[k] = stft_twiddle(k, kRvTw);
    rv->rirs.resize(n_rirs);
    const uint32_t before = rv->rate / 1000, after = rv->rate / 20;
    uint64_t goff = 0;
    for (uint32_t i = 0; i < n_rirs; i++) {
      const float* h = rirs + (size_t)i * stride;
      RvRir& r = rv->rirs[i];
      r.L = rir_lengths[i];
      r.peak = 0;
      for (uint32_t j = 1; j < r.L; j++)
        if (h[j] > h[r.peak]) r.peak = j;
      r.es = r.peak > before ? r.peak - before : 0;
      r.ee = std::min(r.L, r.peak + after);
      r.P = rv_blocks(r.L);
      r.zero = 0;
      r.goff = goff;
      goff += (uint64_t)r.P * kRvN;
      rv->Lmax = std::max(rv->Lmax, r.L);
    }
    rv->G.resize(goff);
    for (uint32_t i = 0; i < n_rirs; i++) {
      const float* h = rirs + (size_t)i * stride;
      const RvRir& r = rv->rirs[i];
      for (uint32_t p = 0; p < r.P; p++) {  // G_p = FFT(h_p + i h_e,p), the second half zero
        StftC* z = rv->G.data() + r.goff + (size_t)p * kRvN;
        for (uint32_t j = 0; j < kRvN; j++) {
          const uint32_t t = p * kRvS + j;
          const bool tap = j < kRvS && t < r.L;
          z[j] = StftC{tap ? h[t] : 0.f, tap && t >= r.es && t < r.ee ? h[t] : 0.f};
        }
        rv_fft_forward(z, rv->tw.data());
      }
    }
  } catch (...) {
    delete rv;
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "reverb");
  }
  if (device >= 0) {
    const int st = reverb_device_upload(rv);
    if (st != MP3G_OK) {
      delete rv;
      return st;
    }
  }
  *out = rv;
  return MP3G_OK;
}

void mp3g_reverb_free(mp3g_reverb* rv) {
  if (!rv) return;
  if (rv->device >= 0) reverb_device_free(rv);
  delete rv;
}

int mp3g_reverb_info(const mp3g_reverb* rv, uint32_t* n_rirs, uint32_t* max_taps, const uint32_t** table,
                     const float** twiddles, const float** spectra, uint64_t* n_spectra) {
  if (!rv) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null reverb");
  static_assert(sizeof(RvRir) == 32, "the table is eight words a response");
  if (n_rirs) *n_rirs = rv->R;
  if (max_taps) *max_taps = rv->Lmax;
  if (table) *table = reinterpret_cast<const uint32_t*>(rv->rirs.data());
  if (twiddles) *twiddles = &rv->tw[0].re;
  if (spectra) *spectra = &rv->G[0].re;
  if (n_spectra) *n_spectra = rv->G.size();
  return MP3G_OK;
}

uint64_t mp3g_reverb_scratch_bytes(const mp3g_reverb* rv, uint32_t n_rows, uint32_t n_planes, uint32_t T) {
  if (augment_shape_check(rv, n_rows, n_planes, T) != MP3G_OK || !n_rows || !T) return 0;
  return rv_layout(rv ? rv->Lmax : 0, (uint64_t)n_rows * n_planes, T).bytes;
}

uint64_t mp3g_row_power_scratch_bytes(uint32_t n_rows, uint32_t T) {
  if (row_power_check(n_rows, T) != MP3G_OK) return 0;
  return (uint64_t)n_rows * rv_blocks(T) * sizeof(double);
}

int mp3g_row_power_host(const float* x, uint32_t n_rows, uint32_t T, const uint32_t* lengths, double* power) {
  const int st = row_power_check(n_rows, T);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!power || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "row power: null buffer");
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths && lengths[r] < T ? lengths[r] : T, nb = rv_blocks(n);
    double s = 0.0;  // (the block sums ascending from +0.0: rv_sum's order)
    for (uint32_t b = 0; b < nb; b++) s += rv_sumsq(x + (size_t)r * T + (size_t)b * kRvS, std::min(kRvS, n - b * kRvS));
    power[r] = rv_mean(s, n);
  }
  return MP3G_OK;
}

int mp3g_augment_host(const mp3g_reverb* rv, const mp3g_augment_args* a) {
  bool work = false;
  int st = augment_check(rv, a, &work);
  if (st != MP3G_OK) return st;
  if (!work) return MP3G_OK;
  st = augment_check_refs(rv, a, a->rir_index, a->noise_lengths, a->slots);
  if (st != MP3G_OK) return st;
  std::atomic<bool> oom{false};
  parallel_for(0, a->n_rows, thread_count(0, a->n_rows), [&](uint32_t row) {
    try {
      std::vector<StftC> X;
      std::vector<double> part;
      for (uint32_t p = 0; p < a->n_planes; p++) augment_plane(rv, *a, row, p, X, part);
    } catch (...) {
      oom = true;
    }
  });
  return oom ? abi_fail(MP3G_ERR_OUT_OF_MEMORY, "augment") : MP3G_OK;
}

}  // extern "C"
