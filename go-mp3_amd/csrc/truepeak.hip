// truepeak.hip -- device side of the true peak, of the momentary and short-term
// maxima and the loudness range, and of the gain against a supplied peak
// (include/mp3g.h "True peak of decoded rows", "Momentary and short-term maxima,
// loudness range").
//
// true_peak_kernel: one block per tile of kTpTile samples of one plane, one
// thread per kTpPer = 16 consecutive outputs.  A thread needs its 16 samples and
// the 11 before them: seven 16-byte words, the plane's samples n0 - 12 ..
// n0 + 15, all loaded before the first is used (4-byte aligned addresses; a
// neighbour's words overlap and come from the cache).  The thread at a plane's
// start has no samples before it: its first three words are zeros, whatever
// lies there in memory (the previous plane's or row's tail).  A word that would
// end past the tensor is fetched from the tensor's last 16 bytes and shifted
// after all loads are issued.  The 36 coefficients are literals of the unrolled
// code: no memory traffic.  The block's maximum goes to the scratch, one float
// per tile; true_peak_row_kernel, one wave per row, folds a row's partial
// maxima.  (atomicMax on the bit pattern into a d_tp that a first launch zeroes
// was measured and is slower -- DESIGN.md 9i has both timings.)
//
// loudness_range_kernel: one block per row over the scratch the loudness
// kernels left: the maxima and the short-term energies in parallel, the
// relative gate's mean by one lane in the written-down order, the two
// percentiles by counting, 63 block-wide counts for both ranks together.
//
// gain_peak_kernel: loudness.hip's gain_kernel with the peak from an array.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "abi_util.h"
#include "loudness.h"
#include "loudness_range.h"
#include "truepeak.h"

namespace mp3g {
namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = tp_max(v, __shfl_xor(v, m));
  return v;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
  return (uint64_t)hi << 32 | lo;
}

struct TpArgs {
  const float* src;
  const uint32_t* lengths;    // may be null: every row is T long
  const uint32_t* row_index;  // may be null: work row i is row i
  float* partial;             // [n_work * n_planes * tiles]
  uint64_t total;             // floats of the whole source tensor
  uint32_t n_rows, n_planes, T, tiles;
};

// kTiny: a tensor of fewer than 4 floats, which has no 16 bytes to read.
template <bool kTiny>
__global__ __launch_bounds__(kTpBlock) void true_peak_kernel(TpArgs a) {
  constexpr uint32_t kWords = (kTpPer + 12) / 4, kLead = 12;  // the 11 samples before n0, rounded up to words
  __shared__ float folded[kTpBlock / 64];
  const uint32_t rp = blockIdx.x / a.tiles, tile = blockIdx.x - rp * a.tiles;
  const uint32_t i = rp / a.n_planes, p = rp - i * a.n_planes;
  const uint32_t row = a.row_index ? a.row_index[i] : i;
  uint32_t len = 0;
  if (row < a.n_rows) {
    len = a.lengths ? a.lengths[row] : a.T;
    len = len < a.T ? len : a.T;
  }
  const uint32_t n0 = tile * kTpTile + threadIdx.x * kTpPer;  // (below T + kTpTile: fits)
  float tp = 0.f;
  if (n0 < len) {
    const uint64_t first = ((uint64_t)row * a.n_planes + p) * a.T + n0;
    const uint64_t last = kTiny ? 0 : a.total - 4;
    struct __attribute__((packed, aligned(4))) Word {
      float v[4];
    };
    float xs[4 * kWords];  // xs[m] = x[n0 - 12 + m]
    // (the words before a plane's first sample are not read from where they
    // would lie: any valid address, their values are replaced below)
#pragma unroll
    for (uint32_t k = 0; k < kWords; k++) {
      const uint64_t e = (4 * k < kLead && n0 == 0) ? first : first + 4 * k - kLead;
      if constexpr (kTiny) {
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) xs[4 * k + c] = e + c < a.total ? a.src[e + c] : 0.f;
      } else {
        const Word w = *reinterpret_cast<const Word*>(a.src + (e < last ? e : last));
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) xs[4 * k + c] = w.v[c];
      }
    }
    if constexpr (!kTiny) {
      // the thread whose words reach past the tensor: the float wanted at c is
      // at c + sh of the word fetched instead (one from past the word lies past
      // the tensor: never a sample)
      if (first + kTpPer > a.total) {
#pragma unroll
        for (uint32_t k = 0; k < kWords; k++) {
          const uint64_t e = (4 * k < kLead && n0 == 0) ? first : first + 4 * k - kLead;
          const uint32_t sh = e < last ? 0u : (uint32_t)(e - last < 4 ? e - last : 4);
          const float v0 = xs[4 * k], v1 = xs[4 * k + 1], v2 = xs[4 * k + 2], v3 = xs[4 * k + 3];
          xs[4 * k] = sh == 0 ? v0 : sh == 1 ? v1 : sh == 2 ? v2 : v3;
          xs[4 * k + 1] = sh == 0 ? v1 : sh == 1 ? v2 : v3;
          xs[4 * k + 2] = sh == 0 ? v2 : v3;
        }
      }
    }
    if (n0 == 0) {
#pragma unroll
      for (uint32_t m = 0; m < kLead; m++) xs[m] = 0.f;  // x[k] = 0 for k < 0
    }
    const uint32_t nvalid = len - n0 < kTpPer ? len - n0 : kTpPer;
#pragma unroll
    for (uint32_t o = 0; o < kTpPer; o++) {
      const float t = tp_sample(xs + kLead + o, tp);
      tp = o < nvalid ? t : tp;
    }
  }
  tp = wave_max(tp);
  if ((threadIdx.x & 63) == 0) folded[threadIdx.x >> 6] = tp;
  __syncthreads();
  if (threadIdx.x == 0 && row < a.n_rows) {
#pragma unroll
    for (uint32_t w = 1; w < kTpBlock / 64; w++) tp = tp_max(tp, folded[w]);
    a.partial[blockIdx.x] = tp;
  }
}

// One wave per work row: the maximum of its per_row partial maxima (0 of none).
__global__ __launch_bounds__(kTpRowBlock) void true_peak_row_kernel(const float* partial, const uint32_t* row_index,
                                                                    uint32_t n_rows, uint32_t per_row, float* tp) {
  const uint32_t i = blockIdx.x;
  const uint32_t row = row_index ? row_index[i] : i;
  if (row >= n_rows) return;
  float v = 0.f;
  for (uint32_t k = threadIdx.x; k < per_row; k += kTpRowBlock) v = tp_max(v, partial[(size_t)i * per_row + k]);
  v = wave_max(v);
  if (threadIdx.x == 0) tp[row] = v;
}

struct RangeArgs {
  const uint32_t* lengths;
  const uint32_t* row_index;
  const double* items;  // the loudness scratch
  double* S;            // [n_work][S1]
  mp3g_loudness_range* out;
  uint32_t n_rows, n_planes, T, H, S1;
};

__global__ __launch_bounds__(kRangeBlock) void loudness_range_kernel(RangeArgs a) {
  constexpr uint32_t kWaves = kRangeBlock / 64, kD = kLoudItemDoubles;
  __shared__ double fold_m[kWaves], fold_s[kWaves];
  __shared__ uint64_t fold_c[2][kWaves];
  __shared__ double gate;
  const uint32_t i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t row = a.row_index ? a.row_index[i] : i;
  if (row >= a.n_rows) return;  // (the whole block)
  uint32_t len = a.lengths ? a.lengths[row] : a.T;
  len = len < a.T ? len : a.T;
  const uint32_t nseg = len / a.H, nb = nseg >= 4 ? nseg - 3 : 0, ns = range_short_count(nseg);
  const double* items = a.items + (size_t)i * a.n_planes * a.S1 * kD;
  double* S = a.S + (size_t)i * a.S1;
  // the maxima (order-free) and the short-term energies
  double M = 0.0, Smax = 0.0;
  for (uint32_t k = tid; k < nb; k += kRangeBlock) {
    const double z = items[(size_t)k * kD + 1];
    M = z > M ? z : M;
  }
  for (uint32_t k = tid; k < ns; k += kRangeBlock) {
    const double s = range_short_energy(items, a.n_planes, a.S1, k, a.H);
    S[k] = s;
    Smax = s > Smax ? s : Smax;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double om = __builtin_bit_cast(double, shfl_xor64(__builtin_bit_cast(uint64_t, M), m));
    const double os = __builtin_bit_cast(double, shfl_xor64(__builtin_bit_cast(uint64_t, Smax), m));
    M = om > M ? om : M;
    Smax = os > Smax ? os : Smax;
  }
  if (lane == 0) {
    fold_m[wave] = M;
    fold_s[wave] = Smax;
  }
  __syncthreads();  // (and every S_k is written)
  // the relative gate: one lane, k ascending
  if (tid == 0) {
    uint32_t n_abs = 0;
    gate = range_rel_gate(S, ns, &n_abs);
  }
  __syncthreads();
  const double rel = gate;
  // block-wide sum of a pair of counts (low and high word), pass by pass
  uint32_t pass = 0;
  auto count2 = [&](uint64_t c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += shfl_xor64(c, m);
    if (lane == 0) fold_c[pass & 1][wave] = c;
    __syncthreads();
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) sum += fold_c[pass & 1][w];
    pass++;  // (the next pass writes the other set: one barrier per pass)
    return sum;
  };
  uint64_t c = 0;
  for (uint32_t k = tid; k < ns; k += kRangeBlock) c += range_gated(S[k], rel) ? 1u : 0u;
  const uint32_t n_range = (uint32_t)count2(c);
  double vlo = 0.0, vhi = 0.0;
  if (n_range) {  // (the whole block)
    const uint32_t rlo = range_rank_lo(n_range), rhi = range_rank_hi(n_range);
    uint64_t plo = 0, phi = 0;
    for (uint32_t b = 63; b-- > 0;) {
      const uint64_t tlo = range_trial(plo, b), thi = range_trial(phi, b);
      c = 0;
      for (uint32_t k = tid; k < ns; k += kRangeBlock) {
        const double s = S[k];
        c += (range_below(s, rel, tlo) ? 1ull : 0ull) + (range_below(s, rel, thi) ? 1ull << 32 : 0ull);
      }
      const uint64_t both = count2(c);
      if ((uint32_t)both <= rlo) plo = tlo;
      if ((uint32_t)(both >> 32) <= rhi) phi = thi;
    }
    vlo = __builtin_bit_cast(double, plo);
    vhi = __builtin_bit_cast(double, phi);
  }
  if (tid == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kWaves; w++) {
      M = fold_m[w] > M ? fold_m[w] : M;
      Smax = fold_s[w] > Smax ? fold_s[w] : Smax;
    }
    range_record(M, Smax, ns, n_range, vlo, vhi, &a.out[row]);
  }
}

// loudness.hip's gain_kernel, the peak of a row from `peaks`.
__global__ __launch_bounds__(kGainBlock) void gain_peak_kernel(float* x, uint32_t n_planes, uint32_t T,
                                                               const uint32_t* lengths,
                                                               const mp3g_loudness_stats* stats, const float* peaks,
                                                               double target_energy, float peak_ceiling,
                                                               float* gain_out, uint32_t blocks_per_plane) {
  const uint32_t rp = blockIdx.x / blocks_per_plane, chunk = blockIdx.x - rp * blocks_per_plane;
  const uint32_t row = rp / n_planes;
  const double energy = stats[row].energy;
  const float peak = peaks[row];
  const bool first = threadIdx.x == 0 && chunk == 0 && rp == row * n_planes;
  if (!(energy > 0.0)) {
    if (first && gain_out) gain_out[row] = 1.0f;
    return;
  }
  uint32_t len = lengths ? lengths[row] : T;
  len = len < T ? len : T;
  float* xp = x + (size_t)rp * T;
  const uint32_t head = (4u - ((uint32_t)((uintptr_t)xp >> 2) & 3u)) & 3u;  // floats before the first aligned word
  float4 v[kGainWords];
  uint64_t e[kGainWords];
  bool whole[kGainWords];
#pragma unroll
  for (uint32_t u = 0; u < kGainWords; u++) {
    const uint64_t slot = ((uint64_t)chunk * kGainWords + u) * kGainBlock + threadIdx.x;
    e[u] = slot ? head + 4 * (slot - 1) : 0;
    whole[u] = slot && e[u] + 4 <= len;
    v[u] = whole[u] ? *reinterpret_cast<const float4*>(xp + e[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float g = loud_gain(energy, peak, target_energy, peak_ceiling);
  if (first && gain_out) gain_out[row] = g;
#pragma unroll
  for (uint32_t u = 0; u < kGainWords; u++) {
    const uint64_t slot = ((uint64_t)chunk * kGainWords + u) * kGainBlock + threadIdx.x;
    if (whole[u]) {
      *reinterpret_cast<float4*>(xp + e[u]) = make_float4(v[u].x * g, v[u].y * g, v[u].z * g, v[u].w * g);
    } else if (slot == 0) {
      for (uint32_t n = 0; n < head && n < len; n++) xp[n] = xp[n] * g;
    } else {
      for (uint64_t n = e[u]; n < len; n++) xp[n] = xp[n] * g;  // the tail, or nothing
    }
  }
}

int hip_fail(int status, const char* what, hipError_t e) {
  const std::string s = std::string(what) + ": " + hipGetErrorString(e);
  return abi_fail(status, s.c_str());
}

// Restores the caller's current device on scope exit.
struct DeviceScope {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceScope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace
}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_true_peak_rows(int device, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                                   const uint32_t* d_lengths, const uint32_t* d_row_index, uint32_t n_index,
                                   void* d_scratch, float* d_tp, void* hip_stream) {
  uint32_t tiles = 0;
  const int st = true_peak_check(n_rows, n_planes, T, &tiles);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  const uint32_t n_work = d_row_index ? n_index : n_rows;
  if (n_work > n_rows) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "true peak: more indices than rows");
  if (n_work == 0) return MP3G_OK;
  if (!d_tp || (T && (!d_src || !d_scratch))) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  if (((uintptr_t)d_src & 3u) || ((uintptr_t)d_scratch & 3u) || ((uintptr_t)d_tp & 3u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "true peak: a misaligned device buffer");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  TpArgs a = {};
  a.src = d_src;
  a.lengths = d_lengths;
  a.row_index = d_row_index;
  a.partial = static_cast<float*>(d_scratch);
  a.total = (uint64_t)n_rows * n_planes * T;
  a.n_rows = n_rows;
  a.n_planes = n_planes;
  a.T = T;
  a.tiles = tiles;
  const uint32_t blocks = n_work * n_planes * tiles;  // (below 2^31: true_peak_check)
  hipError_t e = hipSuccess;
  if (blocks) {
    if (a.total < 4)
      true_peak_kernel<true><<<blocks, kTpBlock, 0, stream>>>(a);
    else
      true_peak_kernel<false><<<blocks, kTpBlock, 0, stream>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "true peak launch", e);
  }
  true_peak_row_kernel<<<n_work, kTpRowBlock, 0, stream>>>(a.partial, d_row_index, n_rows, n_planes * tiles, d_tp);
  e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "true peak row launch", e);
}

extern "C" int mp3g_loudness_range_rows(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                                        const uint32_t* d_lengths, const uint32_t* d_row_index, uint32_t n_index,
                                        const void* d_loudness_scratch, void* d_range_scratch,
                                        mp3g_loudness_range* d_out, void* hip_stream) {
  const int st = loudness_check(ld, n_rows, n_planes, T, nullptr);
  if (st != MP3G_OK) return st;
  if (ld->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness range: a host-only object");
  const uint32_t n_work = d_row_index ? n_index : n_rows;
  if (n_work > n_rows) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness range: more indices than rows");
  if (n_work == 0) return MP3G_OK;
  if (!d_loudness_scratch || !d_range_scratch || !d_out)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  if (((uintptr_t)d_loudness_scratch & 7u) || ((uintptr_t)d_range_scratch & 7u) || ((uintptr_t)d_out & 3u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness range: a misaligned device buffer");
  DeviceScope scope(ld->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  RangeArgs a = {};
  a.lengths = d_lengths;
  a.row_index = d_row_index;
  a.items = static_cast<const double*>(d_loudness_scratch);
  a.S = static_cast<double*>(d_range_scratch);
  a.out = d_out;
  a.n_rows = n_rows;
  a.n_planes = n_planes;
  a.T = T;
  a.H = ld->H;
  a.S1 = loud_items_per_plane(T, ld->H);
  loudness_range_kernel<<<n_work, kRangeBlock, 0, static_cast<hipStream_t>(hip_stream)>>>(a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "loudness range launch", e);
}

extern "C" int mp3g_gain_rows_peak(int device, float* d_x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                                   const uint32_t* d_lengths, const mp3g_loudness_stats* d_stats, double target_energy,
                                   float peak_ceiling, float* d_gain_out, void* hip_stream, const float* d_peak) {
  if (!d_peak)
    return mp3g_gain_rows(device, d_x, n_rows, n_planes, T, d_lengths, d_stats, target_energy, peak_ceiling, d_gain_out,
                          hip_stream);
  const int st = gain_check(n_rows, n_planes, T, target_energy, peak_ceiling);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (n_rows == 0) return MP3G_OK;
  if (!d_stats || (T && !d_x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: null device buffer");
  if (((uintptr_t)d_x & 3u) || ((uintptr_t)d_stats & 7u) || ((uintptr_t)d_peak & 3u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: a misaligned device buffer");
  // slots of a plane: its head, then every aligned word that can hold a sample
  const uint64_t slots = 2 + (uint64_t)T / 4, per_block = (uint64_t)kGainBlock * kGainWords;
  const uint64_t bpp = (slots + per_block - 1) / per_block, blocks = bpp * n_rows * n_planes;
  if (blocks >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "gain: too many samples for one launch");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  gain_peak_kernel<<<(uint32_t)blocks, kGainBlock, 0, static_cast<hipStream_t>(hip_stream)>>>(
      d_x, n_planes, T, d_lengths, d_stats, d_peak, target_energy, peak_ceiling, d_gain_out, (uint32_t)bpp);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "gain launch", e);
}
