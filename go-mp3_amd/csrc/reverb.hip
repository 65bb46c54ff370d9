// reverb.hip -- device side of the reverberation and noise mixing (include/mp3g.h
// "Room reverberation and noise at an SNR"): the table upload, mp3g_row_power_rows
// and mp3g_augment_rows.  A translation unit of its own: the other kernels'
// listings do not see it.
//
// Shape.  The convolution is uniformly partitioned overlap-save at N = 2,048:
//   sumsq    the float64 block sums of x^2 (a workgroup takes four blocks of 1,024
//            through LDS; lane 0 of each wave adds one block in order)
//   forward  one workgroup of 128 lanes per (row, plane, input block m): blocks
//            m - 1 and m of x, the forward network, the spectrum X_m into the
//            caller's scratch in slot order
//   convolve one workgroup per (row, plane, output block k): acc += X_(k-p) G_p
//            over the row's partitions with the 2,048 accumulators in registers
//            (16 to a lane), the inverse network in LDS, the kept real parts to
//            `out` shifted by the peak, the block's sum of the early response's
//            squares (the imaginary parts) to the scratch
//   mix      a workgroup per four blocks: one lane folds the block sums into
//            power_before and signal_power and forms the slots' gains, every
//            lane adds the noises to its samples, writes v and +0 past the length
//            and the block sums of v^2
//   scale    folds those into power_after and the scale and multiplies
// The transforms hold a working set in LDS, value i at float2 slot i + (i >> 5),
// and run two radix-4 passes per round trip through LDS with 16 values in a
// lane's registers, and the block of 8 that is left (radix 4 and radix 2) with
// eight neighbours to a lane: the STFT kernel's schedule at n_fft = 4096, whose
// bank arithmetic DESIGN.md 9f gives.  Which lane runs a butterfly does not
// change its operands, so the bits are the host's.  No atomics, no
// data-dependent grid, and a workgroup whose block a row does not need returns
// before its first barrier.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "abi_util.h"
#include "reverb.h"

namespace mp3g {
namespace {

// two radix-4 passes of the forward network over blocks of len and len / 4
__device__ inline void fwd_double(StftC* z, const StftC* __restrict__ tw, uint32_t len, uint32_t j) {
  const uint32_t q = len >> 2, q2 = len >> 4, step = kRvTw / len;
  const uint32_t n = j & (q2 - 1), i0 = (j - n) * 16 + n;
  StftC e[4][4];
#pragma unroll
  for (uint32_t a = 0; a < 4; a++)
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) e[a][c] = z[rv_skew(i0 + a * q + c * q2)];
#pragma unroll
  for (uint32_t c = 0; c < 4; c++) stft_bfly4(&e[0][c], &e[1][c], &e[2][c], &e[3][c], tw, (n + c * q2) * step, kRvTw);
#pragma unroll
  for (uint32_t a = 0; a < 4; a++) stft_bfly4(&e[a][0], &e[a][1], &e[a][2], &e[a][3], tw, n * step * 4, kRvTw);
#pragma unroll
  for (uint32_t a = 0; a < 4; a++)
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) z[rv_skew(i0 + a * q + c * q2)] = e[a][c];
}

// the same two passes of the inverse network: the one over len / 4 first
__device__ inline void inv_double(StftC* z, const StftC* __restrict__ tw, uint32_t len, uint32_t j) {
  const uint32_t q = len >> 2, q2 = len >> 4, step = kRvTw / len;
  const uint32_t n = j & (q2 - 1), i0 = (j - n) * 16 + n;
  StftC e[4][4];
#pragma unroll
  for (uint32_t a = 0; a < 4; a++)
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) e[a][c] = z[rv_skew(i0 + a * q + c * q2)];
#pragma unroll
  for (uint32_t a = 0; a < 4; a++) rv_ibfly4(&e[a][0], &e[a][1], &e[a][2], &e[a][3], tw, n * step * 4);
#pragma unroll
  for (uint32_t c = 0; c < 4; c++) rv_ibfly4(&e[0][c], &e[1][c], &e[2][c], &e[3][c], tw, (n + c * q2) * step);
#pragma unroll
  for (uint32_t a = 0; a < 4; a++)
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) z[rv_skew(i0 + a * q + c * q2)] = e[a][c];
}

// the forward network on the working set z (natural order in, slot order out);
// every lane of the workgroup of kRvFftLanes calls it, and it ends on a barrier
__device__ inline void fft_forward(StftC* z, const StftC* __restrict__ tw, uint32_t tid) {
  fwd_double(z, tw, 2048, tid);
  __syncthreads();
  fwd_double(z, tw, 128, tid);
  __syncthreads();
#pragma unroll
  for (uint32_t h = 0; h < 2; h++) {  // the blocks of 8: radix 4, then radix 2
    const uint32_t j = tid + h * kRvFftLanes;
    StftC e[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) e[i] = z[rv_skew(8 * j + i)];
    stft_bfly4(&e[0], &e[2], &e[4], &e[6], tw, 0, kRvTw);
    stft_bfly4(&e[1], &e[3], &e[5], &e[7], tw, kRvTw >> 3, kRvTw);
#pragma unroll
    for (uint32_t i = 0; i < 8; i += 2) stft_bfly2(&e[i], &e[i + 1]);
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) z[rv_skew(8 * j + i)] = e[i];
  }
  __syncthreads();
}

// the inverse network (slot order in, natural order out, times 2,048)
__device__ inline void fft_inverse(StftC* z, const StftC* __restrict__ tw, uint32_t tid) {
#pragma unroll
  for (uint32_t h = 0; h < 2; h++) {  // the blocks of 8: radix 2, then radix 4
    const uint32_t j = tid + h * kRvFftLanes;
    StftC e[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) e[i] = z[rv_skew(8 * j + i)];
#pragma unroll
    for (uint32_t i = 0; i < 8; i += 2) stft_bfly2(&e[i], &e[i + 1]);
    rv_ibfly4(&e[0], &e[2], &e[4], &e[6], tw, 0);
    rv_ibfly4(&e[1], &e[3], &e[5], &e[7], tw, kRvTw >> 3);
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) z[rv_skew(8 * j + i)] = e[i];
  }
  __syncthreads();
  inv_double(z, tw, 128, tid);
  __syncthreads();
  inv_double(z, tw, 2048, tid);
  __syncthreads();
}

struct RvDev {
  const RvRir* rirs;
  const StftC* tw;
  const StftC* G;
  uint32_t R;
  double* pb;  // [planes][TB]
  double* pv;  // [planes][TB]
  double* pe;  // [planes][KB]
  StftC* spectra;  // [planes][MB][2048]
  uint32_t TB, KB, MB;
};

// the row's response, or -1
__device__ inline int32_t row_rir(const mp3g_augment_args& a, const RvDev& d, uint32_t row) {
  const int32_t ri = a.rir_index ? a.rir_index[row] : -1;
  return ri >= 0 && (uint32_t)ri < d.R ? ri : -1;
}
__device__ inline uint32_t row_len(const uint32_t* lengths, uint32_t row, uint32_t T) {
  const uint32_t n = lengths ? lengths[row] : T;
  return n < T ? n : T;
}

// part[plane][b] = the sum of squares of block b of x's plane, for the blocks of
// the tile; planes_per_row planes share a length
__global__ __launch_bounds__(kRvMixLanes) void sumsq_kernel(const float* __restrict__ x, uint32_t T,
                                                           const uint32_t* __restrict__ lengths,
                                                           uint32_t planes_per_row, double* __restrict__ part,
                                                           uint32_t TB, uint32_t tiles) {
  __shared__ float tile[kRvTile];
  const uint32_t tid = threadIdx.x, t = blockIdx.x % tiles;
  const size_t plane = blockIdx.x / tiles;
  const uint32_t n = row_len(lengths, (uint32_t)(plane / planes_per_row), T), nb = rv_blocks(n);
  if (t * kRvTileBlocks >= nb) return;  // (the whole workgroup)
  const float* __restrict__ xp = x + plane * T;
#pragma unroll
  for (uint32_t u = 0; u < kRvTile / kRvMixLanes; u++) {
    const uint32_t jl = tid + u * kRvMixLanes, j = t * kRvTile + jl;
    tile[jl] = j < n ? xp[j] : 0.f;
  }
  __syncthreads();
  const uint32_t b = t * kRvTileBlocks + (tid >> 6);
  if ((tid & 63) == 0 && b < nb)
    part[plane * TB + b] = rv_sumsq(tile + (tid >> 6) * kRvS, min(kRvS, n - b * kRvS));
}

__global__ void row_power_kernel(const double* __restrict__ part, uint32_t TB, const uint32_t* __restrict__ lengths,
                                 uint32_t T, uint32_t n_rows, double* __restrict__ power) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t n = row_len(lengths, r, T);
  power[r] = rv_mean(rv_sum(part + (size_t)r * TB, rv_blocks(n)), n);
}

__global__ __launch_bounds__(kRvFftLanes) void forward_kernel(mp3g_augment_args a, RvDev d) {
  __shared__ __align__(16) StftC z[kRvSlots];
  const uint32_t tid = threadIdx.x, m = blockIdx.x % d.MB;
  const size_t plane = blockIdx.x / d.MB;
  const uint32_t row = (uint32_t)(plane / a.n_planes);
  if (row_rir(a, d, row) < 0) return;
  const uint32_t n = row_len(a.lengths, row, a.T), nb = rv_blocks(n);
  if (n == 0 || m > nb) return;
  const float* __restrict__ xp = a.x + plane * a.T;
#pragma unroll
  for (uint32_t u = 0; u < kRvN / kRvFftLanes; u++) {
    const uint32_t i = tid + u * kRvFftLanes;
    const int64_t t = ((int64_t)m - 1) * kRvS + i;
    z[rv_skew(i)] = StftC{t >= 0 && t < (int64_t)n ? xp[t] : 0.f, 0.f};
  }
  __syncthreads();
  fft_forward(z, d.tw, tid);
  StftC* __restrict__ X = d.spectra + (plane * d.MB + m) * kRvN;
#pragma unroll
  for (uint32_t u = 0; u < kRvN / kRvFftLanes; u++) {
    const uint32_t i = tid + u * kRvFftLanes;
    X[i] = z[rv_skew(i)];
  }
}

__global__ __launch_bounds__(kRvFftLanes) void convolve_kernel(mp3g_augment_args a, RvDev d) {
  __shared__ __align__(16) StftC z[kRvSlots];
  __shared__ float early[kRvS];
  const uint32_t tid = threadIdx.x, k = blockIdx.x % d.KB;
  const size_t plane = blockIdx.x / d.KB;
  const uint32_t row = (uint32_t)(plane / a.n_planes);
  const int32_t ri = row_rir(a, d, row);
  if (ri < 0) return;
  const RvRir r = d.rirs[ri];
  const uint32_t n = row_len(a.lengths, row, a.T), nb = rv_blocks(n);
  if (n == 0 || k < rv_k0(r) || k > rv_k1(r, n)) return;
  constexpr uint32_t kPer = kRvN / kRvFftLanes;
  StftC acc[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; u++) acc[u] = StftC{0.f, 0.f};
  const uint32_t plo = k > nb ? k - nb : 0, phi = min(r.P - 1, k);
  for (uint32_t p = plo; p <= phi; p++) {
    const StftC* __restrict__ xs = d.spectra + (plane * d.MB + (k - p)) * kRvN;
    const StftC* __restrict__ gs = d.G + r.goff + (size_t)p * kRvN;
#pragma unroll
    for (uint32_t u = 0; u < kPer; u++) {
      const uint32_t s = tid + u * kRvFftLanes;
      acc[u] = rv_mac(acc[u], xs[s], gs[s]);
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kPer; u++) z[rv_skew(tid + u * kRvFftLanes)] = acc[u];
  __syncthreads();
  fft_inverse(z, d.tw, tid);
  const uint64_t t0 = (uint64_t)k * kRvS;
  float* __restrict__ op = a.out + plane * a.T;
#pragma unroll
  for (uint32_t u = 0; u < kRvS / kRvFftLanes; u++) {
    const uint32_t j = tid + u * kRvFftLanes;
    const StftC v = z[rv_skew(kRvS + j)];
    const uint64_t t = t0 + j;
    if (t >= r.peak && t < (uint64_t)r.peak + n) op[t - r.peak] = v.re * kRvInvN;
    early[j] = v.im * kRvInvN;
  }
  __syncthreads();
  if (tid == 0) {
    const uint64_t e_end = (uint64_t)n + r.ee - 1;
    const uint64_t lo = t0 > r.es ? t0 : r.es, hi = t0 + kRvS < e_end ? t0 + kRvS : e_end;
    d.pe[plane * d.KB + k] = hi > lo ? rv_sumsq(early + (lo - t0), (uint32_t)(hi - lo)) : 0.0;
  }
}

__global__ __launch_bounds__(kRvMixLanes) void mix_kernel(mp3g_augment_args a, RvDev d, uint32_t tiles) {
  __shared__ float tile[kRvTile];
  __shared__ RvMix mix;
  __shared__ double power[2];
  const uint32_t tid = threadIdx.x, t = blockIdx.x % tiles;
  const size_t plane = blockIdx.x / tiles;
  const uint32_t row = (uint32_t)(plane / a.n_planes);
  const uint32_t n = row_len(a.lengths, row, a.T), nb = rv_blocks(n);
  const int32_t ri = n ? row_rir(a, d, row) : -1;
  if (tid == 0) power[0] = rv_mean(rv_sum(d.pb + plane * d.TB, nb), n);
  if (tid == 64 && ri >= 0) {
    const RvRir r = d.rirs[ri];
    const uint32_t k0 = rv_k0(r), k1 = rv_k1(r, n);
    power[1] = rv_mean(rv_sum(d.pe + plane * d.KB + k0, k1 - k0 + 1), (uint64_t)n + (r.ee - r.es) - 1);
  }
  __syncthreads();
  if (tid == 0) {
    const double signal_power = ri >= 0 ? power[1] : power[0];
    power[1] = signal_power;
    for (uint32_t s = 0; s < a.A; s++) {
      const mp3g_augment_slot sl = a.slots[(size_t)row * a.A + s];
      mix.live[s] = false;
      if (sl.noise_index < 0 || (uint32_t)sl.noise_index >= a.n_noise) continue;
      const double pn = a.noise_power[sl.noise_index];
      const uint32_t len = min(a.noise_lengths[sl.noise_index], a.Tn);
      if (pn == 0.0 || sl.offset >= len) continue;  // (the second the host call has refused)
      mix.live[s] = true;
      mix.noise[s] = a.noise + (size_t)sl.noise_index * a.Tn;
      mix.len[s] = len;
      mix.start[s] = sl.start;
      mix.offset[s] = sl.offset;
      mix.wrap[s] = sl.wrap;
      mix.g[s] = rv_gain(sl.snr_ratio, signal_power, pn);
    }
    if (t == 0) {
      a.stats[plane * 4] = power[0];
      a.stats[plane * 4 + 1] = signal_power;
    }
  }
  __syncthreads();
  const float* src = (ri >= 0 ? a.out : a.x) + plane * a.T;  // (out itself for a row with a response: no restrict)
  float* op = a.out + plane * a.T;
#pragma unroll 4
  for (uint32_t u = 0; u < kRvTile / kRvMixLanes; u++) {
    const uint32_t jl = tid + u * kRvMixLanes, j = t * kRvTile + jl;
    float v = 0.f;
    if (j < n) v = rv_mix_sample(mix, a.A, j, src[j]);
    if (j < a.T) op[j] = v;
    tile[jl] = v;
  }
  __syncthreads();
  const uint32_t b = t * kRvTileBlocks + (tid >> 6);
  if ((tid & 63) == 0 && b < nb)
    d.pv[plane * d.TB + b] = rv_sumsq(tile + (tid >> 6) * kRvS, min(kRvS, n - b * kRvS));
}

__global__ __launch_bounds__(kRvMixLanes) void scale_kernel(mp3g_augment_args a, RvDev d, uint32_t tiles) {
  __shared__ double shared_scale;
  const uint32_t tid = threadIdx.x, t = blockIdx.x % tiles;
  const size_t plane = blockIdx.x / tiles;
  const uint32_t row = (uint32_t)(plane / a.n_planes);
  const uint32_t n = row_len(a.lengths, row, a.T);
  const bool normalize = (a.flags & MP3G_AUGMENT_NORMALIZE) != 0;
  if (tid == 0) {
    const double power_after = rv_mean(rv_sum(d.pv + plane * d.TB, rv_blocks(n)), n);
    const double scale = normalize ? rv_scale(a.stats[plane * 4], power_after, n) : 1.0;
    shared_scale = scale;
    if (t == 0) {
      a.stats[plane * 4 + 2] = power_after;
      a.stats[plane * 4 + 3] = scale;
    }
  }
  if (!normalize) return;  // (the whole workgroup)
  __syncthreads();
  const double scale = shared_scale;
  float* op = a.out + plane * a.T;
#pragma unroll 4
  for (uint32_t u = 0; u < kRvTile / kRvMixLanes; u++) {
    const uint32_t j = t * kRvTile + tid + u * kRvMixLanes;
    if (j < n) op[j] = (float)((double)op[j] * scale);
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

template <class V>
int upload(const V& host, void** dev, const char* what) {
  const size_t bytes = host.size() * sizeof(host[0]);
  hipError_t e = hipMalloc(dev, bytes);
  if (e != hipSuccess) {
    *dev = nullptr;
    return hip_fail(MP3G_ERR_OUT_OF_MEMORY, what, e);
  }
  e = hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice);
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, what, e);
}

}  // namespace

int reverb_device_upload(mp3g_reverb* rv) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || rv->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "reverb: no such device");
  hipDeviceProp_t prop;
  const hipError_t e = hipGetDeviceProperties(&prop, rv->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  DeviceScope scope(rv->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  int status = upload(rv->rirs, reinterpret_cast<void**>(&rv->d_rirs), "reverb table");
  if (status == MP3G_OK) status = upload(rv->tw, reinterpret_cast<void**>(&rv->d_tw), "reverb twiddles");
  if (status == MP3G_OK) status = upload(rv->G, reinterpret_cast<void**>(&rv->d_G), "reverb spectra");
  if (status != MP3G_OK) reverb_device_free(rv);
  return status;
}

void reverb_device_free(mp3g_reverb* rv) {
  DeviceScope scope(rv->device);
  (void)hipFree(rv->d_rirs);
  (void)hipFree(rv->d_tw);
  (void)hipFree(rv->d_G);
  rv->d_rirs = nullptr;
  rv->d_tw = rv->d_G = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_reverb_read_spectra(const mp3g_reverb* rv, float* spectra) {
  if (!rv || !spectra) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (rv->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "reverb: a host-only object");
  DeviceScope scope(rv->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  const hipError_t e = hipMemcpy(spectra, rv->d_G, rv->G.size() * sizeof(StftC), hipMemcpyDeviceToHost);
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "reverb spectra", e);
}

extern "C" int mp3g_row_power_rows(int device, const float* d_x, uint32_t n_rows, uint32_t T,
                                   const uint32_t* d_lengths, void* d_scratch, double* d_power, void* hip_stream) {
  const int st = row_power_check(n_rows, T);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (n_rows == 0) return MP3G_OK;
  if (!d_power || (T && (!d_x || !d_scratch))) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "row power: null device buffer");
  if (((uintptr_t)d_x & 3u) || ((uintptr_t)d_scratch & 7u) || ((uintptr_t)d_power & 7u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "row power: a misaligned device buffer");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint32_t TB = rv_blocks(T), tiles = (TB + kRvTileBlocks - 1) / kRvTileBlocks;
  hipError_t e = hipSuccess;
  if (tiles) {  // (n_rows * TB < 2^31: row_power_check)
    sumsq_kernel<<<n_rows * tiles, kRvMixLanes, 0, stream>>>(d_x, T, d_lengths, 1, static_cast<double*>(d_scratch), TB,
                                                             tiles);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "row power launch", e);
  }
  row_power_kernel<<<(n_rows + 255) / 256, 256, 0, stream>>>(static_cast<const double*>(d_scratch), TB, d_lengths, T,
                                                             n_rows, d_power);
  e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "row power fold launch", e);
}

namespace {
// the launches of mp3g_augment_rows whose bit is set in `launches` (all: 31)
int augment_launch(const mp3g_reverb* rv, int device, const mp3g_augment_args* d_args, const int32_t* rir_index,
                   const uint32_t* noise_lengths, const mp3g_augment_slot* slots, void* d_scratch,
                   uint64_t scratch_bytes, void* hip_stream, uint32_t launches) {
  bool work = false;
  int st = augment_check(rv, d_args, &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (rv && rv->device != device) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: the object is of another device");
  if (!work) return MP3G_OK;
  const mp3g_augment_args& a = *d_args;
  if ((a.rir_index && !rir_index) || (a.A && !slots))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: a device table without its host copy");
  if (!a.rir_index) rir_index = nullptr;
  st = augment_check_refs(rv, d_args, rir_index, noise_lengths, slots);
  if (st != MP3G_OK) return st;
  if (a.A && a.noise && (!a.noise_lengths || !a.noise_power))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: null device buffer");
  const uint64_t planes = (uint64_t)a.n_rows * a.n_planes;
  const RvLayout l = rv_layout(rv ? rv->Lmax : 0, planes, a.T);
  if (!d_scratch || scratch_bytes < l.bytes)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: no scratch, or less than mp3g_reverb_scratch_bytes");
  if (((uintptr_t)a.x & 3u) || ((uintptr_t)a.out & 3u) || ((uintptr_t)d_scratch & 7u) || ((uintptr_t)a.stats & 7u) ||
      ((uintptr_t)a.slots & 7u) || ((uintptr_t)a.noise_power & 7u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: a misaligned device buffer");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  RvDev d = {};
  double* dbl = static_cast<double*>(d_scratch);
  d.pb = dbl + l.pb;
  d.pv = dbl + l.pv;
  d.pe = dbl + l.pe;
  d.spectra = reinterpret_cast<StftC*>(static_cast<unsigned char*>(d_scratch) + l.spectra);
  d.TB = l.TB;
  d.KB = l.KB;
  d.MB = l.MB;
  bool reverberate = false;
  if (rv && rir_index)
    for (uint32_t r = 0; r < a.n_rows && !reverberate; r++) reverberate = rir_index[r] >= 0;
  if (rv) {
    d.rirs = rv->d_rirs;
    d.tw = rv->d_tw;
    d.G = rv->d_G;
    d.R = rv->R;
  }
  const uint32_t tiles = (l.TB + kRvTileBlocks - 1) / kRvTileBlocks;  // (planes * (KB + TB + 2) < 2^31: the check)
  if (!reverberate) d.R = 0;  // (no row has a response: the mix reads x)
  const char* what = "augment power launch";
  if (launches & 1u)
    sumsq_kernel<<<(uint32_t)(planes * tiles), kRvMixLanes, 0, stream>>>(a.x, a.T, a.lengths, a.n_planes, d.pb, l.TB,
                                                                        tiles);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && reverberate && (launches & 2u)) {
    what = "augment forward launch";
    forward_kernel<<<(uint32_t)(planes * l.MB), kRvFftLanes, 0, stream>>>(a, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess && reverberate && (launches & 4u)) {
    what = "augment convolve launch";
    convolve_kernel<<<(uint32_t)(planes * l.KB), kRvFftLanes, 0, stream>>>(a, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess && (launches & 8u)) {
    what = "augment mix launch";
    mix_kernel<<<(uint32_t)(planes * tiles), kRvMixLanes, 0, stream>>>(a, d, tiles);
    e = hipGetLastError();
  }
  if (e == hipSuccess && (launches & 16u)) {
    what = "augment scale launch";
    scale_kernel<<<(uint32_t)(planes * tiles), kRvMixLanes, 0, stream>>>(a, d, tiles);
    e = hipGetLastError();
  }
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, what, e);
}
}  // namespace

extern "C" int mp3g_augment_rows(const mp3g_reverb* rv, int device, const mp3g_augment_args* d_args,
                                 const int32_t* rir_index, const uint32_t* noise_lengths,
                                 const mp3g_augment_slot* slots, void* d_scratch, uint64_t scratch_bytes,
                                 void* hip_stream) {
  return augment_launch(rv, device, d_args, rir_index, noise_lengths, slots, d_scratch, scratch_bytes, hip_stream, 31u);
}

extern "C" int mp3g_augment_debug_launch(const mp3g_reverb* rv, int device, const mp3g_augment_args* d_args,
                                         const int32_t* rir_index, const uint32_t* noise_lengths,
                                         const mp3g_augment_slot* slots, void* d_scratch, uint64_t scratch_bytes,
                                         void* hip_stream, uint32_t which) {
  if (which > 4) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "augment: launches are 0 .. 4");
  return augment_launch(rv, device, d_args, rir_index, noise_lengths, slots, d_scratch, scratch_bytes, hip_stream,
                        1u << which);
}
