// logmel.hip -- device side of the log-mel features (include/mp3g.h "log-mel
// features of decoded rows"): the table upload and mp3g_logmel_execute.  A
// translation unit of its own: the decode kernels' listings (kernels.hip,
// kernels_fast.hip) do not see it.
//
// Shape.  One workgroup produces tile_frames consecutive frames of one (row,
// plane).  The tile's source span (tile_frames - 1) hop + n_fft is staged into
// LDS once with coalesced loads, the reflection about the row's ends resolved
// while staging; sample j sits at word j + (j >> skew) (logmel.h: the pad words
// spread the A operand's lanes over the banks).  The STFT is a GEMM on
// v_mfma_f32_32x32x2_f32: A[frame][n] is the Hankel view of the stage, B[n][bin]
// the windowed DFT table from global memory (L2) in the layout of
// logmel_device_table -- one 256-byte run per operand.  A step covers n = 2 n2
// and 2 n2 + 1 in that order and the steps ascend, and the instruction is a
// k-ordered float32 FMA chain, so every accumulator is the contract's chain.
// A wave holds the cos and sin accumulators of one tile of 32 bins (one A read
// for two MFMAs; a workgroup has a wave per bin tile, eight at most): a lane has
// re and im of the same (frame, bin) and forms p = fmaf(re, re, im * im) in
// registers.  Eight steps make a pass: their 24 loads issue before the first
// of the 16 MFMAs, so one memory latency is paid per 1,024 matrix-core cycles.
// p goes to LDS as [bin][33] (frames along a row, the odd stride keeps the
// lanes' writes on distinct banks); the mel stage is the sparse chain over each
// filter's support, its weights staged in LDS, 32 frames to a half wave, then
// mp3g_log10f on the VALU and stores that are contiguous along frames.  With
// MP3G_LOGMEL_CLAMP a wave also folds its features' maximum into the plane's
// word of d_max with one atomicMax on ordered integers (max is exact: the order
// does not matter), and a pointwise kernel behind it applies the clamp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "logmel.h"
#include "logmel_log10.h"

namespace mp3g {
namespace {

constexpr uint32_t kLanes = 256;                       // the clamp kernel's workgroup
constexpr uint32_t kMaxLanes = 64 * kLogmelMaxWaves;  // the feature kernel's, at most
constexpr uint32_t kMaxPlanesPerLaunch = 32768;
// the largest dynamic LDS any configuration asks for (n_fft = 1024)
constexpr uint32_t kMaxLdsBytes = (kLogmelStageFloats + (MP3G_LOGMEL_MAX_FFT / 2 + 1) * (kLogmelPStride + 2)) * 4;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LogmelArgs {
  const float* dft;         // logmel_device_table
  const float* wm;          // logmel_device_filters: the weights ...
  const uint32_t* support;  // ... and [n_mels][3] = lo, hi, offset
  uint32_t* plane_max;      // MP3G_LOGMEL_CLAMP: one word per plane of the launch, else null
  uint32_t n_fft, hop, n_mels, K, tile_frames, span, skew, stage, tiles, n_weights, center;
};

// float -> unsigned, monotonic (0 lies below every float), and back
__device__ inline uint32_t ordered(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ inline float unordered(uint32_t k) {
  return __builtin_bit_cast(float, k & 0x80000000u ? k ^ 0x80000000u : ~k);
}

// S steps of one bin tile: the loads of all of them, then the MFMAs in ascending n
template <int S>
__device__ inline void dft_pass(const float* s_x, uint32_t j, uint32_t skew, const float* __restrict__ b, size_t step,
                                f32x16& re, f32x16& im) {
  float x[S], vc[S], vs[S];
#pragma unroll
  for (int t = 0; t < S; t++) {
    const uint32_t jt = j + 2 * t;
    x[t] = s_x[jt + (jt >> skew)];
    vc[t] = b[t * step];
    vs[t] = b[t * step + 64];
  }
  // (left alone, the scheduler feeds two registers one step ahead of the MFMAs)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < S; t++) {
    re = __builtin_amdgcn_mfma_f32_32x32x2f32(x[t], vc[t], re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_32x32x2f32(x[t], vs[t], im, 0, 0, 0);
  }
}

__global__ __launch_bounds__(kMaxLanes) void logmel_kernel(const float* __restrict__ src, uint32_t T,
                                                        float* __restrict__ out, uint32_t n_frames,
                                                        uint32_t frame_stride, LogmelArgs a, uint32_t plane0) {
  extern __shared__ float smem[];
  float* s_x = smem;                         // [stage]
  float* s_p = smem + a.stage;               // [K][33]
  float* s_w = s_p + a.K * kLogmelPStride;   // [n_weights]
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lanes = blockDim.x;
  const uint32_t f0 = blockIdx.x * a.tile_frames;  // < n_frames (the grid)
  const size_t plane = (size_t)plane0 + blockIdx.y;
  const float* __restrict__ srow = src + plane * T;
  float* __restrict__ orow = out + plane * a.n_mels * frame_stride;

  // samples [f0 hop - pad, .. + span) of the row, reflected about its ends (a
  // frame past the last available one -- computed, never stored -- reads zeros)
  const int64_t base = (int64_t)f0 * a.hop - (a.center ? (int64_t)(a.n_fft / 2) : 0);
  const int64_t last = (int64_t)T - 1;  // (T >= 1: the row has a frame)
  for (uint32_t i0 = tid; i0 < a.span; i0 += 8 * lanes) {
    // eight unconditional loads at clamped indices in flight, then the stores
    float v[8];
    bool in[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) {
      int64_t j = base + (int64_t)(i0 + u * lanes);
      if (a.center) {
        j = j < 0 ? -j : j;
        j = j > last ? 2 * last - j : j;
      }
      in[u] = j >= 0 && j <= last;
      v[u] = srow[min(max(j, (int64_t)0), last)];
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) {
      const uint32_t i = i0 + u * lanes;
      if (i < a.span) s_x[i + (i >> a.skew)] = in[u] ? v[u] : 0.f;
    }
  }
  for (uint32_t i = tid; i < a.n_weights; i += lanes) s_w[i] = a.wm[i];
  __syncthreads();

  // the STFT: lane l holds A[frame l & 31][n = 2 n2 + (l >> 5)] and B[that n][bin l & 31]
  const uint32_t col = lane & 31, half = lane >> 5;
  const uint32_t j0 = min(col, a.tile_frames - 1) * a.hop + half;  // the lane's sample of step 0
  const uint32_t n2s = a.n_fft / 2;
  const size_t step = (size_t)a.tiles * 128;
  for (uint32_t tile = wave; tile < a.tiles; tile += lanes / 64) {
    const float* __restrict__ b = a.dft + (size_t)tile * 128 + lane;
    f32x16 re = {}, im = {};
    uint32_t n2 = 0;
    for (; n2 + 8 <= n2s; n2 += 8, b += 8 * step) dft_pass<8>(s_x, j0 + 2 * n2, a.skew, b, step, re, im);
    for (; n2 < n2s; n2 += 2, b += 2 * step) dft_pass<2>(s_x, j0 + 2 * n2, a.skew, b, step, re, im);  // (n_fft = 0 mod 4)
    // D[frame][bin]: bin = lane & 31, frame = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t k = tile * 32 + col;
    if (k < a.K) {
#pragma unroll
      for (uint32_t r = 0; r < 16; r++)
        s_p[k * kLogmelPStride + (r & 3) + 8 * (r >> 2) + 4 * half] = __builtin_fmaf(re[r], re[r], im[r] * im[r]);
    }
  }
  __syncthreads();

  // mel, log: lane (m, f), 32 frames along a half wave
  const uint32_t f = tid & 31;
  const bool store = f < a.tile_frames && f0 + f < n_frames;
  uint32_t top = 0;  // ordered(the largest feature this lane stored)
  for (uint32_t m = tid >> 5; m < a.n_mels; m += lanes / 32) {
    const uint32_t lo = a.support[3 * m], hi = a.support[3 * m + 1];
    const float* w = s_w + a.support[3 * m + 2] - lo;  // w[k], k in [lo, hi]
    const float* p = s_p + f;
    float mel = 0.f;
#pragma unroll 4
    for (uint32_t k = lo; k <= hi; k++) mel = __builtin_fmaf(w[k], p[k * kLogmelPStride], mel);
    const float y = logmel_log(mel);
    if (store) {
      orow[(size_t)m * frame_stride + f0 + f] = y;
      top = max(top, ordered(y));
    }
  }
  if (a.plane_max) {
    for (uint32_t d = 32; d; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d));
    if (lane == 0 && top) atomicMax(a.plane_max + blockIdx.y, top);
  }
}

// Whisper's normalisation: y <- (max(y, max y - 8) + 4) / 4, the plane's maximum from the kernel above
__global__ __launch_bounds__(kLanes) void logmel_clamp_kernel(float* __restrict__ out, uint32_t n_mels,
                                                              uint32_t n_frames, uint32_t frame_stride,
                                                              const uint32_t* __restrict__ plane_max,
                                                              uint32_t plane0) {
  const uint32_t f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= n_frames) return;
  float* __restrict__ orow = out + ((size_t)plane0 + blockIdx.y) * n_mels * frame_stride + f;
  const float mx = unordered(plane_max[blockIdx.y]);
  for (uint32_t m = blockIdx.z; m < n_mels; m += gridDim.z) {
    float* y = orow + (size_t)m * frame_stride;
    *y = logmel_clamp(*y, mx);
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

// the kernel's dynamic LDS: the stage, the power rows, the filters' weights
uint32_t lds_bytes(const mp3g_logmel& lm) {
  return (lm.geom.stage + lm.K * kLogmelPStride + lm.n_weights) * (uint32_t)sizeof(float);
}

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

int logmel_device_upload(mp3g_logmel* lm) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || lm->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "logmel: no such device");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, lm->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  std::vector<float> table, weights;
  std::vector<uint32_t> support;
  logmel_device_table(*lm, &table);
  logmel_device_filters(*lm, &weights, &support);
  lm->n_weights = (uint32_t)weights.size();
  if (lds_bytes(*lm) > kMaxLdsBytes) return abi_fail(MP3G_ERR_UNSUPPORTED, "logmel: filters too wide for the LDS");
  DeviceScope scope(lm->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  // (the long transforms stage more than the 64 KB a kernel gets by default)
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(logmel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)kMaxLdsBytes);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "hipFuncSetAttribute(logmel)", e);
  int st = upload(table, reinterpret_cast<void**>(&lm->d_dft), "logmel DFT table");
  if (st == MP3G_OK) st = upload(weights, reinterpret_cast<void**>(&lm->d_wm), "logmel mel weights");
  if (st == MP3G_OK) st = upload(support, reinterpret_cast<void**>(&lm->d_support), "logmel supports");
  if (st == MP3G_OK && (lm->flags & MP3G_LOGMEL_CLAMP)) {
    e = hipMalloc(reinterpret_cast<void**>(&lm->d_max), kMaxPlanesPerLaunch * sizeof(uint32_t));
    if (e != hipSuccess) {
      lm->d_max = nullptr;
      st = hip_fail(MP3G_ERR_OUT_OF_MEMORY, "logmel maxima", e);
    }
  }
  if (st != MP3G_OK) logmel_device_free(lm);
  return st;
}

void logmel_device_free(mp3g_logmel* lm) {
  DeviceScope scope(lm->device);
  (void)hipFree(lm->d_dft);
  (void)hipFree(lm->d_wm);
  (void)hipFree(lm->d_support);
  (void)hipFree(lm->d_max);
  lm->d_dft = lm->d_wm = nullptr;
  lm->d_support = lm->d_max = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_logmel_execute(const mp3g_logmel* lm, const float* d_src, uint32_t n_rows, uint32_t n_planes,
                                   uint32_t T, float* d_out, uint32_t n_frames, uint32_t frame_stride,
                                   void* hip_stream) {
  if (!lm) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null logmel");
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: 1 or 2 planes");
  if (lm->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: a host-only object");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "logmel: rows of 2^31 samples or more");
  if (n_frames > mp3g_logmel_frames(lm, T))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: more frames than the rows have");
  if (frame_stride < n_frames) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: frame stride below n_frames");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes >= (1ull << 32)) return abi_fail(MP3G_ERR_UNSUPPORTED, "logmel: 2^32 planes or more");
  if (planes == 0 || n_frames == 0) return MP3G_OK;
  if (!d_src || !d_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  DeviceScope scope(lm->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const LogmelGeom& g = lm->geom;
  const bool clamp = lm->flags & MP3G_LOGMEL_CLAMP;
  const LogmelArgs a = {lm->d_dft, lm->d_wm, lm->d_support, clamp ? lm->d_max : nullptr,
                        lm->n_fft, lm->hop,  lm->n_mels,    lm->K,
                        g.tile_frames, g.span, g.skew, g.stage,
                        g.tiles, lm->n_weights, (lm->flags & MP3G_LOGMEL_CENTER) ? 1u : 0u};
  const uint32_t tiles = (n_frames + g.tile_frames - 1) / g.tile_frames;
  for (uint64_t base = 0; base < planes; base += kMaxPlanesPerLaunch) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(planes - base, kMaxPlanesPerLaunch);
    hipError_t e = clamp ? hipMemsetAsync(lm->d_max, 0, n * sizeof(uint32_t), stream) : hipSuccess;
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "logmel maxima reset", e);
    logmel_kernel<<<dim3(tiles, n), 64 * g.waves, lds_bytes(*lm), stream>>>(d_src, T, d_out, n_frames, frame_stride, a,
                                                                      (uint32_t)base);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "logmel launch", e);
    if (clamp) {
      logmel_clamp_kernel<<<dim3((n_frames + kLanes - 1) / kLanes, n, 8), kLanes, 0, stream>>>(
          d_out, lm->n_mels, n_frames, frame_stride, lm->d_max, (uint32_t)base);
      e = hipGetLastError();
      if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "logmel clamp launch", e);
    }
  }
  return MP3G_OK;
}
