// fbank.hip -- device side of the Kaldi filter-bank features (include/mp3g.h
// "Kaldi filter-bank features of decoded rows"): the table upload and
// mp3g_fbank_execute.  A translation unit of its own: the listings of the
// decode kernels, the resampler and the log-mel features do not see it.
//
// Shape: log-mel's (logmel.hip).  One workgroup produces tile_frames
// consecutive frames of one (row, plane).  The tile's source span
// (tile_frames - 1) hop + n_pad is staged into LDS once with coalesced loads,
// already multiplied by `scale` (s = scale x, the contract's one multiply) and
// with Kaldi's reflection resolved; sample j sits at word j + (j >> skew).  The
// STFT is a GEMM on v_mfma_f32_32x32x2_f32 with the windowed DFT table streamed
// from global memory (L2) in the layout of fbank_device_table, a wave per tile
// of 32 bins holding its cos and sin accumulators, eight steps to a pass.
//
// What differs is the A operand: e[frame][n], the frame after DC removal and
// pre-emphasis, not a Hankel view of the samples.  A lane's frame is fixed
// (lane & 31), so it keeps its frame's mean in a register and forms
//   e[n] = fmaf(-preemph, fmaf(mean, -1, s[n-1]), fmaf(mean, -1, s[n]))
// from two LDS reads and three FMAs per operand (n = 0 reads s[0] twice): the
// same operations on the same values as the host's arrays d and e.  The mean is
// the contract's ascending chain of N additions, one lane per frame on the
// VALU; every wave runs it for its own lanes (no exchange, no barrier).  Without
// MP3G_FBANK_REMOVE_DC the mean is +0 and fmaf(+0, -1, s) = s + -0 = s, bit for
// bit, so the operand code is the same.
//
// The window length need not be a multiple of the pass granularity (551 samples
// is 25 ms at 22.05 kHz): the table has zero rows up to n_pad (fbank_tables.cpp
// says why they leave the accumulators' bits alone) and the operands read for
// n >= N are staged samples or staged zeros, so finite.
//
// p = fmaf(re, re, im * im) goes to LDS as [bin][33].  In the mel stage the
// lanes run along m for a frame, so a store is contiguous along mel_stride
// (time-major output).  A lane walks its own support: the p reads are a gather.
// A 32-bit LDS read has 32 banks and word k * 33 + f lies on bank (k + f) mod
// 32, so two lanes of one frame collide when their bins differ by a multiple of
// 32 -- not at all where neighbouring supports start a bin or two apart, a few
// ways at the top of the bank where they start eight or more apart -- and lanes
// on the same bin read one word (a broadcast).  The stage is 0.3 % of the
// kernel's multiply-adds, so the stride was kept.  Then mp3g_logf on the VALU.
// No clamp, no atomics, one launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "fbank.h"
#include "fbank_log.h"

namespace mp3g {
namespace {

constexpr uint32_t kMaxLanes = 64 * kLogmelMaxWaves;
constexpr uint32_t kMaxPlanesPerLaunch = 32768;
// the largest dynamic LDS any configuration asks for (P = 1024: 512 bins, at most 1,024 weights)
constexpr uint32_t kMaxLdsBytes = (kLogmelStageFloats + (MP3G_FBANK_MAX_WINDOW / 2) * (kLogmelPStride + 2)) * 4;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct FbankArgs {
  const float* dft;         // fbank_device_table
  const float* wm;          // fbank_device_filters: the weights ...
  const uint32_t* support;  // ... and [n_mels][3] = lo, hi, offset
  uint32_t N, n_pad, hop, n_mels, K, tile_frames, span, skew, stage, tiles, n_weights, remove_dc, reflect;
  int32_t shift;            // frame 0's first sample: 0, or hop / 2 - N / 2 without SNIP_EDGES
  float scale, npre, rN;    // npre = -preemph
};

// S steps of one bin tile: the operands of all of them, then the MFMAs in
// ascending n.  j is the lane's sample of step 0 in the stage, first whether it
// is n = 0 of its frame (whose predecessor is itself).
template <int S>
__device__ inline void dft_pass(const float* s_x, uint32_t j, bool first, uint32_t skew, float mean, float npre,
                                const float* __restrict__ b, size_t step, f32x16& re, f32x16& im) {
  float e[S], vc[S], vs[S];
#pragma unroll
  for (int t = 0; t < S; t++) {
    const uint32_t jc = j + 2 * t, jp = jc - ((t == 0 && first) ? 0u : 1u);
    const float dc = __builtin_fmaf(mean, -1.0f, s_x[jc + (jc >> skew)]);
    const float dp = __builtin_fmaf(mean, -1.0f, s_x[jp + (jp >> skew)]);
    e[t] = __builtin_fmaf(npre, dp, dc);
    vc[t] = b[t * step];
    vs[t] = b[t * step + 64];
  }
  // (left alone, the scheduler feeds two registers one step ahead of the MFMAs)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < S; t++) {
    re = __builtin_amdgcn_mfma_f32_32x32x2f32(e[t], vc[t], re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_32x32x2f32(e[t], vs[t], im, 0, 0, 0);
  }
}

__global__ __launch_bounds__(kMaxLanes) void fbank_kernel(const float* __restrict__ src, uint32_t T,
                                                       float* __restrict__ out, uint32_t n_frames,
                                                       uint32_t mel_stride, FbankArgs a, uint32_t plane0) {
  extern __shared__ float smem[];
  float* s_x = smem;                         // [stage]
  float* s_p = smem + a.stage;               // [K][33]
  float* s_w = s_p + a.K * kLogmelPStride;   // [n_weights]
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lanes = blockDim.x;
  const uint32_t f0 = blockIdx.x * a.tile_frames;  // < n_frames (the grid)
  const size_t plane = (size_t)plane0 + blockIdx.y;
  const float* __restrict__ srow = src + plane * T;
  float* __restrict__ orow = out + plane * n_frames * mel_stride;

  // s = scale x over samples [f0 hop + shift, .. + span) of the row, reflected
  // Kaldi's way about its ends (what a stored frame reads is inside the row
  // after one reflection: fbank_tables.cpp; anything else -- frames past the
  // last available one and the n >= N padding, computed but never stored or
  // multiplied by zero taps -- reads zeros)
  const int64_t base = (int64_t)f0 * a.hop + a.shift;
  const int64_t len = (int64_t)T;  // (T >= N: the row has a frame)
  for (uint32_t i0 = tid; i0 < a.span; i0 += 8 * lanes) {
    // eight unconditional loads at clamped indices in flight, then the stores
    float v[8];
    bool in[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) {
      int64_t j = base + (int64_t)(i0 + u * lanes);
      if (a.reflect) {
        j = j < 0 ? -j - 1 : j;
        j = j >= len ? 2 * len - 1 - j : j;
      }
      in[u] = j >= 0 && j < len;
      v[u] = srow[min(max(j, (int64_t)0), len - 1)];
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) {
      const uint32_t i = i0 + u * lanes;
      if (i < a.span) s_x[i + (i >> a.skew)] = in[u] ? a.scale * v[u] : 0.f;
    }
  }
  for (uint32_t i = tid; i < a.n_weights; i += lanes) s_w[i] = a.wm[i];
  __syncthreads();

  // lane l holds A[frame l & 31][n = 2 n2 + (l >> 5)] and B[that n][bin l & 31]
  const uint32_t col = lane & 31, half = lane >> 5;
  const uint32_t jf = min(col, a.tile_frames - 1) * a.hop;  // the lane's frame in the stage
  // the frame's mean: sum = fmaf(s[n], 1, sum) over n ascending, times rN
  float mean = 0.f;
  if (a.remove_dc) {
    // Sixteen samples from a multiple of 16 share their pad offset (a pad word
    // comes every 2^skew >= 16 samples): one address, sixteen reads at constant
    // offsets.  The samples before the first such block and after the last are
    // read one by one.  The order is ascending throughout.
    float sum = 0.f;
    uint32_t j = jf;
    const uint32_t jend = jf + a.N, jhead = min(jend, (jf + 15) & ~15u);
    for (; j < jhead; j++) sum = __builtin_fmaf(s_x[j + (j >> a.skew)], 1.0f, sum);
    for (; j + 16 <= jend; j += 16) {
      const float* p = s_x + j + (j >> a.skew);
      float s[16];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) s[u] = p[u];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) sum = __builtin_fmaf(s[u], 1.0f, sum);
    }
    for (; j < jend; j++) sum = __builtin_fmaf(s_x[j + (j >> a.skew)], 1.0f, sum);
    mean = sum * a.rN;
  }

  // the STFT of e
  const uint32_t j0 = jf + half;  // the lane's sample of step 0
  const uint32_t n2s = a.n_pad / 2;
  const size_t step = (size_t)a.tiles * 128;
  for (uint32_t tile = wave; tile < a.tiles; tile += lanes / 64) {
    const float* __restrict__ b = a.dft + (size_t)tile * 128 + lane;
    f32x16 re = {}, im = {};
    uint32_t n2 = 0;
    for (; n2 + 8 <= n2s; n2 += 8, b += 8 * step)
      dft_pass<8>(s_x, j0 + 2 * n2, n2 == 0 && half == 0, a.skew, mean, a.npre, b, step, re, im);
    for (; n2 < n2s; n2 += 2, b += 2 * step)  // (n_pad = 0 mod 4)
      dft_pass<2>(s_x, j0 + 2 * n2, n2 == 0 && half == 0, a.skew, mean, a.npre, b, step, re, im);
    // D[frame][bin]: bin = lane & 31, frame = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t k = tile * 32 + col;
    if (k < a.K) {
#pragma unroll
      for (uint32_t r = 0; r < 16; r++)
        s_p[k * kLogmelPStride + (r & 3) + 8 * (r >> 2) + 4 * half] = __builtin_fmaf(re[r], re[r], im[r] * im[r]);
    }
  }
  __syncthreads();

  // mel, log: item i = (frame, m), m fastest, so a wave's stores are contiguous along mel_stride
  const uint32_t valid = min(a.tile_frames, n_frames - f0);
  for (uint32_t i = tid; i < valid * a.n_mels; i += lanes) {
    const uint32_t f = i / a.n_mels, m = i - f * a.n_mels;
    const uint32_t lo = a.support[3 * m], hi = a.support[3 * m + 1];
    const float* w = s_w + a.support[3 * m + 2] - lo;  // w[k], k in [lo, hi]
    const float* p = s_p + f;
    float mel = 0.f;
    for (uint32_t k = lo; k <= hi; k++) mel = __builtin_fmaf(w[k], p[k * kLogmelPStride], mel);
    orow[(size_t)(f0 + f) * mel_stride + m] = fbank_log(mel);
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
uint32_t lds_bytes(const mp3g_fbank& fb) {
  return (fb.geom.stage + fb.K * kLogmelPStride + fb.n_weights) * (uint32_t)sizeof(float);
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

int fbank_device_upload(mp3g_fbank* fb) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || fb->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "fbank: no such device");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, fb->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  std::vector<float> table, weights;
  std::vector<uint32_t> support;
  fbank_device_table(*fb, &table);
  fbank_device_filters(*fb, &weights, &support);
  fb->n_weights = (uint32_t)weights.size();
  if (lds_bytes(*fb) > kMaxLdsBytes) return abi_fail(MP3G_ERR_UNSUPPORTED, "fbank: filters too wide for the LDS");
  DeviceScope scope(fb->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  // (the long transforms stage more than the 64 KB a kernel gets by default)
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(fbank_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)kMaxLdsBytes);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "hipFuncSetAttribute(fbank)", e);
  int st = upload(table, reinterpret_cast<void**>(&fb->d_dft), "fbank DFT table");
  if (st == MP3G_OK) st = upload(weights, reinterpret_cast<void**>(&fb->d_wm), "fbank mel weights");
  if (st == MP3G_OK) st = upload(support, reinterpret_cast<void**>(&fb->d_support), "fbank supports");
  if (st != MP3G_OK) fbank_device_free(fb);
  return st;
}

void fbank_device_free(mp3g_fbank* fb) {
  DeviceScope scope(fb->device);
  (void)hipFree(fb->d_dft);
  (void)hipFree(fb->d_wm);
  (void)hipFree(fb->d_support);
  fb->d_dft = fb->d_wm = nullptr;
  fb->d_support = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_fbank_execute(const mp3g_fbank* fb, const float* d_src, uint32_t n_rows, uint32_t n_planes,
                                  uint32_t T, float* d_out, uint32_t n_frames, uint32_t mel_stride,
                                  void* hip_stream) {
  if (!fb) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null fbank");
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: 1 or 2 planes");
  if (fb->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: a host-only object");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "fbank: rows of 2^31 samples or more");
  if (n_frames > mp3g_fbank_frames(fb, T))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: more frames than the rows have");
  if (mel_stride < fb->n_mels) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: mel stride below n_mels");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes >= (1ull << 32)) return abi_fail(MP3G_ERR_UNSUPPORTED, "fbank: 2^32 planes or more");
  if (planes == 0 || n_frames == 0) return MP3G_OK;
  if (!d_src || !d_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  DeviceScope scope(fb->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const FbankGeom& g = fb->geom;
  const bool snip = fb->flags & MP3G_FBANK_SNIP_EDGES;
  FbankArgs a = {};
  a.dft = fb->d_dft;
  a.wm = fb->d_wm;
  a.support = fb->d_support;
  a.N = fb->N;
  a.n_pad = g.n_pad;
  a.hop = fb->hop;
  a.n_mels = fb->n_mels;
  a.K = fb->K;
  a.tile_frames = g.tile_frames;
  a.span = g.span;
  a.skew = g.skew;
  a.stage = g.stage;
  a.tiles = g.tiles;
  a.n_weights = fb->n_weights;
  a.remove_dc = (fb->flags & MP3G_FBANK_REMOVE_DC) ? 1u : 0u;
  a.reflect = snip ? 0u : 1u;
  a.shift = snip ? 0 : (int32_t)(fb->hop / 2) - (int32_t)(fb->N / 2);
  a.scale = fb->scale;
  a.npre = -fb->preemph;
  a.rN = fb->rN;
  const uint32_t tiles = (n_frames + g.tile_frames - 1) / g.tile_frames;
  // (one launch for up to 32,768 planes: the grid's second dimension)
  for (uint64_t base = 0; base < planes; base += kMaxPlanesPerLaunch) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(planes - base, kMaxPlanesPerLaunch);
    fbank_kernel<<<dim3(tiles, n), 64 * g.waves, lds_bytes(*fb), stream>>>(d_src, T, d_out, n_frames, mel_stride, a,
                                                                     (uint32_t)base);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "fbank launch", e);
  }
  return MP3G_OK;
}
