// resample.hip -- device side of the polyphase resampler (include/mp3g.h
// "sample-rate conversion of decoded rows"): the table upload and
// mp3g_resample_rows.  A translation unit of its own: the decode kernels'
// listings (kernels.hip, kernels_fast.hip) do not see it.
//
// The kernel computes y[n] = one float32 FMA chain over the 2W taps in
// ascending k, exactly as mp3g_resample_host does -- explicit fused
// multiply-adds (the build keeps -ffp-contract=off), float32 subnormals kept
// (the compiler's default for kernels) -- so its output equals the host
// reference bit for bit whatever the tiling.
//
// Shape.  One workgroup produces a tile of consecutive outputs of one (row,
// plane).  The source span the tile reads, (tile - 1) M / L + 2W samples, is
// staged into LDS with coalesced loads and zero-filled outside the row's valid
// range (a tap on a zero is bit-neutral: the accumulator never holds -0).
// The table is read in the permuted, transposed layout H'[k][n mod L]
// (resample.h), so the lanes of a wave read consecutive words of a row of H';
// a table of at most kTapsLdsFloats entries (L = 1, 2: 48 -> 16 kHz, 24 -> 16
// kHz, ...) is staged into LDS as well, where a wave's one or two distinct
// words per tap broadcast.  (q, r) of the tile's first output come from 64-bit
// arithmetic once per workgroup; the lanes add 32-bit offsets.
//
// Two kernels (resample.h resample_geometry picks).  The phase-grouped one --
// every MP3 rate pair -- gives a lane four outputs S = m L apart: the same
// phase, so one tap load feeds four independent chains, two packed FMAs.  The
// generic one (L > 512, or a span too long for the stage at that tile) gives
// a lane outputs t and t + 256 of a 512-output tile, one packed FMA per tap
// and two tap loads; when even its span does not fit the stage (extreme
// ratios) it reads the source from global memory with the same bounds checks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "resample.h"

namespace mp3g {
namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kStageFloats = kResampleStageFloats;  // 16 KB: the tile's source span
constexpr uint32_t kTapsLdsFloats = 2048;                // 8 KB: a small table
constexpr uint32_t kMaxRowsPerLaunch = 32768;
static_assert(kResampleTile == 2 * kLanes, "two outputs per lane");

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool kStage, bool kTapsLds>
__global__ __launch_bounds__(kLanes) void resample_rows_kernel(const float* __restrict__ src, uint32_t src_stride,
                                                               float* __restrict__ out, uint32_t out_stride,
                                                               const mp3g_resample_row* __restrict__ rows,
                                                               const float* __restrict__ taps, uint32_t L,
                                                               uint32_t M, uint32_t W) {
  __shared__ float s_x[kStage ? kStageFloats : 1];
  __shared__ float s_h[kTapsLds ? kTapsLdsFloats : 1];
  const mp3g_resample_row row = rows[blockIdx.y];
  const uint32_t n_out = min(row.n_out, out_stride);
  const uint32_t t0 = blockIdx.x * kResampleTile;
  if (t0 >= n_out) return;  // (uniform: before any barrier)
  const uint32_t C = gridDim.z, ch = blockIdx.z, tid = threadIdx.x;
  const uint32_t nt = min(kResampleTile, n_out - t0);
  // the tile's first output: (q0, r0) = divmod(n0 M, L), once, in 64 bits
  const uint64_t n0 = row.out_start + t0;
  const uint64_t nq = n0 / L;
  const uint32_t c0 = (uint32_t)(n0 - nq * L);
  const uint64_t cm = (uint64_t)c0 * M;
  const uint64_t q0 = nq * M + cm / L;
  const uint32_t r0 = (uint32_t)(cm % L);
  const uint32_t n_src = min(row.n_src, src_stride);
  const float* __restrict__ srow = src + ((size_t)row.src_row * C + ch) * src_stride;
  float* __restrict__ orow = out + ((size_t)row.out_row * C + ch) * out_stride + t0;
  const int64_t rel = (int64_t)q0 - (int64_t)W + 1 - (int64_t)row.src_origin;
  const uint32_t n2w = 2 * W;

  if (kStage) {
    // source samples [rel, rel + span) of the row, zero outside [0, n_src)
    const uint32_t span = (r0 + (nt - 1) * M) / L + n2w;  // <= kStageFloats (the host picked kStage)
    for (uint32_t i = tid; i < span; i += kLanes) {
      const int64_t p = rel + (int64_t)i;
      s_x[i] = p >= 0 && p < (int64_t)n_src ? srow[p] : 0.f;
    }
  }
  if (kTapsLds) {
    const uint32_t nh = L * n2w;  // <= kTapsLdsFloats
    for (uint32_t i = tid; i < nh; i += kLanes) s_h[i] = taps[i];
  }
  if (kStage || kTapsLds) __syncthreads();

  // two outputs per lane: a = tid, b = tid + 256 (a lane without one repeats output 0)
  const bool va = tid < nt, vb = tid + kLanes < nt;
  const uint32_t a = va ? tid : 0u, b = vb ? tid + kLanes : 0u;
  const uint32_t ia = (r0 + a * M) / L, ib = (r0 + b * M) / L;  // first tap, relative to `rel`
  const uint32_t ca = (c0 + a) % L, cb = (c0 + b) % L;          // column of H'
  const float* __restrict__ h = kTapsLds ? s_h : taps;
  v2f acc = {0.f, 0.f};
  if (kStage) {
    const float* xa = s_x + ia;
    const float* xb = s_x + ib;
    const float* ha = h + ca;
    const float* hb = h + cb;
#pragma unroll 4
    for (uint32_t k = 0; k < n2w; k++) {
      const v2f hv = {ha[0], hb[0]};
      const v2f xv = {xa[k], xb[k]};
      acc = __builtin_elementwise_fma(hv, xv, acc);
      ha += L;
      hb += L;
    }
  } else {
    const int64_t pa = rel + (int64_t)ia, pb = rel + (int64_t)ib;
    for (uint32_t k = 0; k < n2w; k++) {
      const int64_t ja = pa + (int64_t)k, jb = pb + (int64_t)k;
      const v2f hv = {h[(size_t)k * L + ca], h[(size_t)k * L + cb]};
      const v2f xv = {ja >= 0 && ja < (int64_t)n_src ? srow[ja] : 0.f,
                      jb >= 0 && jb < (int64_t)n_src ? srow[jb] : 0.f};
      acc = __builtin_elementwise_fma(hv, xv, acc);
    }
  }
  if (va) orow[tid] = acc.x;
  if (vb) orow[tid + kLanes] = acc.y;
}

// The phase-grouped kernel (resample.h resample_geometry): a workgroup of
// ceil(S / 64) waves produces 4 S consecutive outputs, lane t the outputs
// t + j S, j = 0..3.  S = m L, so the four share their phase -- one tap load per
// k for four chains, two packed FMAs -- and their first taps lie exactly m M
// source samples apart.  The source span is always staged (the host checked it
// fits); a lane past the tile's end computes on whatever the stage holds and
// stores nothing.
template <bool kTapsLds>
__global__ __launch_bounds__(512) void resample_rows_grouped_kernel(
    const float* __restrict__ src, uint32_t src_stride, float* __restrict__ out, uint32_t out_stride,
    const mp3g_resample_row* __restrict__ rows, const float* __restrict__ taps, uint32_t L, uint32_t M, uint32_t W,
    uint32_t m) {
  __shared__ float s_x[kStageFloats];
  __shared__ float s_h[kTapsLds ? kTapsLdsFloats : 1];
  const uint32_t S = m * L, tile = kResampleGroup * S;
  const mp3g_resample_row row = rows[blockIdx.y];
  const uint32_t n_out = min(row.n_out, out_stride);
  const uint32_t t0 = blockIdx.x * tile;
  if (t0 >= n_out) return;  // (uniform: before any barrier)
  const uint32_t C = gridDim.z, ch = blockIdx.z, tid = threadIdx.x;
  const uint32_t nt = min(tile, n_out - t0);
  const uint64_t n0 = row.out_start + t0;
  const uint64_t nq = n0 / L;
  const uint32_t c0 = (uint32_t)(n0 - nq * L);
  const uint64_t cm = (uint64_t)c0 * M;
  const uint64_t q0 = nq * M + cm / L;
  const uint32_t r0 = (uint32_t)(cm % L);
  const uint32_t n_src = min(row.n_src, src_stride);
  const float* __restrict__ srow = src + ((size_t)row.src_row * C + ch) * src_stride;
  float* __restrict__ orow = out + ((size_t)row.out_row * C + ch) * out_stride + t0;
  const int64_t rel = (int64_t)q0 - (int64_t)W + 1 - (int64_t)row.src_origin;
  const uint32_t n2w = 2 * W;

  const uint32_t span = (r0 + (nt - 1) * M) / L + n2w;  // <= kStageFloats
  for (uint32_t i = tid; i < span; i += blockDim.x) {
    const int64_t p = rel + (int64_t)i;
    s_x[i] = p >= 0 && p < (int64_t)n_src ? srow[p] : 0.f;
  }
  if (kTapsLds) {
    const uint32_t nh = L * n2w;  // <= kTapsLdsFloats
    for (uint32_t i = tid; i < nh; i += blockDim.x) s_h[i] = taps[i];
  }
  __syncthreads();

  const uint32_t t = tid < S ? tid : 0u;  // (the last wave's lanes past S repeat lane 0, and store nothing)
  const uint32_t step = m * M;            // source samples between a lane's outputs
  const float* x = s_x + (r0 + t * M) / L;  // tap 0 of output t; the last read: < the full tile's span
  const float* __restrict__ h = (kTapsLds ? s_h : taps) + (c0 + t) % L;
  v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
#pragma unroll 4
  for (uint32_t k = 0; k < n2w; k++) {
    const float hk = h[0];
    const v2f hv = {hk, hk};
    const v2f x01 = {x[k], x[k + step]};
    const v2f x23 = {x[k + 2 * step], x[k + 3 * step]};
    acc01 = __builtin_elementwise_fma(hv, x01, acc01);
    acc23 = __builtin_elementwise_fma(hv, x23, acc23);
    h += L;
  }
  if (tid < S) {
    if (t < nt) orow[t] = acc01.x;
    if (t + S < nt) orow[t + S] = acc01.y;
    if (t + 2 * S < nt) orow[t + 2 * S] = acc23.x;
    if (t + 3 * S < nt) orow[t + 3 * S] = acc23.y;
  }
}

// fi == fo: y = x (zero outside the row's valid range)
__global__ __launch_bounds__(kLanes) void resample_copy_kernel(const float* __restrict__ src, uint32_t src_stride,
                                                               float* __restrict__ out, uint32_t out_stride,
                                                               const mp3g_resample_row* __restrict__ rows) {
  const mp3g_resample_row row = rows[blockIdx.y];
  const uint32_t n_out = min(row.n_out, out_stride);
  const uint32_t t0 = blockIdx.x * kResampleTile;
  if (t0 >= n_out) return;
  const uint32_t C = gridDim.z, ch = blockIdx.z;
  const uint32_t n_src = min(row.n_src, src_stride);
  const float* __restrict__ srow = src + ((size_t)row.src_row * C + ch) * src_stride;
  float* __restrict__ orow = out + ((size_t)row.out_row * C + ch) * out_stride;
  const int64_t rel = (int64_t)row.out_start - (int64_t)row.src_origin;
  for (uint32_t i = t0 + threadIdx.x; i < min(n_out, t0 + kResampleTile); i += kLanes) {
    const int64_t p = rel + (int64_t)i;
    orow[i] = p >= 0 && p < (int64_t)n_src ? srow[p] : 0.f;
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

int resample_device_upload(mp3g_resampler* r) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || r->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "resampler: no such device");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, r->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  if (r->taps.empty()) return MP3G_OK;  // a copy needs no table
  std::vector<float> perm;
  resample_permute_taps(*r, &perm);
  DeviceScope scope(r->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  e = hipMalloc(&r->d_taps, perm.size() * sizeof(float));
  if (e != hipSuccess) {
    r->d_taps = nullptr;
    return hip_fail(MP3G_ERR_OUT_OF_MEMORY, "hipMalloc(resampler table)", e);
  }
  e = hipMemcpy(r->d_taps, perm.data(), perm.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(r->d_taps);
    r->d_taps = nullptr;
    return hip_fail(MP3G_ERR_DEVICE, "hipMemcpy(resampler table)", e);
  }
  return MP3G_OK;
}

void resample_device_free(mp3g_resampler* r) {
  DeviceScope scope(r->device);
  (void)hipFree(r->d_taps);
  r->d_taps = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_resample_rows(const mp3g_resampler* r, const float* d_src, uint32_t src_stride, float* d_out,
                                  uint32_t out_stride, uint32_t n_channels, const mp3g_resample_row* d_rows,
                                  uint32_t n_rows, void* hip_stream) {
  if (!r) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null resampler");
  if (n_channels != 1 && n_channels != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "resample: 1 or 2 channels");
  if (r->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "resample: a host-only resampler");
  if (n_rows == 0 || out_stride == 0) return MP3G_OK;
  if (!d_src || !d_out || !d_rows) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  DeviceScope scope(r->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint32_t L = r->L, M = r->M, W = r->W;
  // which kernel, and whether the table fits its stage too
  const ResampleGeom geo = resample_geometry(L, M, W);
  const uint32_t tiles = (uint32_t)(((uint64_t)out_stride + geo.tile - 1) / geo.tile);
  const bool stage = geo.staged;
  const bool taps_lds = (uint64_t)L * 2u * W <= kTapsLdsFloats;
  const uint32_t group_lanes = (geo.S + 63u) & ~63u;
  for (uint32_t base = 0; base < n_rows; base += kMaxRowsPerLaunch) {
    const dim3 grid(tiles, std::min(n_rows - base, kMaxRowsPerLaunch), n_channels);
    const mp3g_resample_row* rows = d_rows + base;
    if (W == 0)
      resample_copy_kernel<<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, rows);
    else if (geo.grouped && taps_lds)
      resample_rows_grouped_kernel<true><<<grid, group_lanes, 0, stream>>>(d_src, src_stride, d_out, out_stride,
                                                                           rows, r->d_taps, L, M, W, geo.m);
    else if (geo.grouped)
      resample_rows_grouped_kernel<false><<<grid, group_lanes, 0, stream>>>(d_src, src_stride, d_out, out_stride,
                                                                            rows, r->d_taps, L, M, W, geo.m);
    else if (stage && taps_lds)
      resample_rows_kernel<true, true><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, rows,
                                                                     r->d_taps, L, M, W);
    else if (stage)
      resample_rows_kernel<true, false><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, rows,
                                                                      r->d_taps, L, M, W);
    else if (taps_lds)
      resample_rows_kernel<false, true><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, rows,
                                                                      r->d_taps, L, M, W);
    else
      resample_rows_kernel<false, false><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, rows,
                                                                       r->d_taps, L, M, W);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "resample launch", e);
  }
  return MP3G_OK;
}
