// varresample.hip -- device side of the variable-ratio resampler (include/mp3g.h
// "variable-ratio resampling of decoded rows"): the table upload and
// mp3g_varresample_rows.  A translation unit of its own: the decode kernels'
// and the polyphase resampler's listings do not see it.
//
// Every row carries its own ratio num / den and gain, so nothing about the
// filter is a launch constant: a workgroup reads its row's descriptor, derives
// the cutoff step I, the cutoff c and the half width Wr in integers, and runs
// the per-output arithmetic of varresample.h -- the same inline functions
// mp3g_varresample_host compiles -- so the output equals the host reference bit
// for bit whatever the tiling.
//
// Shape.  ONE launch: grid (rows, tile groups).  A workgroup of 256 lanes makes
// tiles of kVarTile consecutive outputs of one row, a lane the outputs t and
// t + 256 of a tile, for ALL planes: the weight fmaf(eta, D[i], F[i]) is formed
// once per tap and feeds one chain per plane.  The tile's source span,
// (tile - 1) num / den + 2 Wr samples per plane, is staged into LDS with
// coalesced loads when a plane's share of the stage holds it (a decision that
// is uniform over the workgroup), and read from global memory under the same
// bounds otherwise.  The (F, D) table is gathered at stride I from a
// lane-dependent start: from global memory (L2), or -- an object whose table
// has at most kVarTableLdsPairs pairs may ask for it -- from a copy in LDS that
// a workgroup loads once and keeps over the tiles it makes.
//
// Bounds.  A descriptor is untrusted: n_src and n_out are cut at the strides,
// the taps of an output are clamped to [0, n_src) before the loop (var_chain),
// a source position farther than 2^44 from the origin has no taps, and a row
// with den = 0, num = 0 or I = 0 writes +0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "varresample.h"

namespace mp3g {
namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTilesPerGroupLds = 8;  // tiles a workgroup makes per table load
static_assert(kVarTile == 2 * kLanes, "two outputs per lane");

template <int C, bool kTableLds>
__global__ __launch_bounds__(kLanes) void varresample_rows_kernel(const float* __restrict__ src, uint32_t src_stride,
                                                                  float* __restrict__ out, uint32_t out_stride,
                                                                  const mp3g_varresample_row* __restrict__ rows,
                                                                  const float* __restrict__ table, uint32_t Z,
                                                                  uint32_t R, uint32_t P, uint32_t tiles_per_group) {
  __shared__ float s_x[kVarStageFloats];
  __shared__ float s_tab[kTableLds ? 2 * kVarTableLdsPairs : 2];
  constexpr uint32_t kPlane = kVarStageFloats / C;  // a plane's share of the stage
  const mp3g_varresample_row row = rows[blockIdx.x];
  const uint32_t n_out = min(row.n_out, out_stride);
  const uint32_t tid = threadIdx.x;
  const uint32_t tile0 = blockIdx.y * tiles_per_group;
  if ((uint64_t)tile0 * kVarTile >= n_out) return;  // (uniform: before any barrier)
  const uint32_t tile1 = min(tile0 + tiles_per_group, (n_out + kVarTile - 1) / kVarTile);
  const uint32_t n_src = min(row.n_src, src_stride);
  const uint32_t num = row.num, den = row.den;
  const float gain = row.gain;
  const float* __restrict__ srow = src + (size_t)row.src_row * C * src_stride;
  float* __restrict__ orow = out + (size_t)row.out_row * C * out_stride;
  const uint32_t I = den ? var_step(R, num, den) : 0u;

  const uint32_t end = (uint32_t)min((uint64_t)n_out, (uint64_t)tile1 * kVarTile);  // of this workgroup's outputs
  if (num == 0 || I == 0) {  // no such filter: +0
    for (uint32_t i = tile0 * kVarTile + tid; i < end; i += kLanes)
      for (int c = 0; c < C; c++) orow[(size_t)c * out_stride + i] = 0.f;
    return;
  }
  if (num == den) {  // a copy times gain, zero outside the row's valid range
    const uint64_t rel = row.out_start - row.src_origin;
    for (uint32_t i = tile0 * kVarTile + tid; i < end; i += kLanes) {
      const uint64_t p = rel + i;  // (wraps below the origin: >= n_src)
      for (int c = 0; c < C; c++)
        orow[(size_t)c * out_stride + i] = (p < n_src ? srow[(size_t)c * src_stride + p] : 0.f) * gain;
    }
    return;
  }

  if (kTableLds) {  // Z <= kVarTableLdsPairs (the host checked): the pairs a tap can index
    for (uint32_t i = tid; i < 2 * Z; i += kLanes) s_tab[i] = table[i];
  }
  const float* __restrict__ tab = kTableLds ? s_tab : table;
  const float cut = var_cutoff(I, P);
  const uint32_t Wr = (Z + I - 1) / I;

  for (uint32_t tile = tile0; tile < tile1; tile++) {
    const uint32_t t0 = tile * kVarTile;
    const uint32_t nt = min(kVarTile, n_out - t0);
    // the tile's first output: (q0, r0) = divmod(n0 num, den), once, in 64 bits
    uint64_t q0;
    uint32_t r0;
    var_divmod(row.out_start + t0, num, den, &q0, &r0);
    // source positions relative to the origin: the first output's, and how far the last lies beyond it
    const int64_t d0 = (int64_t)(q0 - row.src_origin);
    const uint64_t reach = ((uint64_t)r0 + (uint64_t)(nt - 1) * num) / den;
    const bool small = (uint64_t)r0 + (uint64_t)(kVarTile - 1) * num <= 0xffffffffull;  // 32-bit lane offsets
    const bool near = d0 > -(kVarFar >> 2) && d0 < (kVarFar >> 2);
    const uint64_t span = reach + 2ull * Wr;
    const bool stage = near && span <= kPlane;  // (uniform over the workgroup)
    const int64_t lo = near ? d0 - (int64_t)Wr + 1 : 0;  // the stage holds positions [lo, lo + span)
    if (tile != tile0) __syncthreads();         // the previous tile's readers are done
    if (stage) {
      for (uint32_t i = tid; i < (uint32_t)span; i += kLanes) {
        const int64_t p = lo + (int64_t)i;
        const bool ok = p >= 0 && p < (int64_t)n_src;
        for (int c = 0; c < C; c++) s_x[c * kPlane + i] = ok ? srow[(size_t)c * src_stride + p] : 0.f;
      }
    }
    if (stage || (kTableLds && tile == tile0)) __syncthreads();

    for (uint32_t t = tid; t < nt; t += kLanes) {
      uint64_t dq;
      uint32_t r;
      if (small) {
        const uint32_t tt = r0 + t * num, dq32 = tt / den;
        dq = dq32;
        r = tt - dq32 * den;
      } else {
        const uint64_t tt = (uint64_t)r0 + (uint64_t)t * num;
        dq = tt / den;
        r = (uint32_t)(tt - dq * den);
      }
      const uint64_t q = q0 + dq;
      const VarTaps taps = var_taps(q, r, den, I, Z);
      const int64_t d = var_rel(q, row.src_origin);
      float acc[C];
      if (stage) {
        // (lo <= p < lo + span for every tap of the tile: nL, nR <= Wr)
        var_chain<C>(tab, taps, I, d, (int64_t)n_src,
                     [&](int c, int64_t p) { return s_x[c * kPlane + (uint32_t)(p - lo)]; }, acc);
      } else {
        var_chain<C>(tab, taps, I, d, (int64_t)n_src,
                     [&](int c, int64_t p) { return srow[(size_t)c * src_stride + (size_t)p]; }, acc);
      }
      for (int c = 0; c < C; c++) orow[(size_t)c * out_stride + t0 + t] = var_scale(cut, acc[c], gain);
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

int varresample_device_upload(mp3g_varresampler* r) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || r->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "varresampler: no such device");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, r->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  DeviceScope scope(r->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  const size_t bytes = r->table.size() * sizeof(float);
  e = hipMalloc(&r->d_table, bytes);
  if (e != hipSuccess) {
    r->d_table = nullptr;
    return hip_fail(MP3G_ERR_OUT_OF_MEMORY, "hipMalloc(varresampler table)", e);
  }
  e = hipMemcpy(r->d_table, r->table.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(r->d_table);
    r->d_table = nullptr;
    return hip_fail(MP3G_ERR_DEVICE, "hipMemcpy(varresampler table)", e);
  }
  return MP3G_OK;
}

void varresample_device_free(mp3g_varresampler* r) {
  DeviceScope scope(r->device);
  (void)hipFree(r->d_table);
  r->d_table = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_varresample_rows(const mp3g_varresampler* r, const float* d_src, uint32_t src_stride,
                                     float* d_out, uint32_t out_stride, uint32_t n_channels,
                                     const mp3g_varresample_row* d_rows, uint32_t n_rows, void* hip_stream) {
  if (!r) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null varresampler");
  if (n_channels != 1 && n_channels != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: 1 or 2 channels");
  if (r->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: a host-only varresampler");
  if (n_rows == 0 || out_stride == 0) return MP3G_OK;
  if (!d_src || !d_out || !d_rows) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  if (n_rows > 0x7fffffffu || src_stride > 0x7fffffffu || out_stride > 0x7fffffffu)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: more than 2^31 - 1 rows or samples a row");
  DeviceScope scope(r->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint32_t tiles = (uint32_t)(((uint64_t)out_stride + kVarTile - 1) / kVarTile);
  // the launch shape: n_rows, out_stride and n_channels alone.  (A grid's y
  // extent ends at 65,535; a workgroup makes as many tiles as that asks for.)
  uint32_t per_group = r->table_lds ? kTilesPerGroupLds : 1u;
  per_group = std::max(per_group, (tiles + 65534u) / 65535u);
  const dim3 grid(n_rows, (tiles + per_group - 1) / per_group, 1);
  const uint32_t Z = r->Z, R = r->R, P = r->P;
  if (n_channels == 2 && r->table_lds)
    varresample_rows_kernel<2, true><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, d_rows,
                                                                   r->d_table, Z, R, P, per_group);
  else if (n_channels == 2)
    varresample_rows_kernel<2, false><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, d_rows,
                                                                    r->d_table, Z, R, P, per_group);
  else if (r->table_lds)
    varresample_rows_kernel<1, true><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, d_rows,
                                                                   r->d_table, Z, R, P, per_group);
  else
    varresample_rows_kernel<1, false><<<grid, kLanes, 0, stream>>>(d_src, src_stride, d_out, out_stride, d_rows,
                                                                    r->d_table, Z, R, P, per_group);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "varresample launch", e);
  return MP3G_OK;
}
