// framectx.hip -- delta features and frame context on a time-major feature tensor
// (include/mp3g.h "Delta features and frame context"): Kaldi's add-deltas, and one
// gather that is splice-feats, FunASR's low-frame-rate stacking and
// subsample-feats.  The kernels, their launchers and the host references they
// equal bit for bit; framectx.h holds the scale recurrence, the clamp, the tap
// chain and the output count that both sides compile.  A translation unit of its
// own: the listings of the other kernels do not see it.
//
// Both are one read of the tensor and an (order + 1)- or (left + right + 1)-fold
// write.  A workgroup belongs to ONE plane, so the row's frame count is
// wave-uniform and comes through the scalar cache.  The lanes are dealt over the
// (frame, unit) pairs of the workgroup's tile in row order, a unit being a quad
// of columns (one 16-byte access) when the strides, the bases and n_cols allow
// and a single column otherwise; a lane divides once and then steps by the
// workgroup's size, so no lane idles whatever n_cols is.
//
// delta_kernel, a workgroup per (plane, 64 destination frames, group of up to 128
//   columns).  The tile's source frames and the O * W frames on either side of
//   it, each already clamped to the row, are staged in LDS once: a destination
//   word reads up to 2 O W + 1 source frames and its neighbours read nearly the
//   same ones, and the window is a run-time parameter, so a register ring (which
//   needs a compile-time length) was not an option.  Every order is made from that
//   one staged read; the scales arrive as a kernel argument and are read
//   wave-uniformly.
// stack_kernel, a workgroup per (plane, 64 destination frames).  No staging: a
//   destination frame's blocks are whole source frames, copied four loads at a
//   time; neighbouring destination frames share sources and sit in the same
//   workgroup, so the vector cache serves the reuse.
// No atomics, no scratch; the launch shapes depend on no buffer's contents.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "abi_util.h"
#include "framectx.h"

namespace mp3g {
namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTile = 64;        // destination frames of a workgroup
constexpr uint32_t kGroupCols = 128;  // columns of a delta workgroup: (64 + 2 * 32) x 128 floats are 64 KiB of LDS

extern __shared__ __align__(16) unsigned char s_raw[];

template <int V>
struct UnitOf;
template <>
struct UnitOf<4> {
  using type = float4;
};
template <>
struct UnitOf<1> {
  using type = float;
};

__device__ inline void ldv(const float* p, float4& v) { v = *reinterpret_cast<const float4*>(p); }
__device__ inline void ldv(const float* p, float& v) { v = *p; }
__device__ inline void stv(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ inline void stv(float* p, float v) { *p = v; }
__device__ inline void zerov(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ inline void zerov(float& v) { v = 0.f; }
__device__ inline float4 tapv(float s, float4 x, float4 y) {
  return make_float4(framectx_tap(s, x.x, y.x), framectx_tap(s, x.y, y.y), framectx_tap(s, x.z, y.z),
                     framectx_tap(s, x.w, y.w));
}
__device__ inline float tapv(float s, float x, float y) { return framectx_tap(s, x, y); }

// The (frame, unit) pairs of a tile, in row order, dealt to the lanes: lane tid
// starts at pair tid and steps by kLanes pairs.
struct Walk {
  uint32_t f, u, df, du, upf;
  __device__ inline Walk(uint32_t tid, uint32_t units_per_frame) : upf(units_per_frame) {
    f = tid / upf;
    u = tid - f * upf;
    df = kLanes / upf;
    du = kLanes - df * upf;
  }
  __device__ inline void next() {
    f += df;
    u += du;
    if (u >= upf) {
      u -= upf;
      f++;
    }
  }
};

template <int V>
__global__ __launch_bounds__(kLanes) void delta_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       uint32_t n_planes, uint32_t len_planes, uint32_t n_frames,
                                                       uint32_t n_cols, uint32_t stride, uint32_t stride_out,
                                                       const uint32_t* __restrict__ lengths, uint32_t order,
                                                       uint32_t window, DeltaTaps taps, uint32_t chunks,
                                                       uint32_t cgroups) {
  using T = typename UnitOf<V>::type;
  T* tile = reinterpret_cast<T*>(s_raw);
  const uint32_t tid = threadIdx.x;
  uint32_t bid = blockIdx.x;
  const uint32_t cg = bid % cgroups;
  bid /= cgroups;
  const uint32_t plane = bid / chunks, chunk = bid - plane * chunks;
  const uint32_t n = min(lengths[len_planes == 1 ? plane / n_planes : plane], n_frames);
  const uint32_t f0 = chunk * kTile, fcount = min(kTile, n_frames - f0);
  const uint32_t live = f0 < n ? min(fcount, n - f0) : 0u;  // the tile's frames inside the row
  const uint32_t halo = order * window;
  const uint32_t c0 = cg * kGroupCols, upf = min(kGroupCols, n_cols - c0) / V;  // (V = 4: n_cols % 4 == 0)
  const float* __restrict__ xp = in + (size_t)plane * n_frames * stride + c0;
  float* __restrict__ yp = out + (size_t)plane * n_frames * stride_out + c0;
  if (live) {  // tile row r is source frame f0 - halo + r, clamped to the row
    const uint32_t rows = live + 2 * halo;
    for (Walk w(tid, upf); w.f < rows; w.next()) {
      const uint32_t src = framectx_clamp((int64_t)f0 + (int64_t)w.f - (int64_t)halo, n);
      T v;
      ldv(xp + (size_t)src * stride + V * w.u, v);
      tile[w.f * upf + w.u] = v;
    }
  }
  __syncthreads();
  for (Walk w(tid, upf); w.f < fcount; w.next()) {
    float* __restrict__ y = yp + (size_t)(f0 + w.f) * stride_out + V * w.u;
    if (w.f >= live) {
      T z;
      zerov(z);
      for (uint32_t i = 0; i <= order; i++) stv(y + (size_t)i * n_cols, z);
      continue;
    }
    const T* __restrict__ c = tile + (w.f + halo) * upf + w.u;
    stv(y, *c);
    for (uint32_t i = 1; i <= order; i++) {
      const int32_t h = (int32_t)(i * window);
      T acc;
      zerov(acc);
      for (int32_t j = -h; j <= h; j++) acc = tapv(taps.s[i - 1][j + h], c[j * (int32_t)upf], acc);
      stv(y + (size_t)i * n_cols, acc);
    }
  }
}

template <int V>
__global__ __launch_bounds__(kLanes) void stack_kernel(const float* __restrict__ in, uint32_t n_planes,
                                                       uint32_t len_planes, uint32_t n_frames, uint32_t n_cols,
                                                       uint32_t stride, const uint32_t* __restrict__ lengths,
                                                       uint32_t left, uint32_t ctx, uint32_t step, uint32_t first,
                                                       float* __restrict__ out, uint32_t n_frames_out,
                                                       uint32_t stride_out, uint32_t* __restrict__ lengths_out,
                                                       uint32_t chunks) {
  using T = typename UnitOf<V>::type;
  const uint32_t tid = threadIdx.x;
  const uint32_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const uint32_t n = min(lengths[len_planes == 1 ? plane / n_planes : plane], n_frames);
  const uint32_t m = min(framectx_n_out(n, step, first), n_frames_out);
  if (chunk == 0 && tid == 0) lengths_out[plane] = m;
  const uint32_t upf = n_cols / V;
  const uint32_t j0 = chunk * kTile;
  if (upf == 0 || j0 >= n_frames_out) return;  // (the whole workgroup)
  const uint32_t fcount = min(kTile, n_frames_out - j0);
  const float* __restrict__ xp = in + (size_t)plane * n_frames * stride;
  float* __restrict__ yp = out + (size_t)plane * n_frames_out * stride_out;
  for (Walk w(tid, upf); w.f < fcount; w.next()) {
    const uint32_t j = j0 + w.f;
    float* __restrict__ y = yp + (size_t)j * stride_out + V * w.u;
    if (j >= m) {
      T z;
      zerov(z);
      for (uint32_t k = 0; k < ctx; k++) stv(y + (size_t)k * n_cols, z);
      continue;
    }
    const int64_t t = (int64_t)first + (int64_t)j * (int64_t)step - (int64_t)left;  // block 0's source frame
    const float* __restrict__ x = xp + V * w.u;
    for (uint32_t k = 0; k < ctx; k += 4) {
      T v[4];
#pragma unroll
      for (uint32_t i = 0; i < 4; i++)
        if (k + i < ctx) ldv(x + (size_t)framectx_clamp(t + (int64_t)(k + i), n) * stride, v[i]);
#pragma unroll
      for (uint32_t i = 0; i < 4; i++)
        if (k + i < ctx) stv(y + (size_t)(k + i) * n_cols, v[i]);
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

bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

bool vec_ok(const float* in, const float* out, uint32_t stride, uint32_t stride_out, uint32_t n_cols) {
  return stride % 4 == 0 && stride_out % 4 == 0 && n_cols % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(out) % 16 == 0;
}

// The checks the host and the device call share.  *work: whether anything is to be done.
int delta_check(const float* in, const float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                uint32_t stride, uint32_t n_cols, uint32_t stride_out, const uint32_t* lengths, uint32_t len_planes,
                uint32_t order, uint32_t window, bool* work) {
  *work = false;
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: stride below n_cols");
  if ((uint64_t)stride_out < ((uint64_t)order + 1) * n_cols)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: stride_out below (order + 1) * n_cols");
  if (window == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: a window of no frames");
  if (len_planes != 1 && len_planes != n_planes)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: len_planes is 1 or n_planes");
  if (in && in == out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: out is in (the call is out of place)");
  if (order > kDeltaMaxOrder || (uint64_t)order * window > kDeltaMaxHalo)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "add deltas: order above 4 or order * window above 32");
  if (!n_rows || !n_planes || !n_frames || !n_cols) return MP3G_OK;
  if (!in || !out || !lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: null buffer");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (overlap(in, planes * n_frames * stride * sizeof(float), out, planes * n_frames * stride_out * sizeof(float)))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "add deltas: out overlaps in");
  *work = true;
  return MP3G_OK;
}

int stack_check(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                uint32_t n_cols, const uint32_t* lengths, uint32_t len_planes, uint32_t left, uint32_t right,
                uint32_t step, const float* out, uint32_t n_frames_out, uint32_t stride_out,
                const uint32_t* lengths_out, bool* work) {
  *work = false;
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: stride below n_cols");
  if ((uint64_t)stride_out < ((uint64_t)left + right + 1) * n_cols)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: stride_out below (left + right + 1) * n_cols");
  if (step == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: a step of no frames");
  if (len_planes != 1 && len_planes != n_planes)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: len_planes is 1 or n_planes");
  if (in && in == out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: out is in (the call is out of place)");
  if (left > kStackMaxContext || right > kStackMaxContext)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "stack frames: left or right above 64");
  if (!n_rows || !n_planes) return MP3G_OK;
  if (!lengths || !lengths_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: null buffer");
  const bool reads = n_frames && n_cols && n_frames_out, writes = n_frames_out && n_cols;
  if ((reads && !in) || (writes && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: null buffer");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (in && out && overlap(in, planes * n_frames * stride * sizeof(float), out,
                           planes * n_frames_out * stride_out * sizeof(float)))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stack frames: out overlaps in");
  *work = true;
  return MP3G_OK;
}

inline uint32_t row_frames(const uint32_t* lengths, uint32_t len_planes, uint32_t n_planes, uint32_t r, uint32_t p,
                           uint32_t n_frames) {
  const uint32_t len = lengths[len_planes == 1 ? (size_t)r : (size_t)r * n_planes + p];
  return len < n_frames ? len : n_frames;
}

inline void copy_bits(float* y, const float* x, uint32_t n_cols) { std::memcpy(y, x, (size_t)n_cols * sizeof(float)); }

}  // namespace
}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_delta_scales(uint32_t order, uint32_t window, float* out) {
  if (window == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "delta scales: a window of no frames");
  if (order > kDeltaMaxOrder || (uint64_t)order * window > kDeltaMaxHalo)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "delta scales: order above 4 or order * window above 32");
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "delta scales: null buffer");
  DeltaTaps taps;
  framectx_delta_taps(order, window, &taps);
  *out++ = 1.0f;
  for (uint32_t i = 1; i <= order; i++)
    for (uint32_t k = 0; k < 2 * i * window + 1; k++) *out++ = taps.s[i - 1][k];
  return MP3G_OK;
}

extern "C" int mp3g_add_deltas_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes,
                                    uint32_t n_frames, uint32_t stride, uint32_t n_cols, uint32_t stride_out,
                                    const uint32_t* lengths, uint32_t len_planes, uint32_t order, uint32_t window) {
  bool work;
  const int st = delta_check(in, out, n_rows, n_planes, n_frames, stride, n_cols, stride_out, lengths, len_planes,
                             order, window, &work);
  if (st != MP3G_OK || !work) return st;
  DeltaTaps taps;
  framectx_delta_taps(order, window, &taps);
  for (uint32_t r = 0; r < n_rows; r++)
    for (uint32_t p = 0; p < n_planes; p++) {
      const uint32_t n = row_frames(lengths, len_planes, n_planes, r, p, n_frames);
      const size_t plane = (size_t)r * n_planes + p;
      const float* x = in + plane * n_frames * stride;
      float* y = out + plane * n_frames * stride_out;
      for (uint32_t t = 0; t < n_frames; t++) {
        float* yt = y + (size_t)t * stride_out;
        if (t >= n) {
          for (size_t c = 0; c < ((size_t)order + 1) * n_cols; c++) yt[c] = 0.f;
          continue;
        }
        copy_bits(yt, x + (size_t)t * stride, n_cols);
        for (uint32_t i = 1; i <= order; i++) {
          const int32_t h = (int32_t)(i * window);
          for (uint32_t c = 0; c < n_cols; c++) {
            float acc = 0.f;
            for (int32_t j = -h; j <= h; j++)
              acc = framectx_tap(taps.s[i - 1][j + h], x[(size_t)framectx_clamp((int64_t)t + j, n) * stride + c], acc);
            yt[(size_t)i * n_cols + c] = acc;
          }
        }
      }
    }
  return MP3G_OK;
}

extern "C" int mp3g_add_deltas_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                                    uint32_t n_frames, uint32_t stride, uint32_t n_cols, uint32_t stride_out,
                                    const uint32_t* d_lengths, uint32_t len_planes, uint32_t order, uint32_t window,
                                    void* hip_stream) {
  bool work;
  const int st = delta_check(d_in, d_out, n_rows, n_planes, n_frames, stride, n_cols, stride_out, d_lengths,
                             len_planes, order, window, &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  const uint32_t chunks = (n_frames + kTile - 1) / kTile, cgroups = (n_cols + kGroupCols - 1) / kGroupCols;
  const uint64_t planes = (uint64_t)n_rows * n_planes, blocks = planes * chunks * cgroups;
  if (planes >= (1ull << 32) || blocks >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "add deltas: too many workgroups");
  DeltaTaps taps;
  std::memset(&taps, 0, sizeof(taps));
  framectx_delta_taps(order, window, &taps);
  const size_t lds = (size_t)(kTile + 2 * order * window) * std::min(kGroupCols, n_cols) * sizeof(float);
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const dim3 g((uint32_t)blocks), l(kLanes);
  if (vec_ok(d_in, d_out, stride, stride_out, n_cols))
    delta_kernel<4><<<g, l, lds, stream>>>(d_in, d_out, n_planes, len_planes, n_frames, n_cols, stride, stride_out,
                                           d_lengths, order, window, taps, chunks, cgroups);
  else
    delta_kernel<1><<<g, l, lds, stream>>>(d_in, d_out, n_planes, len_planes, n_frames, n_cols, stride, stride_out,
                                           d_lengths, order, window, taps, chunks, cgroups);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "add deltas launch", e);
}

extern "C" uint32_t mp3g_stack_frames_count(uint32_t n_frames, uint32_t step, uint32_t first) {
  return framectx_n_out(n_frames, step, first);
}

extern "C" int mp3g_stack_frames_host(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                                      uint32_t stride, uint32_t n_cols, const uint32_t* lengths, uint32_t len_planes,
                                      uint32_t left, uint32_t right, uint32_t step, uint32_t first, float* out,
                                      uint32_t n_frames_out, uint32_t stride_out, uint32_t* lengths_out) {
  bool work;
  const int st = stack_check(in, n_rows, n_planes, n_frames, stride, n_cols, lengths, len_planes, left, right, step,
                             out, n_frames_out, stride_out, lengths_out, &work);
  if (st != MP3G_OK || !work) return st;
  const uint32_t ctx = left + right + 1;
  for (uint32_t r = 0; r < n_rows; r++)
    for (uint32_t p = 0; p < n_planes; p++) {
      const uint32_t n = row_frames(lengths, len_planes, n_planes, r, p, n_frames);
      const size_t plane = (size_t)r * n_planes + p;
      const uint32_t n_out = framectx_n_out(n, step, first), m = n_out < n_frames_out ? n_out : n_frames_out;
      lengths_out[plane] = m;
      if (!n_cols || !n_frames_out) continue;  // (no word to write; in and out may be null)
      const float* x = m ? in + plane * n_frames * stride : nullptr;
      float* y = out + plane * n_frames_out * stride_out;
      for (uint32_t j = 0; j < n_frames_out; j++) {
        float* yj = y + (size_t)j * stride_out;
        if (j >= m) {
          for (size_t c = 0; c < (size_t)ctx * n_cols; c++) yj[c] = 0.f;
          continue;
        }
        const int64_t t = (int64_t)first + (int64_t)j * (int64_t)step - (int64_t)left;
        for (uint32_t k = 0; k < ctx; k++)
          copy_bits(yj + (size_t)k * n_cols, x + (size_t)framectx_clamp(t + k, n) * stride, n_cols);
      }
    }
  return MP3G_OK;
}

extern "C" int mp3g_stack_frames_rows(int device, const float* d_in, uint32_t n_rows, uint32_t n_planes,
                                      uint32_t n_frames, uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths,
                                      uint32_t len_planes, uint32_t left, uint32_t right, uint32_t step,
                                      uint32_t first, float* d_out, uint32_t n_frames_out, uint32_t stride_out,
                                      uint32_t* d_lengths_out, void* hip_stream) {
  bool work;
  const int st = stack_check(d_in, n_rows, n_planes, n_frames, stride, n_cols, d_lengths, len_planes, left, right,
                             step, d_out, n_frames_out, stride_out, d_lengths_out, &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  // (no frames to write: one workgroup per plane still writes the count)
  const uint32_t chunks = std::max(1u, (n_frames_out + kTile - 1) / kTile);
  const uint64_t planes = (uint64_t)n_rows * n_planes, blocks = planes * chunks;
  if (planes >= (1ull << 32) || blocks >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "stack frames: too many workgroups");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const dim3 g((uint32_t)blocks), l(kLanes);
  const uint32_t ctx = left + right + 1;
  if (vec_ok(d_in, d_out, stride, stride_out, n_cols))
    stack_kernel<4><<<g, l, 0, stream>>>(d_in, n_planes, len_planes, n_frames, n_cols, stride, d_lengths, left, ctx,
                                         step, first, d_out, n_frames_out, stride_out, d_lengths_out, chunks);
  else
    stack_kernel<1><<<g, l, 0, stream>>>(d_in, n_planes, len_planes, n_frames, n_cols, stride, d_lengths, left, ctx,
                                         step, first, d_out, n_frames_out, stride_out, d_lengths_out, chunks);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "stack frames launch", e);
}
