// stft.hip -- device side of the STFT features (include/mp3g.h "STFT and mel
// spectrograms of decoded rows"): the table upload and mp3g_stft_execute.  A
// translation unit of its own: the other kernels' listings do not see it.
//
// Shape.  One workgroup produces tile_frames consecutive frames of one (row,
// plane), a wave to a frame.  The wave reads its frame's P samples from the row
// with the reflection about the row's ends resolved in the index (lanes read
// neighbouring samples; frames that overlap are served by the L2), multiplies by
// the window and writes z[n] = v[2 n] + i v[2 n + 1] into its working set in LDS:
// N = P / 2 float2 slots, value i at slot i + (i >> 5) (stft.h).  The passes of
// stft_fft.h then run in place, a lane taking every 64th butterfly; from n_fft =
// 2048 two radix-4 passes share one round trip through LDS (16 values to a lane).
// Which lane runs a butterfly, and whether its operands come from LDS or from
// the registers of the pass before, does not change its operands, so the bits
// are the host's.  Then the split step, a lane to a pair (k, N - k): the slots of Z[k]
// and Z[N - k] receive X[k] and X[N - k] (complex output), or their power or
// magnitude in .re; slot 0 holds bins 0 and N in .re and .im.  The epilogue runs
// over the whole tile with the frame as the fastest lane index, so a bin row's
// tile_frames values leave in one contiguous run: either the bins themselves,
// through the logarithm if one is asked for, or the mel chains over each
// filter's support (weights from global memory: the lanes of a filter read the
// same word) and the logarithm.  Workgroup barriers separate the passes; there
// are no atomics, no data-dependent bounds and no scratch shared by launches.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "abi_util.h"
#include "stft.h"

namespace mp3g {
namespace {

constexpr uint32_t kMaxLanes = 64 * kStftMaxWaves;

struct StftArgs {
  const float* window;      // [P]
  const StftC* tw;          // [P]
  const float* wm;          // the filters' weights back to back ...
  const uint32_t* support;  // ... and [n_mels][3] = lo, hi, offset
  uint32_t P, log2n, hop, n_mels, K, tile_frames, slots, output, log, center, tiles;
  float floor;
};

// kWide: n_fft >= 2048, the variant with the register-held double passes (112
// VGPRs; the other keeps to 64 and below, two workgroups to a CU at n_fft <= 1024)
template <bool kWide>
__global__ __launch_bounds__(kMaxLanes) void stft_kernel(const float* __restrict__ src, uint32_t T,
                                                        float* __restrict__ out, uint32_t n_frames,
                                                        uint32_t frame_stride, StftArgs a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  StftC* smem = reinterpret_cast<StftC*>(smem_raw);  // [tile_frames][slots]
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lanes = blockDim.x;
  const uint32_t tile = blockIdx.x % a.tiles;
  const size_t plane = blockIdx.x / a.tiles;
  const uint32_t f0 = tile * a.tile_frames;  // < n_frames (the grid)
  const uint32_t P = a.P, N = P >> 1;
  const bool live = f0 + wave < n_frames;  // (wave-uniform) this wave's frame exists
  StftC* z = smem + (size_t)wave * a.slots;
  const StftC* __restrict__ tw = a.tw;

  if (live) {
    // z[n] = (w[2 n] x[..], w[2 n + 1] x[..]); indices clamped into the row
    const float* __restrict__ srow = src + plane * T;
    const int64_t base = (int64_t)(f0 + wave) * a.hop - (a.center ? (int64_t)N : 0);
    const int64_t last = (int64_t)T - 1;  // (T >= 1: the row has a frame)
    if (base >= 0 && base + (int64_t)P - 1 <= last) {  // (wave-uniform) the frame lies inside the row
      const float* __restrict__ x = srow + base;
      for (uint32_t n = lane; n < N; n += 64)
        z[stft_skew(n)] = StftC{a.window[2 * n] * x[2 * n], a.window[2 * n + 1] * x[2 * n + 1]};
    } else {
      for (uint32_t n = lane; n < N; n += 64) {
        float v[2];
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
          int64_t j = base + (int64_t)(2 * n + h);
          j = j < 0 ? -j : j;
          j = j > last ? 2 * last - j : j;
          j = min(max(j, (int64_t)0), last);
          v[h] = a.window[2 * n + h] * srow[j];
        }
        z[stft_skew(n)] = StftC{v[0], v[1]};
      }
    }
  }
  __syncthreads();

  // the passes.  Two radix-4 passes at a time while a block holds 16 or more: a
  // lane takes the 16 values z[i0 + a q + c q2] (q = len / 4, q2 = len / 16), runs
  // the four butterflies of the pass over len (legs a, at n + c q2) and the four
  // of the pass over q (legs c, at n) in registers -- the butterflies and their
  // operands are stft_fft.h's, only the round trip through LDS between the two
  // passes is gone; then a block of 8 that is left (radix 4, radix 2: eight
  // neighbours to a lane).  The sizes whose N / 16 groups would not fill a wave,
  // and a block of 4 that is left, take one radix-4 pass per round trip.
  uint32_t len = N;
  for (; kWide && len >= 16; len >>= 4) {  // (N / 16 groups: below N = 1,024 they would leave lanes idle)
    const uint32_t q = len >> 2, q2 = len >> 4, step = P / len;
    if (live) {
      for (uint32_t j = lane; j < (N >> 4); j += 64) {
        const uint32_t n = j & (q2 - 1), i0 = (j - n) * 16 + n;  // block (j / q2) len + n
        StftC e[4][4];
#pragma unroll
        for (uint32_t a4 = 0; a4 < 4; a4++)
#pragma unroll
          for (uint32_t c = 0; c < 4; c++) e[a4][c] = z[stft_skew(i0 + a4 * q + c * q2)];
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) stft_bfly4(&e[0][c], &e[1][c], &e[2][c], &e[3][c], tw, (n + c * q2) * step, P);
#pragma unroll
        for (uint32_t a4 = 0; a4 < 4; a4++) stft_bfly4(&e[a4][0], &e[a4][1], &e[a4][2], &e[a4][3], tw, n * step * 4, P);
#pragma unroll
        for (uint32_t a4 = 0; a4 < 4; a4++)
#pragma unroll
          for (uint32_t c = 0; c < 4; c++) z[stft_skew(i0 + a4 * q + c * q2)] = e[a4][c];
      }
    }
    __syncthreads();
  }
  if (kWide && len == 8) {
    len = 1;
    if (live) {
      for (uint32_t j = lane; j < (N >> 3); j += 64) {
        StftC e[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) e[i] = z[stft_skew(8 * j + i)];
        stft_bfly4(&e[0], &e[2], &e[4], &e[6], tw, 0, P);
        stft_bfly4(&e[1], &e[3], &e[5], &e[7], tw, P >> 3, P);
#pragma unroll
        for (uint32_t i = 0; i < 8; i += 2) stft_bfly2(&e[i], &e[i + 1]);
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) z[stft_skew(8 * j + i)] = e[i];
      }
    }
    __syncthreads();
  }
  for (; len >= 4; len >>= 2) {  // one radix-4 pass at a time
    const uint32_t q = len >> 2, step = P / len;
    if (live) {
      for (uint32_t j = lane; j < (N >> 2); j += 64) {
        const uint32_t n = j & (q - 1), i0 = (j - n) * 4 + n;  // block (j / q) len + n
        StftC* p0 = z + stft_skew(i0);
        StftC* p1 = z + stft_skew(i0 + q);
        StftC* p2 = z + stft_skew(i0 + 2 * q);
        StftC* p3 = z + stft_skew(i0 + 3 * q);
        StftC x0 = *p0, x1 = *p1, x2 = *p2, x3 = *p3;
        stft_bfly4(&x0, &x1, &x2, &x3, tw, n * step, P);
        *p0 = x0;
        *p1 = x1;
        *p2 = x2;
        *p3 = x3;
      }
    }
    __syncthreads();
  }
  if (len == 2) {
    if (live) {
      for (uint32_t j = lane; j < (N >> 1); j += 64) {
        StftC* p0 = z + stft_skew(2 * j);
        StftC* p1 = z + stft_skew(2 * j + 1);
        StftC x0 = *p0, x1 = *p1;
        stft_bfly2(&x0, &x1);
        *p0 = x0;
        *p1 = x1;
      }
    }
    __syncthreads();
  }

  // the split step in place: pair (k, N - k) -> the slots of Z[k] and Z[N - k]
  if (live) {
    const bool cplx = a.output == MP3G_STFT_COMPLEX;
    for (uint32_t k = lane; k <= (N >> 1); k += 64) {
      if (k == 0) {
        StftC x0, xn;
        stft_split0(z[0], &x0, &xn);
        z[0] = cplx ? StftC{x0.re, xn.re} : StftC{stft_scalar(x0, a.output), stft_scalar(xn, a.output)};
      } else {
        StftC* pk = z + stft_skew(stft_slot(k, a.log2n));
        StftC* pn = z + stft_skew(stft_slot(N - k, a.log2n));
        StftC xk, xn;
        stft_split(*pk, *pn, tw, k, P, &xk, &xn);
        if (!cplx) {
          xk.re = stft_scalar(xk, a.output);
          xn.re = stft_scalar(xn, a.output);
        }
        *pn = xn;  // (k = N / 2: one slot, xk = xn)
        *pk = xk;
      }
    }
  }
  __syncthreads();

  // the epilogue over the tile: frame = the fastest lane index
  const uint32_t f = tid & (a.tile_frames - 1), r0 = tid / a.tile_frames, rows = lanes / a.tile_frames;
  if (f0 + f >= n_frames) return;  // (no barrier below)
  const StftC* zf = smem + (size_t)f * a.slots;
  if (a.output == MP3G_STFT_COMPLEX) {
    float* __restrict__ orow = out + (plane * a.K * frame_stride + f0 + f) * 2;
    for (uint32_t k = r0; k < a.K; k += rows) {
      StftC x = k < N ? zf[stft_skew(stft_slot(k, a.log2n))] : StftC{zf[0].im, 0.f};
      if (k == 0) x.im = 0.f;
      orow[(size_t)k * frame_stride * 2] = x.re;
      orow[(size_t)k * frame_stride * 2 + 1] = x.im;
    }
  } else if (a.n_mels == 0) {
    float* __restrict__ orow = out + plane * a.K * frame_stride + f0 + f;
    for (uint32_t k = r0; k < a.K; k += rows) {
      const float s = k < N ? zf[stft_skew(stft_slot(k, a.log2n))].re : zf[0].im;
      orow[(size_t)k * frame_stride] = stft_log(s, a.log, a.floor);
    }
  } else {
    float* __restrict__ orow = out + plane * a.n_mels * frame_stride + f0 + f;
    for (uint32_t m = r0; m < a.n_mels; m += rows) {
      const uint32_t lo = a.support[3 * m], hi = a.support[3 * m + 1];
      const float* __restrict__ w = a.wm + a.support[3 * m + 2] - lo;  // w[k], k in [lo, hi]
      float mel = 0.f;
      for (uint32_t k = lo; k <= hi; k++) {
        const float s = k < N ? zf[stft_skew(stft_slot(k, a.log2n))].re : zf[0].im;
        mel = __builtin_fmaf(w[k], s, mel);
      }
      orow[(size_t)m * frame_stride] = stft_log(mel, a.log, a.floor);
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

// the kernel's dynamic LDS: a working set per frame of the tile
uint32_t lds_bytes(const mp3g_stft& st) {
  return st.tile_frames * stft_frame_slots(st.n_fft) * (uint32_t)sizeof(StftC);
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

int stft_device_upload(mp3g_stft* st) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || st->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "stft: no such device");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, st->device);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", e);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  // the filters' non-zero weights back to back, and [n_mels][3] = lo, hi, offset
  std::vector<float> weights;
  std::vector<uint32_t> support((size_t)st->n_mels * 3 + 1, 0);
  for (uint32_t m = 0; m < st->n_mels; m++) {
    const uint32_t lo = st->support[2 * m], hi = st->support[2 * m + 1];
    support[3 * m] = lo;
    support[3 * m + 1] = hi;
    support[3 * m + 2] = (uint32_t)weights.size();
    for (uint32_t k = lo; k <= hi; k++) weights.push_back(st->wm[(size_t)m * st->K + k]);
  }
  if (weights.empty()) weights.push_back(0.f);  // (no filter, or every filter empty: still a buffer)
  DeviceScope scope(st->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  // (the long transforms' working sets are more than the 64 KB a kernel gets by default)
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(stft_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)kStftLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(stft_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStftLdsBudget);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "hipFuncSetAttribute(stft)", e);
  int status = upload(st->window, reinterpret_cast<void**>(&st->d_window), "stft window");
  if (status == MP3G_OK) status = upload(st->tw, reinterpret_cast<void**>(&st->d_tw), "stft twiddles");
  if (status == MP3G_OK) status = upload(weights, reinterpret_cast<void**>(&st->d_wm), "stft mel weights");
  if (status == MP3G_OK) status = upload(support, reinterpret_cast<void**>(&st->d_support), "stft supports");
  if (status != MP3G_OK) stft_device_free(st);
  return status;
}

void stft_device_free(mp3g_stft* st) {
  DeviceScope scope(st->device);
  (void)hipFree(st->d_window);
  (void)hipFree(st->d_tw);
  (void)hipFree(st->d_wm);
  (void)hipFree(st->d_support);
  st->d_window = st->d_wm = nullptr;
  st->d_tw = nullptr;
  st->d_support = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_stft_execute(const mp3g_stft* st, const float* d_src, uint32_t n_rows, uint32_t n_planes,
                                 uint32_t T, float* d_out, uint32_t n_frames, uint32_t frame_stride,
                                 void* hip_stream) {
  if (!st) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null stft");
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: 1 or 2 planes");
  if (st->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: a host-only object");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "stft: rows of 2^31 samples or more");
  if (n_frames > mp3g_stft_frames(st, T))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: more frames than the rows have");
  if (frame_stride < n_frames) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: frame stride below n_frames");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes == 0 || n_frames == 0) return MP3G_OK;
  const uint32_t tiles = (n_frames + st->tile_frames - 1) / st->tile_frames;
  if (planes * tiles >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "stft: 2^31 workgroups or more in one launch");
  if (!d_src || !d_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  DeviceScope scope(st->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const StftArgs a = {st->d_window, st->d_tw, st->d_wm, st->d_support, st->n_fft, st->log2n, st->hop, st->n_mels,
                      st->K, st->tile_frames, stft_frame_slots(st->n_fft), st->output, st->log,
                      (st->flags & MP3G_STFT_CENTER) ? 1u : 0u, tiles, st->floor};
  const dim3 grid((uint32_t)(planes * tiles)), block(64 * st->tile_frames);
  if (st->n_fft >= 2048)
    stft_kernel<true><<<grid, block, lds_bytes(*st), stream>>>(d_src, T, d_out, n_frames, frame_stride, a);
  else
    stft_kernel<false><<<grid, block, lds_bytes(*st), stream>>>(d_src, T, d_out, n_frames, frame_stride, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "stft launch", e);
  return MP3G_OK;
}
