// specaug.hip -- SpecAugment on a feature tensor (include/mp3g.h "SpecAugment"):
// the two-segment cubic time warp, then the union of up to 16 time and 4
// frequency masks, per row from a descriptor in device memory.  The kernels,
// their launcher and the host reference they equal bit for bit; specaug.h holds
// the descriptor's reading, the source position, the weights and the tap chain
// that both sides compile.  A translation unit of its own: the listings of the
// other kernels do not see it.
//
// The work is one read and one write of the tensor.  A workgroup belongs to ONE
// plane, so its row descriptor is wave-uniform: the compiler loads it through
// the scalar cache, and the interval tests run once per frame or once per
// column, never per word.
//
// tm_kernel (time-major [plane][frame][stride]), a workgroup per (plane, 64
//   destination frames).  Lanes 0..63 first settle their frame -- past the row,
//   time-masked, copied or warped, with the four source frames and weights of a
//   warped one -- into LDS.  Then the lanes are laid over the tile as (frame,
//   unit): a unit is a quad of columns (one 16-byte access) when the stride and
//   the bases allow, a single column otherwise and for the up to three columns
//   after the last whole quad.  A lane keeps its unit and walks the frames, so a
//   unit's frequency-mask bits are made once.  A warped quad reads its four
//   source frames with four 16-byte loads; neighbouring destination frames share
//   three of them and sit in the same workgroup, so the vector cache serves the
//   reuse.
// fm_kernel (frequency-major [plane][bin][stride], frames along the last axis), a
//   workgroup per (plane, chunk of frames, group of 16 bins).  Lanes run along
//   frames, V = 4 frames a lane when 16-byte accesses are possible and 1
//   otherwise; a lane settles its V frames once (each has its own position and
//   weights, kept in registers) and walks the group's bins; a bin's frequency
//   mask is one test per bin.  A warped frame gathers its four sources along the
//   row the lane is in: neighbouring lanes read neighbouring words.
// The in-place instantiations (no warp, out == in) issue no load at all: they
//   store the fill to the masked words and touch nothing else.
// sums_kernel (MP3G_SPECAUG_FILL_MEAN, a launch before the other), a workgroup
//   per plane: a lane per frame adds the frame's bins in float64, ascending; the
//   256 frame sums go to LDS, lanes 0..7 add their blocks of 32 and lane 0 adds
//   the blocks, which is the blocked order of specaug.h.  No atomics; the launch
//   shapes depend on no buffer's contents.
#include <hip/hip_runtime.h>

#include <string>

#include "abi_util.h"
#include "specaug.h"

static_assert(sizeof(mp3g_specaug_row) == 176, "mp3g_specaug_row is 176 bytes");

namespace mp3g {
namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTmFrames = 64;  // destination frames of a time-major workgroup
constexpr uint32_t kFmBins = 16;    // bins of a frequency-major workgroup
constexpr uint32_t kKnownFlags = MP3G_SPECAUG_FREQ_MAJOR | MP3G_SPECAUG_WARP | MP3G_SPECAUG_FILL_MEAN;

enum : uint32_t { kPast = 0, kCopy = 1, kFill = 2, kTap = 3 };  // what a destination frame is

// Whether position x (below extent) lies in one of the first `count` masks.
MP3G_SA_HD inline bool in_masks(const uint32_t (*m)[2], uint32_t count, uint32_t extent, uint32_t x) {
  bool hit = false;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t lo, hi;
    specaug_clip(m[k][0], m[k][1], extent, &lo, &hi);
    hit = hit || (x >= lo && x < hi);
  }
  return hit;
}

// What destination frame j of a row of n frames is; a warped one's taps to *tap.
MP3G_SA_HD inline uint32_t frame_kind(const mp3g_specaug_row& d, uint32_t j, uint32_t n, bool warp, SpecaugTap* tap) {
  if (j >= n) return kPast;
  if (in_masks(d.time, specaug_count(d.n_time, MP3G_SPECAUG_MAX_TIME_MASKS), n, j)) return kFill;
  if (!warp) return kCopy;
  specaug_tap(j, d.warp_center, d.warp_to, n, tap);
  return kTap;
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

template <bool VEC, bool INPLACE>
__global__ __launch_bounds__(kLanes) void tm_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                    uint32_t n_planes, uint32_t n_frames, uint32_t n_bins,
                                                    uint32_t stride, const uint32_t* __restrict__ lengths,
                                                    const mp3g_specaug_row* __restrict__ desc, uint32_t flags,
                                                    float fill_value, const float* __restrict__ fills,
                                                    uint32_t chunks, uint32_t lpf_shift) {
  __shared__ SpecaugTap s_tap[kTmFrames];
  __shared__ uint32_t s_kind[kTmFrames];
  const uint32_t tid = threadIdx.x;
  const uint32_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const uint32_t row = plane / n_planes;
  const uint32_t n = min(lengths[row], n_frames);
  const uint32_t f0 = chunk * kTmFrames, fcount = min(kTmFrames, n_frames - f0);
  if (INPLACE && f0 >= n) return;  // (the whole workgroup: nothing past the row is written)
  const mp3g_specaug_row& d = desc[row];
  const bool warp = !INPLACE && (flags & MP3G_SPECAUG_WARP) && specaug_warps(d.warp_center, d.warp_to, n);
  const float fill = (flags & MP3G_SPECAUG_FILL_MEAN) ? fills[plane] : fill_value;
  if (tid < fcount) {
    SpecaugTap tap;
    const uint32_t kind = frame_kind(d, f0 + tid, n, warp, &tap);
    s_kind[tid] = kind;
    if (kind == kTap) s_tap[tid] = tap;
  }
  __syncthreads();

  const uint32_t nq = VEC ? n_bins / 4 : 0u, upf = nq + (n_bins - 4 * nq);  // units of a frame
  const uint32_t lpf = 1u << lpf_shift, fpp = kLanes >> lpf_shift;
  const uint32_t fs = tid >> lpf_shift;
  const uint32_t n_freq = specaug_count(d.n_freq, MP3G_SPECAUG_MAX_FREQ_MASKS);
  const size_t base = (size_t)plane * n_frames * stride;
  const float* __restrict__ xp = in + base;
  float* __restrict__ yp = out + base;
  for (uint32_t u = tid & (lpf - 1); u < upf; u += lpf) {
    const bool quad = VEC && u < nq;
    const uint32_t col = quad ? 4 * u : 4 * nq + (u - nq);
    if (quad) {
      uint32_t fm = 0;  // bit k: column col + k is frequency-masked
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) fm |= in_masks(d.freq, n_freq, n_bins, col + k) ? 1u << k : 0u;
      for (uint32_t f = fs; f < fcount; f += fpp) {
        const uint32_t kind = s_kind[f];
        const size_t at = (size_t)(f0 + f) * stride + col;
        if (INPLACE) {
          if (kind == kPast) continue;
          const uint32_t m = kind == kFill ? 0xFu : fm;
          if (m == 0xFu) {
            st4(yp + at, make_float4(fill, fill, fill, fill));
          } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
              if (m >> k & 1u) yp[at + k] = fill;
          }
          continue;
        }
        float4 v;
        if (kind == kFill) {
          v = make_float4(fill, fill, fill, fill);
        } else {
          if (kind == kTap) {
            const SpecaugTap tap = s_tap[f];
            const float4 a = ld4(xp + (size_t)tap.src[0] * stride + col), b = ld4(xp + (size_t)tap.src[1] * stride + col),
                         c = ld4(xp + (size_t)tap.src[2] * stride + col), e = ld4(xp + (size_t)tap.src[3] * stride + col);
            v.x = specaug_interp(tap.w, a.x, b.x, c.x, e.x);
            v.y = specaug_interp(tap.w, a.y, b.y, c.y, e.y);
            v.z = specaug_interp(tap.w, a.z, b.z, c.z, e.z);
            v.w = specaug_interp(tap.w, a.w, b.w, c.w, e.w);
          } else {
            v = ld4(xp + at);
          }
          if (kind != kPast && fm) {
            v.x = fm & 1u ? fill : v.x;
            v.y = fm & 2u ? fill : v.y;
            v.z = fm & 4u ? fill : v.z;
            v.w = fm & 8u ? fill : v.w;
          }
        }
        st4(yp + at, v);
      }
    } else {
      const bool fm = in_masks(d.freq, n_freq, n_bins, col);
      for (uint32_t f = fs; f < fcount; f += fpp) {
        const uint32_t kind = s_kind[f];
        const size_t at = (size_t)(f0 + f) * stride + col;
        const bool masked = kind == kFill || (fm && kind != kPast);
        if (INPLACE) {
          if (masked) yp[at] = fill;
          continue;
        }
        float v = fill;
        if (!masked) {
          if (kind == kTap) {
            const SpecaugTap tap = s_tap[f];
            v = specaug_interp(tap.w, xp[(size_t)tap.src[0] * stride + col], xp[(size_t)tap.src[1] * stride + col],
                               xp[(size_t)tap.src[2] * stride + col], xp[(size_t)tap.src[3] * stride + col]);
          } else {
            v = xp[at];
          }
        }
        yp[at] = v;
      }
    }
  }
}

template <int V, bool INPLACE>
__global__ __launch_bounds__(kLanes) void fm_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                    uint32_t n_planes, uint32_t n_frames, uint32_t n_bins,
                                                    uint32_t stride, const uint32_t* __restrict__ lengths,
                                                    const mp3g_specaug_row* __restrict__ desc, uint32_t flags,
                                                    float fill_value, const float* __restrict__ fills,
                                                    uint32_t chunks, uint32_t bgroups, uint32_t lpr_shift) {
  const uint32_t tid = threadIdx.x;
  uint32_t bid = blockIdx.x;
  const uint32_t bg = bid % bgroups;
  bid /= bgroups;
  const uint32_t plane = bid / chunks, chunk = bid - plane * chunks;
  const uint32_t row = plane / n_planes;
  const uint32_t n = min(lengths[row], n_frames);
  const uint32_t lpr = 1u << lpr_shift, bpp = kLanes >> lpr_shift;
  const uint64_t j0w = ((uint64_t)chunk * lpr + (tid & (lpr - 1))) * V;  // the lane's first frame
  if (j0w >= (INPLACE ? n : n_frames)) return;
  const uint32_t j0 = (uint32_t)j0w;
  const mp3g_specaug_row& d = desc[row];
  const bool warp = !INPLACE && (flags & MP3G_SPECAUG_WARP) && specaug_warps(d.warp_center, d.warp_to, n);
  const float fill = (flags & MP3G_SPECAUG_FILL_MEAN) ? fills[plane] : fill_value;
  const uint32_t live = min((uint32_t)V, n_frames - j0);  // frames of the lane inside the tensor
  uint32_t kind[V];
  SpecaugTap tap[V];
  bool need_load = false;
#pragma unroll
  for (int k = 0; k < V; k++) {
    kind[k] = (uint32_t)k < live ? frame_kind(d, j0 + k, n, warp, &tap[k]) : (uint32_t)kPast;
    need_load = need_load || kind[k] == kPast || kind[k] == kCopy;
  }
  const uint32_t n_freq = specaug_count(d.n_freq, MP3G_SPECAUG_MAX_FREQ_MASKS);
  const size_t base = (size_t)plane * n_bins * stride;
  const uint32_t b_end = min(n_bins, (bg + 1) * kFmBins);
  for (uint32_t b = bg * kFmBins + (tid >> lpr_shift); b < b_end; b += bpp) {
    const bool fm = in_masks(d.freq, n_freq, n_bins, b);
    const float* __restrict__ xr = in + base + (size_t)b * stride;
    float* __restrict__ yr = out + base + (size_t)b * stride;
    bool masked[V];
#pragma unroll
    for (int k = 0; k < V; k++) masked[k] = kind[k] == kFill || (fm && kind[k] != kPast);
    if (INPLACE) {
      bool all = live == (uint32_t)V;
#pragma unroll
      for (int k = 0; k < V; k++) all = all && masked[k];
      if (V == 4 && all) {
        st4(yr + j0, make_float4(fill, fill, fill, fill));
      } else {
#pragma unroll
        for (int k = 0; k < V; k++)
          if ((uint32_t)k < live && masked[k]) yr[j0 + k] = fill;
      }
      continue;
    }
    float v[V];
    const bool whole = V == 4 && live == (uint32_t)V;
    if (whole) {
      if constexpr (V == 4) {
        if (need_load) {
          const float4 t = ld4(xr + j0);
          v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; k++)
        if ((uint32_t)k < live && !masked[k] && kind[k] != kTap) v[k] = xr[j0 + k];
    }
#pragma unroll
    for (int k = 0; k < V; k++) {
      if (masked[k]) {
        v[k] = fill;
      } else if (kind[k] == kTap) {
        v[k] = specaug_interp(tap[k].w, xr[tap[k].src[0]], xr[tap[k].src[1]], xr[tap[k].src[2]], xr[tap[k].src[3]]);
      }
    }
    if (whole) {
      if constexpr (V == 4) st4(yr + j0, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
      for (int k = 0; k < V; k++)
        if ((uint32_t)k < live) yr[j0 + k] = v[k];
    }
  }
}

// The fills of FILL_MEAN: fills[plane] from the input's live region.
template <bool FREQ_MAJOR, bool VEC>
__global__ __launch_bounds__(kLanes) void sums_kernel(const float* __restrict__ in, uint32_t n_planes,
                                                      uint32_t n_frames, uint32_t n_bins, uint32_t stride,
                                                      const uint32_t* __restrict__ lengths, float* __restrict__ fills) {
  __shared__ double s_s[kLanes];
  __shared__ double s_b[kLanes / kSpecaugBlock];
  const uint32_t tid = threadIdx.x, plane = blockIdx.x;
  const uint32_t n = min(lengths[plane / n_planes], n_frames);
  const float* __restrict__ xp = in + (size_t)plane * (FREQ_MAJOR ? n_bins : n_frames) * stride;
  double bp = 0.0, part = 0.0;  // lane 0's
  for (uint32_t f0 = 0; f0 < n; f0 += kLanes) {  // (n is the workgroup's: every lane passes the barriers)
    const uint32_t f = f0 + tid;
    double s = 0.0;
    if (f < n) {
      if (FREQ_MAJOR) {
        const float* __restrict__ p = xp + f;
        uint32_t b = 0;
        for (; b + 8 <= n_bins; b += 8) {
          float v[8];
#pragma unroll
          for (uint32_t u = 0; u < 8; u++) v[u] = p[(size_t)(b + u) * stride];
#pragma unroll
          for (uint32_t u = 0; u < 8; u++) s += (double)v[u];
        }
        for (; b < n_bins; b++) s += (double)p[(size_t)b * stride];
      } else {
        const float* __restrict__ p = xp + (size_t)f * stride;
        uint32_t b = 0;
        if (VEC) {
          for (; b + 8 <= n_bins; b += 8) {
            const float4 a = ld4(p + b), c = ld4(p + b + 4);
            s += (double)a.x, s += (double)a.y, s += (double)a.z, s += (double)a.w;
            s += (double)c.x, s += (double)c.y, s += (double)c.z, s += (double)c.w;
          }
        }
        for (; b < n_bins; b++) s += (double)p[b];
      }
    }
    s_s[tid] = s;
    __syncthreads();
    const uint32_t cnt = min(kLanes, n - f0);
    if (tid < kLanes / kSpecaugBlock) {
      const uint32_t k0 = tid * kSpecaugBlock, k1 = min(k0 + kSpecaugBlock, cnt);
      double b = 0.0;
      for (uint32_t k = k0; k < k1; k++) b += s_s[k];
      s_b[tid] = b;
    }
    __syncthreads();
    if (tid == 0) {
      for (uint32_t k = 0; k * kSpecaugBlock < cnt; k++) {
        if ((k + 1) * kSpecaugBlock <= cnt) {
          bp += s_b[k];
        } else {
          part = s_b[k];  // (the row's last, partial block)
        }
      }
    }
    // (the next pass writes s_s after the barrier above, s_b after its own first barrier)
  }
  if (tid == 0) fills[plane] = specaug_mean(bp + part, n, n_bins);
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

// The checks the host and the device call share.  *work: whether anything is to
// be done; *inplace: out is in.
int specaug_check(const float* in, const float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                  uint32_t n_bins, uint32_t stride, const uint32_t* lengths, const mp3g_specaug_row* desc,
                  uint32_t flags, const float* fills, bool* work, bool* inplace) {
  *work = false;
  *inplace = false;
  if (flags & ~kKnownFlags) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: unknown flag");
  const bool fm = flags & MP3G_SPECAUG_FREQ_MAJOR;
  if (stride < (fm ? n_frames : n_bins))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: stride below the live count");
  if ((flags & MP3G_SPECAUG_WARP) && in && in == out)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: out is in (the warp is out of place)");
  if ((flags & MP3G_SPECAUG_WARP) && n_frames > kSpecaugMaxWarpFrames)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "specaug: more than 2^22 frames with the warp");
  if (!n_rows || !n_planes) return MP3G_OK;
  if ((flags & MP3G_SPECAUG_FILL_MEAN) && !fills)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: FILL_MEAN without a buffer for the fills");
  if (!n_frames || !n_bins) {  // (no word to write; the fills of FILL_MEAN are all +0.0)
    if (!(flags & MP3G_SPECAUG_FILL_MEAN)) return MP3G_OK;
    if (!lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: null buffer");
    *work = true;
    return MP3G_OK;
  }
  if (!in || !out || !lengths || !desc) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: null buffer");
  if (in == out) {
    *inplace = true;
  } else {
    const uint64_t bytes = (uint64_t)n_rows * n_planes * (fm ? n_bins : n_frames) * stride * sizeof(float);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(in), pb = reinterpret_cast<uintptr_t>(out);
    if (pa < pb + bytes && pb < pa + bytes) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "specaug: out overlaps in");
  }
  *work = true;
  return MP3G_OK;
}

uint32_t shift_for(uint32_t units) {  // the smallest s with 2^s >= units, at most log2(kLanes)
  uint32_t s = 0;
  while (s < 8 && (1u << s) < units) s++;
  return s;
}

}  // namespace
}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_specaug_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                                 uint32_t n_bins, uint32_t stride, const uint32_t* lengths,
                                 const mp3g_specaug_row* desc, uint32_t flags, float fill_value, float* fills) {
  bool work, inplace;
  const int st = specaug_check(in, out, n_rows, n_planes, n_frames, n_bins, stride, lengths, desc, flags, fills, &work,
                               &inplace);
  if (st != MP3G_OK || !work) return st;
  const bool fm = flags & MP3G_SPECAUG_FREQ_MAJOR, mean = flags & MP3G_SPECAUG_FILL_MEAN;
  const size_t fstep = fm ? 1 : stride, bstep = fm ? stride : 1;
  const size_t plane_words = (size_t)(fm ? n_bins : n_frames) * stride;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths[r] < n_frames ? lengths[r] : n_frames;
    for (uint32_t p = 0; p < n_planes; p++) {
      const size_t plane = (size_t)r * n_planes + p;
      float fill = fill_value;
      if (mean) {
        SpecaugTotal tot;
        for (uint32_t f = 0; f < n; f++) {
          double s = 0.0;
          for (uint32_t b = 0; b < n_bins; b++) s += (double)in[plane * plane_words + f * fstep + b * bstep];
          tot.add(s);
        }
        fill = fills[plane] = specaug_mean(tot.total(), n, n_bins);
      }
      if (!n_frames || !n_bins) continue;
      const mp3g_specaug_row& d = desc[r];
      const float* x = in + plane * plane_words;
      float* y = out + plane * plane_words;
      const bool warp = !inplace && (flags & MP3G_SPECAUG_WARP) && specaug_warps(d.warp_center, d.warp_to, n);
      const uint32_t n_freq = specaug_count(d.n_freq, MP3G_SPECAUG_MAX_FREQ_MASKS);
      for (uint32_t j = 0; j < n_frames; j++) {
        SpecaugTap tap;
        const uint32_t kind = frame_kind(d, j, n, warp, &tap);
        for (uint32_t b = 0; b < n_bins; b++) {
          const size_t at = j * fstep + b * bstep;
          const bool masked = kind == kFill || (kind != kPast && in_masks(d.freq, n_freq, n_bins, b));
          if (masked) {
            y[at] = fill;
          } else if (inplace) {
            continue;
          } else if (kind == kTap) {
            y[at] = specaug_interp(tap.w, x[tap.src[0] * fstep + b * bstep], x[tap.src[1] * fstep + b * bstep],
                                   x[tap.src[2] * fstep + b * bstep], x[tap.src[3] * fstep + b * bstep]);
          } else {
            y[at] = x[at];
          }
        }
      }
    }
  }
  return MP3G_OK;
}

extern "C" int mp3g_specaug_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                                 uint32_t n_frames, uint32_t n_bins, uint32_t stride, const uint32_t* d_lengths,
                                 const mp3g_specaug_row* d_desc, uint32_t flags, float fill_value, float* d_fill,
                                 void* hip_stream) {
  bool work, inplace;
  const int st = specaug_check(d_in, d_out, n_rows, n_planes, n_frames, n_bins, stride, d_lengths, d_desc, flags,
                               d_fill, &work, &inplace);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  const bool fm = flags & MP3G_SPECAUG_FREQ_MAJOR, mean = flags & MP3G_SPECAUG_FILL_MEAN;
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "specaug: 2^31 planes or more");
  const bool vec = stride % 4 == 0 && reinterpret_cast<uintptr_t>(d_in) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
  // the main launch's shape
  uint64_t blocks = 0;
  uint32_t chunks = 0, bgroups = 0, shift = 0;
  if (n_frames && n_bins) {
    if (fm) {
      const uint32_t units = vec ? (n_frames + 3) / 4 : n_frames;
      shift = shift_for(units);
      chunks = (units + (1u << shift) - 1) >> shift;
      bgroups = (n_bins + kFmBins - 1) / kFmBins;
      blocks = planes * chunks * bgroups;
    } else {
      const uint32_t nq = vec ? n_bins / 4 : 0u;
      shift = shift_for(nq + (n_bins - 4 * nq));
      chunks = (n_frames + kTmFrames - 1) / kTmFrames;
      blocks = planes * chunks;
    }
    if (blocks >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "specaug: too many workgroups");
  }
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (mean) {
    const dim3 g((uint32_t)planes), l(kLanes);
    if (fm)
      sums_kernel<true, false><<<g, l, 0, stream>>>(d_in, n_planes, n_frames, n_bins, stride, d_lengths, d_fill);
    else if (vec)
      sums_kernel<false, true><<<g, l, 0, stream>>>(d_in, n_planes, n_frames, n_bins, stride, d_lengths, d_fill);
    else
      sums_kernel<false, false><<<g, l, 0, stream>>>(d_in, n_planes, n_frames, n_bins, stride, d_lengths, d_fill);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "specaug sums launch", e);
  }
  if (!blocks) return MP3G_OK;
  const dim3 g((uint32_t)blocks), l(kLanes);
#define MP3G_SA_TM(VEC, INP)                                                                                         \
  tm_kernel<VEC, INP><<<g, l, 0, stream>>>(d_in, d_out, n_planes, n_frames, n_bins, stride, d_lengths, d_desc, flags, \
                                           fill_value, d_fill, chunks, shift)
#define MP3G_SA_FM(V, INP)                                                                                         \
  fm_kernel<V, INP><<<g, l, 0, stream>>>(d_in, d_out, n_planes, n_frames, n_bins, stride, d_lengths, d_desc, flags, \
                                         fill_value, d_fill, chunks, bgroups, shift)
  if (fm) {
    if (vec && inplace) MP3G_SA_FM(4, true);
    else if (vec) MP3G_SA_FM(4, false);
    else if (inplace) MP3G_SA_FM(1, true);
    else MP3G_SA_FM(1, false);
  } else {
    if (vec && inplace) MP3G_SA_TM(true, true);
    else if (vec) MP3G_SA_TM(true, false);
    else if (inplace) MP3G_SA_TM(false, true);
    else MP3G_SA_TM(false, false);
  }
#undef MP3G_SA_TM
#undef MP3G_SA_FM
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "specaug launch", e);
}
