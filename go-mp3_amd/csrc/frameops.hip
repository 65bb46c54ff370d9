// frameops.hip -- the frame-level steps between the MFCC features and a speaker
// network (include/mp3g.h "Sliding-window CMN, energy VAD and voiced-frame
// selection"): Kaldi's apply-cmvn-sliding, compute-vad-energy and
// select-voiced-frames on a time-major feature tensor.  The kernels, their
// launchers and the host references they equal bit for bit; frameops.h holds the
// window rule and the blocked sums both sides compile.  A translation unit of its
// own: the listings of the other kernels do not see it.
//
// scmn_kernel, ONE launch, a workgroup per (plane, group of 16 columns) over the
// whole row.  Columns are independent, so splitting the columns needs no exchange
// between workgroups; splitting the frames would need the block prefixes of
// everything before a chunk, that is a second launch and a device workspace.
// 16 columns are one 64-byte segment of a frame, so a wave's loads still come as
// whole segments, and a batch of few long rows still fills the device (128 planes
// of 30 columns: 256 workgroups).
//   copy    frames f >= n of the live columns, in to out
//   pass A  item (block j, column c), c fastest: b[j] of the full blocks -- 32
//           loads, sixteen in flight, added in ascending order -- to LDS at j + 1
//   pass B  lanes 0..15 (the sums) and 16..31 (the squares) of wave 0 turn b into
//           Bp in place: n / 32 dependent float64 additions out of LDS
//   pass C  item (run of 32 consecutive t, column c), c fastest: the two prefix
//           chains P[s] and P[e] are started at their blocks' first frames (at
//           most 31 additions each) and walked forward; s and e grow by at most
//           one per frame, so a batch of eight frames issues its 24 loads (x[t],
//           the frame s passed, the frame e passed) before its additions.  A step
//           of more than one frame, which the window rule does not produce, would
//           take the general walk.
// LDS: (n_frames / 32 + 1) x 16 doubles, twice with NORM_VARS -- 160 KB hold
// 20,479 frames with NORM_VARS and 40,959 without; longer rows are refused.  Two
// workgroup barriers, every wave passes each once; no atomics.
//
// vad_kernel, one launch, a workgroup per plane: the column's block sums 256 at a
// time into LDS and lane 0 adds them in order (the threshold wants one number per
// plane); then a lane per frame counts its context -- (2 c + 1) loads, clipped to
// the row -- and the ones are counted by ballot and popcount, wave totals through
// LDS, a running count carried over the chunks of 256 frames.
//
// select_kernel, one launch, a workgroup per (plane, group of 16 columns): the
// same scan gives every voiced frame of a chunk its place; the chunk's source
// frames go to LDS in output order and all lanes copy (frame, column) items,
// column fastest.  Every column group repeats the scan of the flags -- one byte
// per frame -- instead of exchanging it.  Integer sums: no order to keep.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "abi_util.h"
#include "frameops.h"

namespace mp3g {
namespace {

constexpr uint32_t kCols = 16;     // columns of a workgroup
constexpr uint32_t kRun = 32;      // frames of a pass-C item
constexpr uint32_t kLanes = 256;   // lanes of a workgroup
constexpr uint32_t kWaves = kLanes / 64;
constexpr uint32_t kScmnMaxLdsBytes = 160 * 1024;

// Walks `ch` forward to `target` (<= last + 1), eight loads in flight.
__device__ inline void chain_walk(PrefixChain& ch, const float* __restrict__ xc, size_t stride, uint32_t target,
                                  uint32_t last) {
  while (ch.pos < target) {
    const uint32_t p = ch.pos;
    float v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) v[u] = xc[(size_t)min(p + u, last) * stride];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++)
      if (p + u < target) ch.add(v[u]);
  }
}

__global__ __launch_bounds__(kLanes) void scmn_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                                                      uint32_t n_cols, uint32_t groups,
                                                      const uint32_t* __restrict__ lengths, uint32_t W,
                                                      uint32_t min_window, uint32_t center, uint32_t norm_vars) {
  extern __shared__ double s_bp[];  // [n_frames / 32 + 1][kCols]: Bp; with norm_vars the squares' after it
  const uint32_t tid = threadIdx.x;
  const uint32_t plane = blockIdx.x / groups, g = blockIdx.x - plane * groups;
  const uint32_t c0 = g * kCols, cw = min(kCols, n_cols - c0);
  const uint32_t n = min(lengths[plane / n_planes], n_frames);
  const size_t base = (size_t)plane * n_frames * stride + c0;
  const float* __restrict__ x = in + base;
  float* __restrict__ y = out + base;
  double* s_bp2 = s_bp + (size_t)(n_frames / kFrameBlock + 1) * kCols;

  // frames past the row's length: copied
  for (uint32_t i = tid; i < (n_frames - n) * cw; i += kLanes) {
    const uint32_t f = n + i / cw, c = i % cw;
    y[(size_t)f * stride + c] = x[(size_t)f * stride + c];
  }
  if (n == 0) return;  // (the whole workgroup)

  // pass A: b[j] of the full blocks, at j + 1
  const uint32_t nfull = n / kFrameBlock;
  for (uint32_t i = tid; i < nfull * cw; i += kLanes) {
    const uint32_t j = i / cw, c = i % cw;
    const float* p = x + (size_t)j * kFrameBlock * stride + c;
    double b = 0.0, b2 = 0.0;
#pragma unroll
    for (uint32_t h = 0; h < kFrameBlock; h += 16) {
      float v[16];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) v[u] = p[(size_t)(h + u) * stride];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) {
        const double d = (double)v[u];
        b += d;
        b2 += d * d;
      }
    }
    s_bp[(j + 1) * kCols + c] = b;
    if (norm_vars) s_bp2[(j + 1) * kCols + c] = b2;
  }
  __syncthreads();

  // pass B: Bp[j + 1] = Bp[j] + b[j], in place
  if ((tid & (kCols - 1)) < cw && (tid < kCols || (norm_vars && tid < 2 * kCols))) {
    double* s = tid < kCols ? s_bp + tid : s_bp2 + (tid - kCols);
    double acc = 0.0;
    s[0] = acc;
    for (uint32_t j = 1; j <= nfull; j++) {
      acc += s[j * kCols];
      s[j * kCols] = acc;
    }
  }
  __syncthreads();

  // pass C: runs of kRun frames
  const uint32_t runs = (n + kRun - 1) / kRun, last = n - 1;
  for (uint32_t i = tid; i < runs * cw; i += kLanes) {
    const uint32_t r = i / cw, c = i % cw;
    const float* __restrict__ xc = x + c;
    float* __restrict__ yc = y + c;
    const uint32_t t0 = r * kRun, tend = min(t0 + kRun, n);
    uint32_t s, e;
    scmn_window(t0, n, W, min_window, center, &s, &e);
    PrefixChain cs, ce;
    cs.start(s & ~(kFrameBlock - 1));
    ce.start(e & ~(kFrameBlock - 1));
    chain_walk(cs, xc, stride, s, last);
    chain_walk(ce, xc, stride, e, last);
    for (uint32_t tb = t0; tb < tend; tb += 8) {
      uint32_t ss[8], ee[8];
      float vx[8], vs[8], ve[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        const uint32_t t = min(tb + u, last);
        scmn_window(t, n, W, min_window, center, &ss[u], &ee[u]);
        vx[u] = xc[(size_t)t * stride];
        vs[u] = xc[(size_t)(max(ss[u], 1u) - 1) * stride];  // the frame s passed, if it moved
        ve[u] = xc[(size_t)(ee[u] - 1) * stride];           // the frame e passed, if it moved (e >= 1)
      }
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        if (tb + u < tend) {
          if (cs.pos + 1 == ss[u]) cs.add(vs[u]);
          if (ce.pos + 1 == ee[u]) ce.add(ve[u]);
          chain_walk(cs, xc, stride, ss[u], last);  // (a longer step: the window rule has none)
          chain_walk(ce, xc, stride, ee[u], last);
          const uint32_t js = (ss[u] / kFrameBlock) * kCols + c, je = (ee[u] / kFrameBlock) * kCols + c;
          const double Ps = s_bp[js] + cs.part, Pe = s_bp[je] + ce.part;
          double P2s = 0.0, P2e = 0.0;
          if (norm_vars) {
            P2s = s_bp2[js] + cs.part2;
            P2e = s_bp2[je] + ce.part2;
          }
          yc[(size_t)(tb + u) * stride] = scmn_value(vx[u], Ps, Pe, P2s, P2e, ee[u] - ss[u], norm_vars);
        }
      }
    }
  }
}

// The ones among the workgroup's flags, every lane's count of the ones before it
// (*before) included: ballot and popcount in the wave, the waves' totals through
// s_tot[kWaves].  Two barriers; every lane of the workgroup calls it.
__device__ inline uint32_t block_count(bool flag, uint32_t* s_tot, uint32_t* before) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(flag);
  const uint32_t in_wave = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();  // (the last call's totals have been read)
  if (lane == 0) s_tot[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t total = 0, wbase = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; w++) {
    const uint32_t c = s_tot[w];
    wbase += w < wave ? c : 0u;
    total += c;
  }
  *before = wbase + in_wave;
  return total;
}

__global__ __launch_bounds__(kLanes) void vad_kernel(const float* __restrict__ in, uint32_t n_planes, uint32_t n_frames,
                                                     uint32_t stride, uint32_t col,
                                                     const uint32_t* __restrict__ lengths, float energy_threshold,
                                                     float energy_mean_scale, float proportion_threshold,
                                                     uint32_t context, uint8_t* __restrict__ voiced,
                                                     uint32_t* __restrict__ counts) {
  __shared__ double s_b[kLanes];
  __shared__ float s_thr;
  __shared__ uint32_t s_tot[kWaves];
  const uint32_t tid = threadIdx.x, plane = blockIdx.x;
  const uint32_t n = min(lengths[plane / n_planes], n_frames);
  const float* __restrict__ xc = in + (size_t)plane * n_frames * stride + col;
  uint8_t* __restrict__ v = voiced + (size_t)plane * n_frames;
  for (uint32_t f = n + tid; f < n_frames; f += kLanes) v[f] = 0;
  if (n == 0) {  // (the whole workgroup)
    if (tid == 0) counts[plane] = 0;
    return;
  }
  float thr = energy_threshold;
  if (energy_mean_scale != 0.f) {  // (a kernel argument: the whole workgroup)
    const uint32_t nfull = n / kFrameBlock;
    double bp = 0.0;  // lane 0's: Bp
    for (uint32_t j0 = 0; j0 < nfull; j0 += kLanes) {
      const uint32_t j = j0 + tid;
      double b = 0.0;
      if (j < nfull) {
        const float* p = xc + (size_t)j * kFrameBlock * stride;
#pragma unroll
        for (uint32_t h = 0; h < kFrameBlock; h += 16) {
          float w[16];
#pragma unroll
          for (uint32_t u = 0; u < 16; u++) w[u] = p[(size_t)(h + u) * stride];
#pragma unroll
          for (uint32_t u = 0; u < 16; u++) b += (double)w[u];
        }
      }
      s_b[tid] = b;
      __syncthreads();
      if (tid == 0) {
        const uint32_t m = min(kLanes, nfull - j0);
        for (uint32_t k = 0; k < m; k++) bp += s_b[k];
      }
      __syncthreads();
    }
    if (tid == 0) {
      double part = 0.0;
      for (uint32_t f = nfull * kFrameBlock; f < n; f++) part += (double)xc[(size_t)f * stride];
      s_thr = vad_threshold(energy_threshold, energy_mean_scale, bp + part, n);
    }
    __syncthreads();
    thr = s_thr;
  }
  uint32_t count = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += kLanes) {
    const uint32_t t = t0 + tid;
    bool vo = false;
    if (t < n) {
      const uint32_t lo = t > context ? t - context : 0u;
      const uint32_t hi = (uint32_t)min((uint64_t)t + context, (uint64_t)n - 1);
      uint32_t num = 0;
      for (uint32_t t2 = lo; t2 <= hi; t2++) num += xc[(size_t)t2 * stride] > thr ? 1u : 0u;
      vo = vad_decision(num, hi - lo + 1, proportion_threshold);
      v[t] = vo ? 1 : 0;
    }
    uint32_t before;
    count += block_count(vo, s_tot, &before);
  }
  if (tid == 0) counts[plane] = count;
}

__global__ __launch_bounds__(kLanes) void select_kernel(const float* __restrict__ in, uint32_t n_planes,
                                                        uint32_t n_frames, uint32_t stride, uint32_t n_cols,
                                                        uint32_t groups, const uint8_t* __restrict__ voiced,
                                                        const uint32_t* __restrict__ lengths, float* __restrict__ out,
                                                        uint32_t n_frames_out, uint32_t stride_out,
                                                        uint32_t* __restrict__ lengths_out) {
  __shared__ uint32_t s_tot[kWaves];
  __shared__ uint32_t s_src[kLanes];
  const uint32_t tid = threadIdx.x;
  const uint32_t plane = blockIdx.x / groups, g = blockIdx.x - plane * groups;
  const uint32_t c0 = g * kCols, cw = min(kCols, n_cols - c0);
  const uint32_t n = min(lengths[plane / n_planes], n_frames);
  const uint8_t* __restrict__ v = voiced + (size_t)plane * n_frames;
  const float* __restrict__ x = in + (size_t)plane * n_frames * stride + c0;
  float* __restrict__ y = out + (size_t)plane * n_frames_out * stride_out + c0;
  uint32_t count = 0;  // the voiced frames before this chunk
  for (uint32_t t0 = 0; t0 < n && count < n_frames_out; t0 += kLanes) {
    const uint32_t t = t0 + tid;
    const bool flag = t < n && v[t] != 0;
    uint32_t before;
    const uint32_t total = block_count(flag, s_tot, &before);
    if (flag) s_src[before] = t;  // (before < total <= kLanes)
    __syncthreads();
    for (uint32_t i = tid; i < total * cw; i += kLanes) {
      const uint32_t jl = i / cw, c = i % cw, j = count + jl;
      if (j < n_frames_out) y[(size_t)j * stride_out + c] = x[(size_t)s_src[jl] * stride + c];
    }
    count += total;
    // (the next chunk writes s_src after block_count's barriers)
  }
  // lengths_out is min(count, n_frames_out): a count cut short at n_frames_out is enough
  const uint32_t m = min(count, n_frames_out);
  for (uint64_t i = tid; i < (uint64_t)(n_frames_out - m) * cw; i += kLanes)
    y[(size_t)(m + i / cw) * stride_out + i % cw] = 0.f;
  if (g == 0 && tid == 0) lengths_out[plane] = m;
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

// The checks the host and the device call share.  *work: whether anything is to be done.
int scmn_check(const float* in, const float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
               uint32_t stride, uint32_t n_cols, const uint32_t* lengths, uint32_t W, uint32_t min_window,
               uint32_t flags, bool* work) {
  *work = false;
  if (flags & ~(uint32_t)(MP3G_SCMN_CENTER | MP3G_SCMN_NORM_VARS))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: unknown flag");
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: stride below n_cols");
  if (W == 0 || min_window == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: a window of no frames");
  if (in && in == out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: out is in (the call is out of place)");
  if (!n_rows || !n_planes || !n_frames || !n_cols) return MP3G_OK;
  if (!in || !out || !lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: null buffer");
  const uint64_t bytes = (uint64_t)n_rows * n_planes * n_frames * stride * sizeof(float);
  if (overlap(in, bytes, out, bytes)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "sliding cmn: out overlaps in");
  *work = true;
  return MP3G_OK;
}

int vad_check(const float* feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
              uint32_t n_cols, uint32_t col, const uint32_t* lengths, const uint8_t* voiced, const uint32_t* counts,
              bool* work) {
  *work = false;
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "vad: stride below n_cols");
  if (col >= n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "vad: col is not below n_cols");
  if (!n_rows || !n_planes) return MP3G_OK;
  if (!lengths || !counts || (n_frames && (!feats || !voiced)))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "vad: null buffer");
  *work = true;
  return MP3G_OK;
}

int select_check(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                 uint32_t n_cols, const uint8_t* voiced, const uint32_t* lengths, const float* out,
                 uint32_t n_frames_out, uint32_t stride_out, const uint32_t* lengths_out, bool* work) {
  *work = false;
  if (stride < n_cols || stride_out < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "select: stride below n_cols");
  if (!n_rows || !n_planes) return MP3G_OK;
  if (!lengths || !lengths_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "select: null buffer");
  const bool reads = n_frames && n_cols && n_frames_out, writes = n_frames_out && n_cols;
  if ((n_frames && !voiced) || (reads && !in) || (writes && !out))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "select: null buffer");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (in && out && overlap(in, planes * n_frames * stride * sizeof(float), out,
                           planes * n_frames_out * stride_out * sizeof(float)))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "select: out overlaps in");
  *work = true;
  return MP3G_OK;
}

// P[0..n] of one column in the blocked order (and the squares' when p2 is given).
void blocked_prefix(const float* xc, size_t stride, uint32_t n, std::vector<double>* p, std::vector<double>* p2) {
  p->resize((size_t)n + 1);
  if (p2) p2->resize((size_t)n + 1);
  double bp = 0.0, bp2 = 0.0;
  PrefixChain ch;
  ch.start(0);
  for (uint32_t f = 0;; f++) {
    (*p)[f] = bp + ch.part;
    if (p2) (*p2)[f] = bp2 + ch.part2;
    if (f == n) break;
    const double b = ch.part + (double)xc[(size_t)f * stride];  // (the block's sum, when f ends it)
    const double b2 = ch.part2 + (double)xc[(size_t)f * stride] * (double)xc[(size_t)f * stride];
    ch.add(xc[(size_t)f * stride]);
    if (ch.pos % kFrameBlock == 0) {
      bp += b;
      bp2 += b2;
    }
  }
}

uint32_t groups_of(uint32_t n_cols) { return (n_cols + kCols - 1) / kCols; }

}  // namespace
}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_sliding_cmn_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes,
                                     uint32_t n_frames, uint32_t stride, uint32_t n_cols, const uint32_t* lengths,
                                     uint32_t cmn_window, uint32_t min_window, uint32_t flags) {
  bool work;
  const int st = scmn_check(in, out, n_rows, n_planes, n_frames, stride, n_cols, lengths, cmn_window, min_window, flags,
                            &work);
  if (st != MP3G_OK || !work) return st;
  const bool center = flags & MP3G_SCMN_CENTER, vars = flags & MP3G_SCMN_NORM_VARS;
  std::vector<double> P, P2;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths[r] < n_frames ? lengths[r] : n_frames;
    for (uint32_t p = 0; p < n_planes; p++) {
      const size_t base = ((size_t)r * n_planes + p) * n_frames * stride;
      for (uint32_t c = 0; c < n_cols; c++) {
        const float* xc = in + base + c;
        float* yc = out + base + c;
        for (uint32_t f = n; f < n_frames; f++) yc[(size_t)f * stride] = xc[(size_t)f * stride];
        if (n == 0) continue;
        blocked_prefix(xc, stride, n, &P, vars ? &P2 : nullptr);
        for (uint32_t t = 0; t < n; t++) {
          uint32_t s, e;
          scmn_window(t, n, cmn_window, min_window, center, &s, &e);
          yc[(size_t)t * stride] = scmn_value(xc[(size_t)t * stride], P[s], P[e], vars ? P2[s] : 0.0,
                                              vars ? P2[e] : 0.0, e - s, vars);
        }
      }
    }
  }
  return MP3G_OK;
}

extern "C" int mp3g_sliding_cmn_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                                     uint32_t n_frames, uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths,
                                     uint32_t cmn_window, uint32_t min_window, uint32_t flags, void* hip_stream) {
  bool work;
  const int st = scmn_check(d_in, d_out, n_rows, n_planes, n_frames, stride, n_cols, d_lengths, cmn_window, min_window,
                            flags, &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  const bool vars = flags & MP3G_SCMN_NORM_VARS;
  const uint64_t planes = (uint64_t)n_rows * n_planes, blocks = planes * groups_of(n_cols);
  if (planes >= (1ull << 32) || blocks >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "sliding cmn: too many columns");
  const uint64_t lds = (uint64_t)(n_frames / kFrameBlock + 1) * kCols * sizeof(double) * (vars ? 2 : 1);
  if (lds > kScmnMaxLdsBytes) return abi_fail(MP3G_ERR_UNSUPPORTED, "sliding cmn: the row's block sums do not fit the LDS");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  if (lds > 64 * 1024) {  // (more than a kernel gets by default)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(scmn_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kScmnMaxLdsBytes);
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "hipFuncSetAttribute(sliding cmn)", e);
  }
  scmn_kernel<<<(uint32_t)blocks, kLanes, (size_t)lds, static_cast<hipStream_t>(hip_stream)>>>(
      d_in, d_out, n_planes, n_frames, stride, n_cols, groups_of(n_cols), d_lengths, cmn_window, min_window,
      (flags & MP3G_SCMN_CENTER) ? 1u : 0u, vars ? 1u : 0u);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "sliding cmn launch", e);
}

extern "C" int mp3g_vad_energy_host(const float* feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                                    uint32_t stride, uint32_t n_cols, uint32_t col, const uint32_t* lengths,
                                    float energy_threshold, float energy_mean_scale, float proportion_threshold,
                                    uint32_t frames_context, uint8_t* voiced, uint32_t* counts) {
  bool work;
  const int st = vad_check(feats, n_rows, n_planes, n_frames, stride, n_cols, col, lengths, voiced, counts, &work);
  if (st != MP3G_OK || !work) return st;
  std::vector<double> P;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths[r] < n_frames ? lengths[r] : n_frames;
    for (uint32_t p = 0; p < n_planes; p++) {
      const size_t plane = (size_t)r * n_planes + p;
      const float* xc = feats + plane * n_frames * stride + col;
      uint8_t* v = voiced + plane * n_frames;
      for (uint32_t f = n; f < n_frames; f++) v[f] = 0;
      uint32_t count = 0;
      if (n) {
        float thr = energy_threshold;
        if (energy_mean_scale != 0.f) {
          blocked_prefix(xc, stride, n, &P, nullptr);
          thr = vad_threshold(energy_threshold, energy_mean_scale, P[n], n);
        }
        for (uint32_t t = 0; t < n; t++) {
          const uint32_t lo = t > frames_context ? t - frames_context : 0u;
          const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)t + frames_context, (uint64_t)n - 1);
          uint32_t num = 0;
          for (uint32_t t2 = lo; t2 <= hi; t2++) num += xc[(size_t)t2 * stride] > thr ? 1u : 0u;
          v[t] = vad_decision(num, hi - lo + 1, proportion_threshold) ? 1 : 0;
          count += v[t];
        }
      }
      counts[plane] = count;
    }
  }
  return MP3G_OK;
}

extern "C" int mp3g_vad_energy_rows(int device, const float* d_feats, uint32_t n_rows, uint32_t n_planes,
                                    uint32_t n_frames, uint32_t stride, uint32_t n_cols, uint32_t col,
                                    const uint32_t* d_lengths, float energy_threshold, float energy_mean_scale,
                                    float proportion_threshold, uint32_t frames_context, uint8_t* d_voiced,
                                    uint32_t* d_counts, void* hip_stream) {
  bool work;
  const int st = vad_check(d_feats, n_rows, n_planes, n_frames, stride, n_cols, col, d_lengths, d_voiced, d_counts,
                           &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "vad: 2^31 planes or more");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  vad_kernel<<<(uint32_t)planes, kLanes, 0, static_cast<hipStream_t>(hip_stream)>>>(
      d_feats, n_planes, n_frames, stride, col, d_lengths, energy_threshold, energy_mean_scale, proportion_threshold,
      frames_context, d_voiced, d_counts);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "vad launch", e);
}

extern "C" int mp3g_select_frames_host(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                                       uint32_t stride, uint32_t n_cols, const uint8_t* voiced,
                                       const uint32_t* lengths, float* out, uint32_t n_frames_out,
                                       uint32_t stride_out, uint32_t* lengths_out) {
  bool work;
  const int st = select_check(in, n_rows, n_planes, n_frames, stride, n_cols, voiced, lengths, out, n_frames_out,
                              stride_out, lengths_out, &work);
  if (st != MP3G_OK || !work) return st;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths[r] < n_frames ? lengths[r] : n_frames;
    for (uint32_t p = 0; p < n_planes; p++) {
      const size_t plane = (size_t)r * n_planes + p;
      const uint8_t* v = voiced + plane * n_frames;
      const float* x = in + plane * n_frames * stride;
      float* y = out + plane * n_frames_out * stride_out;
      uint32_t m = 0;
      for (uint32_t t = 0; t < n && m < n_frames_out; t++) {
        if (!v[t]) continue;
        for (uint32_t c = 0; c < n_cols; c++) y[(size_t)m * stride_out + c] = x[(size_t)t * stride + c];
        m++;
      }
      for (uint32_t j = m; j < n_frames_out; j++)
        for (uint32_t c = 0; c < n_cols; c++) y[(size_t)j * stride_out + c] = 0.f;
      lengths_out[plane] = m;
    }
  }
  return MP3G_OK;
}

extern "C" int mp3g_select_frames_rows(int device, const float* d_in, uint32_t n_rows, uint32_t n_planes,
                                       uint32_t n_frames, uint32_t stride, uint32_t n_cols, const uint8_t* d_voiced,
                                       const uint32_t* d_lengths, float* d_out, uint32_t n_frames_out,
                                       uint32_t stride_out, uint32_t* d_lengths_out, void* hip_stream) {
  bool work;
  const int st = select_check(d_in, n_rows, n_planes, n_frames, stride, n_cols, d_voiced, d_lengths, d_out,
                              n_frames_out, stride_out, d_lengths_out, &work);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (!work) return MP3G_OK;
  // (no columns: one group still counts the frames)
  const uint32_t groups = std::max(1u, groups_of(n_cols));
  const uint64_t planes = (uint64_t)n_rows * n_planes, blocks = planes * groups;
  if (planes >= (1ull << 32) || blocks >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "select: too many columns");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  select_kernel<<<(uint32_t)blocks, kLanes, 0, static_cast<hipStream_t>(hip_stream)>>>(
      d_in, n_planes, n_frames, stride, n_cols, groups, d_voiced, d_lengths, d_out, n_frames_out, stride_out,
      d_lengths_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "select launch", e);
}
