// mfcc.hip -- device side of the Kaldi MFCC features (include/mp3g.h "Kaldi MFCC
// features of decoded rows") and of the per-row normalisation ("Per-row mean
// and variance normalisation"): the upload of the tables the owned front end
// does not have, mp3g_mfcc_execute and mp3g_cmvn_rows.  A translation unit of
// its own: the listings of the other kernels do not see it.
//
// Shape: the filter-bank kernel's (fbank.hip), with its own copy of that front
// end -- the choice fbank.hip made against logmel.hip: the two kernels' register
// budgets stay independent and fbank.hip's listing stays what it was.  One
// workgroup produces tile_frames consecutive frames of one (row, plane): the
// span staged once in LDS (s = scale x, Kaldi's reflection resolved, sample j at
// word j + (j >> skew)), the per-lane mean chain, the DFT of e on
// v_mfma_f32_32x32x2_f32 with the table streamed in fbank_device_table's layout,
// p = fmaf(re, re, im * im) to LDS as [bin][33].  The DFT table is the owned
// mp3g_fbank's own device buffer; the filters come from fbank_device_filters
// into one buffer with this kernel's other small tables.
//
// What follows the power rows:
//   mel, log   items (frame, m) as in fbank.hip, but L = mp3g_logf(max(mel,
//              2^-23)) goes to an LDS tile [tile_frames][M + 1]
//   energy     wave 0 alone, a lane per frame, right after its mean chain and
//              before its DFT: N dependent FMAs over the stage (the raw form
//              reads the samples the mean read; the windowed form forms e[n] as
//              the DFT's operand code does and multiplies by w[n], staged in
//              LDS: the lanes' n differ only where their frames start at
//              different offsets modulo 16, so with hop = 160 every lane reads
//              one word).  le goes to 32 words of LDS.
//              The other waves start their DFT meanwhile.
//   DCT        items (frame group, i), i fastest, so a wave's stores run along
//              cep_stride.  An item is coefficient i of J = 1, 2 or 4 frames --
//              as many as let one round of the lanes cover the tile: J
//              independent chains of M FMAs, each over its frame's L row, that
//              share every read of D.  D is read transposed ([m][n_ceps]: the
//              lanes of one frame group read consecutive words), from LDS where
//              it has at most kMfccDctLdsFloats entries and from global memory
//              otherwise; one multiply by lift[i]; column 0 replaced by le with
//              MP3G_MFCC_USE_ENERGY.
//
// The small tables -- the filters' weights and supports, the lifter, the window
// for the energy after it, D transposed where staged -- are one device buffer
// laid out as they lie in LDS and copied by one loop: a loop per table, or a
// read of the supports or the lifter from global memory in the last stages,
// each pays a trip to memory that nothing hides (DESIGN.md 9g has the timings).
//
// LDS banks (ds_read_b32 and every ds_write: 32 banks, the two 32-lane halves of
// a wave are served apart, equal addresses are one broadcast).  The L tile is
// written at word f (M + 1) + m by lanes on consecutive (f, m): consecutive
// words with one word skipped per frame boundary, so at most two lanes of a half
// share a bank, once per boundary inside the half.  The DCT reads L[f][m] at one
// m for all lanes: the lanes of a frame group read one word and the groups of a
// half are M + 1 words apart -- distinct banks while (M + 1) g mod 32 are
// distinct over the ceil(32 / n_ceps) + 1 groups a half can touch, which an odd
// M + 1 (M = 40, 80, 128) always gives and M + 1 = 24 gives for four groups
// (n_ceps >= 11); n_ceps = 1 with M = 23 is the worst case, eight lanes to a
// bank.  D transposed is read at word m n_ceps + i: the lanes of a half cover at
// most 32 consecutive i modulo n_ceps, so no two share a bank for n_ceps <= 32
// and at most two do for n_ceps up to 64.  Three workgroup barriers, every wave
// passes each once; no atomics, no loop bound that depends on data, one launch.
//
// mp3g_cmvn_rows is a plain two-pass kernel, a lane per (plane, column).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "fbank_log.h"
#include "mfcc.h"

namespace mp3g {
namespace {

constexpr uint32_t kMaxLanes = 64 * kLogmelMaxWaves;
constexpr uint32_t kMaxPlanesPerLaunch = 32768;
// The largest dynamic LDS any configuration asks for: the filter-bank kernel's
// (P = 1024: 512 bins, at most 1,024 weights), the largest L tile (32 frames of
// 128 + 1 words), the log energies, and the small tables' most: the lifter,
// the supports, the window (the energy after it), D transposed where staged.
constexpr uint32_t kMaxLdsBytes =
    (kLogmelStageFloats + (MP3G_FBANK_MAX_WINDOW / 2) * (kLogmelPStride + 2) +
     kMfccMaxTileFrames * (MP3G_FBANK_MAX_MELS + 1) + kMfccMaxTileFrames + 4 * MP3G_FBANK_MAX_MELS +
     MP3G_FBANK_MAX_WINDOW + kMfccDctLdsFloats) * 4;
static_assert(kMaxLdsBytes <= 160 * 1024, "the LDS of a CU");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MfccArgs {
  const float* dft;         // fbank_device_table
  const float* aux;         // the small tables, as the kernel lays them out in LDS (mfcc_device_upload)
  const float* dct;         // [n_mels][n_ceps]: D transposed
  uint32_t N, n_pad, hop, n_mels, K, tile_frames, span, skew, stage, tiles, n_weights, remove_dc, reflect;
  uint32_t n_ceps, n_aux, energy, dct_in_lds;  // energy: 0 none, 1 raw, 2 windowed
  int32_t shift;            // frame 0's first sample: 0, or hop / 2 - N / 2 without SNIP_EDGES
  float scale, npre, rN;    // npre = -preemph
  float lef;                // the log energy's floor (-inf: none)
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

// The frame's energy: en = fmaf(v[n], v[n], en), n ascending over the stage from
// jf, with v = d (raw) or w[n] e[n] (windowed), d and e formed as the DFT's
// operand code forms them.  dprev carries d[n - 1]; d[-1] is d[0].
template <bool kWindowed>
__device__ inline float energy_chain(const float* s_x, uint32_t jf, uint32_t N, uint32_t skew, float mean, float npre,
                                     const float* win) {
  float en = 0.f;
  float dprev = __builtin_fmaf(mean, -1.0f, s_x[jf + (jf >> skew)]);
  uint32_t j = jf, n = 0;
  auto term = [&](float s) {
    const float d = __builtin_fmaf(mean, -1.0f, s);
    float v = d;
    if (kWindowed) {
      const float e = __builtin_fmaf(npre, dprev, d);
      v = win[n] * e;
      dprev = d;
    }
    en = __builtin_fmaf(v, v, en);
    n++;
  };
  // (the mean chain's walk: sixteen samples from a multiple of 16 share their pad offset)
  const uint32_t jend = jf + N, jhead = min(jend, (jf + 15) & ~15u);
  for (; j < jhead; j++) term(s_x[j + (j >> skew)]);
  for (; j + 16 <= jend; j += 16) {
    const float* p = s_x + j + (j >> skew);
    float s[16];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) s[u] = p[u];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) term(s[u]);
  }
  for (; j < jend; j++) term(s_x[j + (j >> skew)]);
  return en;
}

// The DCT stage.  An item is one coefficient q of J frames fg, fg + G, ..: J
// independent chains c = fmaf(D[q][m], L[f][m], c) over m ascending that share
// every read of D.  Items run with q fastest, so a wave's stores are contiguous
// along cep_stride.  dt is D transposed, row stride n_ceps.  (A frame past
// `valid` repeats the last one and is not stored.)
template <int J>
__device__ inline void dct_items(const float* __restrict__ dt, uint32_t n_ceps, uint32_t M, const float* s_l,
                                 const float* s_lift, const float* s_le, bool energy, float* __restrict__ o,
                                 uint32_t valid, uint32_t cep_stride, uint32_t tid, uint32_t lanes) {
  const uint32_t G = (valid + J - 1) / J, lrow = M + 1;
  for (uint32_t i = tid; i < G * n_ceps; i += lanes) {
    const uint32_t fg = i / n_ceps, q = i - fg * n_ceps;
    const float* d = dt + q;
    const float* L[J];
    float c[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
      L[j] = s_l + min(fg + j * G, valid - 1) * lrow;
      c[j] = 0.f;
    }
    uint32_t m = 0;
    for (; m + 4 <= M; m += 4) {
      float dv[4], lv[J][4];
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) {
        dv[u] = d[(size_t)(m + u) * n_ceps];
#pragma unroll
        for (int j = 0; j < J; j++) lv[j][u] = L[j][m + u];
      }
#pragma unroll
      for (uint32_t u = 0; u < 4; u++)
#pragma unroll
        for (int j = 0; j < J; j++) c[j] = __builtin_fmaf(dv[u], lv[j][u], c[j]);
    }
    for (; m < M; m++) {
      const float dv = d[(size_t)m * n_ceps];
#pragma unroll
      for (int j = 0; j < J; j++) c[j] = __builtin_fmaf(dv, L[j][m], c[j]);
    }
    const float lift = s_lift[q];
#pragma unroll
    for (int j = 0; j < J; j++) {
      const uint32_t f = fg + j * G;
      float y = c[j] * lift;
      if (energy && q == 0) y = s_le[min(f, valid - 1)];
      if (f < valid) o[(size_t)f * cep_stride + q] = y;
    }
  }
}

__global__ __launch_bounds__(kMaxLanes) void mfcc_kernel(const float* __restrict__ src, uint32_t T,
                                                      float* __restrict__ out, uint32_t n_frames,
                                                      uint32_t cep_stride, MfccArgs a, uint32_t plane0) {
  extern __shared__ float smem[];
  float* s_x = smem;                               // [stage]
  float* s_p = smem + a.stage;                     // [K][33]
  float* s_w = s_p + a.K * kLogmelPStride;         // a.aux: [n_weights], ...
  uint32_t* s_sup = reinterpret_cast<uint32_t*>(s_w + a.n_weights);  // ... [n_mels][3] = lo, hi, offset, ...
  float* s_lift = s_w + a.n_weights + 3 * a.n_mels;  // ... [n_ceps], ...
  float* s_win = s_lift + a.n_ceps;                // ... [N] for the windowed energy, ...
  float* s_d = s_win + (a.energy == 2 ? a.N : 0);  // ... [n_mels][n_ceps] where staged
  float* s_l = s_w + a.n_aux;                      // [tile_frames][n_mels + 1]
  float* s_le = s_l + a.tile_frames * (a.n_mels + 1);  // [32]
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lanes = blockDim.x;
  const uint32_t f0 = blockIdx.x * a.tile_frames;  // < n_frames (the grid)
  const size_t plane = (size_t)plane0 + blockIdx.y;
  const float* __restrict__ srow = src + plane * T;
  float* __restrict__ orow = out + plane * n_frames * cep_stride;

  // s = scale x over samples [f0 hop + shift, .. + span) of the row, reflected
  // Kaldi's way about its ends; frames past the last available one and the
  // n >= N padding read zeros (fbank.hip)
  const int64_t base = (int64_t)f0 * a.hop + a.shift;
  const int64_t len = (int64_t)T;  // (T >= N: the row has a frame)
  for (uint32_t i0 = tid; i0 < a.span; i0 += 8 * lanes) {
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
  // The small tables in one copy, eight loads in flight: the weights, and the
  // supports and the lifter too -- a global load in the last stages is latency
  // nothing hides, and a loop per table pays a trip to memory each.
  for (uint32_t i0 = tid; i0 < a.n_aux; i0 += 8 * lanes) {
    float v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) v[u] = a.aux[min(i0 + u * lanes, a.n_aux - 1)];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++)
      if (i0 + u * lanes < a.n_aux) s_w[i0 + u * lanes] = v[u];
  }
  __syncthreads();

  // lane l holds A[frame l & 31][n = 2 n2 + (l >> 5)] and B[that n][bin l & 31]
  const uint32_t col = lane & 31, half = lane >> 5;
  const uint32_t jf = min(col, a.tile_frames - 1) * a.hop;  // the lane's frame in the stage
  // the frame's mean: sum = fmaf(s[n], 1, sum) over n ascending, times rN
  float mean = 0.f;
  if (a.remove_dc) {
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

  // the log energy, once per frame: wave 0 (a wave-uniform branch, no barrier inside)
  if (a.energy && wave == 0) {
    const float en = a.energy == 1 ? energy_chain<false>(s_x, jf, a.N, a.skew, mean, a.npre, s_win)
                                   : energy_chain<true>(s_x, jf, a.N, a.skew, mean, a.npre, s_win);
    float le = fbank_log(en);
    le = le < a.lef ? a.lef : le;
    if (half == 0) s_le[col] = le;
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

  // mel, log: item i = (frame, m), m fastest, into the L tile
  const uint32_t valid = min(a.tile_frames, n_frames - f0);
  const uint32_t lrow = a.n_mels + 1;
  for (uint32_t i = tid; i < valid * a.n_mels; i += lanes) {
    const uint32_t f = i / a.n_mels, m = i - f * a.n_mels;
    const uint32_t lo = s_sup[3 * m], hi = s_sup[3 * m + 1];
    const float* w = s_w + s_sup[3 * m + 2] - lo;  // w[k], k in [lo, hi]
    const float* p = s_p + f;
    float mel = 0.f;
    for (uint32_t k = lo; k <= hi; k++) mel = __builtin_fmaf(w[k], p[k * kLogmelPStride], mel);
    s_l[f * lrow + m] = fbank_log(mel);
  }
  __syncthreads();

  // DCT, lifter, c0: as many frames to an item as let one round of the
  // workgroup's lanes cover the tile (1, 2 or 4)
  {
    const uint32_t total = valid * a.n_ceps;
    float* o = orow + (size_t)f0 * cep_stride;
    const bool e = a.energy != 0;
    if (a.dct_in_lds) {
      if (total <= lanes)
        dct_items<1>(s_d, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
      else if (total <= 2 * lanes)
        dct_items<2>(s_d, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
      else
        dct_items<4>(s_d, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
    } else {
      if (total <= lanes)
        dct_items<1>(a.dct, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
      else if (total <= 2 * lanes)
        dct_items<2>(a.dct, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
      else
        dct_items<4>(a.dct, a.n_ceps, a.n_mels, s_l, s_lift, s_le, e, o, valid, cep_stride, tid, lanes);
    }
  }
}

// One lane per (plane, column), consecutive lanes on consecutive columns: a
// frame's columns are one coalesced read.  Two passes over the row's own frames.
__global__ __launch_bounds__(256) void cmvn_kernel(float* __restrict__ feats, uint64_t n_items, uint32_t n_planes,
                                                   uint32_t n_frames, uint32_t stride, uint32_t n_cols,
                                                   const uint32_t* __restrict__ lengths, uint32_t norm_vars) {
  const uint64_t item = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= n_items) return;
  const uint64_t plane = item / n_cols;
  const uint32_t c = (uint32_t)(item - plane * n_cols);
  const uint32_t n = min(lengths[plane / n_planes], n_frames);
  if (n == 0) return;
  float* x = feats + (size_t)plane * n_frames * stride + c;
  // (sixteen loads in flight, then their additions in order: a lane's frames are
  // `stride` words apart and each load is a trip to memory)
  double sum = 0.0, sq = 0.0;
  uint32_t f = 0;
  for (; f + 16 <= n; f += 16) {
    float v[16];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) v[u] = x[(size_t)(f + u) * stride];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) {
      sum += (double)v[u];
      sq += (double)v[u] * (double)v[u];
    }
  }
  for (; f < n; f++) {
    const double v = (double)x[(size_t)f * stride];
    sum += v;
    sq += v * v;
  }
  const double mean = sum / (double)n;
  float scale = 1.0f;
  if (norm_vars) {
    const double var = sq / (double)n - mean * mean;
    const float v32 = (float)var;
    const float vf = v32 > 1e-20f ? v32 : 1e-20f;
    scale = 1.0f / __builtin_sqrtf(vf);
  }
  for (f = 0; f + 16 <= n; f += 16) {
    float v[16];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) v[u] = x[(size_t)(f + u) * stride];
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) {
      float y = (float)((double)v[u] - mean);
      if (norm_vars) y = y * scale;
      x[(size_t)(f + u) * stride] = y;
    }
  }
  for (; f < n; f++) {
    float y = (float)((double)x[(size_t)f * stride] - mean);
    if (norm_vars) y = y * scale;
    x[(size_t)f * stride] = y;
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

// the kernel's dynamic LDS: the stage, the power rows, the small tables, the L tile, the log energies
bool windowed_energy(const mp3g_mfcc& mf) {
  return (mf.flags & MP3G_MFCC_USE_ENERGY) && !(mf.flags & MP3G_MFCC_RAW_ENERGY);
}
// the small tables of a.aux: the filters' weights and supports, the lifter, the
// window for the energy after it, D transposed where staged
uint32_t aux_floats(const mp3g_mfcc& mf) {
  const mp3g_fbank& fb = *mf.fb;
  return fb.n_weights + 3 * fb.n_mels + mf.n_ceps + (windowed_energy(mf) ? fb.N : 0) +
         (mf.dct_in_lds ? fb.n_mels * mf.n_ceps : 0);
}
uint32_t lds_bytes(const mp3g_mfcc& mf) {
  const mp3g_fbank& fb = *mf.fb;
  return (fb.geom.stage + fb.K * kLogmelPStride + aux_floats(mf) + fb.geom.tile_frames * (fb.n_mels + 1) +
          kMfccMaxTileFrames) *
         (uint32_t)sizeof(float);
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

// (the owned mp3g_fbank was created on the same device: the device is a gfx950
// and the front end's tables are uploaded)
int mfcc_device_upload(mp3g_mfcc* mf) {
  const mp3g_fbank& fb = *mf->fb;
  const uint32_t M = fb.n_mels, C = mf->n_ceps;
  mf->dct_in_lds = M * C <= kMfccDctLdsFloats ? 1u : 0u;
  if (fb.geom.tile_frames > kMfccMaxTileFrames || lds_bytes(*mf) > kMaxLdsBytes)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "mfcc: the tile does not fit the LDS");
  std::vector<float> dt((size_t)M * C), aux;
  for (uint32_t i = 0; i < C; i++)
    for (uint32_t m = 0; m < M; m++) dt[(size_t)m * C + i] = mf->dct[(size_t)i * M + m];
  std::vector<uint32_t> support;
  fbank_device_filters(fb, &aux, &support);  // (fb.n_weights floats: the front end's own upload counted them)
  const size_t at = aux.size();
  aux.resize(at + support.size());
  std::memcpy(aux.data() + at, support.data(), support.size() * sizeof(uint32_t));
  aux.insert(aux.end(), mf->lift.begin(), mf->lift.end());
  if (windowed_energy(*mf)) aux.insert(aux.end(), fb.w.begin(), fb.w.end());
  if (mf->dct_in_lds) aux.insert(aux.end(), dt.begin(), dt.end());
  if (aux.size() != aux_floats(*mf)) return abi_fail(MP3G_ERR_DEVICE, "mfcc: table sizes");
  DeviceScope scope(fb.device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  // (the long transforms stage more than the 64 KB a kernel gets by default)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mfcc_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "hipFuncSetAttribute(mfcc)", e);
  int st = upload(dt, reinterpret_cast<void**>(&mf->d_dct), "mfcc DCT matrix");
  if (st == MP3G_OK) st = upload(aux, reinterpret_cast<void**>(&mf->d_aux), "mfcc small tables");
  if (st != MP3G_OK) mfcc_device_free(mf);
  return st;
}

void mfcc_device_free(mp3g_mfcc* mf) {
  DeviceScope scope(mf->fb->device);
  (void)hipFree(mf->d_dct);
  (void)hipFree(mf->d_aux);
  mf->d_dct = mf->d_aux = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_mfcc_execute(const mp3g_mfcc* mf, const float* d_src, uint32_t n_rows, uint32_t n_planes,
                                 uint32_t T, float* d_out, uint32_t n_frames, uint32_t cep_stride,
                                 void* hip_stream) {
  if (!mf) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null mfcc");
  const mp3g_fbank* fb = mf->fb;
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: 1 or 2 planes");
  if (fb->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: a host-only object");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "mfcc: rows of 2^31 samples or more");
  if (n_frames > mp3g_fbank_frames(fb, T))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: more frames than the rows have");
  if (cep_stride < mf->n_ceps) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: cepstral stride below n_ceps");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  if (planes >= (1ull << 32)) return abi_fail(MP3G_ERR_UNSUPPORTED, "mfcc: 2^32 planes or more");
  if (planes == 0 || n_frames == 0) return MP3G_OK;
  if (!d_src || !d_out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  DeviceScope scope(fb->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const FbankGeom& g = fb->geom;
  const bool snip = fb->flags & MP3G_FBANK_SNIP_EDGES;
  MfccArgs a = {};
  a.dft = fb->d_dft;
  a.aux = mf->d_aux;
  a.dct = mf->d_dct;
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
  a.n_ceps = mf->n_ceps;
  a.n_aux = aux_floats(*mf);
  a.energy = !(mf->flags & MP3G_MFCC_USE_ENERGY) ? 0u : windowed_energy(*mf) ? 2u : 1u;
  a.dct_in_lds = mf->dct_in_lds;
  a.shift = snip ? 0 : (int32_t)(fb->hop / 2) - (int32_t)(fb->N / 2);
  a.scale = fb->scale;
  a.npre = -fb->preemph;
  a.rN = fb->rN;
  a.lef = mf->energy_floor > 0.f ? mf->lef : -__builtin_inff();
  const uint32_t tiles = (n_frames + g.tile_frames - 1) / g.tile_frames;
  // (one launch for up to 32,768 planes: the grid's second dimension)
  for (uint64_t base = 0; base < planes; base += kMaxPlanesPerLaunch) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(planes - base, kMaxPlanesPerLaunch);
    mfcc_kernel<<<dim3(tiles, n), 64 * g.waves, lds_bytes(*mf), stream>>>(d_src, T, d_out, n_frames, cep_stride, a,
                                                                    (uint32_t)base);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "mfcc launch", e);
  }
  return MP3G_OK;
}

extern "C" int mp3g_cmvn_rows(int device, float* d_feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                              uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths, uint32_t flags,
                              void* hip_stream) {
  if (flags & ~(uint32_t)MP3G_CMVN_NORM_VARS) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: unknown flag");
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: stride below n_cols");
  if (!n_rows || !n_planes || !n_frames || !n_cols) return MP3G_OK;
  if (!d_feats || !d_lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: null device buffer");
  const uint64_t planes = (uint64_t)n_rows * n_planes;
  const uint64_t items = planes * n_cols, blocks = (items + 255) / 256;
  if (planes >= (1ull << 32) || blocks >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "cmvn: too many columns");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  cmvn_kernel<<<(uint32_t)blocks, 256, 0, static_cast<hipStream_t>(hip_stream)>>>(
      d_feats, items, n_planes, n_frames, stride, n_cols, d_lengths, flags & MP3G_CMVN_NORM_VARS);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "cmvn launch", e);
}
