// loudness.hip -- device side of the BS.1770 loudness measure and the gain stage
// (include/mp3g.h "Integrated loudness of decoded rows").
//
// loudness_segment_kernel: one lane per (row, plane, 100 ms segment) runs the
// K-weighting over its H samples from zero state, in the arithmetic of
// loudness_filter.h.  The lanes of a wave share the sample index n, so V[n][.]
// is one uniform 32-byte address per step: a broadcast read of the strip's 1 KB
// of V, which the wave stages in LDS with the samples (a scalar load from L2 in
// the loop was waited for at every sample).  A lane's samples lie H floats from
// its neighbour's, so a wave stages kLoudChunk = 32 samples of each of its 64
// items through LDS: eight lanes fetch one item's 128-byte strip as eight
// 16-byte words (eight items per load instruction, 4-byte aligned addresses)
// and store the floats in the item's row of kLoudLdsStride = 33 dwords -- odd,
// so the 32 lanes of a half wave read 32 different banks, and a half wave's
// stores (4 items x 8 words) fall on 32 different banks too.  The next strip's
// loads are issued before the current strip is filtered and land in registers.
//
// loudness_row_kernel: one lane per (row, plane) scans the segments in order
// (the 4 x 4 state recurrence), then one lane per row forms the blocks, the two
// gates and the record.
//
// gain_kernel: y = x * g in place, 16-byte accesses from the row's first
// aligned word, scalar head and tail.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "abi_util.h"
#include "loudness.h"

namespace mp3g {
namespace {

struct SegArgs {
  const float* src;
  const uint32_t* lengths;    // may be null: every row is T long
  const uint32_t* row_index;  // may be null: item row i is row i
  const double* V;            // [H][4]
  double* items;              // [n_items][9]
  float* peaks;               // [n_items]
  uint64_t total;             // floats of the whole source tensor
  uint32_t n_rows, n_planes, T, H, S1, n_items;
  LoudCoef c;
};

// kTiny: a tensor of fewer than 4 floats, which has no 16 bytes to read.
template <bool kTiny>
__global__ __launch_bounds__(kLoudBlock) void loudness_segment_kernel(SegArgs a) {
  constexpr uint32_t kWaves = kLoudBlock / 64, kRow = kLoudLdsStride, kImage = 64 * kRow;
  __shared__ float stage[kWaves][kImage];
  __shared__ double vtab[kWaves][kLoudChunk * 4];  // V[n0 .. n0 + 32): 1 KB, one 16-byte load per lane
  __shared__ uint64_t item_off[kWaves][64];
  __shared__ uint32_t item_n[kWaves][64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t id = blockIdx.x * kLoudBlock + threadIdx.x;
  // this lane's item: where its samples start and how many it has
  uint64_t off = 0;
  uint32_t nvalid = 0, filter = 0;
  if (id < a.n_items) {
    const uint32_t rp = id / a.S1, j = id - rp * a.S1;
    const uint32_t i = rp / a.n_planes, p = rp - i * a.n_planes;
    const uint32_t row = a.row_index ? a.row_index[i] : i;
    if (row < a.n_rows) {
      uint32_t len = a.lengths ? a.lengths[row] : a.T;
      len = len < a.T ? len : a.T;
      const uint32_t nseg = len / a.H;
      off = ((uint64_t)row * a.n_planes + p) * a.T + (uint64_t)j * a.H;
      filter = j < nseg;
      nvalid = filter ? a.H : (j == nseg ? len - nseg * a.H : 0u);
    }
  }
  item_off[wave][lane] = off;
  item_n[wave][lane] = nvalid;
  __syncthreads();
  // the loader's view: lane l fetches word l % 8 of items l / 8 + 8 t
  const uint32_t lw = lane & 7, li = lane >> 3;
  uint64_t loff[8];
  uint32_t ln[8];
#pragma unroll
  for (uint32_t t = 0; t < 8; t++) {
    loff[t] = item_off[wave][li + 8 * t];
    ln[t] = item_n[wave][li + 8 * t];
  }
  // word[t]: 16 bytes of item (li + 8 t)'s strip at n0, samples n0 + 4 lw .. + 3.
  // The address is only 4-byte aligned (the hardware takes that); a word that
  // would end past the tensor is fetched from the tensor's last 16 bytes
  // instead and shifted in store().  No branch: the eight loads stay in flight.
  struct __attribute__((packed, aligned(4))) Word {
    float v[4];
  };
  Word word[8];
  const uint64_t last = kTiny ? ~0ull : a.total - 4;
  double2 vword;
  auto fetch = [&](uint32_t n0) {
    // (V has H rows: the strip's last rows may lie past it)
    const uint32_t vn = n0 + (lane >> 1);
    vword = vn < a.H ? *reinterpret_cast<const double2*>(a.V + 4 * (size_t)vn + 2 * (lane & 1)) : make_double2(0.0, 0.0);
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const uint64_t e = loff[t] + n0 + 4 * lw;
      if constexpr (kTiny) {
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) word[t].v[c] = e + c < a.total ? a.src[e + c] : 0.f;
      } else {
        word[t] = *reinterpret_cast<const Word*>(a.src + (e < last ? e : last));
      }
    }
  };
  // the floats of word[t] to their places in the item's row: sample n0 + m at
  // dword m, zero where the item has no sample
  auto store = [&](uint32_t n0, float* image) {
    *reinterpret_cast<double2*>(&vtab[wave][2 * lane]) = vword;
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const uint64_t e = loff[t] + n0 + 4 * lw;
      const uint32_t sh = e < last ? 0u : (uint32_t)(e - last < 4 ? e - last : 4);
      const float v0 = word[t].v[0], v1 = word[t].v[1], v2 = word[t].v[2], v3 = word[t].v[3];
      // (a float shifted in from past the word lies past the tensor: never a sample)
      const float x0 = sh == 0 ? v0 : sh == 1 ? v1 : sh == 2 ? v2 : v3;
      const float x1 = sh == 0 ? v1 : sh == 1 ? v2 : v3;
      const float x2 = sh == 0 ? v2 : v3;
      const float x[4] = {x0, x1, x2, v3};
      float* row = image + (li + 8 * t) * kRow + 4 * lw;
      const uint32_t n = n0 + 4 * lw;
#pragma unroll
      for (uint32_t c = 0; c < 4; c++) row[c] = (n + c < ln[t]) ? x[c] : 0.f;
    }
  };
  double s[4] = {0.0, 0.0, 0.0, 0.0}, g[4] = {0.0, 0.0, 0.0, 0.0}, ezs = 0.0;
  float peak = 0.f;
  fetch(0);
  for (uint32_t n0 = 0; n0 < a.H; n0 += kLoudChunk) {
    store(n0, stage[wave]);
    __syncthreads();
    if (n0 + kLoudChunk < a.H) fetch(n0 + kLoudChunk);
    const float* mine = stage[wave] + lane * kRow;
    const uint32_t cnt = a.H - n0 < kLoudChunk ? a.H - n0 : kLoudChunk;
#pragma unroll 8  // (eight samples' LDS reads in flight ahead of the recurrence)
    for (uint32_t m = 0; m < cnt; m++) {
      const float x = mine[m];
      const double* Vn = &vtab[wave][4 * m];  // (one address for the wave: a broadcast read)
      const double w = loud_step(a.c, s, (double)x);
      ezs += w * w;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) g[k] += Vn[k] * w;
      const float ax = __builtin_fabsf(x);
      peak = ax > peak ? ax : peak;
    }
    __syncthreads();
  }
  if (id < a.n_items) {
    a.peaks[id] = peak;
    if (filter) {
      double* it = a.items + (size_t)id * kLoudItemDoubles;
      it[0] = ezs;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        it[1 + k] = g[k];
        it[5 + k] = s[k];
      }
    }
  }
}

struct RowArgs {
  const uint32_t* lengths;
  const uint32_t* row_index;
  const double* tab;  // AH[16], then G[16]
  double* items;
  const float* peaks;
  mp3g_loudness_stats* stats;
  uint32_t n_rows, n_index, n_planes, T, H, S1;
};

__global__ __launch_bounds__(kLoudRowBlock) void loudness_row_kernel(RowArgs a) {
  const uint32_t rp = blockIdx.x * kLoudRowBlock + threadIdx.x;  // (kLoudRowBlock is even: a row's planes share a block)
  const uint32_t i = rp / a.n_planes, p = rp - i * a.n_planes;
  uint32_t row = 0, nseg = 0;
  bool live = false;
  if (i < a.n_index) {
    row = a.row_index ? a.row_index[i] : i;
    if (row < a.n_rows) {
      live = true;
      uint32_t len = a.lengths ? a.lengths[row] : a.T;
      len = len < a.T ? len : a.T;
      nseg = len / a.H;
    }
  }
  if (live) {
    double AH[16], G[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      AH[k] = a.tab[k];
      G[k] = a.tab[16 + k];
    }
    loud_scan_plane(a.items + (size_t)rp * a.S1 * kLoudItemDoubles, nseg, G, AH);
  }
  __syncthreads();
  if (live && p == 0)
    loud_row_record(a.items + (size_t)rp * a.S1 * kLoudItemDoubles, a.peaks + (size_t)rp * a.S1, a.n_planes, a.S1,
                    nseg, a.H, &a.stats[row]);
}

// One block per kGainBlock * kGainWords float4 words of one plane.  A thread
// issues its words' loads, then forms the row's gain (every thread does: the
// record is one uniform address, and the division and the square root run while
// the loads are in flight), then multiplies and stores.  Slot 0 of a plane is
// its unaligned head.
__global__ __launch_bounds__(kGainBlock) void gain_kernel(float* x, uint32_t n_planes, uint32_t T,
                                                          const uint32_t* lengths, const mp3g_loudness_stats* stats,
                                                          double target_energy, float peak_ceiling, float* gain_out,
                                                          uint32_t blocks_per_plane) {
  const uint32_t rp = blockIdx.x / blocks_per_plane, chunk = blockIdx.x - rp * blocks_per_plane;
  const uint32_t row = rp / n_planes;
  const double energy = stats[row].energy;
  const float peak = stats[row].peak;
  const bool first = threadIdx.x == 0 && chunk == 0 && rp == row * n_planes;
  if (!(energy > 0.0)) {
    if (first && gain_out) gain_out[row] = 1.0f;
    return;
  }
  uint32_t len = lengths ? lengths[row] : T;
  len = len < T ? len : T;
  float* xp = x + (size_t)rp * T;
  const uint32_t head = (4u - ((uint32_t)((uintptr_t)xp >> 2) & 3u)) & 3u;  // floats before the first aligned word
  float4 v[kGainWords];
  uint64_t e[kGainWords];
  bool whole[kGainWords];
#pragma unroll
  for (uint32_t u = 0; u < kGainWords; u++) {
    const uint64_t slot = ((uint64_t)chunk * kGainWords + u) * kGainBlock + threadIdx.x;
    e[u] = slot ? head + 4 * (slot - 1) : 0;
    whole[u] = slot && e[u] + 4 <= len;
    v[u] = whole[u] ? *reinterpret_cast<const float4*>(xp + e[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float g = loud_gain(energy, peak, target_energy, peak_ceiling);
  if (first && gain_out) gain_out[row] = g;
#pragma unroll
  for (uint32_t u = 0; u < kGainWords; u++) {
    const uint64_t slot = ((uint64_t)chunk * kGainWords + u) * kGainBlock + threadIdx.x;
    if (whole[u]) {
      *reinterpret_cast<float4*>(xp + e[u]) = make_float4(v[u].x * g, v[u].y * g, v[u].z * g, v[u].w * g);
    } else if (slot == 0) {
      for (uint32_t n = 0; n < head && n < len; n++) xp[n] = xp[n] * g;
    } else {
      for (uint64_t n = e[u]; n < len; n++) xp[n] = xp[n] * g;  // the tail, or nothing
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

int loudness_device_upload(mp3g_loudness* ld) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || ld->device >= n)
    return abi_fail(MP3G_ERR_NO_DEVICE, "loudness: no such device");
  hipDeviceProp_t prop;
  const hipError_t pe = hipGetDeviceProperties(&prop, ld->device);
  if (pe != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipGetDeviceProperties", pe);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return abi_fail(MP3G_ERR_NO_DEVICE, "device is not gfx950");
  DeviceScope scope(ld->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  std::vector<double> tab(ld->V);
  tab.insert(tab.end(), ld->AH, ld->AH + 16);
  tab.insert(tab.end(), ld->G, ld->G + 16);
  const size_t bytes = tab.size() * sizeof(double);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&ld->d_tab), bytes);
  if (e != hipSuccess) {
    ld->d_tab = nullptr;
    return hip_fail(MP3G_ERR_OUT_OF_MEMORY, "loudness tables", e);
  }
  e = hipMemcpy(ld->d_tab, tab.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    loudness_device_free(ld);
    return hip_fail(MP3G_ERR_DEVICE, "loudness tables", e);
  }
  return MP3G_OK;
}

void loudness_device_free(mp3g_loudness* ld) {
  DeviceScope scope(ld->device);
  (void)hipFree(ld->d_tab);
  ld->d_tab = nullptr;
}

}  // namespace mp3g

using namespace mp3g;

extern "C" int mp3g_loudness_rows(const mp3g_loudness* ld, const float* d_src, uint32_t n_rows, uint32_t n_planes,
                                  uint32_t T, const uint32_t* d_lengths, const uint32_t* d_row_index,
                                  uint32_t n_index, void* d_scratch, mp3g_loudness_stats* d_stats,
                                  void* hip_stream) {
  const int st = loudness_check(ld, n_rows, n_planes, T, nullptr);
  if (st != MP3G_OK) return st;
  if (ld->device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: a host-only object");
  const uint32_t n_work = d_row_index ? n_index : n_rows;
  if (n_work > n_rows) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: more indices than rows");
  if (n_work == 0) return MP3G_OK;
  if (!d_scratch || !d_stats || (T && !d_src)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null device buffer");
  if (((uintptr_t)d_src & 3u) || ((uintptr_t)d_scratch & 7u) || ((uintptr_t)d_stats & 7u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: a misaligned device buffer");
  DeviceScope scope(ld->device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint32_t H = ld->H, S1 = loud_items_per_plane(T, H);
  const uint32_t n_items = n_work * n_planes * S1;  // (below 2^31: loudness_check)
  double* items = static_cast<double*>(d_scratch);
  float* peaks = reinterpret_cast<float*>(items + (size_t)n_items * kLoudItemDoubles);
  SegArgs s = {};
  s.src = d_src;
  s.lengths = d_lengths;
  s.row_index = d_row_index;
  s.V = ld->d_tab;
  s.items = items;
  s.peaks = peaks;
  s.total = (uint64_t)n_rows * n_planes * T;
  s.n_rows = n_rows;
  s.n_planes = n_planes;
  s.T = T;
  s.H = H;
  s.S1 = S1;
  s.n_items = n_items;
  s.c = ld->coef;
  const uint32_t seg_blocks = (n_items + kLoudBlock - 1) / kLoudBlock;
  if (s.total < 4)
    loudness_segment_kernel<true><<<seg_blocks, kLoudBlock, 0, stream>>>(s);
  else
    loudness_segment_kernel<false><<<seg_blocks, kLoudBlock, 0, stream>>>(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(MP3G_ERR_DEVICE, "loudness segment launch", e);
  RowArgs r = {};
  r.lengths = d_lengths;
  r.row_index = d_row_index;
  r.tab = ld->d_tab + (size_t)H * 4;
  r.items = items;
  r.peaks = peaks;
  r.stats = d_stats;
  r.n_rows = n_rows;
  r.n_index = n_work;
  r.n_planes = n_planes;
  r.T = T;
  r.H = H;
  r.S1 = S1;
  const uint32_t planes = n_work * n_planes;
  loudness_row_kernel<<<(planes + kLoudRowBlock - 1) / kLoudRowBlock, kLoudRowBlock, 0, stream>>>(r);
  e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "loudness row launch", e);
}

extern "C" int mp3g_gain_rows(int device, float* d_x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                              const uint32_t* d_lengths, const mp3g_loudness_stats* d_stats, double target_energy,
                              float peak_ceiling, float* d_gain_out, void* hip_stream) {
  const int st = gain_check(n_rows, n_planes, T, target_energy, peak_ceiling);
  if (st != MP3G_OK) return st;
  if (device < 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (n_rows == 0) return MP3G_OK;
  if (!d_stats || (T && !d_x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: null device buffer");
  if (((uintptr_t)d_x & 3u) || ((uintptr_t)d_stats & 7u))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: a misaligned device buffer");
  // slots of a plane: its head, then every aligned word that can hold a sample
  const uint64_t slots = 2 + (uint64_t)T / 4, per_block = (uint64_t)kGainBlock * kGainWords;
  const uint64_t bpp = (slots + per_block - 1) / per_block, blocks = bpp * n_rows * n_planes;
  if (blocks >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "gain: too many samples for one launch");
  DeviceScope scope(device);
  if (scope.err != hipSuccess) return hip_fail(MP3G_ERR_NO_DEVICE, "hipSetDevice", scope.err);
  gain_kernel<<<(uint32_t)blocks, kGainBlock, 0, static_cast<hipStream_t>(hip_stream)>>>(
      d_x, n_planes, T, d_lengths, d_stats, target_energy, peak_ceiling, d_gain_out, (uint32_t)bpp);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MP3G_OK : hip_fail(MP3G_ERR_DEVICE, "gain launch", e);
}
