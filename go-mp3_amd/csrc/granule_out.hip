// granule_out.hip -- the PCM output stage of the one-wave granule kernels
// (gfx950): everything between the window sums and memory.
//
// The window of the fast kernel v3 (granule_fast.hip), of the exact kernel v4
// (granule_wexact.hip) and of the standalone polyphase kernel
// (granule_synth.hip) leaves lane (ch, k) the sums of output k, acc2[p] =
// slots (2p, 2p + 1) times 32767.  From there on the kernels share this
// stage, one instantiation per output format kFmt (MP3G_OUT_*, or the
// windowed kFmtWinPlanar / kFmtWinMono of kernels.h):
//   pack_granule<kFmt>   the sums -> the registers a lane stores (PcmRegs);
//   store_granule<kFmt>  those registers -> memory, as many stores for a
//                        replayed granule (`out` false) as for an output one,
//                        through a resource with no records.
// (compiled in kernels_fast.hip in front of the three kernels)
#pragma clang fp contract(fast)
#include <type_traits>

#include "pk.h"

// cache policy of the PCM stores (2 = nt: streamed past the caches)
#ifndef MP3G_PCM_STORE_AUX
#define MP3G_PCM_STORE_AUX 2
#endif

namespace mp3g {
namespace v3 {
namespace {

using pk::f2;

// The lane id, recomputed where it is used (asm volatile: not hoisted out of
// the granule loop).  Values derived from it once and kept for the whole loop
// cost a VGPR each; at the 128-VGPR budget the allocator spilled some to
// scratch, and a reload is a VMEM load whose s_waitcnt also waits for the
// in-flight PCM stores and prefetch.
__device__ __forceinline__ int lane_fresh() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// a lane offset past the records of every buffer resource of these kernels:
// the access returns 0 / is dropped without touching memory
constexpr int kNoRecord = 0x40000000;

// (L, R) sample pairs without LDS staging: one v_permlane32_swap per slot
// pair hands lane i slot 2p's (L, R) and lane 32 + i slot 2p + 1's, so every
// lane stores one dword per slot pair and the wave 2 x 128 contiguous bytes.
// Mono: the swap hands lane i channel 0's slot 2p and lane 32 + i its slot
// 2p + 1, stored in both halves (frame.go:671-678).  acc2 holds sum * 32767.
// (Each lane storing its own channel's samples as 16-bit stores, no swap and
// no merge, measured slower: DESIGN.md section 6, round 6.)
__device__ __forceinline__ void pack_pcm(const f2 acc2[9], int nch, uint32_t pk[9]) {
  auto pack = [&](auto mono) {
#pragma unroll
    for (int p = 0; p < 9; p++) {
      // int(sum * 32767) clamped to +-32767 (frame.go:663-669); no decodable
      // input gets near NaN or |t| >= 2^63 (|sum| < 1e12)
      const int a = (int)__builtin_amdgcn_fmed3f(acc2[p].x, -32767.0f, 32767.0f);
      const int b = (int)__builtin_amdgcn_fmed3f(acc2[p].y, -32767.0f, 32767.0f);
      const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
      // low halves of (r[0], r[1]) -> one dword: L | R << 16 (R = L for mono)
      pk[p] = __builtin_amdgcn_perm((uint32_t)(decltype(mono)::value ? r[0] : r[1]), (uint32_t)r[0], 0x05040100u);
    }
  };
  if (nch == 2) pack(std::false_type{});
  else pack(std::true_type{});
}

// The same dwords with the clamp made by the integer pack (the fast kernel's
// s16 path): the sums truncated to int32 first (v_cvt_i32_f32, which
// saturates at the int32 range), swapped as integers, then one
// v_cvt_pk_i16_i32 of (L, R) -- it saturates each half to [-32768, 32767] --
// and one v_pk_max_i16 that lifts -32768 to -32767: int(sum * 32767) clamped
// to +-32767 for every finite sum, as above, without the two float clamps per
// slot pair.  (Swap first, pack last: packed before the swap, the swap's tied
// operands cost copies)
__device__ __forceinline__ void pack_pcm_sat(const f2 acc2[9], int nch, uint32_t pk[9]) {
  typedef short s2 __attribute__((ext_vector_type(2)));
  // (the swap in front of the channel-count branch: inside it, each branch
  // copied the integers it shares with the other before its tied swap)
  int l[9], r[9];
#pragma unroll
  for (int p = 0; p < 9; p++) {
    const auto sw = __builtin_amdgcn_permlane32_swap((int)acc2[p].x, (int)acc2[p].y, false, false);
    l[p] = (int)sw[0];
    r[p] = (int)sw[1];
  }
  // (the mono pack as an asm statement: written like the stereo one, the
  // compiler merges the two branches into one pack behind a copy of L or R
  // per slot pair -- 18 v_mov_b32 on the stereo path)
  if (nch == 2) {
#pragma unroll
    for (int p = 0; p < 9; p++) {
      const s2 lr = __builtin_bit_cast(s2, __builtin_amdgcn_cvt_pk_i16(l[p], r[p]));
      pk[p] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(lr, (s2){-32767, -32767}));
    }
  } else {
#pragma unroll
    for (int p = 0; p < 9; p++) {
      s2 ll;
      asm("v_cvt_pk_i16_i32 %0, %1, %1" : "=v"(ll) : "v"(l[p]));
      pk[p] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(ll, (s2){-32767, -32767}));
    }
  }
}

// PCM of granule g: one dword per lane and slot pair, non-temporal (c2
// -1.9 %, c3 -0.8 %).  Issued for replayed granules too, through a resource
// with no records (straight-line vmcnt accounting).
__device__ __forceinline__ void store_pcm(int16_t* pcm, uint32_t g, bool out, const uint32_t pk[9], int hi, int k) {
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
      pcm + (size_t)g * 1152, (short)0, out ? MP3G_PCM_BYTES_PER_GRANULE : 0, 0x00020000);
#pragma unroll
  for (int p = 0; p < 9; p++)
    __builtin_amdgcn_raw_buffer_store_b32(pk[p], rp, 4 * (32 * (2 * p + hi) + k), 0, MP3G_PCM_STORE_AUX);
}

// ---- float32 output (MP3G_OUT_F32 / MP3G_OUT_F32_PLANAR) ----
// The window leaves lane (ch, k) slots 2p and 2p + 1 of output k in acc2[p]
// (sum * 32767): the float sample is the s16 sample's clamp without the
// truncation, scaled by 2^-15 (exact), so trunc(f * 32768) is the s16 sample.
// A float store from this layout needs no cross-lane pack.  Mono: channel 0's
// values go to the channel-1 lanes (v_permlane32_swap of a value with itself
// hands every lane the low half's), which then write them to the other
// channel / plane (frame.go:671-678).
__device__ __forceinline__ void pack_pcm(const f2 acc2[9], int nch, float pf[18]) {
#pragma unroll
  for (int p = 0; p < 9; p++) {
    pf[2 * p] = __builtin_amdgcn_fmed3f(acc2[p].x, -32767.0f, 32767.0f) * (1.0f / 32768.0f);
    pf[2 * p + 1] = __builtin_amdgcn_fmed3f(acc2[p].y, -32767.0f, 32767.0f) * (1.0f / 32768.0f);
  }
  if (nch != 2) {  // (wave-uniform)
#pragma unroll
    for (int i = 0; i < 18; i++) {
      const uint32_t u = __builtin_bit_cast(uint32_t, pf[i]);
      pf[i] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_permlane32_swap(u, u, false, false)[0]);
    }
  }
}

// Where a chunk's stream lies (planar output: ChunkDesc::stream_first / stream_n).
struct StreamGeom {
  uint32_t first, n;
};

// Float samples of granule g, one dword per lane and slot, non-temporal like
// the s16 stores and issued for replayed granules too (no records).
//   F32:    float [g][32 slot + k][ch]: a store covers 256 contiguous bytes;
//           the resource spans the granule's block (4,608 B).  (A swap and
//           one 64-bit (L, R) store per slot pair measured no faster:
//           DESIGN.md section 9a.)
//   planar: plane(ch) + 576 (g - first) + 32 slot + k: two 128-B runs; the
//           resource starts at the granule's place in plane 0 and ends with
//           its place in plane 1 (the lane offset n * 2304 + 2300 stays below
//           2^31: MP3G_PLANAR_MAX_GRANULES).
template <int kFmt>
__device__ __forceinline__ void store_pcm_f32(int16_t* pcm, StreamGeom sg, uint32_t g, bool out, const float pf[18],
                                              int ch, int k) {
  float* const o = reinterpret_cast<float*>(pcm);
  if constexpr (kFmt == (int)MP3G_OUT_F32) {
    const __amdgpu_buffer_rsrc_t rp =
        __builtin_amdgcn_make_buffer_rsrc(o + (size_t)g * 1152, (short)0, out ? 2 * MP3G_PCM_BYTES_PER_GRANULE : 0, 0x00020000);
#pragma unroll
    for (int sl = 0; sl < 18; sl++)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[sl]), rp, 8 * (32 * sl + k) + 4 * ch, 0,
                                            MP3G_PCM_STORE_AUX);
  } else {
    const uint32_t plane = sg.n * (uint32_t)MP3G_PCM_BYTES_PER_GRANULE;  // bytes of one plane
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
        o + (size_t)sg.first * 1152 + (size_t)(g - sg.first) * MP3G_LINES, (short)0,
        out ? (int)(plane + MP3G_PCM_BYTES_PER_GRANULE) : 0, 0x00020000);
    const int base = (int)(ch ? plane : 0u) + 4 * k;
#pragma unroll
    for (int sl = 0; sl < 18; sl++)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[sl]), rp, base + 128 * sl, 0,
                                            MP3G_PCM_STORE_AUX);
  }
}

// ---- mono downmix output (MP3G_OUT_S16_MONO / MP3G_OUT_F32_MONO) ----
// The s16 pack's v_permlane32_swap brings the two channels of a sample into
// one lane: lane i holds slot 2p's (L, R), lane 32 + i slot 2p + 1's.  The
// downmix is one add there, and every lane owns ONE sample per slot pair:
// sample 64 p + lane of the granule's 576, so a store of the wave covers 64
// consecutive samples.
//   s16:   m = (L + R) >> 1 on the s16 samples (arithmetic shift: floor)
//   float: m = (fL + fR) * 0.5f on the float samples (one rounded add; the
//          halving is exact)
// A mono granule gives channel 0's sample as it is (wave-uniform branch).
constexpr bool fmt_is_mono(int fmt) {
  return fmt == (int)MP3G_OUT_S16_MONO || fmt == (int)MP3G_OUT_F32_MONO || fmt == kFmtWinMono;
}
// the windowed formats (kernels.h): float planar / float mono samples placed
// with sample granularity into dense rows
constexpr bool fmt_is_windowed(int fmt) { return fmt == kFmtWinPlanar || fmt == kFmtWinMono; }
__device__ __forceinline__ void pack_pcm_mono(const f2 acc2[9], int nch, uint32_t pm[9]) {
  auto pack = [&](auto mono) {
#pragma unroll
    for (int p = 0; p < 9; p++) {
      const int a = (int)__builtin_amdgcn_fmed3f(acc2[p].x, -32767.0f, 32767.0f);
      const int b = (int)__builtin_amdgcn_fmed3f(acc2[p].y, -32767.0f, 32767.0f);
      const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
      const int m = decltype(mono)::value ? (int)r[0] : ((int)r[0] + (int)r[1]) >> 1;
      pm[p] = (uint32_t)m;
    }
  };
  if (nch == 2) pack(std::false_type{});
  else pack(std::true_type{});
}

__device__ __forceinline__ void pack_pcm_mono(const f2 acc2[9], int nch, float pm[9]) {
  auto pack = [&](auto mono) {
#pragma unroll
    for (int p = 0; p < 9; p++) {
      const float a = __builtin_amdgcn_fmed3f(acc2[p].x, -32767.0f, 32767.0f) * (1.0f / 32768.0f);
      const float b = __builtin_amdgcn_fmed3f(acc2[p].y, -32767.0f, 32767.0f) * (1.0f / 32768.0f);
      const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                                                      false, false);
      const float fl = __builtin_bit_cast(float, (uint32_t)r[0]), fr = __builtin_bit_cast(float, (uint32_t)r[1]);
      pm[p] = decltype(mono)::value ? fl : (fl + fr) * 0.5f;
    }
  };
  if (nch == 2) pack(std::false_type{});
  else pack(std::true_type{});
}

// The registers a lane hands the store stage, per format: s16 (L, R) dwords,
// the lane's 18 float samples, or one mono sample per slot pair.
template <int kFmt>
struct PcmRegs {
  typedef float type[18];
};
template <>
struct PcmRegs<(int)MP3G_OUT_S16> {
  typedef uint32_t type[9];
};
template <>
struct PcmRegs<(int)MP3G_OUT_S16_MONO> {
  typedef uint32_t type[9];
};
template <>
struct PcmRegs<(int)MP3G_OUT_F32_MONO> {
  typedef float type[9];
};
template <>
struct PcmRegs<kFmtWinMono> {
  typedef float type[9];
};

// Mono samples of granule g: sample 64 p + lane, non-temporal and issued for
// replayed granules too (no records), nine stores per lane like the s16 path.
// The resource spans exactly the granule: 1,152 B (s16) or 2,304 B (float).
//   s16:   16-bit stores, 128 contiguous bytes per store of the wave
//          (neighbouring lanes' samples paired into dwords by a DPP move
//          measured slower: DESIGN.md section 9a)
//   float: one dword per lane, 256 contiguous bytes
__device__ __forceinline__ void store_pcm_mono(int16_t* pcm, uint32_t g, bool out, const uint32_t pm[9], int lane) {
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
      pcm + (size_t)g * MP3G_LINES, (short)0, out ? MP3G_PCM_BYTES_PER_GRANULE / 2 : 0, 0x00020000);
#pragma unroll
  for (int p = 0; p < 9; p++)
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)pm[p], rp, 2 * (64 * p + lane), 0, MP3G_PCM_STORE_AUX);
}

__device__ __forceinline__ void store_pcm_mono(int16_t* pcm, uint32_t g, bool out, const float pm[9], int lane) {
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<float*>(pcm) + (size_t)g * MP3G_LINES, (short)0, out ? MP3G_PCM_BYTES_PER_GRANULE : 0, 0x00020000);
#pragma unroll
  for (int p = 0; p < 9; p++)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pm[p]), rp, 4 * (64 * p + lane), 0,
                                          MP3G_PCM_STORE_AUX);
}

// ---- windowed output (kFmtWinPlanar / kFmtWinMono, kernels.h WindowRow) ----
// The registers are those of the float planar / float mono formats; only the
// placement differs: sample i of granule g goes to row index r = 576 (g - lo)
// - skip + i when 0 <= r < n_valid.  The resource starts at the row (plane 0)
// and spans it up to the last valid sample of its last plane; as many stores
// as the other formats, replayed granules included (no records).  Every lane
// is masked explicitly, by forcing its offset to kNoRecord:
//   * the shift is negative in the window's first granule -- it is part of
//     the VECTOR offset, never of the scalar offset operand, and a lane in
//     front of the row is masked before its offset could wrap;
//   * the range check alone cannot clip plane 0 at n_valid (the next bytes are
//     plane 1's, or the next row's).
// kNoRecord (2^30) lies past the records: 8 T <= 2^29 (MP3G_WINDOW_MAX_SAMPLES).
// The mask is an add, a compare and a select per store.  A granule wholly
// inside the window (a wave-uniform test) takes an unmasked path instead, the
// slot as the instruction's immediate offset like the plain formats; both
// paths issue the same number of stores.  The ISA and the measurement pull in
// opposite directions here, and the measurement decides (DESIGN.md section
// 9b): with two store sequences joining in front of the loop's back edge the
// wait-count pass turns the back edge's s_waitcnt vmcnt(18) -- wait for the
// prefetch, leave the 18 stores in flight, section 6 -- into vmcnt(0), yet
// full-length windows run 2.1 % faster in the fast kernel and the 2-second
// windows of c3 4.6 % faster than with every store masked
// (-DMP3G_WIN_INSIDE_PATH=0: one straight line of masked stores, vmcnt(18)
// kept): on this issue-bound kernel the 54 VALU instructions of the masks cost
// more than the wait, which the SIMD's other waves cover.
#ifndef MP3G_WIN_INSIDE_PATH
#define MP3G_WIN_INSIDE_PATH 1
#endif
// The row of a chunk's stream as wave-uniform scalars, loaded once per chunk
// -- in front of the granule loop and of the chunk's first store, so the
// loads are settled with the prologue's (a load inside the loop would make the
// store stage wait for the previous granule's stores).  off0 = 576 lo + skip
// modulo 2^32: sample i of granule g has row index 576 g - off0 + i.
struct WinGeom {
  float* o;  // the row's first float (plane 0)
  uint32_t off0, nv, plane;
};
__device__ __forceinline__ WinGeom win_geom(int16_t* pcm, const void* table, uint32_t stream) {
  const WindowRow* row = static_cast<const WindowRow*>(table) + stream;
  const uint64_t base = row->base;
  const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t bhi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  return WinGeom{reinterpret_cast<float*>(pcm) + (((uint64_t)bhi << 32) | blo),
                 (uint32_t)__builtin_amdgcn_readfirstlane(576u * row->lo + row->skip),
                 (uint32_t)__builtin_amdgcn_readfirstlane(row->n_valid),
                 (uint32_t)__builtin_amdgcn_readfirstlane(row->plane)};
}

template <int kFmt>
__device__ __forceinline__ void store_pcm_win(const WinGeom& wg, uint32_t g, bool out, const float* pf, int lane) {
  const uint32_t nv = wg.nv;
  const int shift = (int)(576u * g - wg.off0);
  // (wave-uniform; constant false with -DMP3G_WIN_INSIDE_PATH=0)
  const bool inside = MP3G_WIN_INSIDE_PATH && shift >= 0 && (uint32_t)shift + 576u <= nv;
  if constexpr (kFmt == kFmtWinPlanar) {
    const uint32_t plane = wg.plane;
    const __amdgpu_buffer_rsrc_t rp =
        __builtin_amdgcn_make_buffer_rsrc(wg.o, (short)0, out ? (int)(4u * (plane + nv)) : 0, 0x00020000);
    const int r0 = shift + (lane & 31);
    const int b4 = 4 * ((lane >> 5 ? (int)plane : 0) + r0);
    if (inside) {
#pragma unroll
      for (int sl = 0; sl < 18; sl++)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[sl]), rp, b4 + 128 * sl, 0,
                                              MP3G_PCM_STORE_AUX);
    } else {
#pragma unroll
      for (int sl = 0; sl < 18; sl++)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[sl]), rp,
                                              (uint32_t)(r0 + 32 * sl) < nv ? b4 + 128 * sl : kNoRecord, 0,
                                              MP3G_PCM_STORE_AUX);
    }
  } else {
    const __amdgpu_buffer_rsrc_t rp =
        __builtin_amdgcn_make_buffer_rsrc(wg.o, (short)0, out ? (int)(4u * nv) : 0, 0x00020000);
    const int r0 = shift + lane;
    const int b4 = 4 * r0;
    if (inside) {
#pragma unroll
      for (int p = 0; p < 9; p++)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[p]), rp, b4 + 256 * p, 0,
                                              MP3G_PCM_STORE_AUX);
    } else {
#pragma unroll
      for (int p = 0; p < 9; p++)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, pf[p]), rp,
                                              (uint32_t)(r0 + 64 * p) < nv ? b4 + 256 * p : kNoRecord, 0,
                                              MP3G_PCM_STORE_AUX);
    }
  }
}

// ---- the stage's two entries ----
// The window sums of a granule into the format's registers.
template <int kFmt>
__device__ __forceinline__ void pack_granule(const f2 acc2[9], int nch, typename PcmRegs<kFmt>::type& pr) {
  if constexpr (fmt_is_mono(kFmt)) pack_pcm_mono(acc2, nch, pr);
  else pack_pcm(acc2, nch, pr);
}

// The format's stores of granule g; sg is read by MP3G_OUT_F32_PLANAR only and
// wg by the windowed formats only.  (The lane id is recomputed at the store,
// not handed in: see lane_fresh.)
template <int kFmt>
__device__ __forceinline__ void store_granule(int16_t* pcm, const StreamGeom& sg, const WinGeom& wg, uint32_t g,
                                              bool out, const typename PcmRegs<kFmt>::type& pr) {
  if constexpr (fmt_is_windowed(kFmt)) store_pcm_win<kFmt>(wg, g, out, pr, lane_fresh());
  else if constexpr (fmt_is_mono(kFmt)) store_pcm_mono(pcm, g, out, pr, lane_fresh());
  else if constexpr (kFmt == (int)MP3G_OUT_S16) store_pcm(pcm, g, out, pr, lane_fresh() >> 5, lane_fresh() & 31);
  else store_pcm_f32<kFmt>(pcm, sg, g, out, pr, lane_fresh() >> 5, lane_fresh() & 31);
}

}  // namespace
}  // namespace v3
}  // namespace mp3g
