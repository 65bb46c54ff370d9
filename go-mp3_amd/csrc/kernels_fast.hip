// kernels_fast.hip -- device translation unit of the one-wave-per-chunk
// granule kernels: fast mode v3 (granule_fast.hip, MP3G_MODE_FAST), the
// standalone polyphase kernel (granule_synth.hip) and exact mode v4
// (granule_wexact.hip, the default MP3G_MODE_EXACT kernel), with the PCM
// output stage they share (granule_out.hip) and their own copy of the fast
// tables.
//
// Own TU so it gets its own codegen options (Makefile): it is compiled with
// machine LICM off.  The kernel's packed-FP32 transforms take their constants
// from SGPR pairs (VOP3P has no literal operand); hoisted out of the granule
// loop, ~90 of them overflow the wave's SGPRs and were spilled to VGPR lanes,
// costing a v_readlane (VALU) per use inside the loop.  Left in place they are
// s_mov_b32 (SALU) next to their use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../../include/mp3g.h"
#include "dsp_tables.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace mp3g {
__constant__ FastTables g_fast;
// DspTables::req (131 KB, global memory): the exact requantization of the
// reference-order fallback for hot granules (granule_fast.hip)
__device__ float g_req[4][8207];
}  // namespace mp3g

#include "granule_hdr.h"
#include "granule_out.hip"
#include "granule_fast.hip"
#include "granule_synth.hip"
#include "granule_wexact.hip"

#ifndef MP3G_ZONE_CHUNKS_PER_WG
// zone-launch workgroups: one per this many chunks (16 .. 512).  32 since the
// round-6 chunk model halved c3's chunk count (128 granules per chunk): c3
// keeps its 512 workgroups (at 256 the ~10 %-hot batch took 8.2 ms instead of
// 6.3), c2 gets 128
#define MP3G_ZONE_CHUNKS_PER_WG 32
#endif

namespace mp3g {

hipError_t upload_fast_tables(const FastTables& fast, const float* req) {
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_fast), &fast, sizeof(FastTables), 0, hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_req), req, sizeof(float) * 4 * 8207, 0, hipMemcpyHostToDevice);
}

hipError_t fast_kernel_attributes(hipFuncAttributes* a, int* waves_per_block) {
  *waves_per_block = v3::kWaves;
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(&v3::granule_fast_kernel<false>));
}

hipError_t zone_scratch_init(void* p, uint32_t cap) {
  uint32_t h[8] = {0, 0, cap, 0, 0, 0, 0, 0};
  return hipMemcpy(p, h, sizeof(h), hipMemcpyHostToDevice);
}

namespace {

// The fast launch pair of one output format: the fast kernel (with or
// without the hot counters), then the zone launch in the same format.
template <int kFmt>
hipError_t launch_fast_fmt(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                           const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out,
                           int16_t* d_pcm, const ZoneScratch* zones, bool hot_stats, hipStream_t stream) {
  const dim3 grid((n_chunks + v3::kWaves - 1) / v3::kWaves), block(64 * v3::kWaves);
  uint32_t* aux = zones->aux;
  if (hot_stats)
    hipLaunchKernelGGL((v3::granule_fast_kernel<false, true, kFmt>), grid, block, 0, stream, d_chunks, n_chunks, d_gran,
                       d_coef, d_state_in, d_state_out, d_pcm, static_cast<void*>(aux));
  else
    hipLaunchKernelGGL((v3::granule_fast_kernel<false, false, kFmt>), grid, block, 0, stream, d_chunks, n_chunks,
                       d_gran, d_coef, d_state_in, d_state_out, d_pcm, static_cast<void*>(aux));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the zone launch: the exact v4 kernel over the list, its waves taking zone
  // after zone; one workgroup of 8 waves per MP3G_ZONE_CHUNKS_PER_WG chunks of
  // the launch, at most two per CU (an empty list ends every workgroup at
  // once: the fewer, the cheaper -- c2's 4,096 chunks get 128)
  const uint32_t blocks = std::max(16u, std::min<uint32_t>(n_chunks / MP3G_ZONE_CHUNKS_PER_WG, 512u));
  hipLaunchKernelGGL((v4::granule_wexact_kernel<true, kFmt>), dim3(blocks), dim3(64 * v4::kXWaves), 0, stream,
                     reinterpret_cast<const ChunkDesc*>(aux + 8), zones->cap, d_gran, d_coef, d_state_in,
                     d_state_out, d_pcm, aux);
  e = hipGetLastError();
  // the fast kernel ran (or will) and may have listed zones that no zone
  // launch will empty: reset the count and done words behind it on the
  // stream, so that the next launch does not decode stale zones into its own
  // buffers (the error is returned either way)
  if (e != hipSuccess) (void)hipMemsetAsync(aux, 0, 2 * sizeof(uint32_t), stream);
  return e;
}

template <int kFmt>
hipError_t launch_wexact_fmt(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                             const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out,
                             int16_t* d_pcm, hipStream_t stream) {
  const dim3 grid((n_chunks + v4::kXWaves - 1) / v4::kXWaves), block(64 * v4::kXWaves);
  hipLaunchKernelGGL((v4::granule_wexact_kernel<false, kFmt>), grid, block, 0, stream, d_chunks, n_chunks, d_gran,
                     d_coef, d_state_in, d_state_out, d_pcm, nullptr);
  return hipGetLastError();
}

// The instantiation of a runtime output format: f(the format as an integral
// constant) for MP3G_OUT_* and for the formats of a windowed plan (kernels.h:
// the WindowRow table then travels in d_state_out).
template <class F>
hipError_t with_format(uint32_t out_format, F f) {
  switch (out_format) {
    case MP3G_OUT_S16: return f(std::integral_constant<int, (int)MP3G_OUT_S16>{});
    case MP3G_OUT_F32: return f(std::integral_constant<int, (int)MP3G_OUT_F32>{});
    case MP3G_OUT_F32_PLANAR: return f(std::integral_constant<int, (int)MP3G_OUT_F32_PLANAR>{});
    case MP3G_OUT_S16_MONO: return f(std::integral_constant<int, (int)MP3G_OUT_S16_MONO>{});
    case MP3G_OUT_F32_MONO: return f(std::integral_constant<int, (int)MP3G_OUT_F32_MONO>{});
    case kFmtWinPlanar: return f(std::integral_constant<int, kFmtWinPlanar>{});
    case kFmtWinMono: return f(std::integral_constant<int, kFmtWinMono>{});
  }
  return hipErrorInvalidValue;
}

}  // namespace

// (diagnostic: zones redone in the wave, no list; s16 only)
hipError_t launch_fast_stamped(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                               const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out,
                               int16_t* d_pcm, unsigned long long* d_stamps, hipStream_t stream) {
  if (n_chunks == 0) return hipSuccess;
  if (!d_stamps) return hipErrorInvalidValue;
  const dim3 grid((n_chunks + v3::kWaves - 1) / v3::kWaves), block(64 * v3::kWaves);
  hipLaunchKernelGGL(v3::granule_fast_kernel<true>, grid, block, 0, stream, d_chunks, n_chunks, d_gran, d_coef,
                     d_state_in, d_state_out, d_pcm, static_cast<void*>(d_stamps));
  return hipGetLastError();
}

// (the kernels take the output as int16_t* whatever the format: the float
// instantiations cast it where they build their store resources)
hipError_t launch_fast(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                       const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out,
                       void* d_out, uint32_t out_format, const ZoneScratch* zones, bool hot_stats,
                       hipStream_t stream) {
  if (n_chunks == 0) return hipSuccess;
  // the production builds defer every hot zone to the plan's zone list (only
  // the stamped build redoes them in the wave)
  if (!zones || !zones->aux || zones->cap < (uint64_t)kZoneListPerChunk * n_chunks) return hipErrorInvalidValue;
  return with_format(out_format, [&](auto fmt) {
    return launch_fast_fmt<decltype(fmt)::value>(d_chunks, n_chunks, d_gran, d_coef, d_state_in, d_state_out,
                                                 static_cast<int16_t*>(d_out), zones, hot_stats, stream);
  });
}

hipError_t wexact_kernel_attributes(hipFuncAttributes* a, int* waves_per_block) {
  *waves_per_block = v4::kXWaves;
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(&v4::granule_wexact_kernel<false>));
}

hipError_t launch_wexact(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                         const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out,
                         void* d_out, uint32_t out_format, hipStream_t stream) {
  if (n_chunks == 0) return hipSuccess;
  return with_format(out_format, [&](auto fmt) {
    return launch_wexact_fmt<decltype(fmt)::value>(d_chunks, n_chunks, d_gran, d_coef, d_state_in, d_state_out,
                                                   static_cast<int16_t*>(d_out), stream);
  });
}

hipError_t launch_synth(const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran, const float* d_lines,
                        const mp3g_state* d_state_in, mp3g_state* d_state_out, int16_t* d_pcm, hipStream_t stream) {
  if (n_chunks == 0) return hipSuccess;
  const dim3 grid((n_chunks + v3::kSynthWaves - 1) / v3::kSynthWaves), block(64 * v3::kSynthWaves);
  hipLaunchKernelGGL(v3::granule_synth_kernel, grid, block, 0, stream, d_chunks, n_chunks, d_gran, d_lines, d_state_in,
                     d_state_out, d_pcm);
  return hipGetLastError();
}

}  // namespace mp3g
