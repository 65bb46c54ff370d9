// abi_util.h -- shared helpers of the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/mp3g.h"

namespace mp3g {
struct ChunkDesc;  // kernels.h
// Records `what` as this thread's mp3g_last_error() text and returns status.
int abi_fail(int status, const char* what);
// Whether the plan kernel of `mode` reads only coefficient lines below count1
// (fast v3, exact v4): the main-data kernel may then skip the zero tails
// (MP3G_HUFF_ROWS_COUNT1).
bool mode_reads_to_count1(unsigned mode);
// The device's constant tables uploaded (once per device).
int ensure_device_ready(int device);
// A plan's chunk table, built on the host (mp3g_plan_create's checks and
// chunking: granules_per_chunk 0 = the cost model), and the launch of a table
// already on the device -- for pipelines that upload tables asynchronously
// (mp3g_decode_streams_into) instead of through a plan's blocking copy.
int plan_chunks(int device, const mp3g_stream* streams, uint32_t n_streams, uint32_t granules_per_chunk,
                uint32_t mode, std::vector<ChunkDesc>* chunks, uint64_t* n_granules, uint64_t* n_halo);
struct ZoneScratch;  // kernels.h
// (out_format: MP3G_OUT_*)
int plan_launch_out(uint32_t mode, const ChunkDesc* d_chunks, uint32_t n_chunks, const mp3g_granule* d_gran,
                    const int16_t* d_coef, const mp3g_state* d_state_in, mp3g_state* d_state_out, void* d_out,
                    uint32_t out_format, const ZoneScratch* zones, hipStream_t stream);

// Threads for a batch of n_streams: the caller's n_threads (<= 0: one per
// hardware thread), at most one per stream, at least one.
inline int thread_count(int n_threads, uint32_t n_streams) {
  const int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
  return std::max(1, std::min<int>(nt, (int)std::max<uint32_t>(1, n_streams)));
}
// fn(k) for k in [k0, k1) on up to nt threads (the calling thread included)
template <class Fn>
void parallel_for(uint32_t k0, uint32_t k1, int nt, Fn&& fn) {
  std::atomic<uint32_t> next{k0};
  auto work = [&]() {
    for (uint32_t k; (k = next.fetch_add(1)) < k1;) fn(k);
  };
  nt = std::max(1, std::min<int>(nt, (int)(k1 - k0)));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; t++) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
}
}  // namespace mp3g
