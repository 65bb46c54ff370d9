// resample.h -- the polyphase resampler object shared by its host file
// (resample_tables.cpp: filter design, host reference) and its device file
// (resample.hip: table upload, kernels).  include/mp3g.h states the contract.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"

struct mp3g_resampler {
  int device = -1;
  uint32_t L = 1, M = 1, W = 0;
  std::vector<float> taps;  // [L][2W]; empty for a copy (fi == fo)
  float* d_taps = nullptr;  // device: the table permuted and transposed (resample_permute_taps)
};

namespace mp3g {

// How the device call tiles a row (resample.hip).  The phase-grouped kernel
// gives a lane kResampleGroup outputs S = m L apart -- the same phase, so one
// tap load feeds them all -- and a workgroup a tile of kResampleGroup * S
// consecutive outputs; it needs L <= 512 and the tile's source span in the LDS
// stage.  Every other filter runs the generic kernel: two outputs per lane,
// tiles of kResampleTile.
constexpr uint32_t kResampleTile = 512;
constexpr uint32_t kResampleGroup = 4;
constexpr uint32_t kResampleStageFloats = 4096;  // 16 KB of LDS: a tile's source span
struct ResampleGeom {
  bool grouped = false;
  uint32_t m = 0, S = 0;  // grouped: S = m L outputs between a lane's outputs
  uint32_t tile = kResampleTile;
  bool staged = false;    // the tile's source span fits the LDS stage
};
inline ResampleGeom resample_geometry(uint32_t L, uint32_t M, uint32_t W) {
  ResampleGeom g;
  if (W == 0) return g;  // a copy
  auto span = [&](uint32_t tile) { return ((uint64_t)(L - 1) + (uint64_t)(tile - 1) * M) / L + 2ull * W; };
  if (L <= 512) {
    const uint32_t m = L > 320 ? 1u : 320u / L, S = m * L;  // 192 < S <= 512
    if (span(kResampleGroup * S) <= kResampleStageFloats) {
      g.grouped = g.staged = true;
      g.m = m;
      g.S = S;
      g.tile = kResampleGroup * S;
      return g;
    }
  }
  g.staged = span(kResampleTile) <= kResampleStageFloats;
  return g;
}

// (q, r) = divmod(n M, L) without forming n M: exact for every n with
// n M / L < 2^64 (M, L < 2^18).
inline void resample_divmod(uint64_t n, uint32_t M, uint32_t L, uint64_t* q, uint32_t* r) {
  const uint64_t t = (n % L) * M;
  *q = (n / L) * M + t / L;
  *r = (uint32_t)(t % L);
}

// The device layout of the table: H'[k][c] = h[(c M) mod L][k], c = n mod L --
// consecutive outputs read consecutive words of a row (gcd(M, L) = 1 makes
// c -> (c M) mod L a permutation).
void resample_permute_taps(const mp3g_resampler& r, std::vector<float>* out);

// resample.hip: the permuted table uploaded to r->device (synchronous), and
// its release.  Return an mp3g_status.
int resample_device_upload(mp3g_resampler* r);
void resample_device_free(mp3g_resampler* r);

}  // namespace mp3g
