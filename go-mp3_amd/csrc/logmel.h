// logmel.h -- the log-mel feature object shared by its host file
// (logmel_tables.cpp: table design, argument checks, host reference) and its
// device file (logmel.hip: table upload, kernels).  include/mp3g.h states the
// contract.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"

namespace mp3g {

// How the device call tiles a row (logmel.hip).  A workgroup produces
// tile_frames consecutive frames of one (row, plane); its source span
// (tile_frames - 1) hop + n_fft is staged in LDS (at most kLogmelSpanFloats).
// The MFMA tile is 32 frames tall: a shorter tile (long hops) repeats its last
// frame in the unused rows.  Bins come in tiles of 32, one wave to a tile (its
// cos and sin accumulators), at most kLogmelMaxWaves waves: with more tiles a
// wave takes every waves-th.
//
// The A operand's lanes read s_x[frame hop + n]: 32 frames `hop` words apart.
// hop = 160 puts them on two of the 64 banks, so sample j is stored at word
// j + (j >> skew): one pad word every 2^skew samples.  logmel_geometry takes the
// skew (6, 5, 4, or 31 = none) under which a read's lanes share banks least
// (hop = 160: skew 4, no two of the 64 lanes on one bank).
constexpr uint32_t kLogmelSpanFloats = 9216;
constexpr uint32_t kLogmelStageFloats = kLogmelSpanFloats + kLogmelSpanFloats / 16;  // 38.25 KB, pad words included
constexpr uint32_t kLogmelMaxWaves = 8;
constexpr uint32_t kLogmelPStride = 33;  // power rows in LDS: [k][33], frames along a row
struct LogmelGeom {
  uint32_t tile_frames = 32;
  uint32_t span = 0;   // (tile_frames - 1) hop + n_fft
  uint32_t skew = 31;  // sample j lives at word j + (j >> skew)
  uint32_t stage = 0;  // words of the stage, pad words included
  uint32_t tiles = 0;  // ceil(K / 32) bin tiles
  uint32_t waves = 0;  // min(tiles, kLogmelMaxWaves)
};
inline uint32_t logmel_bank_cost(uint32_t tile_frames, uint32_t hop, uint32_t skew) {
  uint32_t cost = 0;  // over 64 steps: the most distinct words of one read that share a bank
  for (uint32_t n = 0; n < 128; n += 2) {
    uint32_t words[64][64], count[64] = {};
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t f = (l & 31) < tile_frames ? (l & 31) : tile_frames - 1, j = f * hop + n + (l >> 5);
      const uint32_t w = j + (j >> skew), b = w & 63;
      bool seen = false;
      for (uint32_t i = 0; i < count[b]; i++) seen = seen || words[b][i] == w;
      if (!seen) words[b][count[b]++] = w;
    }
    uint32_t worst = 0;
    for (uint32_t b = 0; b < 64; b++) worst = count[b] > worst ? count[b] : worst;
    cost += worst;
  }
  return cost;
}
inline LogmelGeom logmel_geometry(uint32_t n_fft, uint32_t hop) {
  LogmelGeom g;
  while ((g.tile_frames - 1) * hop + n_fft > kLogmelSpanFloats) g.tile_frames /= 2;  // hop <= n_fft <= 1024: >= 8
  g.span = (g.tile_frames - 1) * hop + n_fft;
  uint32_t best = logmel_bank_cost(g.tile_frames, hop, 31);
  for (uint32_t skew = 6; skew >= 4; skew--) {
    const uint32_t c = logmel_bank_cost(g.tile_frames, hop, skew);
    if (c < best) {
      best = c;
      g.skew = skew;
    }
  }
  g.stage = g.span + (g.span >> g.skew);
  g.tiles = (n_fft / 2 + 1 + 31) / 32;
  g.waves = g.tiles < kLogmelMaxWaves ? g.tiles : kLogmelMaxWaves;
  return g;
}

}  // namespace mp3g

struct mp3g_logmel {
  int device = -1;
  uint32_t rate = 0, n_fft = 0, hop = 0, n_mels = 0, flags = 0, K = 0;
  std::vector<float> cw, sw;      // [K][n_fft]: the windowed DFT rows
  std::vector<float> wm;          // [n_mels][K]: the mel weights
  std::vector<uint32_t> support;  // [n_mels][2]: lo, hi (lo > hi: an empty filter)
  // device (logmel.hip)
  float* d_dft = nullptr;         // [n_fft / 2][tiles][2][64]: logmel_device_table
  float* d_wm = nullptr;          // the filters' non-zero weights, one after the other (logmel_device_filters)
  uint32_t* d_support = nullptr;  // [n_mels][3]: lo, hi, the filter's offset in d_wm
  uint32_t* d_max = nullptr;      // MP3G_LOGMEL_CLAMP: the planes' maxima of one launch (ordered integers)
  uint32_t n_weights = 0;         // floats of d_wm
  mp3g::LogmelGeom geom;          // logmel_geometry(n_fft, hop), taken once
};

namespace mp3g {

// The device layout of the DFT table: for step n2 (samples 2 n2, 2 n2 + 1) and
// bin tile t, two runs of 64 floats -- cos, sin -- each [n & 1][bin & 31]: the
// f32 MFMA's B operand, one coalesced 256-byte read per run.  Bins >= K are zero.
void logmel_device_table(const mp3g_logmel& lm, std::vector<float>* out);
// The mel filters for the device: the weights of every support back to back
// (a bin lies inside at most two neighbouring triangles: at most 2 K floats)
// and [n_mels][3] = lo, hi, offset.
void logmel_device_filters(const mp3g_logmel& lm, std::vector<float>* weights, std::vector<uint32_t>* support);

// logmel.hip: the tables uploaded to lm->device (synchronous), and their
// release.  Return an mp3g_status.
int logmel_device_upload(mp3g_logmel* lm);
void logmel_device_free(mp3g_logmel* lm);

}  // namespace mp3g
