// fbank.h -- the Kaldi filter-bank feature object shared by its host file
// (fbank_tables.cpp: table design, argument checks, host reference) and its
// device file (fbank.hip: table upload, kernel).  include/mp3g.h states the
// contract.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"
#include "logmel.h"

namespace mp3g {

// How the device call tiles a row (fbank.hip): log-mel's shape (logmel.h).  A
// workgroup produces tile_frames consecutive frames of one (row, plane) from
// one staged span, sample j at word j + (j >> skew), the skew taken by counting
// bank collisions (logmel_bank_cost: the A operand's lanes are `hop` words
// apart here too).  What differs: the window length N is any integer, so the
// DFT table is extended with zero rows to n_pad = N rounded up to 4 (the
// granularity of the kernel's shortest pass) and the span covers n_pad samples
// of the last frame; and K = P / 2 bins, 32 to a tile, which is whole tiles from
// P = 64 on.
struct FbankGeom {
  uint32_t tile_frames = 32;
  uint32_t n_pad = 0;  // N rounded up to a multiple of 4
  uint32_t span = 0;   // (tile_frames - 1) hop + n_pad
  uint32_t skew = 31;  // sample j lives at word j + (j >> skew)
  uint32_t stage = 0;  // words of the stage, pad words included
  uint32_t tiles = 0;  // ceil(K / 32) bin tiles
  uint32_t waves = 0;  // min(tiles, kLogmelMaxWaves)
};
inline FbankGeom fbank_geometry(uint32_t N, uint32_t hop, uint32_t K) {
  FbankGeom g;
  g.n_pad = (N + 3) & ~3u;
  while ((g.tile_frames - 1) * hop + g.n_pad > kLogmelSpanFloats) g.tile_frames /= 2;  // hop <= N <= 1024: >= 8
  g.span = (g.tile_frames - 1) * hop + g.n_pad;
  uint32_t best = logmel_bank_cost(g.tile_frames, hop, 31);
  for (uint32_t skew = 6; skew >= 4; skew--) {
    const uint32_t c = logmel_bank_cost(g.tile_frames, hop, skew);
    if (c < best) {
      best = c;
      g.skew = skew;
    }
  }
  g.stage = g.span + (g.span >> g.skew);
  g.tiles = (K + 31) / 32;
  g.waves = g.tiles < kLogmelMaxWaves ? g.tiles : kLogmelMaxWaves;
  return g;
}

}  // namespace mp3g

struct mp3g_fbank {
  int device = -1;
  uint32_t rate = 0, N = 0, hop = 0, n_mels = 0, flags = 0, window = 0, P = 0, K = 0;
  float preemph = 0.f, scale = 1.f, rN = 0.f;
  std::vector<float> w;           // [N]: the window
  std::vector<float> cw, sw;      // [K][N]: the windowed DFT rows
  std::vector<float> wm;          // [n_mels][K]: the mel weights
  std::vector<uint32_t> support;  // [n_mels][2]: lo, hi (lo > hi: an empty filter)
  // device (fbank.hip)
  float* d_dft = nullptr;         // [n_pad / 2][tiles][2][64]: fbank_device_table
  float* d_wm = nullptr;          // the filters' non-zero weights, one after the other (fbank_device_filters)
  uint32_t* d_support = nullptr;  // [n_mels][3]: lo, hi, the filter's offset in d_wm
  uint32_t n_weights = 0;         // floats of d_wm
  mp3g::FbankGeom geom;           // fbank_geometry(N, hop, K), taken once
};

namespace mp3g {

// The device layout of the DFT table: for step n2 (samples 2 n2, 2 n2 + 1) and
// bin tile t, two runs of 64 floats -- cos, sin -- each [n & 1][bin & 31]: the
// f32 MFMA's B operand, one coalesced 256-byte read per run.  Rows n >= N (up
// to n_pad) and bins >= K are zero.
void fbank_device_table(const mp3g_fbank& fb, std::vector<float>* out);
// The mel filters for the device: the weights of every support back to back
// (a bin lies inside at most two neighbouring triangles: at most 2 K floats)
// and [n_mels][3] = lo, hi, offset.
void fbank_device_filters(const mp3g_fbank& fb, std::vector<float>* weights, std::vector<uint32_t>* support);

// fbank.hip: the tables uploaded to fb->device (synchronous), and their
// release.  Return an mp3g_status.
int fbank_device_upload(mp3g_fbank* fb);
void fbank_device_free(mp3g_fbank* fb);

}  // namespace mp3g
