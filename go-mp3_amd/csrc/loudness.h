// loudness.h -- the BS.1770 loudness object shared by its host file
// (loudness_tables.cpp: the K-weighting design, the segment tables, argument
// checks, mp3g_loudness_host, mp3g_gain_host) and its device file
// (loudness.hip: table upload, the kernels, mp3g_loudness_rows,
// mp3g_gain_rows).  include/mp3g.h states the contract.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"
#include "loudness_filter.h"

namespace mp3g {

constexpr int kLoudMinRate = 8000, kLoudMaxRate = 192000;
// the segment kernel: samples of every item staged per step, and the odd LDS
// row stride that keeps a wave's reads on 32 different banks
constexpr uint32_t kLoudChunk = 32, kLoudLdsStride = 33, kLoudBlock = 256;
// the row kernel's and the gain kernel's blocks; float4 words a gain thread moves
constexpr uint32_t kLoudRowBlock = 64, kGainBlock = 256, kGainWords = 4;

// the segments a row of T samples can have, plus one for its ragged tail
inline uint32_t loud_items_per_plane(uint32_t T, uint32_t H) { return T / H + 1; }

}  // namespace mp3g

struct mp3g_loudness {
  int device = -1;
  int rate = 0;
  uint32_t H = 0;
  mp3g::LoudCoef coef = {};
  double shelf[5] = {}, highpass[5] = {};  // b0 b1 b2 a1 a2 of each section
  std::vector<double> V;                   // [H][4]
  double AH[16] = {}, G[16] = {};          // [m][k], [a][b]
  // device (loudness.hip)
  double* d_tab = nullptr;  // V, then AH, then G
};

namespace mp3g {

// loudness.hip: the tables uploaded to ld->device (synchronous), and their
// release.  Return an mp3g_status.
int loudness_device_upload(mp3g_loudness* ld);
void loudness_device_free(mp3g_loudness* ld);

// loudness_tables.cpp: the argument checks both forms of a call share.
int loudness_check(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T, uint64_t* n_items);
int gain_check(uint32_t n_rows, uint32_t n_planes, uint32_t T, double target_energy, float peak_ceiling);

}  // namespace mp3g
