// mfcc.h -- the Kaldi MFCC feature object shared by its host file
// (mfcc_tables.cpp: the DCT and lifter tables, argument checks, host reference,
// mp3g_cmvn_host) and its device file (mfcc.hip: table upload, the kernel,
// mp3g_cmvn_rows).  include/mp3g.h states the contract.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"
#include "fbank.h"

namespace mp3g {

// The transposed DCT matrix is staged in LDS when it has at most this many
// entries (16 KB; (40, 40) and (80, 20) have 1,600); a larger one -- (128, 128)
// is 64 KB -- is read from global memory.
constexpr uint32_t kMfccDctLdsFloats = 4096;
constexpr uint32_t kMfccMaxTileFrames = 32;

}  // namespace mp3g

struct mp3g_mfcc {
  mp3g_fbank* fb = nullptr;    // the owned front end (mp3g_fbank_create with the same device)
  uint32_t n_ceps = 0, flags = 0;
  float energy_floor = 0.f, lef = 0.f;  // lef = mp3g_logf(energy_floor) when the floor is positive
  std::vector<float> dct;      // [n_ceps][n_mels]: D
  std::vector<float> lift;     // [n_ceps]
  // device (mfcc.hip)
  float* d_dct = nullptr;      // [n_mels][n_ceps]: D transposed
  float* d_aux = nullptr;      // the filters' weights and supports, the lifter, the window for the energy
                               // after it and D transposed where staged: what the kernel copies to LDS
  uint32_t dct_in_lds = 0;     // whether the kernel stages d_dct in LDS
};

namespace mp3g {

// mfcc.hip: the tables the owned front end does not have, uploaded to
// mf->fb->device (synchronous), and their release.  Return an mp3g_status.
int mfcc_device_upload(mp3g_mfcc* mf);
void mfcc_device_free(mp3g_mfcc* mf);

}  // namespace mp3g
