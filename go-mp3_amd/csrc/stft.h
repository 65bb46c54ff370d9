// stft.h -- the STFT feature object shared by its host file (stft_tables.cpp:
// table design, argument checks, host reference) and its device file (stft.hip:
// table upload, kernel).  include/mp3g.h states the contract, stft_fft.h holds
// the transform both sides compile.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mp3g.h"
#include "stft_fft.h"

namespace mp3g {

// How the device call tiles a row (stft.hip).  A workgroup produces tile_frames
// consecutive frames of one (row, plane), a wave to a frame.  A frame's working
// set is its N = P / 2 complex values in LDS, value i at float2 slot i + (i >> 5)
// (one pad slot every 32: the passes' power-of-two strides then spread over the
// banks); the spectrum replaces it in place.  tile_frames is 16, or 8 at P =
// 4096, where 16 working sets do not fit a CU's 160 KiB.  DESIGN.md 9f has the
// bank arithmetic and the sizes.
constexpr uint32_t kStftMaxWaves = 16;
constexpr uint32_t kStftLdsBudget = 144 * 1024;
MP3G_L10_HD inline uint32_t stft_skew(uint32_t i) { return i + (i >> 5); }
inline uint32_t stft_frame_slots(uint32_t n_fft) { return stft_skew(n_fft / 2 - 1) + 1; }  // float2 slots of a frame
inline uint32_t stft_tile_frames(uint32_t n_fft) {
  uint32_t t = kStftMaxWaves;
  while (t * stft_frame_slots(n_fft) * 8 > kStftLdsBudget) t /= 2;
  return t;
}

}  // namespace mp3g

struct mp3g_stft {
  int device = -1;
  uint32_t rate = 0, n_fft = 0, win_length = 0, hop = 0, output = 0, n_mels = 0, log = 0, flags = 0;
  uint32_t K = 0, log2n = 0, tile_frames = 0;
  float floor = 0.f;
  std::vector<float> window;        // [n_fft]
  std::vector<mp3g::StftC> tw;      // [n_fft]
  std::vector<float> wm;            // [n_mels][K]
  std::vector<uint32_t> support;    // [n_mels][2]: lo, hi (lo > hi: an empty filter)
  // device (stft.hip)
  float* d_window = nullptr;
  mp3g::StftC* d_tw = nullptr;
  float* d_wm = nullptr;            // the filters' non-zero weights, one after the other
  uint32_t* d_support = nullptr;    // [n_mels][3]: lo, hi, the filter's offset in d_wm
};

namespace mp3g {

// stft.hip: the tables uploaded to st->device (synchronous), and their release.
// Return an mp3g_status.
int stft_device_upload(mp3g_stft* st);
void stft_device_free(mp3g_stft* st);

}  // namespace mp3g
