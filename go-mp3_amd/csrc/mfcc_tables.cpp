// mfcc_tables.cpp -- host side of the Kaldi MFCC features (include/mp3g.h
// "Kaldi MFCC features of decoded rows") and of the per-row normalisation
// ("Per-row mean and variance normalisation"): Kaldi's DCT matrix and lifter in
// float64, the feature object around an owned mp3g_fbank, mp3g_mfcc_host and
// mp3g_cmvn_host -- the plain-C++ statements that the device calls (mfcc.hip)
// equal bit for bit.  No HIP call is made here.
#include <cfloat>
#include <cmath>
#include <new>

#include "abi_util.h"
#include "fbank_log.h"
#include "mfcc.h"

using namespace mp3g;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr uint32_t kFlags = MP3G_FBANK_REMOVE_DC | MP3G_FBANK_SNIP_EDGES | MP3G_MFCC_USE_ENERGY | MP3G_MFCC_RAW_ENERGY;

}  // namespace

extern "C" {

int mp3g_mfcc_create(int device, int rate, int N, int hop, int n_mels, int n_ceps, double low_freq, double high_freq,
                     double preemph, double scale, double cepstral_lifter, double energy_floor, int window,
                     uint32_t flags, mp3g_mfcc** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (flags & ~kFlags) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: unknown flag");
  if (n_ceps <= 0 || (n_mels > 0 && n_ceps > n_mels))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: n_ceps outside 1..n_mels");
  if (!std::isfinite(cepstral_lifter) || !(cepstral_lifter >= 0.0))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: cepstral_lifter negative or not finite");
  const float ffloor = (float)energy_floor;
  if (!std::isfinite(energy_floor) || !std::isfinite(ffloor) || !(energy_floor >= 0.0) ||
      (energy_floor > 0.0 && ffloor < FLT_MIN))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: energy_floor not 0 or a normal positive float32");
  // the front end: mp3g_fbank_create's checks and status codes, its tables, its upload
  mp3g_fbank* fb = nullptr;
  const int st = mp3g_fbank_create(device, rate, N, hop, n_mels, low_freq, high_freq, preemph, scale, window,
                                   flags & (MP3G_FBANK_REMOVE_DC | MP3G_FBANK_SNIP_EDGES), &fb);
  if (st != MP3G_OK) return st;
  mp3g_mfcc* mf = new (std::nothrow) mp3g_mfcc;
  if (!mf) {
    mp3g_fbank_free(fb);
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "mfcc");
  }
  mf->fb = fb;
  mf->n_ceps = (uint32_t)n_ceps;
  mf->flags = flags;
  mf->energy_floor = ffloor;
  mf->lef = ffloor > 0.f ? mp3g_logf(ffloor) : 0.f;
  const uint32_t M = fb->n_mels, C = mf->n_ceps;
  try {
    mf->dct.resize((size_t)C * M);
    mf->lift.resize(C);
  } catch (...) {
    mp3g_mfcc_free(mf);
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "mfcc tables");
  }
  // Kaldi's ComputeDctMatrix, its first n_ceps rows
  for (uint32_t m = 0; m < M; m++) mf->dct[m] = (float)std::sqrt(1.0 / (double)M);
  for (uint32_t i = 1; i < C; i++)
    for (uint32_t m = 0; m < M; m++)
      mf->dct[(size_t)i * M + m] =
          (float)(std::sqrt(2.0 / (double)M) * std::cos(kPi / (double)M * ((double)m + 0.5) * (double)i));
  for (uint32_t i = 0; i < C; i++)
    mf->lift[i] = cepstral_lifter > 0.0
                      ? (float)(1.0 + 0.5 * cepstral_lifter * std::sin(kPi * (double)i / cepstral_lifter))
                      : 1.0f;
  if (device >= 0) {
    const int up = mfcc_device_upload(mf);
    if (up != MP3G_OK) {
      mp3g_mfcc_free(mf);
      return up;
    }
  }
  *out = mf;
  return MP3G_OK;
}

void mp3g_mfcc_free(mp3g_mfcc* mf) {
  if (!mf) return;
  if (mf->d_dct || mf->d_aux) mfcc_device_free(mf);
  mp3g_fbank_free(mf->fb);
  delete mf;
}

int mp3g_mfcc_info(const mp3g_mfcc* mf, const mp3g_fbank** fbank, uint32_t* n_ceps, const float** dct,
                   const float** lifter, float* log_energy_floor, uint32_t* dct_in_lds) {
  if (!mf) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null mfcc");
  if (fbank) *fbank = mf->fb;
  if (n_ceps) *n_ceps = mf->n_ceps;
  if (dct) *dct = mf->dct.data();
  if (lifter) *lifter = mf->lift.data();
  if (log_energy_floor) *log_energy_floor = mf->lef;
  if (dct_in_lds) *dct_in_lds = mf->dct_in_lds;
  return MP3G_OK;
}

uint64_t mp3g_mfcc_frames(const mp3g_mfcc* mf, uint64_t T) { return mf ? mp3g_fbank_frames(mf->fb, T) : 0; }

int mp3g_mfcc_host(const mp3g_mfcc* mf, const float* x, uint64_t T, uint64_t n_frames, float* out,
                   uint64_t cep_stride) {
  if (!mf || (T && !x) || (n_frames && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (cep_stride < mf->n_ceps) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: cepstral stride below n_ceps");
  const mp3g_fbank& fb = *mf->fb;
  const uint32_t N = fb.N, M = fb.n_mels, C = mf->n_ceps;
  if (n_frames > mp3g_fbank_frames(&fb, T) || (n_frames && T < N))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "mfcc: more frames than the row has");
  if (n_frames == 0) return MP3G_OK;
  std::vector<float> L, s, v;
  try {
    L.resize((size_t)n_frames * M);
    s.resize(N);
    v.resize(N);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "mfcc frames");
  }
  // L[f][m]: the filter-bank features of the same front end
  const int st = mp3g_fbank_host(&fb, x, T, n_frames, L.data(), M);
  if (st != MP3G_OK) return st;
  const bool snip = fb.flags & MP3G_FBANK_SNIP_EDGES, dc = fb.flags & MP3G_FBANK_REMOVE_DC;
  const bool use_energy = mf->flags & MP3G_MFCC_USE_ENERGY, raw = mf->flags & MP3G_MFCC_RAW_ENERGY;
  const int64_t shift = snip ? 0 : (int64_t)(fb.hop / 2) - (int64_t)(N / 2), len = (int64_t)T;
  const float npre = -fb.preemph;
  for (uint64_t f = 0; f < n_frames; f++) {
    float* y = out + (size_t)f * cep_stride;
    const float* Lf = L.data() + (size_t)f * M;
    for (uint32_t i = 0; i < C; i++) {
      const float* D = mf->dct.data() + (size_t)i * M;
      float c = 0.f;
      for (uint32_t m = 0; m < M; m++) c = std::fmaf(D[m], Lf[m], c);
      y[i] = c * mf->lift[i];
    }
    if (!use_energy) continue;
    // s, mean, d and e as mp3g_fbank_host forms them (one reflection is enough: fbank_tables.cpp)
    for (uint32_t n = 0; n < N; n++) {
      int64_t j = (int64_t)(f * fb.hop) + shift + (int64_t)n;
      if (j < 0) j = -j - 1;
      if (j >= len) j = 2 * len - 1 - j;
      s[n] = fb.scale * x[j];
    }
    if (dc) {
      float sum = 0.f;
      for (uint32_t n = 0; n < N; n++) sum = std::fmaf(s[n], 1.0f, sum);
      const float mean = sum * fb.rN;
      for (uint32_t n = 0; n < N; n++) s[n] = std::fmaf(mean, -1.0f, s[n]);
    }
    if (raw) {
      for (uint32_t n = 0; n < N; n++) v[n] = s[n];
    } else {
      v[0] = fb.w[0] * std::fmaf(npre, s[0], s[0]);
      for (uint32_t n = 1; n < N; n++) v[n] = fb.w[n] * std::fmaf(npre, s[n - 1], s[n]);
    }
    float en = 0.f;
    for (uint32_t n = 0; n < N; n++) en = std::fmaf(v[n], v[n], en);
    float le = fbank_log(en);
    if (mf->energy_floor > 0.f && le < mf->lef) le = mf->lef;
    y[0] = le;
  }
  return MP3G_OK;
}

int mp3g_cmvn_host(float* feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                   uint32_t n_cols, const uint32_t* lengths, uint32_t flags) {
  if (flags & ~(uint32_t)MP3G_CMVN_NORM_VARS) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: unknown flag");
  if (stride < n_cols) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: stride below n_cols");
  if (!n_rows || !n_planes || !n_frames || !n_cols) return MP3G_OK;
  if (!feats || !lengths) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "cmvn: null buffer");
  const bool vars = flags & MP3G_CMVN_NORM_VARS;
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t n = lengths[r] < n_frames ? lengths[r] : n_frames;
    if (n == 0) continue;
    for (uint32_t p = 0; p < n_planes; p++) {
      float* x = feats + ((size_t)r * n_planes + p) * n_frames * stride;
      for (uint32_t c = 0; c < n_cols; c++) {
        double sum = 0.0, sq = 0.0;
        for (uint32_t f = 0; f < n; f++) {
          const double v = (double)x[(size_t)f * stride + c];
          sum += v;
          sq += v * v;
        }
        const double mean = sum / (double)n;
        float scale = 1.0f;
        if (vars) {
          const double var = sq / (double)n - mean * mean;
          const float v32 = (float)var;
          const float vf = v32 > 1e-20f ? v32 : 1e-20f;
          scale = 1.0f / __builtin_sqrtf(vf);
        }
        for (uint32_t f = 0; f < n; f++) {
          float y = (float)((double)x[(size_t)f * stride + c] - mean);
          if (vars) y = y * scale;
          x[(size_t)f * stride + c] = y;
        }
      }
    }
  }
  return MP3G_OK;
}

}  // extern "C"
