// logmel_tables.cpp -- host side of the log-mel features (include/mp3g.h
// "log-mel features of decoded rows"): the windowed DFT rows and the Slaney mel
// filter bank in float64, the feature object, and mp3g_logmel_host, the
// plain-C++ statement of the features that the device call (logmel.hip) equals
// bit for bit.  No HIP call is made here.
#include <cmath>
#include <cstring>
#include <new>

#include "abi_util.h"
#include "logmel.h"
#include "logmel_log10.h"

using namespace mp3g;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr uint64_t kIndexLimit = 1ull << 62;  // sample indices stay signed-64-bit safe

// Slaney's mel scale (librosa's default, htk = false): linear below 1 kHz,
// logarithmic above, 27 steps to 6.4 kHz.
constexpr double kFsp = 200.0 / 3.0, kMinLogHz = 1000.0;
double hz_to_mel(double f) {
  const double min_log_mel = kMinLogHz / kFsp, logstep = std::log(6.4) / 27.0;
  return f >= kMinLogHz ? min_log_mel + std::log(f / kMinLogHz) / logstep : f / kFsp;
}
double mel_to_hz(double m) {
  const double min_log_mel = kMinLogHz / kFsp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? kMinLogHz * std::exp(logstep * (m - min_log_mel)) : kFsp * m;
}

uint64_t frames_of(const mp3g_logmel& lm, uint64_t T) {
  if (lm.flags & MP3G_LOGMEL_CENTER) return T > lm.n_fft / 2 ? T / lm.hop + 1 : 0;
  return T >= lm.n_fft ? (T - lm.n_fft) / lm.hop + 1 : 0;
}

}  // namespace

void mp3g::logmel_device_table(const mp3g_logmel& lm, std::vector<float>* out) {
  const LogmelGeom& g = lm.geom;
  const size_t n2s = lm.n_fft / 2;
  out->assign(n2s * g.tiles * 128, 0.f);
  for (size_t n2 = 0; n2 < n2s; n2++)
    for (uint32_t t = 0; t < g.tiles; t++)
      for (uint32_t q = 0; q < 2; q++) {
        const std::vector<float>& tab = q ? lm.sw : lm.cw;
        float* run = out->data() + ((n2 * g.tiles + t) * 2 + q) * 64;
        for (uint32_t l = 0; l < 64; l++) {
          const uint32_t k = t * 32 + (l & 31);
          if (k < lm.K) run[l] = tab[(size_t)k * lm.n_fft + 2 * n2 + (l >> 5)];
        }
      }
}

void mp3g::logmel_device_filters(const mp3g_logmel& lm, std::vector<float>* weights, std::vector<uint32_t>* support) {
  weights->clear();
  support->assign((size_t)lm.n_mels * 3, 0);
  for (uint32_t m = 0; m < lm.n_mels; m++) {
    const uint32_t lo = lm.support[2 * m], hi = lm.support[2 * m + 1];
    (*support)[3 * m] = lo;
    (*support)[3 * m + 1] = hi;
    (*support)[3 * m + 2] = (uint32_t)weights->size();
    for (uint32_t k = lo; k <= hi; k++) weights->push_back(lm.wm[(size_t)m * lm.K + k]);
  }
  if (weights->empty()) weights->push_back(0.f);  // (every filter empty: still a buffer)
}

extern "C" {

int mp3g_logmel_create(int device, int rate, int n_fft, int hop, int n_mels, double fmin, double fmax,
                       uint32_t flags, mp3g_logmel** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (rate <= 0 || n_fft <= 0 || hop <= 0 || n_mels <= 0)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: rate, n_fft, hop or n_mels not positive");
  if (flags & ~(uint32_t)(MP3G_LOGMEL_CENTER | MP3G_LOGMEL_CLAMP))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: unknown flag");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (hop > n_fft) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: hop beyond n_fft");
  const double nyquist = 0.5 * (double)rate;
  if (!(fmin >= 0.0) || !(fmax >= 0.0) || !(fmax <= nyquist))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: fmin < 0 or fmax outside [0, rate / 2]");
  if (fmax == 0.0) fmax = nyquist;
  if (!(fmin < fmax)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: fmin not below fmax");
  if (n_fft < MP3G_LOGMEL_MIN_FFT || n_fft > MP3G_LOGMEL_MAX_FFT || n_fft % 4 != 0)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "logmel: n_fft not a multiple of 4 in 16..1024");
  if (n_mels > MP3G_LOGMEL_MAX_MELS) return abi_fail(MP3G_ERR_UNSUPPORTED, "logmel: more than 128 mel bands");

  mp3g_logmel* lm = new (std::nothrow) mp3g_logmel;
  if (!lm) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "logmel");
  lm->device = device;
  lm->rate = (uint32_t)rate;
  lm->n_fft = (uint32_t)n_fft;
  lm->hop = (uint32_t)hop;
  lm->n_mels = (uint32_t)n_mels;
  lm->flags = flags;
  lm->geom = logmel_geometry(lm->n_fft, lm->hop);
  const uint32_t N = lm->n_fft, K = N / 2 + 1, nm = lm->n_mels;
  lm->K = K;
  std::vector<double> hz;
  try {
    lm->cw.resize((size_t)K * N);
    lm->sw.resize((size_t)K * N);
    lm->wm.assign((size_t)nm * K, 0.f);
    lm->support.resize((size_t)nm * 2);
    hz.resize(nm + 2);
  } catch (...) {
    delete lm;
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "logmel tables");
  }
  // the periodic Hann window folded into the DFT rows; (k n) mod N in integers
  for (uint32_t k = 0; k < K; k++)
    for (uint32_t n = 0; n < N; n++) {
      const double w = 0.5 - 0.5 * std::cos(2.0 * kPi * (double)n / (double)N);
      const double a = 2.0 * kPi * (double)(((uint64_t)k * n) % N) / (double)N;
      lm->cw[(size_t)k * N + n] = (float)(w * std::cos(a));
      lm->sw[(size_t)k * N + n] = (float)(-w * std::sin(a));
    }
  // the mel filter bank: nm + 2 points equally spaced in mel, triangles between
  // neighbours, each scaled by 2 / (its width in Hz) (Slaney's area normalisation)
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (uint32_t i = 0; i < nm + 2; i++) hz[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(nm + 1));
  for (uint32_t m = 0; m < nm; m++) {
    uint32_t lo = 1, hi = 0;
    for (uint32_t k = 0; k < K; k++) {
      const double f = (double)k * (double)rate / (double)N;
      const double lower = (f - hz[m]) / (hz[m + 1] - hz[m]);
      const double upper = (hz[m + 2] - f) / (hz[m + 2] - hz[m + 1]);
      const double t = lower < upper ? lower : upper;
      const float w = t > 0.0 ? (float)(t * (2.0 / (hz[m + 2] - hz[m]))) : 0.f;
      lm->wm[(size_t)m * K + k] = w;
      if (w != 0.f) {
        if (lo > hi) lo = k;
        hi = k;
      }
    }
    lm->support[2 * m] = lo;
    lm->support[2 * m + 1] = hi;
  }
  if (device >= 0) {
    const int st = logmel_device_upload(lm);
    if (st != MP3G_OK) {
      delete lm;
      return st;
    }
  }
  *out = lm;
  return MP3G_OK;
}

void mp3g_logmel_free(mp3g_logmel* lm) {
  if (!lm) return;
  if (lm->d_dft || lm->d_wm || lm->d_support || lm->d_max) logmel_device_free(lm);
  delete lm;
}

int mp3g_logmel_info(const mp3g_logmel* lm, uint32_t* K, const float** cw, const float** sw, const float** wm,
                     const uint32_t** support, uint32_t* tile_frames) {
  if (!lm) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null logmel");
  if (K) *K = lm->K;
  if (cw) *cw = lm->cw.data();
  if (sw) *sw = lm->sw.data();
  if (wm) *wm = lm->wm.data();
  if (support) *support = lm->support.data();
  if (tile_frames) *tile_frames = lm->geom.tile_frames;
  return MP3G_OK;
}

uint64_t mp3g_logmel_frames(const mp3g_logmel* lm, uint64_t T) {
  if (!lm || T >= kIndexLimit) return 0;
  return frames_of(*lm, T);
}

void mp3g_logmel_log10f(const float* x, uint64_t n, float* y) {
  for (uint64_t i = 0; i < n; i++) y[i] = mp3g_log10f(x[i]);
}

int mp3g_logmel_host(const mp3g_logmel* lm, const float* x, uint64_t T, uint64_t n_frames, float* out,
                     uint64_t frame_stride) {
  if (!lm || (T && !x) || (n_frames && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (T >= kIndexLimit) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: sample index beyond 2^62");
  if (n_frames > frames_of(*lm, T)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: more frames than the row has");
  if (frame_stride < n_frames) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "logmel: frame stride below n_frames");
  if (n_frames == 0) return MP3G_OK;
  const uint32_t N = lm->n_fft, K = lm->K;
  const int64_t pad = lm->flags & MP3G_LOGMEL_CENTER ? (int64_t)(N / 2) : 0, last = (int64_t)T - 1;
  std::vector<float> frame, power;
  try {
    frame.resize(N);
    power.resize(K);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "logmel frame");
  }
  for (uint64_t f = 0; f < n_frames; f++) {
    for (uint32_t n = 0; n < N; n++) {  // the signal reflected about both ends
      int64_t j = (int64_t)(f * lm->hop) - pad + (int64_t)n;
      if (j < 0) j = -j;
      if (j > last) j = 2 * last - j;
      frame[n] = x[j];
    }
    for (uint32_t k = 0; k < K; k++) {
      const float* c = lm->cw.data() + (size_t)k * N;
      const float* s = lm->sw.data() + (size_t)k * N;
      float re = 0.f, im = 0.f;
      for (uint32_t n = 0; n < N; n++) {
        re = std::fmaf(c[n], frame[n], re);
        im = std::fmaf(s[n], frame[n], im);
      }
      power[k] = std::fmaf(re, re, im * im);
    }
    for (uint32_t m = 0; m < lm->n_mels; m++) {
      const float* w = lm->wm.data() + (size_t)m * K;
      float mel = 0.f;
      for (uint32_t k = lm->support[2 * m]; k <= lm->support[2 * m + 1]; k++) mel = std::fmaf(w[k], power[k], mel);
      out[(size_t)m * frame_stride + f] = logmel_log(mel);
    }
  }
  if (lm->flags & MP3G_LOGMEL_CLAMP) {
    float mx = out[0];
    for (uint32_t m = 0; m < lm->n_mels; m++)
      for (uint64_t f = 0; f < n_frames; f++) {
        const float y = out[(size_t)m * frame_stride + f];
        mx = y > mx ? y : mx;
      }
    for (uint32_t m = 0; m < lm->n_mels; m++)
      for (uint64_t f = 0; f < n_frames; f++) {
        float* y = out + (size_t)m * frame_stride + f;
        *y = logmel_clamp(*y, mx);
      }
  }
  return MP3G_OK;
}

}  // extern "C"
