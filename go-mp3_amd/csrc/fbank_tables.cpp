// fbank_tables.cpp -- host side of the Kaldi filter-bank features
// (include/mp3g.h "Kaldi filter-bank features of decoded rows"): the window,
// the windowed DFT rows and Kaldi's mel bank in float64, the feature object,
// and mp3g_fbank_host, the plain-C++ statement of the features that the device
// call (fbank.hip) equals bit for bit.  No HIP call is made here.
#include <cmath>
#include <cstring>
#include <new>

#include "abi_util.h"
#include "fbank.h"
#include "fbank_log.h"

using namespace mp3g;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr uint64_t kIndexLimit = 1ull << 62;  // sample indices stay signed-64-bit safe

double mel_of(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

uint64_t frames_of(const mp3g_fbank& fb, uint64_t T) {
  if (T < fb.N) return 0;
  return fb.flags & MP3G_FBANK_SNIP_EDGES ? 1 + (T - fb.N) / fb.hop : (T + fb.hop / 2) / fb.hop;
}

double window_at(int window, uint32_t n, uint32_t N) {
  const double a = 2.0 * kPi * (double)n / (double)(N - 1);
  switch (window) {
    case MP3G_FBANK_WINDOW_POVEY: return std::pow(0.5 - 0.5 * std::cos(a), 0.85);
    case MP3G_FBANK_WINDOW_HAMMING: return 0.54 - 0.46 * std::cos(a);
    case MP3G_FBANK_WINDOW_HANNING: return 0.5 - 0.5 * std::cos(a);
    default: return 1.0;
  }
}

}  // namespace

void mp3g::fbank_device_table(const mp3g_fbank& fb, std::vector<float>* out) {
  const FbankGeom& g = fb.geom;
  const size_t n2s = g.n_pad / 2;
  // Rows N .. n_pad - 1 stay zero.  A zero tap times a finite operand is +-0, and
  // an accumulator that started at +0 is never -0 (x + -x is +0 in round to
  // nearest), so adding +-0 leaves its bits as they are: the padded steps do
  // not change the contract's chain over n < N.
  out->assign(n2s * g.tiles * 128, 0.f);
  for (size_t n2 = 0; n2 < n2s; n2++)
    for (uint32_t t = 0; t < g.tiles; t++)
      for (uint32_t q = 0; q < 2; q++) {
        const std::vector<float>& tab = q ? fb.sw : fb.cw;
        float* run = out->data() + ((n2 * g.tiles + t) * 2 + q) * 64;
        for (uint32_t l = 0; l < 64; l++) {
          const uint32_t k = t * 32 + (l & 31), n = (uint32_t)(2 * n2) + (l >> 5);
          if (k < fb.K && n < fb.N) run[l] = tab[(size_t)k * fb.N + n];
        }
      }
}

void mp3g::fbank_device_filters(const mp3g_fbank& fb, std::vector<float>* weights, std::vector<uint32_t>* support) {
  weights->clear();
  support->assign((size_t)fb.n_mels * 3, 0);
  for (uint32_t m = 0; m < fb.n_mels; m++) {
    const uint32_t lo = fb.support[2 * m], hi = fb.support[2 * m + 1];
    (*support)[3 * m] = lo;
    (*support)[3 * m + 1] = hi;
    (*support)[3 * m + 2] = (uint32_t)weights->size();
    for (uint32_t k = lo; k <= hi; k++) weights->push_back(fb.wm[(size_t)m * fb.K + k]);
  }
  if (weights->empty()) weights->push_back(0.f);  // (every filter empty: still a buffer)
}

extern "C" {

int mp3g_fbank_create(int device, int rate, int N, int hop, int n_mels, double low_freq, double high_freq,
                      double preemph, double scale, int window, uint32_t flags, mp3g_fbank** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (rate <= 0 || N <= 0 || hop <= 0 || n_mels <= 0)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: rate, window length, hop or n_mels not positive");
  if (flags & ~(uint32_t)(MP3G_FBANK_REMOVE_DC | MP3G_FBANK_SNIP_EDGES))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: unknown flag");
  if (window < MP3G_FBANK_WINDOW_POVEY || window > MP3G_FBANK_WINDOW_RECTANGULAR)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: unknown window");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (hop > N) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: hop beyond the window");
  const double nyquist = 0.5 * (double)rate;
  if (!std::isfinite(low_freq) || !std::isfinite(high_freq))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: low_freq or high_freq not finite");
  if (high_freq <= 0.0) high_freq += nyquist;
  if (!(low_freq >= 0.0) || !(low_freq < high_freq) || !(high_freq <= nyquist))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: not 0 <= low_freq < high_freq <= rate / 2");
  if (!(preemph >= 0.0) || !(preemph <= 1.0)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: preemph outside [0, 1]");
  const float fscale = (float)scale;
  if (!std::isfinite(scale) || !std::isfinite(fscale) || !(fscale > 0.f))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: scale not a positive finite float32");
  if (N < MP3G_FBANK_MIN_WINDOW || N > MP3G_FBANK_MAX_WINDOW)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "fbank: window length outside 16..1024");
  if (n_mels > MP3G_FBANK_MAX_MELS) return abi_fail(MP3G_ERR_UNSUPPORTED, "fbank: more than 128 mel bands");

  mp3g_fbank* fb = new (std::nothrow) mp3g_fbank;
  if (!fb) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "fbank");
  fb->device = device;
  fb->rate = (uint32_t)rate;
  fb->N = (uint32_t)N;
  fb->hop = (uint32_t)hop;
  fb->n_mels = (uint32_t)n_mels;
  fb->flags = flags;
  fb->window = (uint32_t)window;
  fb->preemph = (float)preemph;
  fb->scale = fscale;
  fb->rN = (float)(1.0 / (double)N);
  uint32_t P = 16;
  while (P < fb->N) P *= 2;
  const uint32_t Nw = fb->N, K = P / 2, nm = fb->n_mels;
  fb->P = P;
  fb->K = K;
  fb->geom = fbank_geometry(Nw, fb->hop, K);
  try {
    fb->w.resize(Nw);
    fb->cw.resize((size_t)K * Nw);
    fb->sw.resize((size_t)K * Nw);
    fb->wm.assign((size_t)nm * K, 0.f);
    fb->support.resize((size_t)nm * 2);
  } catch (...) {
    delete fb;
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "fbank tables");
  }
  // the window folded into the DFT rows; (k n) mod P in integers
  for (uint32_t n = 0; n < Nw; n++) fb->w[n] = (float)window_at(window, n, Nw);
  for (uint32_t k = 0; k < K; k++)
    for (uint32_t n = 0; n < Nw; n++) {
      const double w = window_at(window, n, Nw);
      const double a = 2.0 * kPi * (double)(((uint64_t)k * n) % P) / (double)P;
      fb->cw[(size_t)k * Nw + n] = (float)(w * std::cos(a));
      fb->sw[(size_t)k * Nw + n] = (float)(-w * std::sin(a));
    }
  // Kaldi's mel bank: n_mels triangles of equal width in mel, half overlapped, not normalised
  const double mlo = mel_of(low_freq), delta = (mel_of(high_freq) - mlo) / (double)(nm + 1);
  for (uint32_t m = 0; m < nm; m++) {
    const double left = mlo + (double)m * delta, centre = left + delta, right = centre + delta;
    uint32_t lo = 1, hi = 0;
    for (uint32_t k = 0; k < K; k++) {
      const double mk = mel_of((double)k * (double)rate / (double)P);
      const double up = (mk - left) / delta, down = (right - mk) / delta;
      const double t = up < down ? up : down;
      const float wgt = t > 0.0 ? (float)t : 0.f;
      fb->wm[(size_t)m * K + k] = wgt;
      if (wgt != 0.f) {
        if (lo > hi) lo = k;
        hi = k;
      }
    }
    fb->support[2 * m] = lo;
    fb->support[2 * m + 1] = hi;
  }
  if (device >= 0) {
    const int st = fbank_device_upload(fb);
    if (st != MP3G_OK) {
      delete fb;
      return st;
    }
  }
  *out = fb;
  return MP3G_OK;
}

void mp3g_fbank_free(mp3g_fbank* fb) {
  if (!fb) return;
  if (fb->d_dft || fb->d_wm || fb->d_support) fbank_device_free(fb);
  delete fb;
}

int mp3g_fbank_info(const mp3g_fbank* fb, uint32_t* P, uint32_t* K, const float** cw, const float** sw,
                    const float** wm, const uint32_t** support, const float** w, uint32_t* tile_frames) {
  if (!fb) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null fbank");
  if (P) *P = fb->P;
  if (K) *K = fb->K;
  if (cw) *cw = fb->cw.data();
  if (sw) *sw = fb->sw.data();
  if (wm) *wm = fb->wm.data();
  if (support) *support = fb->support.data();
  if (w) *w = fb->w.data();
  if (tile_frames) *tile_frames = fb->geom.tile_frames;
  return MP3G_OK;
}

uint64_t mp3g_fbank_frames(const mp3g_fbank* fb, uint64_t T) {
  if (!fb || T >= kIndexLimit) return 0;
  return frames_of(*fb, T);
}

void mp3g_fbank_logf(const float* x, uint64_t n, float* y) {
  for (uint64_t i = 0; i < n; i++) y[i] = mp3g_logf(x[i]);
}

int mp3g_fbank_host(const mp3g_fbank* fb, const float* x, uint64_t T, uint64_t n_frames, float* out,
                    uint64_t mel_stride) {
  if (!fb || (T && !x) || (n_frames && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (T >= kIndexLimit) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: sample index beyond 2^62");
  if (n_frames > frames_of(*fb, T)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: more frames than the row has");
  if (mel_stride < fb->n_mels) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "fbank: mel stride below n_mels");
  if (n_frames == 0) return MP3G_OK;
  const uint32_t N = fb->N, K = fb->K;
  const bool snip = fb->flags & MP3G_FBANK_SNIP_EDGES, dc = fb->flags & MP3G_FBANK_REMOVE_DC;
  const int64_t shift = snip ? 0 : (int64_t)(fb->hop / 2) - (int64_t)(N / 2), len = (int64_t)T;
  const float npre = -fb->preemph;
  std::vector<float> s, e, power;
  try {
    s.resize(N);
    e.resize(N);
    power.resize(K);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "fbank frame");
  }
  for (uint64_t f = 0; f < n_frames; f++) {
    // Kaldi's reflection repeats the edge sample.  One reflection is enough: a
    // row with a frame has T >= N; the first frame starts at hop / 2 - N / 2 >=
    // -N / 2, so -j - 1 < N / 2 <= T; the last starts at (F - 1) hop + hop / 2 -
    // N / 2 with (F - 1) hop <= T - hop + hop / 2, so its last index is at most
    // T - 1 + (N + 1) / 2 and 2 T - 1 - j >= T - (N + 1) / 2 >= 0.
    for (uint32_t n = 0; n < N; n++) {
      int64_t j = (int64_t)(f * fb->hop) + shift + (int64_t)n;
      if (j < 0) j = -j - 1;
      if (j >= len) j = 2 * len - 1 - j;
      s[n] = fb->scale * x[j];
    }
    if (dc) {
      float sum = 0.f;
      for (uint32_t n = 0; n < N; n++) sum = std::fmaf(s[n], 1.0f, sum);
      const float mean = sum * fb->rN;
      for (uint32_t n = 0; n < N; n++) s[n] = std::fmaf(mean, -1.0f, s[n]);
    }
    e[0] = std::fmaf(npre, s[0], s[0]);
    for (uint32_t n = 1; n < N; n++) e[n] = std::fmaf(npre, s[n - 1], s[n]);
    for (uint32_t k = 0; k < K; k++) {
      const float* c = fb->cw.data() + (size_t)k * N;
      const float* sn = fb->sw.data() + (size_t)k * N;
      float re = 0.f, im = 0.f;
      for (uint32_t n = 0; n < N; n++) {
        re = std::fmaf(c[n], e[n], re);
        im = std::fmaf(sn[n], e[n], im);
      }
      power[k] = std::fmaf(re, re, im * im);
    }
    for (uint32_t m = 0; m < fb->n_mels; m++) {
      const float* w = fb->wm.data() + (size_t)m * K;
      float mel = 0.f;
      for (uint32_t k = fb->support[2 * m]; k <= fb->support[2 * m + 1]; k++) mel = std::fmaf(w[k], power[k], mel);
      out[(size_t)f * mel_stride + m] = fbank_log(mel);
    }
  }
  return MP3G_OK;
}

}  // extern "C"
