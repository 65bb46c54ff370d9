// stft_tables.cpp -- host side of the STFT features (include/mp3g.h "STFT and mel
// spectrograms of decoded rows"): the argument checks, the window, the twiddles
// and the mel filter bank in float64, the feature object, and mp3g_stft_host,
// which walks stft_fft.h's butterflies frame by frame in plain loops -- the
// statement the device call (stft.hip) equals bit for bit.  No HIP call is made
// here.
#include <cfloat>
#include <cmath>
#include <new>

#include "abi_util.h"
#include "stft.h"

using namespace mp3g;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr uint64_t kIndexLimit = 1ull << 62;  // sample indices stay signed-64-bit safe

// Slaney's mel scale (librosa's default): linear below 1 kHz, logarithmic above
constexpr double kFsp = 200.0 / 3.0, kMinLogHz = 1000.0;
double hz_to_mel(double f, bool htk) {
  if (htk) return 2595.0 * std::log10(1.0 + f / 700.0);
  const double min_log_mel = kMinLogHz / kFsp, logstep = std::log(6.4) / 27.0;
  return f >= kMinLogHz ? min_log_mel + std::log(f / kMinLogHz) / logstep : f / kFsp;
}
double mel_to_hz(double m, bool htk) {
  if (htk) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
  const double min_log_mel = kMinLogHz / kFsp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? kMinLogHz * std::exp(logstep * (m - min_log_mel)) : kFsp * m;
}

uint64_t frames_of(const mp3g_stft& st, uint64_t T) {
  if (st.flags & MP3G_STFT_CENTER) return T > st.n_fft / 2 ? T / st.hop + 1 : 0;
  return T >= st.n_fft ? (T - st.n_fft) / st.hop + 1 : 0;
}

}  // namespace

extern "C" {

int mp3g_stft_create(int device, int rate, int n_fft, int win_length, int hop, int output, int n_mels, double fmin,
                     double fmax, int log, float floor, uint32_t flags, mp3g_stft** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (rate <= 0 || win_length <= 0 || hop <= 0)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: rate, win_length or hop not positive");
  if (flags & ~(uint32_t)(MP3G_STFT_CENTER | MP3G_STFT_MEL_HTK | MP3G_STFT_MEL_NORM))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: unknown flag");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  if (output != MP3G_STFT_COMPLEX && output != MP3G_STFT_POWER && output != MP3G_STFT_MAGNITUDE)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: unknown output");
  if (log != MP3G_STFT_LOG_NONE && log != MP3G_STFT_LOG_LN && log != MP3G_STFT_LOG_LOG10)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: unknown logarithm");
  if (output == MP3G_STFT_COMPLEX && (n_mels > 0 || log != MP3G_STFT_LOG_NONE))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: complex output takes no mel bank and no logarithm");
  if (log != MP3G_STFT_LOG_NONE && !(floor >= FLT_MIN && floor <= FLT_MAX))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: the logarithm's floor is not a normal positive float32");
  const double nyquist = 0.5 * (double)rate;
  if (!(fmin >= 0.0) || !(fmax >= 0.0) || !(fmax <= nyquist))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: fmin < 0 or fmax outside [0, rate / 2]");
  if (fmax == 0.0) fmax = nyquist;
  if (!(fmin < fmax)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: fmin not below fmax");
  uint32_t log2n = 0;
  for (uint32_t p = MP3G_STFT_MIN_FFT, l = 7; p <= MP3G_STFT_MAX_FFT; p *= 2, l++)
    if ((uint32_t)n_fft == p && n_fft > 0) log2n = l;
  if (!log2n) return abi_fail(MP3G_ERR_UNSUPPORTED, "stft: n_fft is not 256, 512, 1024, 2048 or 4096");
  if (n_mels < 0 || n_mels > MP3G_STFT_MAX_MELS) return abi_fail(MP3G_ERR_UNSUPPORTED, "stft: n_mels outside 0..128");
  if (win_length > n_fft) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: win_length beyond n_fft");
  if (hop > n_fft) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: hop beyond n_fft");

  mp3g_stft* st = new (std::nothrow) mp3g_stft;
  if (!st) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "stft");
  st->device = device;
  st->rate = (uint32_t)rate;
  st->n_fft = (uint32_t)n_fft;
  st->win_length = (uint32_t)win_length;
  st->hop = (uint32_t)hop;
  st->output = (uint32_t)output;
  st->n_mels = (uint32_t)n_mels;
  st->log = (uint32_t)log;
  st->floor = log != MP3G_STFT_LOG_NONE ? floor : 0.f;
  st->flags = flags;
  st->log2n = log2n;
  st->tile_frames = stft_tile_frames(st->n_fft);
  const uint32_t P = st->n_fft, K = P / 2 + 1, nm = st->n_mels, L = st->win_length;
  st->K = K;
  std::vector<double> hz;
  try {
    st->window.assign(P, 0.f);
    st->tw.resize(P);
    st->wm.assign((size_t)nm * K, 0.f);
    st->support.resize((size_t)nm * 2);
    hz.resize(nm + 2);
  } catch (...) {
    delete st;
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "stft tables");
  }
  const uint32_t left = (P - L) / 2;
  for (uint32_t j = 0; j < L; j++)
    st->window[left + j] = L == 1 ? 1.f : (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)j / (double)L));
  for (uint32_t k = 0; k < P; k++) st->tw[k] = stft_twiddle(k, P);
  // the mel filter bank: nm + 2 points equally spaced in mel, triangles in Hz
  // between neighbours, with MP3G_STFT_MEL_NORM each scaled by 2 / (its width)
  const bool htk = flags & MP3G_STFT_MEL_HTK, norm = flags & MP3G_STFT_MEL_NORM;
  const double m0 = hz_to_mel(fmin, htk), m1 = hz_to_mel(fmax, htk);
  for (uint32_t i = 0; i < nm + 2; i++) hz[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(nm + 1), htk);
  for (uint32_t m = 0; m < nm; m++) {
    uint32_t lo = 1, hi = 0;
    for (uint32_t k = 0; k < K; k++) {
      const double f = (double)k * (double)rate / (double)P;
      const double lower = (f - hz[m]) / (hz[m + 1] - hz[m]);
      const double upper = (hz[m + 2] - f) / (hz[m + 2] - hz[m + 1]);
      const double t = lower < upper ? lower : upper;
      const float w = t > 0.0 ? (float)(norm ? t * (2.0 / (hz[m + 2] - hz[m])) : t) : 0.f;
      st->wm[(size_t)m * K + k] = w;
      if (w != 0.f) {
        if (lo > hi) lo = k;
        hi = k;
      }
    }
    st->support[2 * m] = lo;
    st->support[2 * m + 1] = hi;
  }
  if (device >= 0) {
    const int status = stft_device_upload(st);
    if (status != MP3G_OK) {
      delete st;
      return status;
    }
  }
  *out = st;
  return MP3G_OK;
}

void mp3g_stft_free(mp3g_stft* st) {
  if (!st) return;
  if (st->d_window || st->d_tw || st->d_wm || st->d_support) stft_device_free(st);
  delete st;
}

int mp3g_stft_info(const mp3g_stft* st, uint32_t* K, const float** window, const float** twiddles, const float** wm,
                   const uint32_t** support, uint32_t* tile_frames) {
  if (!st) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null stft");
  if (K) *K = st->K;
  if (window) *window = st->window.data();
  if (twiddles) *twiddles = &st->tw[0].re;
  if (wm) *wm = st->n_mels ? st->wm.data() : nullptr;
  if (support) *support = st->n_mels ? st->support.data() : nullptr;
  if (tile_frames) *tile_frames = st->tile_frames;
  return MP3G_OK;
}

uint64_t mp3g_stft_frames(const mp3g_stft* st, uint64_t T) {
  if (!st || T >= kIndexLimit) return 0;
  return frames_of(*st, T);
}

int mp3g_stft_host(const mp3g_stft* st, const float* x, uint64_t T, uint64_t n_frames, float* out,
                   uint64_t frame_stride) {
  if (!st || (T && !x) || (n_frames && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (T >= kIndexLimit) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: sample index beyond 2^62");
  if (n_frames > frames_of(*st, T)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: more frames than the row has");
  if (frame_stride < n_frames) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "stft: frame stride below n_frames");
  if (n_frames == 0) return MP3G_OK;
  const uint32_t P = st->n_fft, N = P / 2, K = st->K;
  const int64_t pad = st->flags & MP3G_STFT_CENTER ? (int64_t)(P / 2) : 0, last = (int64_t)T - 1;
  const StftC* tw = st->tw.data();
  const bool complex_out = st->output == MP3G_STFT_COMPLEX;
  std::vector<StftC> z, X;
  std::vector<float> s;
  try {
    z.resize(N);
    X.resize(K);
    s.resize(K);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "stft frame");
  }
  for (uint64_t f = 0; f < n_frames; f++) {
    for (uint32_t n = 0; n < P; n++) {  // the signal reflected about both ends, windowed
      int64_t j = (int64_t)(f * st->hop) - pad + (int64_t)n;
      if (j < 0) j = -j;
      if (j > last) j = 2 * last - j;
      const float v = st->window[n] * x[j];
      if (n & 1) z[n >> 1].im = v;
      else z[n >> 1].re = v;
    }
    uint32_t len = N;
    for (; len >= 4; len >>= 2) {
      const uint32_t q = len >> 2, step = P / len;
      for (uint32_t base = 0; base < N; base += len)
        for (uint32_t n = 0; n < q; n++) {
          StftC* p = z.data() + base + n;
          stft_bfly4(p, p + q, p + 2 * q, p + 3 * q, tw, n * step, P);
        }
    }
    if (len == 2)
      for (uint32_t base = 0; base < N; base += 2) stft_bfly2(z.data() + base, z.data() + base + 1);
    stft_split0(z[0], &X[0], &X[N]);
    for (uint32_t k = 1; k <= N / 2; k++) {
      StftC xk, xn;
      stft_split(z[stft_slot(k, st->log2n)], z[stft_slot(N - k, st->log2n)], tw, k, P, &xk, &xn);
      X[N - k] = xn;
      X[k] = xk;  // (k = N / 2: X[k]'s formula stands)
    }
    if (complex_out) {
      for (uint32_t k = 0; k < K; k++) {
        out[((size_t)k * frame_stride + f) * 2] = X[k].re;
        out[((size_t)k * frame_stride + f) * 2 + 1] = X[k].im;
      }
      continue;
    }
    for (uint32_t k = 0; k < K; k++) s[k] = stft_scalar(X[k], st->output);
    if (!st->n_mels) {
      for (uint32_t k = 0; k < K; k++) out[(size_t)k * frame_stride + f] = stft_log(s[k], st->log, st->floor);
      continue;
    }
    for (uint32_t m = 0; m < st->n_mels; m++) {
      const float* w = st->wm.data() + (size_t)m * K;
      float mel = 0.f;
      for (uint32_t k = st->support[2 * m]; k <= st->support[2 * m + 1]; k++) mel = std::fmaf(w[k], s[k], mel);
      out[(size_t)m * frame_stride + f] = stft_log(mel, st->log, st->floor);
    }
  }
  return MP3G_OK;
}

}  // extern "C"
