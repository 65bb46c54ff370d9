// resample_tables.cpp -- host side of the polyphase resampler (include/mp3g.h
// "sample-rate conversion of decoded rows"): the windowed-sinc filter design
// in float64, the resampler object, and mp3g_resample_host, the plain-C++
// statement of the resampled signal that the device call (resample.hip)
// equals bit for bit.  No HIP call is made here.
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>

#include "abi_util.h"
#include "resample.h"

using namespace mp3g;

namespace {

// Modified Bessel function of the first kind, order 0: the power series
// sum ((x / 2)^m / m!)^2, all terms positive (x <= ~15 here: < 60 terms).
double bessel_i0(double x) {
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int m = 1; m < 500; m++) {
    term *= h / m;
    const double t2 = term * term;
    sum += t2;
    if (t2 < 1e-18 * sum) break;
  }
  return sum;
}

constexpr double kPi = 3.14159265358979323846;
constexpr uint64_t kIndexLimit = 1ull << 62;  // sample indices stay signed-64-bit safe

}  // namespace

void mp3g::resample_permute_taps(const mp3g_resampler& r, std::vector<float>* out) {
  const size_t n2w = 2 * (size_t)r.W;
  out->assign((size_t)r.L * n2w, 0.f);
  for (uint32_t c = 0; c < r.L; c++) {
    const uint32_t ph = (uint32_t)(((uint64_t)c * r.M) % r.L);
    for (size_t k = 0; k < n2w; k++) (*out)[k * r.L + c] = r.taps[(size_t)ph * n2w + k];
  }
}

extern "C" {

int mp3g_resampler_create(int device, int fi, int fo, int zeros, double rolloff, double beta,
                          mp3g_resampler** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (fi <= 0 || fo <= 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "resampler: rate not positive");
  if (!(rolloff > 0.0 && rolloff <= 1.0) || !(beta >= 0.0 && beta <= 64.0))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "resampler: rolloff outside (0, 1] or beta outside [0, 64]");
  if (zeros < 1 || zeros > 64) return abi_fail(MP3G_ERR_UNSUPPORTED, "resampler: zeros outside 1..64");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  const int g = std::gcd(fi, fo);
  const uint64_t M = (uint64_t)(fi / g), L = (uint64_t)(fo / g);
  uint64_t W = 0;
  double c = 0.0;
  if (fi != fo) {
    c = rolloff * (L < M ? (double)L / (double)M : 1.0);
    const double w = std::ceil((double)zeros / c);
    if (!(w * 2.0 * (double)L <= (double)MP3G_RESAMPLE_MAX_TAPS))
      return abi_fail(MP3G_ERR_UNSUPPORTED, "resampler: table of more than MP3G_RESAMPLE_MAX_TAPS entries");
    W = (uint64_t)w;
  }
  mp3g_resampler* r = new (std::nothrow) mp3g_resampler;
  if (!r) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "resampler");
  r->device = device;
  r->L = (uint32_t)L;
  r->M = (uint32_t)M;
  r->W = (uint32_t)W;
  if (W) {
    try {
      r->taps.resize((size_t)(L * 2 * W));
    } catch (...) {
      delete r;
      return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "resampler table");
    }
    const double i0b = bessel_i0(beta);
    for (uint64_t ph = 0; ph < L; ph++) {
      for (uint64_t k = 0; k < 2 * W; k++) {
        const double t = (double)k - (double)(W - 1) - (double)ph / (double)L;
        const double u = t / (double)W;
        const double a = kPi * c * t;
        const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
        const double in = 1.0 - u * u;
        const double win = std::fabs(u) <= 1.0 ? bessel_i0(beta * std::sqrt(in > 0.0 ? in : 0.0)) / i0b : 0.0;
        r->taps[(size_t)(ph * 2 * W + k)] = (float)(c * sinc * win);
      }
    }
  }
  if (device >= 0) {
    const int st = resample_device_upload(r);
    if (st != MP3G_OK) {
      delete r;
      return st;
    }
  }
  *out = r;
  return MP3G_OK;
}

void mp3g_resampler_free(mp3g_resampler* r) {
  if (!r) return;
  if (r->d_taps) resample_device_free(r);
  delete r;
}

int mp3g_resampler_info(const mp3g_resampler* r, uint32_t* L, uint32_t* M, uint32_t* W, const float** taps,
                        uint32_t* tile) {
  if (!r) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null resampler");
  if (L) *L = r->L;
  if (M) *M = r->M;
  if (W) *W = r->W;
  if (taps) *taps = r->taps.empty() ? nullptr : r->taps.data();
  if (tile) *tile = resample_geometry(r->L, r->M, r->W).tile;
  return MP3G_OK;
}

int mp3g_resample_host(const mp3g_resampler* r, const float* src, uint64_t src_origin, uint64_t n_src,
                       uint64_t out_start, uint64_t n_out, float* out) {
  if (!r || (n_src && !src) || (n_out && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (n_out == 0) return MP3G_OK;
  // every index below fits a signed 64-bit integer with room to spare
  if (src_origin >= kIndexLimit || n_src >= kIndexLimit || out_start >= kIndexLimit || n_out >= kIndexLimit ||
      (out_start + n_out) / r->L >= kIndexLimit / r->M - 1)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "resample: sample index beyond 2^62");
  const int64_t lo = (int64_t)src_origin, hi = (int64_t)(src_origin + n_src);
  if (r->W == 0) {  // fi == fo: a copy
    for (uint64_t i = 0; i < n_out; i++) {
      const int64_t j = (int64_t)(out_start + i);
      out[i] = j >= lo && j < hi ? src[j - lo] : 0.f;
    }
    return MP3G_OK;
  }
  const uint32_t L = r->L, M = r->M;
  const int64_t n2w = 2 * (int64_t)r->W;
  uint64_t q;
  uint32_t ph;
  resample_divmod(out_start, M, L, &q, &ph);
  for (uint64_t i = 0; i < n_out; i++) {
    const float* h = r->taps.data() + (size_t)ph * (size_t)n2w;
    const int64_t base = (int64_t)q - (int64_t)r->W + 1;  // source index of tap 0
    const int64_t k0 = lo > base ? lo - base : 0;
    const int64_t k1 = hi - base < n2w ? hi - base : n2w;
    float acc = 0.f;
    for (int64_t k = k0; k < k1; k++) acc = std::fmaf(h[k], src[base + k - lo], acc);
    out[i] = acc;
    const uint64_t t = (uint64_t)ph + M;  // (q, ph) of the next output
    q += t / L;
    ph = (uint32_t)(t % L);
  }
  return MP3G_OK;
}

}  // extern "C"
