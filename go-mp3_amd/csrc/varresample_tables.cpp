// varresample_tables.cpp -- host side of the variable-ratio resampler
// (include/mp3g.h "variable-ratio resampling of decoded rows"): the prototype
// table in float64, the object, and mp3g_varresample_host, the plain-C++
// statement of one resampled row that the device call (varresample.hip) equals
// bit for bit.  No HIP call is made here.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "abi_util.h"
#include "varresample.h"

using namespace mp3g;

namespace {

// Modified Bessel function of the first kind, order 0: the power series of
// resample_tables.cpp, term for term.
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

extern "C" {

int mp3g_varresampler_create(int device, int zeros, double rolloff, double beta, int precision,
                             mp3g_varresampler** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (!(rolloff > 0.0 && rolloff <= 1.0) || !(beta >= 0.0 && beta <= 64.0))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresampler: rolloff outside (0, 1] or beta outside [0, 64]");
  if (zeros < 1 || zeros > 64) return abi_fail(MP3G_ERR_UNSUPPORTED, "varresampler: zeros outside 1..64");
  if (precision < 5 || precision > 9) return abi_fail(MP3G_ERR_UNSUPPORTED, "varresampler: precision outside 5..9");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  const uint32_t P = (uint32_t)precision, Z = (uint32_t)zeros << P;
  const uint32_t R = (uint32_t)std::floor(rolloff * (double)(1u << P));
  if (R == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresampler: rolloff below 2^-precision");
  mp3g_varresampler* r = new (std::nothrow) mp3g_varresampler;
  if (!r) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "varresampler");
  r->device = device;
  r->zeros = (uint32_t)zeros;
  r->P = P;
  r->Z = Z;
  r->R = R;
  try {
    r->table.assign(2 * ((size_t)Z + 1), 0.f);
  } catch (...) {
    delete r;
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "varresampler table");
  }
  // f(v) = sinc(v) kaiser(v / zeros) at v = i / 2^P, i = 0..Z (f(zeros) = 0:
  // the table's last entry is written as the zero it stands for)
  const double i0b = bessel_i0(beta), scale = (double)(1u << P);
  auto f = [&](uint32_t i) {
    if (i >= Z) return 0.0;
    const double v = (double)i / scale, u = v / (double)zeros, a = kPi * v;
    const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
    const double in = 1.0 - u * u;
    return sinc * (bessel_i0(beta * std::sqrt(in > 0.0 ? in : 0.0)) / i0b);
  };
  double cur = f(0);
  for (uint32_t i = 0; i < Z; i++) {
    const double nxt = f(i + 1);
    r->table[2 * (size_t)i] = (float)cur;
    r->table[2 * (size_t)i + 1] = (float)(nxt - cur);
    cur = nxt;
  }
  // the table in LDS when it fits: the faster of the two on every leg measured
  // (MP3G_VARRESAMPLE_TABLE=l2 keeps it in global memory, for
  // that A/B)
  const char* where = std::getenv("MP3G_VARRESAMPLE_TABLE");
  r->table_lds = Z <= kVarTableLdsPairs && !(where && std::strcmp(where, "l2") == 0);
  if (device >= 0) {
    const int st = varresample_device_upload(r);
    if (st != MP3G_OK) {
      delete r;
      return st;
    }
  }
  *out = r;
  return MP3G_OK;
}

void mp3g_varresampler_free(mp3g_varresampler* r) {
  if (!r) return;
  if (r->d_table) varresample_device_free(r);
  delete r;
}

int mp3g_varresampler_info(const mp3g_varresampler* r, uint32_t* precision, uint32_t* Z, uint32_t* R,
                           const float** table, uint32_t* tile, uint32_t* stage) {
  if (!r) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null varresampler");
  if (precision) *precision = r->P;
  if (Z) *Z = r->Z;
  if (R) *R = r->R;
  if (table) *table = r->table.data();
  if (tile) *tile = kVarTile;
  if (stage) *stage = kVarStageFloats;
  return MP3G_OK;
}

int mp3g_varresample_host(const mp3g_varresampler* r, const float* src, uint64_t src_origin, uint64_t n_src,
                          uint64_t out_start, uint64_t n_out, float* out, uint32_t num, uint32_t den, float gain) {
  if (!r || (n_src && !src) || (n_out && !out)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  if (num == 0 || den == 0 || num >= (1u << 31) || den >= (1u << 31))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: num and den in [1, 2^31)");
  const uint32_t I = var_step(r->R, num, den);
  if (I == 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: ratio beyond the table's resolution");
  if (n_out == 0) return MP3G_OK;
  // every index below fits a signed 64-bit integer with room to spare
  if (src_origin >= kIndexLimit || n_src >= kIndexLimit || out_start >= kIndexLimit || n_out >= kIndexLimit ||
      (out_start + n_out) / den >= kIndexLimit / num - 1)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "varresample: sample index beyond 2^62");
  if (num == den) {  // a copy times gain
    for (uint64_t i = 0; i < n_out; i++) {
      const uint64_t p = out_start + i - src_origin;  // (wraps below the origin: >= n_src)
      out[i] = (p < n_src ? src[p] : 0.f) * gain;
    }
    return MP3G_OK;
  }
  const float c = var_cutoff(I, r->P);
  const float* tab = r->table.data();
  for (uint64_t i = 0; i < n_out; i++) {
    uint64_t q;
    uint32_t rr;
    var_divmod(out_start + i, num, den, &q, &rr);
    const VarTaps t = var_taps(q, rr, den, I, r->Z);
    float acc;
    var_chain<1>(tab, t, I, var_rel(q, src_origin), (int64_t)n_src, [&](int, int64_t p) { return src[p]; }, &acc);
    out[i] = var_scale(c, acc, gain);
  }
  return MP3G_OK;
}

}  // extern "C"
