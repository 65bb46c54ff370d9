// loudness_tables.cpp -- host side of the BS.1770 loudness measure and the gain
// stage (include/mp3g.h "Integrated loudness of decoded rows"): the K-weighting
// designed in float64 from its analog prototypes, the segment tables made by the
// shared filter code itself, the object, mp3g_loudness_host and mp3g_gain_host
// -- the plain-C++ statements that the device calls (loudness.hip) equal bit for
// bit.  No HIP call is made here.
#include <cmath>
#include <new>

#include "abi_util.h"
#include "loudness.h"

using namespace mp3g;

namespace {

constexpr double kPi = 3.14159265358979323846;

// the segment pass of one item: H samples from zero state
void segment_item(const mp3g_loudness& ld, const float* x, double* it) {
  double s[4] = {0.0, 0.0, 0.0, 0.0}, ezs = 0.0, g[4] = {0.0, 0.0, 0.0, 0.0};
  const double* V = ld.V.data();
  for (uint32_t n = 0; n < ld.H; n++) {
    const double w = loud_step(ld.coef, s, (double)x[n]);
    ezs += w * w;
    for (uint32_t k = 0; k < 4; k++) g[k] += V[4 * (size_t)n + k] * w;
  }
  it[0] = ezs;
  for (uint32_t k = 0; k < 4; k++) {
    it[1 + k] = g[k];
    it[5 + k] = s[k];
  }
}

float peak_of(const float* x, uint32_t n) {
  float peak = 0.f;
  for (uint32_t i = 0; i < n; i++) {
    const float a = __builtin_fabsf(x[i]);
    peak = a > peak ? a : peak;
  }
  return peak;
}

}  // namespace

namespace mp3g {

int loudness_check(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T, uint64_t* n_items) {
  if (!ld) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null loudness");
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: 1 or 2 planes");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "loudness: rows of 2^31 samples or more");
  const uint64_t items = (uint64_t)n_rows * n_planes * loud_items_per_plane(T, ld->H);
  if (items >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "loudness: 2^31 segments or more");
  if (n_items) *n_items = items;
  return MP3G_OK;
}

int gain_check(uint32_t n_rows, uint32_t n_planes, uint32_t T, double target_energy, float peak_ceiling) {
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: 1 or 2 planes");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "gain: rows of 2^31 samples or more");
  if (!std::isfinite(target_energy) || !(target_energy > 0.0))
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: target energy not positive and finite");
  if (!std::isfinite(peak_ceiling) || peak_ceiling < 0.f)
    return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: peak ceiling negative or not finite");
  if ((uint64_t)n_rows * n_planes >= (1ull << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "gain: 2^31 planes or more");
  return MP3G_OK;
}

}  // namespace mp3g

extern "C" {

int mp3g_loudness_create(int device, int rate, mp3g_loudness** out) {
  if (!out) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (rate <= 0) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: rate not positive");
  if (rate < kLoudMinRate || rate > kLoudMaxRate)
    return abi_fail(MP3G_ERR_UNSUPPORTED, "loudness: rate outside 8000..192000");
  if (device < -1) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "device index");
  mp3g_loudness* ld = new (std::nothrow) mp3g_loudness;
  if (!ld) return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "loudness");
  ld->device = device;
  ld->rate = rate;
  ld->H = (uint32_t)((rate + 5) / 10);
  // the shelf and the high-pass from their analog prototypes (the parameters
  // that reproduce the standard's 48 kHz table)
  {
    const double f0 = 1681.974450955533, GdB = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(kPi * f0 / (double)rate), Vh = std::pow(10.0, GdB / 20.0);
    const double Vb = std::pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
    ld->shelf[0] = (Vh + Vb * K / Q + K * K) / a0;
    ld->shelf[1] = 2.0 * (K * K - Vh) / a0;
    ld->shelf[2] = (Vh - Vb * K / Q + K * K) / a0;
    ld->shelf[3] = 2.0 * (K * K - 1.0) / a0;
    ld->shelf[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(kPi * f0 / (double)rate), a0 = 1.0 + K / Q + K * K;
    ld->highpass[0] = 1.0;
    ld->highpass[1] = -2.0;
    ld->highpass[2] = 1.0;
    ld->highpass[3] = 2.0 * (K * K - 1.0) / a0;
    ld->highpass[4] = (1.0 - K / Q + K * K) / a0;
  }
  ld->coef = {ld->shelf[0], ld->shelf[1], ld->shelf[2], ld->shelf[3], ld->shelf[4], ld->highpass[3], ld->highpass[4]};
  const uint32_t H = ld->H;
  try {
    ld->V.assign((size_t)H * 4, 0.0);
  } catch (...) {
    mp3g_loudness_free(ld);
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "loudness tables");
  }
  // the zero-input response of each unit state, by the shared filter code
  for (uint32_t k = 0; k < 4; k++) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[k] = 1.0;
    for (uint32_t n = 0; n < H; n++) ld->V[4 * (size_t)n + k] = loud_step(ld->coef, s, 0.0);
    for (uint32_t m = 0; m < 4; m++) ld->AH[4 * m + k] = s[m];
  }
  for (uint32_t a = 0; a < 4; a++)
    for (uint32_t b = 0; b < 4; b++) {
      double sum = 0.0;
      for (uint32_t n = 0; n < H; n++) sum += ld->V[4 * (size_t)n + a] * ld->V[4 * (size_t)n + b];
      ld->G[4 * a + b] = sum;
    }
  if (device >= 0) {
    const int up = loudness_device_upload(ld);
    if (up != MP3G_OK) {
      mp3g_loudness_free(ld);
      return up;
    }
  }
  *out = ld;
  return MP3G_OK;
}

void mp3g_loudness_free(mp3g_loudness* ld) {
  if (!ld) return;
  if (ld->d_tab) loudness_device_free(ld);
  delete ld;
}

int mp3g_loudness_info(const mp3g_loudness* ld, uint32_t* H, const double** shelf, const double** highpass,
                       const double** V, const double** AH, const double** G) {
  if (!ld) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null loudness");
  if (H) *H = ld->H;
  if (shelf) *shelf = ld->shelf;
  if (highpass) *highpass = ld->highpass;
  if (V) *V = ld->V.data();
  if (AH) *AH = ld->AH;
  if (G) *G = ld->G;
  return MP3G_OK;
}

uint64_t mp3g_loudness_blocks(const mp3g_loudness* ld, uint64_t n_samples) {
  if (!ld) return 0;
  const uint64_t nseg = n_samples / ld->H;
  return nseg >= 4 ? nseg - 3 : 0;
}

uint64_t mp3g_loudness_scratch_bytes(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T) {
  uint64_t items = 0;
  if (loudness_check(ld, n_rows, n_planes, T, &items) != MP3G_OK) return 0;
  return items * (kLoudItemDoubles * sizeof(double) + sizeof(float));
}

double mp3g_loudness_target_energy(double lufs) { return std::pow(10.0, (lufs + 0.691) / 10.0); }

int mp3g_loudness_host(const mp3g_loudness* ld, const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                       const uint32_t* lengths, mp3g_loudness_stats* stats) {
  uint64_t n_items = 0;
  const int st = loudness_check(ld, n_rows, n_planes, T, &n_items);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!stats || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness: null buffer");
  const uint32_t H = ld->H, S1 = loud_items_per_plane(T, H);
  std::vector<double> items;
  std::vector<float> peaks;
  try {
    items.resize((size_t)n_planes * S1 * kLoudItemDoubles);
    peaks.resize((size_t)n_planes * S1);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "loudness segments");
  }
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t len = lengths && lengths[r] < T ? lengths[r] : T;
    const uint32_t nseg = len / H;
    for (uint32_t p = 0; p < n_planes; p++) {
      const float* xp = x + ((size_t)r * n_planes + p) * T;
      double* ip = items.data() + (size_t)p * S1 * kLoudItemDoubles;
      for (uint32_t j = 0; j < nseg; j++) {
        segment_item(*ld, xp + (size_t)j * H, ip + (size_t)j * kLoudItemDoubles);
        peaks[(size_t)p * S1 + j] = peak_of(xp + (size_t)j * H, H);
      }
      peaks[(size_t)p * S1 + nseg] = peak_of(xp + (size_t)nseg * H, len - nseg * H);
      loud_scan_plane(ip, nseg, ld->G, ld->AH);
    }
    loud_row_record(items.data(), peaks.data(), n_planes, S1, nseg, H, &stats[r]);
  }
  return MP3G_OK;
}

int mp3g_gain_host(float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                   const mp3g_loudness_stats* stats, double target_energy, float peak_ceiling, float* gain_out) {
  const int st = gain_check(n_rows, n_planes, T, target_energy, peak_ceiling);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!stats || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: null buffer");
  for (uint32_t r = 0; r < n_rows; r++) {
    const float g = loud_gain(stats[r].energy, stats[r].peak, target_energy, peak_ceiling);
    if (gain_out) gain_out[r] = g;
    if (!(stats[r].energy > 0.0)) continue;
    const uint32_t len = lengths && lengths[r] < T ? lengths[r] : T;
    for (uint32_t p = 0; p < n_planes; p++) {
      float* xp = x + ((size_t)r * n_planes + p) * T;
      for (uint32_t n = 0; n < len; n++) xp[n] = xp[n] * g;
    }
  }
  return MP3G_OK;
}

}  // extern "C"
