// truepeak_tables.cpp -- host side of the true peak, of the momentary and
// short-term maxima and the loudness range, and of the gain against a supplied
// peak (include/mp3g.h "True peak of decoded rows", "Momentary and short-term
// maxima, loudness range"): the argument checks, mp3g_true_peak_host,
// mp3g_loudness_range_host and mp3g_gain_host_peak -- the plain-C++ statements
// that the device calls (truepeak.hip) equal bit for bit.  No HIP call is made
// here.
#include <new>

#include "abi_util.h"
#include "loudness.h"
#include "loudness_range.h"
#include "truepeak.h"

using namespace mp3g;

namespace {

constexpr float kCoefs[kTpPhases][kTpTaps] = {MP3G_TRUE_PEAK_COEFS};

// the segment pass of one item, as mp3g_loudness_host runs it: H samples from zero state
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

}  // namespace

namespace mp3g {

int true_peak_check(uint32_t n_rows, uint32_t n_planes, uint32_t T, uint32_t* tiles) {
  if (n_planes != 1 && n_planes != 2) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "true peak: 1 or 2 planes");
  if (T >= (1u << 31)) return abi_fail(MP3G_ERR_UNSUPPORTED, "true peak: rows of 2^31 samples or more");
  const uint64_t blocks = (uint64_t)n_rows * n_planes * tp_tiles(T);
  if (blocks >= (1ull << 31) || (uint64_t)n_rows * n_planes >= (1ull << 31))
    return abi_fail(MP3G_ERR_UNSUPPORTED, "true peak: 2^31 tiles or more");
  if (tiles) *tiles = tp_tiles(T);
  return MP3G_OK;
}

}  // namespace mp3g

extern "C" {

int mp3g_true_peak_coefs(const float** c) {
  if (!c) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "null argument");
  *c = &kCoefs[0][0];
  return MP3G_OK;
}

uint32_t mp3g_true_peak_tile(void) { return kTpTile; }

uint64_t mp3g_true_peak_scratch_bytes(uint32_t n_rows, uint32_t n_planes, uint32_t T) {
  uint32_t tiles = 0;
  if (true_peak_check(n_rows, n_planes, T, &tiles) != MP3G_OK) return 0;
  return (uint64_t)n_rows * n_planes * tiles * sizeof(float);
}

int mp3g_true_peak_host(const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                        float* tp) {
  const int st = true_peak_check(n_rows, n_planes, T, nullptr);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!tp || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "true peak: null buffer");
  std::vector<float> buf;  // a plane behind kTpHalo zeros: x[k] = 0 for k < 0
  try {
    buf.resize((size_t)kTpHalo + T);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "true peak");
  }
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t len = lengths && lengths[r] < T ? lengths[r] : T;
    float v = 0.f;
    for (uint32_t p = 0; p < n_planes; p++) {
      const float* xp = x + ((size_t)r * n_planes + p) * T;
      for (uint32_t n = 0; n < kTpHalo; n++) buf[n] = 0.f;
      for (uint32_t n = 0; n < len; n++) buf[kTpHalo + n] = xp[n];
      for (uint32_t n = 0; n < len; n++) v = tp_sample(buf.data() + kTpHalo + n, v);
    }
    tp[r] = v;
  }
  return MP3G_OK;
}

uint64_t mp3g_loudness_range_scratch_bytes(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T) {
  if (loudness_check(ld, n_rows, n_planes, T, nullptr) != MP3G_OK) return 0;
  return (uint64_t)n_rows * loud_items_per_plane(T, ld->H) * sizeof(double);
}

int mp3g_loudness_range_host(const mp3g_loudness* ld, const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                             const uint32_t* lengths, mp3g_loudness_range* out) {
  const int st = loudness_check(ld, n_rows, n_planes, T, nullptr);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!out || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "loudness range: null buffer");
  const uint32_t H = ld->H, S1 = loud_items_per_plane(T, H);
  std::vector<double> items, S;
  std::vector<float> peaks;
  try {
    items.resize((size_t)n_planes * S1 * kLoudItemDoubles);
    peaks.assign((size_t)n_planes * S1, 0.f);  // (the sample peak is not this record's)
    S.resize(S1);
  } catch (...) {
    return abi_fail(MP3G_ERR_OUT_OF_MEMORY, "loudness range");
  }
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t len = lengths && lengths[r] < T ? lengths[r] : T;
    const uint32_t nseg = len / H, nb = nseg >= 4 ? nseg - 3 : 0, ns = range_short_count(nseg);
    for (uint32_t p = 0; p < n_planes; p++) {
      const float* xp = x + ((size_t)r * n_planes + p) * T;
      double* ip = items.data() + (size_t)p * S1 * kLoudItemDoubles;
      for (uint32_t j = 0; j < nseg; j++) segment_item(*ld, xp + (size_t)j * H, ip + (size_t)j * kLoudItemDoubles);
      loud_scan_plane(ip, nseg, ld->G, ld->AH);
    }
    mp3g_loudness_stats unused;
    loud_row_record(items.data(), peaks.data(), n_planes, S1, nseg, H, &unused);  // z_i into plane 0's second doubles
    double M = 0.0, Smax = 0.0;
    for (uint32_t i = 0; i < nb; i++) {
      const double z = items[(size_t)i * kLoudItemDoubles + 1];
      M = z > M ? z : M;
    }
    for (uint32_t k = 0; k < ns; k++) {
      S[k] = range_short_energy(items.data(), n_planes, S1, k, H);
      Smax = S[k] > Smax ? S[k] : Smax;
    }
    uint32_t n_abs = 0, n_range = 0;
    const double rel = range_rel_gate(S.data(), ns, &n_abs);
    for (uint32_t k = 0; k < ns; k++) n_range += range_gated(S[k], rel) ? 1u : 0u;
    double vlo = 0.0, vhi = 0.0;
    if (n_range) {
      vlo = range_select(S.data(), ns, rel, range_rank_lo(n_range));
      vhi = range_select(S.data(), ns, rel, range_rank_hi(n_range));
    }
    range_record(M, Smax, ns, n_range, vlo, vhi, &out[r]);
  }
  return MP3G_OK;
}

int mp3g_gain_host_peak(float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                        const mp3g_loudness_stats* stats, double target_energy, float peak_ceiling, float* gain_out,
                        const float* peak) {
  const int st = gain_check(n_rows, n_planes, T, target_energy, peak_ceiling);
  if (st != MP3G_OK) return st;
  if (n_rows == 0) return MP3G_OK;
  if (!stats || (T && !x)) return abi_fail(MP3G_ERR_INVALID_ARGUMENT, "gain: null buffer");
  for (uint32_t r = 0; r < n_rows; r++) {
    const float g = loud_gain(stats[r].energy, peak ? peak[r] : stats[r].peak, target_energy, peak_ceiling);
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
