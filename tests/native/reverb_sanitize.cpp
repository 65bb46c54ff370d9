// reverb_sanitize.cpp -- the reverberation's and the noise mixing's host code
// under ASan + UBSan (go-mp3_amd/csrc/Makefile target asan-reverb; run by
// tests/test_reverb_cpu.py).  Host buffers of exactly the sizes the contract
// names: host-only objects over the edges of the tap count, mp3g_row_power_host
// and mp3g_augment_host over every length, partition and slot edge, and the
// argument refusals of the host and the device calls.  No device call is made.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mp3g.h"

// (the library's error-text sink lives in mp3g_abi.cpp, which is not linked)
namespace mp3g {
int abi_fail(int status, const char*) { return status; }
}  // namespace mp3g

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

static uint32_t g_seed = 2468;
static float rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) / 8388608.0f - 1.0f;
}

int main() {
  const int inv = MP3G_ERR_INVALID_ARGUMENT;
  // ---- a bank whose rows are exactly as long as their responses' stride
  const uint32_t stride = 2500, taps[6] = {1, 2, 1023, 1024, 1025, 2500};
  std::vector<float> bank((size_t)6 * stride);
  for (float& v : bank) v = 0.1f * rnd();
  bank[0 * stride] = 1.0f;          // peak at 0
  bank[2 * stride + 1022] = 1.0f;   // at L - 1
  bank[4 * stride + 512] = 1.0f;    // in the middle
  bank[5 * stride + 2499] = 1.0f;   // the last tap of the last row
  for (int rate : {8000, 16000, 44100}) {
    mp3g_reverb* rv = nullptr;
    CHECK(mp3g_reverb_create(-1, rate, bank.data(), 6, stride, taps, &rv) == MP3G_OK && rv);
    if (!rv) continue;
    uint32_t n_rirs = 0, lmax = 0;
    const uint32_t* table = nullptr;
    uint64_t n_spectra = 0;
    CHECK(mp3g_reverb_info(rv, &n_rirs, &lmax, &table, nullptr, nullptr, &n_spectra) == MP3G_OK);
    CHECK(n_rirs == 6 && lmax == 2500 && n_spectra == (uint64_t)(1 + 1 + 1 + 1 + 2 + 3) * 2048);
    CHECK(table[8 * 5 + 1] == 2499 && table[8 * 5 + 3] == 2500);
    // noise bank: rows of exactly Tn, one silent, one of a single sample
    const uint32_t M = 3, Tn = 700, nlen[M] = {700, 1, 300};
    std::vector<float> noise((size_t)M * Tn);
    for (float& v : noise) v = rnd();
    for (uint32_t j = 0; j < 300; j++) noise[2 * Tn + j] = 0.f;
    double pn[M];
    CHECK(mp3g_row_power_host(noise.data(), M, Tn, nlen, pn) == MP3G_OK);
    CHECK(pn[0] > 0 && pn[1] > 0 && pn[2] == 0.0);
    for (uint32_t T : {1u, 2u, 1023u, 1024u, 1025u, 3100u}) {
      const uint32_t rows = 7, A = 3;
      const uint32_t lengths[rows] = {0, 1, T / 2, T - 1, T, T + 9, 0xffffffffu};
      const int32_t rir[rows] = {0, 1, 2, 3, 4, 5, -1};
      for (uint32_t planes : {1u, 2u}) {
        std::vector<float> x((size_t)rows * planes * T), y(x.size(), -1.0f);
        for (float& v : x) v = rnd();
        std::vector<double> stats((size_t)rows * planes * 4, -1.0);
        std::vector<mp3g_augment_slot> slots((size_t)rows * A);
        for (uint32_t r = 0; r < rows; r++) {
          slots[r * A + 0] = {0, r % 2 ? T / 3 : 0u, 699, 1, 0.1};        // wraps from the last sample
          slots[r * A + 1] = {(int32_t)(r % 3) - 1, T + 5, 0, 0, 1.0};    // starts past the row, or none
          slots[r * A + 2] = {2 - (int32_t)(r % 2), 0, 0, r % 2, 0.5};    // silent, or one sample
        }
        for (uint32_t flags : {0u, MP3G_AUGMENT_NORMALIZE}) {
          mp3g_augment_args a = {};
          a.x = x.data();
          a.out = y.data();
          a.lengths = lengths;
          a.rir_index = rir;
          a.noise = noise.data();
          a.noise_lengths = nlen;
          a.noise_power = pn;
          a.slots = slots.data();
          a.stats = stats.data();
          a.n_rows = rows;
          a.n_planes = planes;
          a.T = T;
          a.n_noise = M;
          a.Tn = Tn;
          a.A = A;
          a.flags = flags;
          CHECK(mp3g_augment_host(rv, &a) == MP3G_OK);
          for (uint32_t r = 0; r < rows; r++) {
            const uint32_t n = lengths[r] < T ? lengths[r] : T;
            for (uint32_t p = 0; p < planes; p++) {
              const float* o = y.data() + ((size_t)r * planes + p) * T;
              for (uint32_t j = 0; j < T; j++) CHECK(j < n ? std::isfinite(o[j]) : (o[j] == 0.f && !std::signbit(o[j])));
              const double* s = stats.data() + ((size_t)r * planes + p) * 4;
              CHECK(s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[3] > 0);
              if (!flags || n == 0) CHECK(s[3] == 1.0);
            }
          }
        }
      }
    }
    // ---- refusals with an object (host, then the device call: before any device call)
    {
      std::vector<float> x(16), y(16);
      double st[8];
      uint32_t n[2] = {8, 8};
      int32_t ri[2] = {0, 6};
      mp3g_augment_slot sl[2] = {{0, 0, 700, 0, 1.0}, {-1, 0, 0, 0, 1.0}};
      mp3g_augment_args a = {};
      a.x = x.data();
      a.out = y.data();
      a.lengths = n;
      a.stats = st;
      a.n_rows = 2;
      a.n_planes = 1;
      a.T = 8;
      a.rir_index = ri;
      CHECK(mp3g_augment_host(rv, &a) == inv);  // rir_index past the bank
      ri[1] = 5;
      CHECK(mp3g_augment_host(rv, &a) == MP3G_OK);
      CHECK(mp3g_augment_host(nullptr, &a) == inv);  // a response without an object
      a.rir_index = nullptr;
      CHECK(mp3g_augment_host(nullptr, &a) == MP3G_OK);
      a.noise = noise.data();
      a.noise_lengths = nlen;
      a.noise_power = pn;
      a.n_noise = M;
      a.Tn = Tn;
      a.slots = sl;
      a.A = 1;
      CHECK(mp3g_augment_host(rv, &a) == inv);  // offset == the noise's length
      sl[0].offset = 699;
      CHECK(mp3g_augment_host(rv, &a) == MP3G_OK);
      sl[0].noise_index = 1;
      sl[0].offset = 1;
      CHECK(mp3g_augment_host(rv, &a) == inv);  // offset past a noise of one sample
      sl[0].noise_index = 3;
      sl[0].offset = 0;
      CHECK(mp3g_augment_host(rv, &a) == inv);  // noise_index past the bank
      sl[0].noise_index = 0;
      a.A = 9;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      CHECK(mp3g_augment_rows(rv, 0, &a, nullptr, nlen, sl, st, 1 << 20, nullptr) == inv);
      a.A = 1;
      a.flags = 2;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      a.flags = 1;
      a.n_planes = 3;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      a.n_planes = 1;
      a.out = x.data();
      CHECK(mp3g_augment_host(rv, &a) == inv);  // in place
      CHECK(mp3g_augment_rows(rv, 0, &a, nullptr, nlen, sl, st, 1 << 20, nullptr) == inv);
      a.out = x.data() + 4;
      CHECK(mp3g_augment_host(rv, &a) == inv);  // overlapping
      a.out = nullptr;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      a.out = y.data();
      a.stats = nullptr;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      a.stats = st;
      a.slots = nullptr;
      CHECK(mp3g_augment_host(rv, &a) == inv);
      a.slots = sl;
      CHECK(mp3g_augment_rows(rv, -1, &a, nullptr, nlen, sl, st, 1 << 20, nullptr) == inv);  // (a host-only object)
      a.n_rows = 0;
      CHECK(mp3g_augment_host(rv, &a) == MP3G_OK);
      CHECK(mp3g_augment_host(rv, nullptr) == inv);
      CHECK(mp3g_reverb_scratch_bytes(rv, 2, 1, 8) == (2 * 1 * 2 + 2 * 3) * 8 + 2 * 2 * 2048 * 8);
      CHECK(mp3g_reverb_scratch_bytes(nullptr, 2, 2, 1025) == 2 * 2 * 2 * 2 * 8);
      CHECK(mp3g_reverb_scratch_bytes(rv, 2, 3, 8) == 0 && mp3g_reverb_scratch_bytes(rv, 0, 1, 8) == 0);
    }
    mp3g_reverb_free(rv);
  }
  // ---- the object's refusals
  {
    mp3g_reverb* rv = reinterpret_cast<mp3g_reverb*>(1);
    std::vector<float> h(65537, 0.5f);
    uint32_t L = 65536;
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 65537, &L, &rv) == MP3G_OK && rv);
    mp3g_reverb_free(rv);
    L = 65537;
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 65537, &L, &rv) == inv && !rv);
    L = 0;
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 65537, &L, &rv) == inv);
    L = 9;
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 8, &L, &rv) == inv);
    CHECK(mp3g_reverb_create(-1, 0, h.data(), 1, 9, &L, &rv) == inv);
    CHECK(mp3g_reverb_create(-1, 400000, h.data(), 1, 9, &L, &rv) == MP3G_ERR_UNSUPPORTED);
    for (int low : {1, 10, 19}) CHECK(mp3g_reverb_create(-1, low, h.data(), 1, 9, &L, &rv) == MP3G_ERR_UNSUPPORTED && !rv);
    CHECK(mp3g_reverb_create(-1, 20, h.data(), 1, 9, &L, &rv) == MP3G_OK && rv);
    {  // the lowest rate: the early window is the peak alone, a row of one sample and one past a block
      const uint32_t* table = nullptr;
      CHECK(mp3g_reverb_info(rv, nullptr, nullptr, &table, nullptr, nullptr, nullptr) == MP3G_OK);
      CHECK(table[1] == 0 && table[2] == 0 && table[3] == 1);
      std::vector<float> x(2 * 1025, 0.25f), y(2 * 1025, -1.0f);
      const uint32_t n[2] = {1, 1025};
      const int32_t ri[2] = {0, 0};
      double st[8];
      mp3g_augment_args a = {};
      a.x = x.data();
      a.out = y.data();
      a.lengths = n;
      a.rir_index = ri;
      a.stats = st;
      a.n_rows = 2;
      a.n_planes = 1;
      a.T = 1025;
      CHECK(mp3g_augment_host(rv, &a) == MP3G_OK);
      for (float v : y) CHECK(v >= 0.f && v < 10.f);  // every word written
    }
    mp3g_reverb_free(rv);
    rv = nullptr;
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 0, 9, &L, &rv) == inv);
    CHECK(mp3g_reverb_create(-1, 16000, nullptr, 1, 9, &L, &rv) == inv);
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 9, nullptr, &rv) == inv);
    CHECK(mp3g_reverb_create(-1, 16000, h.data(), 1, 9, &L, nullptr) == inv);
    CHECK(mp3g_reverb_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == inv);
    mp3g_reverb_free(nullptr);
    double p[2];
    CHECK(mp3g_row_power_host(nullptr, 2, 4, nullptr, p) == inv);
    CHECK(mp3g_row_power_host(h.data(), 2, 4, nullptr, nullptr) == inv);
    CHECK(mp3g_row_power_host(nullptr, 0, 4, nullptr, nullptr) == MP3G_OK);
    CHECK(mp3g_row_power_host(nullptr, 2, 0, nullptr, p) == MP3G_OK && p[0] == 0.0 && p[1] == 0.0);
    CHECK(mp3g_row_power_host(h.data(), 2, 1025, nullptr, p) == MP3G_OK && p[0] == 0.25 && p[1] == 0.25);
    CHECK(mp3g_row_power_rows(-1, h.data(), 2, 4, nullptr, p, p, nullptr) == inv);
    CHECK(mp3g_row_power_scratch_bytes(3, 1025) == 3 * 2 * 8);
  }
  if (g_failed) {
    std::fprintf(stderr, "reverb_sanitize: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("reverb_sanitize ok\n");
  return 0;
}
