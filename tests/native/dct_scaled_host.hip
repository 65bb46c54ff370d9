// dct_scaled_host.hip -- TEST INFRASTRUCTURE: the fast kernel's scaled
// transforms (go-mp3_amd/csrc/dct32.h dct2_32_scaled_to, dct4_18.h
// dct4_18_pk_scaled) and their scale tables compiled for the CPU, so
// tests/test_dct_scaled.py can check them against float64 without a GPU.  Not
// linked into libmp3g.so.
#include "../../go-mp3_amd/csrc/dct32.h"
#include "../../go-mp3_amd/csrc/dct4_18.h"

using mp3g::dct32::f2;

// S[n][32] -> X[n][32] / kScale, natural m order (what the ring holds)
extern "C" void dct32_scaled_host(const float* S, float* X, int n) {
  for (int i = 0; i < n; i++) {
    f2 sp[16];
    for (int j = 0; j < 16; j++) sp[j] = (f2){S[32 * i + 2 * j], S[32 * i + 2 * j + 1]};
    mp3g::dct32::dct2_32_scaled_to(sp, [&](int t, f2 v) {
      X[32 * i + mp3g::dct32::kPairM[t][0]] = v.x;
      X[32 * i + mp3g::dct32::kPairM[t][1]] = v.y;
    });
  }
}

extern "C" void dct32_scales(float* scale, float* inv) {
  for (int m = 0; m < 32; m++) {
    scale[m] = mp3g::dct32::kScale[m];
    inv[m] = mp3g::dct32::kInvScale[m];
  }
}

// x[n][18] -> X[n][18] / kScaleX (scaled, packed) and X[n][18] (dct4_18)
extern "C" void dct4_18_scaled_host(const float* x, float* Xs, float* X, int n) {
  for (int i = 0; i < n; i++) {
    mp3g::dct4::dct4_18(x + 18 * i, X + 18 * i);
    mp3g::pk::f2 P[9];
    mp3g::dct4::dct4_18_pk_scaled(x + 18 * i, P);
    for (int k = 0; k < 9; k++) {
      Xs[18 * i + 2 * k] = P[k].x;
      Xs[18 * i + 17 - 2 * k] = P[k].y;
    }
  }
}

// scale9[k][2] (per pair: X[2k], X[17-2k]) and scalex[18] (by X index)
extern "C" void dct4_18_scales(float* scale9, float* scalex) {
  for (int k = 0; k < 9; k++) {
    scale9[2 * k] = mp3g::dct4::kScale9[k][0];
    scale9[2 * k + 1] = mp3g::dct4::kScale9[k][1];
  }
  for (int n = 0; n < 18; n++) scalex[n] = mp3g::dct4::kScaleX(n);
}
