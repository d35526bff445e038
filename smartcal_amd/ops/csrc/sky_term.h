// The source term of sky prediction, shared by coherency.hip and
// shapelet.hip: every formula below exists once.
//
// Per-source table row (SKY_ROW = 11 doubles, precomputed host-side):
//   [l, m, n,  flux,  gflag,  gu1, gv1, gw1,  gu2, gv2, gw2]
// φ = u·l + v·m + w·n (uvw pre-scaled by 2π f / c);
// smearing: amp *= |sinc(φ · fdelta/2 / π)| (fdelta = bw/f, 0 = off);
// Gaussian: amp *= π/2 · exp(−(uut² + vvt²)) with uut = gu1·u+gv1·v+gw1·w,
// vvt = gu2·u+gv2·v+gw2·w (the projected-envelope rotation is linear in
// uvw, so it collapses to 6 coefficients per source).
//
// Station beam (beam.hip builds E): source s of timeslot ts on baseline
// b = (P[b], Q[b]) is weighted by E[ts, sbase+s, p] · conj(E[ts, sbase+s, q]).
#pragma once

#include "common.h"

#define SKY_ROW 11
#define SKY_CHUNK 128   // sources staged per LDS pass (128*11*8 = 11 KB)

// |sinc(x/pi)| in the numpy convention = |sin(x)/x|, x = φ · fdelta/2
__device__ __forceinline__ double sky_smear(double ph, double fdelta) {
  const double x = ph * (0.5 * fdelta);
  return (fabs(x) < 1e-12) ? 1.0 : fabs(sin(x) / x);
}

// flux × smearing × Gaussian envelope of table row r at (u, v, w)
__device__ __forceinline__ double sky_amp(const double* r, double u, double v,
                                          double w, double ph,
                                          double fdelta) {
  double amp = r[3];
  if (fdelta > 0.0) amp *= sky_smear(ph, fdelta);
  if (r[4] != 0.0) {
    const double uut = r[5] * u + r[6] * v + r[7] * w;
    const double vvt = r[8] * u + r[9] * v + r[10] * w;
    amp *= 0.5 * M_PI * exp(-(uut * uut + vvt * vvt));
  }
  return amp;
}

struct BeamGain {
  const double* E;     // (Tt, Sall, N) interleaved complex128
  const int* P;        // (B) station p of baseline b
  const int* Q;        // (B) station q of baseline b
  int B, N, Sall, sbase;
};

// ep, eq → E[ts, sbase, p], E[ts, sbase, q] of baseline b
__device__ __forceinline__ void beam_rows(const BeamGain& g, int ts, int b,
                                          const double*& ep,
                                          const double*& eq) {
  const double* et = &g.E[((long)ts * g.Sall + g.sbase) * g.N * 2];
  ep = &et[2 * min(max(g.P[b], 0), g.N - 1)];
  eq = &et[2 * min(max(g.Q[b], 0), g.N - 1)];
}

// gain = E_p · conj(E_q) of the source at offset o = s · N · 2
__device__ __forceinline__ void beam_gain(const double* ep, const double* eq,
                                          long o, double& g_re,
                                          double& g_im) {
  const double pr = ep[o], pi = ep[o + 1];
  const double qr = eq[o], qi = eq[o + 1];
  g_re = pr * qr + pi * qi;
  g_im = pi * qr - pr * qi;
}

// Stokes-I coherency: XX = YY = (re, im), XY = YX = 0 — 4 complex64
__device__ __forceinline__ void sky_store_I(float* o, double re, double im) {
  o[0] = (float)re;               // XX
  o[1] = (float)im;
  o[2] = 0.f;                     // XY
  o[3] = 0.f;
  o[4] = 0.f;                     // YX
  o[5] = 0.f;
  o[6] = (float)re;               // YY
  o[7] = (float)im;
}
