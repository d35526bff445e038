// Coherency (model visibility) prediction — N8 of SURVEY.md §2.2.
//
// Reference: `calibration_tools.skytocoherencies[_torch|_uvw]`
// (calibration_tools.py:215-464) — a python loop over sources. The
// torch rewrite (radio/coherency.py) is ~10 kernels per source-chunk
// per cluster; these kernels do the WHOLE prediction in ONE launch: each
// thread owns one sample t and loops the cluster's sources from an
// LDS-staged table (rows and source term: sky_term.h), accumulating the
// complex double sum  Σ_s amp_s(u,v,w) · e^{i φ_s}  in registers, rounded
// once to complex64.
//
// One body, two kernels:
//   coherency_kernel       grid (T-tiles × clusters);
//   coherency_beam_kernel  every term weighted by the station beam gain
//     E[t,p,s] · conj(E[t,q,s]) of beam.hip. Grid (baseline tiles ×
//     timeslots × clusters): a block never straddles a timeslot, so its E
//     reads stay inside one [s][station] slab.

#include "sky_term.h"

// Sample t (live = inside the table) of cluster k; sources OFF[k]..OFF[k+1]
// clamped to Smax rows. BEAM = false compiles every beam statement out and
// leaves `gain`, `ts` and `b` unused.
template <bool BEAM>
__device__ __forceinline__ void coherency_body(
    const double* __restrict__ UVW,  // (T, 3) pre-scaled
    const double* __restrict__ SRC,  // (Stot, 11)
    const int* __restrict__ OFF,     // (K+1) cluster offsets into SRC
    float* __restrict__ C,           // (K, T, 4) interleaved complex64
    double fdelta, long T, int k, long t, bool live, int Smax,
    const BeamGain& gain, int ts, int b) {
  __shared__ double tab[SKY_CHUNK * SKY_ROW];
  const int s_lo = max(OFF[k], 0), s_hi = min(OFF[k + 1], Smax);

  double u = 0.0, v = 0.0, w = 0.0;
  const double* ep = nullptr;
  const double* eq = nullptr;
  if (live) {
    u = UVW[3 * t + 0];
    v = UVW[3 * t + 1];
    w = UVW[3 * t + 2];
    if constexpr (BEAM) beam_rows(gain, ts, b, ep, eq);
  }
  double acc_re = 0.0, acc_im = 0.0;
  for (int c0 = s_lo; c0 < s_hi; c0 += SKY_CHUNK) {
    const int cn = min(SKY_CHUNK, s_hi - c0);
    for (int i = threadIdx.x; i < cn * SKY_ROW; i += blockDim.x)
      tab[i] = SRC[(long)(c0) * SKY_ROW + i];
    __syncthreads();
    if (live) {
      for (int s = 0; s < cn; ++s) {
        const double* r = &tab[s * SKY_ROW];
        const double ph = u * r[0] + v * r[1] + w * r[2];
        const double amp = sky_amp(r, u, v, w, ph, fdelta);
        if constexpr (BEAM) {
          double g_re, g_im;
          beam_gain(ep, eq, (long)(c0 + s) * gain.N * 2, g_re, g_im);
          const double cr = amp * cos(ph), ci = amp * sin(ph);
          acc_re += g_re * cr - g_im * ci;
          acc_im += g_re * ci + g_im * cr;
        } else {
          acc_re += amp * cos(ph);
          acc_im += amp * sin(ph);
        }
      }
    }
    __syncthreads();
  }
  if (live) sky_store_I(&C[((long)k * T + t) * 8], acc_re, acc_im);
}

// Stot sits next to T so that both arrive in one kernel-argument load at
// the top: a load of its own, issued where the source range is clamped,
// put a serial memory round trip (1.8 µs of 50, measured) before the loop.
extern "C" __global__ __launch_bounds__(256) void coherency_kernel(
    const double* __restrict__ UVW, const double* __restrict__ SRC,
    const int* __restrict__ OFF, float* __restrict__ C, double fdelta, int T,
    int Stot, int K) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  coherency_body<false>(UVW, SRC, OFF, C, fdelta, T, blockIdx.y, t, t < T,
                        Stot, BeamGain{}, 0, 0);
}

extern "C" __global__ __launch_bounds__(256) void coherency_beam_kernel(
    const double* __restrict__ UVW,  // (Tt*B, 3)
    const double* __restrict__ SRC, const int* __restrict__ OFF,
    const double* __restrict__ E, const int* __restrict__ P,
    const int* __restrict__ Q,
    float* __restrict__ C,           // (K, Tt*B, 4)
    double fdelta, int B, int Tt, int K, int N, int Stot, int Sall) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int ts = blockIdx.y;
  // source rows index E too: keep them inside both tables
  coherency_body<true>(UVW, SRC, OFF, C, fdelta, (long)Tt * B, blockIdx.z,
                       (long)ts * B + b, b < B, min(Stot, Sall),
                       BeamGain{E, P, Q, B, N, Sall, 0}, ts, b);
}
