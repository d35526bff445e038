// Station array-factor beam for coherency prediction.
//
// Station p beam-forms Ne elements at offsets (u_e, v_e, w_e) from its
// centre (uvw frame of timeslot t, meters), steered at the phase centre:
//   E[t, p, s] = (1/Ne) · Σ_e exp(+i · scale · (u_e·l_s + v_e·m_s + w_e·n_s))
// with scale = 2πf/c and n_s the (n − 1) of the source tables. The
// beam-weighted coherency of baseline b = (p, q) at timeslot t is
//   C_k[t·B + b] = Σ_s E[t,p,s] · conj(E[t,q,s]) · amp_s · e^{iφ_s}
// with amp_s·e^{iφ_s} exactly the term of coherency.hip.
//
// Two kernels, one launch each for the whole sky:
//
// station_beam_kernel builds E for every source of every cluster (point /
// Gaussian rows first, shapelet centres after them). Grid (source tiles ×
// stations × timeslots); the block stages the element coordinates of its
// (t, station) in LDS, pre-scaled, and every thread owns one source and
// loops the elements with f64 sincos — all lanes read the same LDS word
// (broadcast). E is stored [t][s][station] so that the consumer's lanes,
// which run over consecutive q at (nearly) uniform p, read consecutive
// 16-byte entries.
//
// coherency_beam_kernel is the twin of coherency_kernel: same 11-double
// source table staged in LDS by chunks of 128, same smearing and Gaussian
// envelope, f64 accumulation rounded once to complex64. Grid (baseline
// tiles × timeslots × clusters): a block never straddles a timeslot, so
// its E reads stay inside one [s][station] slab.

#include "common.h"

#define BEAM_THREADS 128
#define BEAM_ECHUNK 256   // elements staged per LDS pass (256*3*8 = 6 KB)
#define COH_CHUNK 128     // sources staged per LDS pass (as coherency.hip)

extern "C" __global__ __launch_bounds__(BEAM_THREADS) void station_beam_kernel(
    const double* __restrict__ ELEM,  // (Tt, N, Ne, 3) meters
    const double* __restrict__ LMN,   // (Sall, 3)
    double* __restrict__ E,           // (Tt, Sall, N) interleaved complex128
    double scale, int Tt, int N, int Ne, int Sall) {
  __shared__ double el[BEAM_ECHUNK * 3];
  const int s = blockIdx.x * BEAM_THREADS + threadIdx.x;
  const int p = blockIdx.y;
  const int t = blockIdx.z;
  const double* src = &ELEM[((long)t * N + p) * Ne * 3];

  double l = 0.0, m = 0.0, n = 0.0;
  if (s < Sall) {
    l = LMN[3 * (long)s + 0];
    m = LMN[3 * (long)s + 1];
    n = LMN[3 * (long)s + 2];
  }
  double acc_re = 0.0, acc_im = 0.0;
  for (int e0 = 0; e0 < Ne; e0 += BEAM_ECHUNK) {
    const int en = min(BEAM_ECHUNK, Ne - e0);
    for (int i = threadIdx.x; i < en * 3; i += BEAM_THREADS)
      el[i] = scale * src[(long)e0 * 3 + i];
    __syncthreads();
    if (s < Sall) {
      for (int e = 0; e < en; ++e) {
        const double ph = el[3 * e] * l + el[3 * e + 1] * m + el[3 * e + 2] * n;
        double sn, cs;
        sincos(ph, &sn, &cs);
        acc_re += cs;
        acc_im += sn;
      }
    }
    __syncthreads();
  }
  if (s < Sall) {
    const double inv = 1.0 / (double)Ne;
    const long o = (((long)t * Sall + s) * N + p) * 2;
    E[o + 0] = acc_re * inv;
    E[o + 1] = acc_im * inv;
  }
}

extern "C" __global__ __launch_bounds__(256) void coherency_beam_kernel(
    const double* __restrict__ UVW,  // (Tt*B, 3) pre-scaled
    const double* __restrict__ SRC,  // (Stot, 11)
    const int* __restrict__ OFF,     // (K+1) cluster offsets into SRC
    const double* __restrict__ E,    // (Tt, Sall, N) interleaved complex128
    const int* __restrict__ P,       // (B) station p of baseline b
    const int* __restrict__ Q,       // (B) station q of baseline b
    float* __restrict__ C,           // (K, Tt*B, 4) interleaved complex64
    double fdelta, int B, int Tt, int K, int N, int Stot, int Sall) {
  __shared__ double tab[COH_CHUNK * 11];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int ts = blockIdx.y;
  const int k = blockIdx.z;
  // source rows index E too: keep them inside both tables
  const int s_lo = max(OFF[k], 0), s_hi = min(OFF[k + 1], min(Stot, Sall));
  const bool live = b < B;
  const long t = (long)ts * B + b;

  double u = 0.0, v = 0.0, w = 0.0;
  int p = 0, q = 0;
  if (live) {
    u = UVW[3 * t + 0];
    v = UVW[3 * t + 1];
    w = UVW[3 * t + 2];
    p = min(max(P[b], 0), N - 1);
    q = min(max(Q[b], 0), N - 1);
  }
  const double* Et = &E[(long)ts * Sall * N * 2];
  double acc_re = 0.0, acc_im = 0.0;
  for (int c0 = s_lo; c0 < s_hi; c0 += COH_CHUNK) {
    const int cn = min(COH_CHUNK, s_hi - c0);
    for (int i = threadIdx.x; i < cn * 11; i += blockDim.x)
      tab[i] = SRC[(long)(c0) * 11 + i];
    __syncthreads();
    if (live) {
      for (int s = 0; s < cn; ++s) {
        const double* r = &tab[s * 11];
        const double ph = u * r[0] + v * r[1] + w * r[2];
        double amp = r[3];
        if (fdelta > 0.0) {
          const double x = ph * (0.5 * fdelta);
          // |sinc(x/pi)| in the numpy convention = |sin(x)/x|
          amp *= (fabs(x) < 1e-12) ? 1.0 : fabs(sin(x) / x);
        }
        if (r[4] != 0.0) {
          const double uut = r[5] * u + r[6] * v + r[7] * w;
          const double vvt = r[8] * u + r[9] * v + r[10] * w;
          amp *= 0.5 * M_PI * exp(-(uut * uut + vvt * vvt));
        }
        // gain = E_p · conj(E_q)
        const double* es = &Et[(long)(c0 + s) * N * 2];
        const double pr = es[2 * p], pi = es[2 * p + 1];
        const double qr = es[2 * q], qi = es[2 * q + 1];
        const double g_re = pr * qr + pi * qi;
        const double g_im = pi * qr - pr * qi;
        const double cr = amp * cos(ph), ci = amp * sin(ph);
        acc_re += g_re * cr - g_im * ci;
        acc_im += g_re * ci + g_im * cr;
      }
    }
    __syncthreads();
  }
  if (live) {
    const long o = ((long)k * Tt * B + t) * 8;   // 4 complex = 8 floats
    C[o + 0] = (float)acc_re;               // XX
    C[o + 1] = (float)acc_im;
    C[o + 2] = 0.f;                         // XY
    C[o + 3] = 0.f;
    C[o + 4] = 0.f;                         // YX
    C[o + 5] = 0.f;
    C[o + 6] = (float)acc_re;               // YY
    C[o + 7] = (float)acc_im;
  }
}
