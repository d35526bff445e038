// Station array-factor beam for coherency prediction.
//
// Station p beam-forms Ne elements at offsets (u_e, v_e, w_e) from its
// centre (uvw frame of timeslot t, meters), steered at the phase centre:
//   E[t, p, s] = (1/Ne) · Σ_e exp(+i · scale · (u_e·l_s + v_e·m_s + w_e·n_s))
// with scale = 2πf/c and n_s the (n − 1) of the source tables. The
// beam-weighted coherency of baseline b = (p, q) at timeslot t is
//   C_k[t·B + b] = Σ_s E[t,p,s] · conj(E[t,q,s]) · amp_s · e^{iφ_s}
// with amp_s·e^{iφ_s} the source term of sky_term.h; the consumers are
// coherency_beam_kernel (coherency.hip) and shapelet_beam_kernel
// (shapelet.hip).
//
// station_beam_kernel builds E for every source of every cluster (point /
// Gaussian rows first, shapelet centres after them) in one launch. Grid
// (source tiles × stations × timeslots); the block stages the element
// coordinates of its (t, station) in LDS, pre-scaled, and every thread owns
// one source and loops the elements with f64 sincos — all lanes read the
// same LDS word (broadcast). E is stored [t][s][station] so that the
// consumers' lanes, which run over consecutive q at (nearly) uniform p,
// read consecutive 16-byte entries.

#include "common.h"

#define BEAM_THREADS 128
#define BEAM_ECHUNK 256   // elements staged per LDS pass (256*3*8 = 6 KB)

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
