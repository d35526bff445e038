// Shapelet (diffuse-sky) source prediction, added on top of the
// point/Gaussian coherencies of coherency.hip.
//
// A shapelet source contributes  G = smear(φ0) · e^{iφ0} · F(u,v)  with
//   u' = cosθ·u + sinθ·v,  v' = −sinθ·u + cosθ·v
//   F  = 2πβab · Σ_{i,j<n0} c[i·n0+j] · i^(i+j) · ψ_i(βa·u') · ψ_j(βb·v')
// (ψ_n the normalised Hermite functions; definition in
// radio/shapelet.py) and  XX += (sI+sQ)·G, YY += (sI−sQ)·G,
// XY = YX += sU·G.
//
// ONE launch covers every shapelet source of every cluster: grid
// (T-tiles × clusters-with-shapelets), one thread per sample t, looping
// the cluster's sources. Per source the block stages the n0² mode
// coefficients in LDS with the real sign of i^i · i^j folded in, so the
// loops only split by parity (even → real, odd → imaginary) and hold no
// complex multiply. Each thread writes its ψ_j(βb·v') column to an LDS
// table laid out [j][thread] (consecutive lanes → consecutive doubles,
// conflict-free; only the owning thread reads it back), then runs the
// ψ_i(βa·u') recurrence in registers in the outer loop — no run-time
// indexed register array, hence no scratch.
//
// ψ is evaluated with the normalised three-term recurrence in f64, never
// as H_n · exp: once e^(−t²/2) underflows every ψ_n is an exact 0, so on
// long baselines the kernel adds exact zeros.
//
// The sums are added into C by plain read-modify-write: one block owns
// all shapelet sources of its cluster, so each (k, t) has one writer.
//
// Per-source header row (12 doubles, precomputed host-side):
//   [l0, m0, n0c, sI_f, sQ_f, sU_f, βa, βb, cosθ, sinθ, 2πβab, n0]

#include "sky_term.h"

#define SHP_THREADS 128
#define SHP_MAXN 32      // n0 cap: 32² doubles of coefficients = 8 KB
#define SHP_HDR 12
#define PI_M14 0.75112554446494248      // π^(−1/4)

// BEAM = false is shapelet_kernel as it has always been: `gain` is unused
// and every beam statement is compiled out. BEAM = true weights source s of
// sample t = ts·B + b by the station-beam gain (sky_term.h) at its centre.
template <bool BEAM>
__device__ __forceinline__ void shapelet_body(
    const double* __restrict__ UVW,   // (T, 3) pre-scaled by 2πf/c
    const double* __restrict__ HDR,   // (Ns, 12)
    const int* __restrict__ COFF,     // (Ns) offsets into COEF
    const double* __restrict__ COEF,  // packed n0² blocks
    const int* __restrict__ CLK,      // (Kc) cluster index k in C
    const int* __restrict__ SOFF,     // (Kc+1) source ranges per cluster
    float* __restrict__ C,            // (K, T, 4) interleaved complex64
    double fdelta, int T, int K, int Ns, long ncoef, const BeamGain& gain) {
  __shared__ double cs[SHP_MAXN * SHP_MAXN];          // 8 KB
  __shared__ double pv[SHP_MAXN * SHP_THREADS];       // 32 KB, [j][thread]
  __shared__ double r1[SHP_MAXN], r2[SHP_MAXN];
  const int tid = threadIdx.x;
  const int t = blockIdx.x * SHP_THREADS + tid;
  const int k = CLK[blockIdx.y];
  const int s_lo = max(SOFF[blockIdx.y], 0);
  const int s_hi = min(SOFF[blockIdx.y + 1], Ns);
  if (k < 0 || k >= K) return;       // block-uniform: malformed table

  // recurrence coefficients ψ_{n+1} = t·r1[n]·ψ_n − r2[n]·ψ_{n−1}
  if (tid < SHP_MAXN) {
    const double n1 = (double)(tid + 1);
    r1[tid] = sqrt(2.0 / n1);
    r2[tid] = sqrt((double)tid / n1);
  }
  __syncthreads();

  double u = 0.0, v = 0.0, w = 0.0;
  if (t < T) {
    u = UVW[3 * t + 0];
    v = UVW[3 * t + 1];
    w = UVW[3 * t + 2];
  }
  double xx_re = 0.0, xx_im = 0.0, yy_re = 0.0, yy_im = 0.0;
  double xy_re = 0.0, xy_im = 0.0;     // YX = XY
  const double* ep = nullptr;          // E[t/B, ·, p], E[t/B, ·, q]
  const double* eq = nullptr;
  if constexpr (BEAM) {
    if (t < T) {
      const int ts = t / gain.B;
      beam_rows(gain, ts, t - ts * gain.B, ep, eq);
    }
  }

  for (int s = s_lo; s < s_hi; ++s) {
    const double* h = &HDR[(long)s * SHP_HDR];
    const int n0 = min(max((int)h[11], 1), SHP_MAXN);
    const int n0p = (n0 + 1) & ~1;     // even row stride, zero padded
    const long coff = COFF[s];
    // stage c[i][j] · sgn(i) · sgn(j), sgn(n) = +,+,−,− for n mod 4
    // (i^n = sgn(n) · {1 or i})
    for (int e = tid; e < n0 * n0p; e += SHP_THREADS) {
      const int i = e / n0p, j = e - i * n0p;
      const long g = coff + (long)i * n0 + j;
      double c = 0.0;
      if (j < n0 && g >= 0 && g < ncoef) c = COEF[g];
      cs[e] = (((i ^ j) & 2) != 0) ? -c : c;
    }
    const double up = h[8] * u + h[9] * v;
    const double vp = -h[9] * u + h[8] * v;
    if (t < T) {
      // ψ_j(βb·v') column → LDS (row n0 of an odd n0 meets zero padding)
      const double tv = h[7] * vp;
      double pm = 0.0;
      double p = PI_M14 * exp(-0.5 * tv * tv);
      for (int j = 0; j < n0p; ++j) {
        pv[j * SHP_THREADS + tid] = p;
        const double pn = tv * r1[j] * p - r2[j] * pm;
        pm = p;
        p = pn;
      }
    }
    __syncthreads();
    if (t < T) {
      const double tu = h[6] * up;
      double qm = 0.0;
      double q = PI_M14 * exp(-0.5 * tu * tu);       // ψ_i(βa·u')
      double f_re = 0.0, f_im = 0.0;
      for (int i = 0; i < n0; ++i) {
        // row sums: even j → real part, odd j → imaginary part
        double a = 0.0, b = 0.0;
        const double* cr = &cs[i * n0p];
        for (int j = 0; j < n0p; j += 2) {
          a += cr[j] * pv[j * SHP_THREADS + tid];
          b += cr[j + 1] * pv[(j + 1) * SHP_THREADS + tid];
        }
        if (i & 1) {            // × i
          f_re -= q * b;
          f_im += q * a;
        } else {
          f_re += q * a;
          f_im += q * b;
        }
        const double qn = tu * r1[i] * q - r2[i] * qm;
        qm = q;
        q = qn;
      }
      const double ph = u * h[0] + v * h[1] + w * h[2];
      double amp = h[10];
      if (fdelta > 0.0) amp *= sky_smear(ph, fdelta);
      const double cp = amp * cos(ph), sp = amp * sin(ph);
      double g_re = cp * f_re - sp * f_im;
      double g_im = cp * f_im + sp * f_re;
      if constexpr (BEAM) {
        double b_re, b_im;
        beam_gain(ep, eq, (long)s * gain.N * 2, b_re, b_im);
        const double t_re = b_re * g_re - b_im * g_im;
        g_im = b_re * g_im + b_im * g_re;
        g_re = t_re;
      }
      const double fx = h[3] + h[4], fy = h[3] - h[4], fu = h[5];
      xx_re += fx * g_re;  xx_im += fx * g_im;
      yy_re += fy * g_re;  yy_im += fy * g_im;
      xy_re += fu * g_re;  xy_im += fu * g_im;
    }
    __syncthreads();      // cs is restaged for the next source
  }
  if (t < T) {
    float* o = &C[((long)k * T + t) * 8];     // 4 complex = 8 floats
    o[0] = (float)((double)o[0] + xx_re);     // XX
    o[1] = (float)((double)o[1] + xx_im);
    o[2] = (float)((double)o[2] + xy_re);     // XY
    o[3] = (float)((double)o[3] + xy_im);
    o[4] = (float)((double)o[4] + xy_re);     // YX
    o[5] = (float)((double)o[5] + xy_im);
    o[6] = (float)((double)o[6] + yy_re);     // YY
    o[7] = (float)((double)o[7] + yy_im);
  }
}

extern "C" __global__ __launch_bounds__(SHP_THREADS) void shapelet_kernel(
    const double* __restrict__ UVW, const double* __restrict__ HDR,
    const int* __restrict__ COFF, const double* __restrict__ COEF,
    const int* __restrict__ CLK, const int* __restrict__ SOFF,
    float* __restrict__ C, double fdelta, int T, int K, int Ns,
    long ncoef) {
  shapelet_body<false>(UVW, HDR, COFF, COEF, CLK, SOFF, C, fdelta, T, K, Ns,
                       ncoef, BeamGain{});
}

extern "C" __global__ __launch_bounds__(SHP_THREADS) void shapelet_beam_kernel(
    const double* __restrict__ UVW, const double* __restrict__ HDR,
    const int* __restrict__ COFF, const double* __restrict__ COEF,
    const int* __restrict__ CLK, const int* __restrict__ SOFF,
    float* __restrict__ C, double fdelta, int T, int K, int Ns, long ncoef,
    const double* __restrict__ E, const int* __restrict__ P,
    const int* __restrict__ Q, int B, int N, int Sall, int sbase) {
  shapelet_body<true>(UVW, HDR, COFF, COEF, CLK, SOFF, C, fdelta, T, K, Ns,
                      ncoef, BeamGain{E, P, Q, B, N, Sall, sbase});
}
