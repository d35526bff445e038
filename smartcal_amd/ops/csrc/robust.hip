// Residual, robust (Student's-t) weights and their sums for the
// calibration solver (radio/solver.py::calibrate), in one launch.
//
// One thread per sample (f, t, b), grid (ceil(TB / 256), F):
//     M  = sum_k J_p(t_i) C_k J_q(t_i)^H      row-major 2x2, as apply_jones
//     r  = V - M
//     e2 = sum of the 8 real components of r, squared
//     w  = m (nu_f + 8) / (nu_f + e2 / sigma2_f)
// m is the prior weight (flags, uv cut, user weights), nu and sigma2 are
// per-frequency device arrays, so the robust loop never reads anything
// back to the host. Each block also leaves the float64 partial sums of
// m, w e2, w and m (ln w - w) over its samples in part[f][block][0..3]:
// butterfly shuffles within the wave, then the four wave totals through
// LDS, added in wave order by one thread. The order is fixed, so two runs
// give the same bits; torch.sum over the block axis finishes the sums.
// No atomics.

#include "common.h"

#define ROBUST_THREADS 256
#define ROBUST_WAVES (ROBUST_THREADS / WAVE)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

extern "C" __global__ __launch_bounds__(ROBUST_THREADS)
void vis_residual_weights_kernel(
    const c32* __restrict__ C22,      // (F,K,T,B,2,2)
    const c32* __restrict__ V22,      // (F,T,B,2,2)
    const c32* __restrict__ J,        // (F,Ts,K,N,2,2)
    const float* __restrict__ m,      // (F,T,B) prior weights >= 0
    const float* __restrict__ nu,     // (F,)
    const float* __restrict__ sigma2, // (F,)
    const int* __restrict__ p_idx,    // (B,)
    const int* __restrict__ q_idx,    // (B,)
    const int* __restrict__ t_int,    // (T,)
    c32* __restrict__ r,              // (F,T*B,4)
    float* __restrict__ e2_out,       // (F,T,B)
    float* __restrict__ w_out,        // (F,T,B)
    double* __restrict__ part,        // (F,nblk,4)
    int K, int T, int B, int N, int Ts) {
  __shared__ double sh[ROBUST_WAVES][4];
  const int f = blockIdx.y;
  const long TB = (long)T * B;
  const long tb = (long)blockIdx.x * ROBUST_THREADS + threadIdx.x;
  // threads past the last sample stay for the reduction and add zeros
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (tb < TB) {
    const int t = (int)(tb / B);
    const int b = (int)(tb % B);
    const int ti = t_int[t];
    const int pp = p_idx[b];
    const int qq = q_idx[b];
    const long s = (long)f * TB + tb;
    c32 M[2][2] = {{{0.f, 0.f}, {0.f, 0.f}}, {{0.f, 0.f}, {0.f, 0.f}}};
    for (int k = 0; k < K; ++k) {
      const c32* cp = C22 + (((long)f * K + k) * TB + tb) * 4;
      const c32* jb = J + ((((long)f * Ts + ti) * K + k) * N) * 4;
      const c32* jp = jb + (long)pp * 4;
      const c32* jq = jb + (long)qq * 4;
      const c32 Cm[2][2] = {{cp[0], cp[1]}, {cp[2], cp[3]}};
      const c32 Jp[2][2] = {{jp[0], jp[1]}, {jp[2], jp[3]}};
      const c32 Jq[2][2] = {{jq[0], jq[1]}, {jq[2], jq[3]}};
      // P = Jp Cm, then M += P Jq^H
      c32 P[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          P[i][j] = cadd(cmul(Jp[i][0], Cm[0][j]), cmul(Jp[i][1], Cm[1][j]));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          M[i][j] = cadd(M[i][j], cadd(cmulj(P[i][0], Jq[j][0]),
                                       cmulj(P[i][1], Jq[j][1])));
    }
    const c32* vp = V22 + s * 4;
    c32* rp = r + s * 4;
    float e2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const c32 v = vp[2 * i + j];
        const c32 d = {v.x - M[i][j].x, v.y - M[i][j].y};
        rp[2 * i + j] = d;
        e2 += d.x * d.x;
        e2 += d.y * d.y;
      }
    const float ms = m[s];
    const float nuf = nu[f];
    const float w = ms * ((nuf + 8.f) / (nuf + e2 / sigma2[f]));
    e2_out[s] = e2;
    w_out[s] = w;
    acc[0] = (double)ms;
    acc[1] = (double)w * (double)e2;
    acc[2] = (double)w;
    // a sample without prior weight adds nothing, and ln 0 is never taken
    acc[3] = (ms > 0.f && w > 0.f)
                 ? (double)ms * (log((double)w) - (double)w) : 0.0;
  }
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double tot = wave_sum_f64(acc[i]);
    if (threadIdx.x % WAVE == 0) sh[wave][i] = tot;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double tot = sh[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < ROBUST_WAVES; ++wv) tot += sh[wv][threadIdx.x];
    part[((long)f * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = tot;
  }
}
