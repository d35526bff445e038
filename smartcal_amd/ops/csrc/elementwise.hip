// Fused elementwise kernels: tanh-Gaussian sampling + log-prob (N3) and the
// flat-pool Adam step. One pass each — the reference composes ~10 torch ops
// for the sampler (enet_sac.py:446-466) and torch Adam runs ~6 kernels.
// The *_head_* kernels are the sampler on the actor head's raw output, and
// fused_adam_polyak2_kernel steps both critics and their targets at once.

#include "common.h"

#define LOG_SQRT_2PI 0.9189385332046727f
#define REPARAM_NOISE 1e-6f

// One element of the sampler: writes tanh(z) and the action, returns the
// element's log-probability term. Shared by the two forward kernels so that
// both round alike.
__device__ __forceinline__ float tanh_gauss_elem(float mu, float ls, float e,
                                                 float max_action,
                                                 float* __restrict__ at_out,
                                                 float* __restrict__ act_out) {
  const float sig = expf(ls);
  const float z = mu + sig * e;
  const float at = tanhf(z);
  *at_out = at;
  *act_out = at * max_action;
  return -0.5f * e * e - ls - LOG_SQRT_2PI
         - logf(max_action * (1.f - at * at) + REPARAM_NOISE);
}

// action = M*tanh(mu + sigma*eps); per-row logprob summed over action dim.
// One workgroup per batch row (action dims are tiny: 2..128).
extern "C" __global__ void tanh_gauss_fwd_kernel(
    const float* __restrict__ MU, const float* __restrict__ LOGSIG,
    const float* __restrict__ EPS, float* __restrict__ ACT,
    float* __restrict__ LOGP, float* __restrict__ AT, float max_action,
    int B, int A) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x;  // blockDim.x == 64 (one wave)
  float lp = 0.f;
  for (int c = lane; c < A; c += WAVE) {
    const long i = (long)row * A + c;
    lp += tanh_gauss_elem(MU[i], LOGSIG[i], EPS[i], max_action, &AT[i],
                          &ACT[i]);
  }
  lp = wave_sum(lp);
  if (lane == 0) LOGP[row] = lp;
}

// torch.clamp on floats: NaN passes through, else min(max(v, lo), hi)
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {
  return v != v ? v : fminf(fmaxf(v, lo), hi);
}

// The same sampler reading the actor head's raw output OUT (B, 2A):
// mu = OUT[:, :A], logsigma = clamp(OUT[:, A:], lo, hi). Replaces the slice
// copy, the clamp and the contiguous() in front of tanh_gauss_fwd_kernel.
extern "C" __global__ void tanh_gauss_head_fwd_kernel(
    const float* __restrict__ OUT, const float* __restrict__ EPS,
    float* __restrict__ ACT, float* __restrict__ LOGP,
    float* __restrict__ AT, float max_action, float lo, float hi, int B,
    int A) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x;  // blockDim.x == 64 (one wave)
  const float* o = OUT + (long)row * 2 * A;
  float lp = 0.f;
  for (int c = lane; c < A; c += WAVE) {
    const long i = (long)row * A + c;
    lp += tanh_gauss_elem(o[c], clamp_nan(o[A + c], lo, hi), EPS[i],
                          max_action, &AT[i], &ACT[i]);
  }
  lp = wave_sum(lp);
  if (lane == 0) LOGP[row] = lp;
}

// Backward for the reparameterized path.
// dmu = dact*M*(1-at^2) + dlogp * dlp_dz
// dlogsig = dact*M*(1-at^2)*sig*eps + dlogp * (-1 + dlp_dz*sig*eps)
// dlp_dz = 2*M*at*(1-at^2) / (M*(1-at^2)+1e-6)
extern "C" __global__ void tanh_gauss_bwd_kernel(
    const float* __restrict__ DACT, const float* __restrict__ DLOGP,
    const float* __restrict__ LOGSIG, const float* __restrict__ EPS,
    const float* __restrict__ AT, float* __restrict__ DMU,
    float* __restrict__ DLOGSIG, float max_action, int B, int A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * A) return;
  const int row = i / A;
  const float at = AT[i];
  const float one_m = 1.f - at * at;
  const float sig = expf(LOGSIG[i]);
  const float se = sig * EPS[i];
  const float dl = DLOGP[row];
  const float da = DACT[i];
  const float dlp_dz = 2.f * max_action * at * one_m
                       / (max_action * one_m + REPARAM_NOISE);
  const float dz = da * max_action * one_m + dl * dlp_dz;
  DMU[i] = dz;
  DLOGSIG[i] = dz * se - dl;
}

// Backward onto the head's raw output: DOUT[:, :A] = dmu and DOUT[:, A:] =
// dlogsigma where lo <= OUT <= hi, 0 elsewhere (NaN included), which is
// clamp's backward. The "+ 0.f" is the sum of the two padded slice
// gradients that autograd formed before (it turns -0 into +0).
// Contraction is off and the two fmas are written out: they are the ones
// the compiler forms in tanh_gauss_bwd_kernel (1 - at^2 and dz*se - dl;
// the sums in dlp_dz's denominator and in dz stay separate roundings
// there), so both kernels give the same bits
// (tests/test_gpu_sac_glue.py compares them).
extern "C" __global__ void tanh_gauss_head_bwd_kernel(
    const float* __restrict__ DACT, const float* __restrict__ DLOGP,
    const float* __restrict__ OUT, const float* __restrict__ EPS,
    const float* __restrict__ AT, float* __restrict__ DOUT, float max_action,
    float lo, float hi, int B, int A) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * A) return;
  const int row = i / A;
  const int c = i - (long)row * A;
  const long j = (long)row * 2 * A + A + c;  // the logsigma column
  const float raw = OUT[j];
  const float at = AT[i];
  const float one_m = __builtin_fmaf(-at, at, 1.f);
  const float sig = expf(clamp_nan(raw, lo, hi));
  const float se = sig * EPS[i];
  const float dl = DLOGP[row];
  const float da = DACT[i];
  const float dlp_dz = 2.f * max_action * at * one_m
                       / (max_action * one_m + REPARAM_NOISE);
  const float dz = da * max_action * one_m + dl * dlp_dz;
  DOUT[j - A] = dz + 0.f;
  DOUT[j] = (raw >= lo && raw <= hi) ? __builtin_fmaf(dz, se, -dl) + 0.f
                                     : 0.f;
}

// One element of bias-corrected Adam (torch defaults); returns the new
// parameter. Shared by fused_adam_kernel and fused_adam_polyak2_kernel.
__device__ __forceinline__ float adam_elem(float p, float g,
                                           float* __restrict__ M,
                                           float* __restrict__ V, float t,
                                           float lr, float b1, float b2,
                                           float eps) {
  const float bc1 = 1.f - powf(b1, t);
  const float bc2 = 1.f - powf(b2, t);
  const float m = b1 * *M + (1.f - b1) * g;
  const float v = b2 * *V + (1.f - b2) * g * g;
  *M = m;
  *V = v;
  const float mhat = m / bc1;
  const float vhat = v / bc2;
  p -= lr * mhat / (sqrtf(vhat) + eps);
  return p;
}

// Fused Adam over a flat parameter pool (bias-corrected, torch defaults).
// The step counter lives on the DEVICE (tptr) so the whole optimizer step
// is hipGraph-capturable: a separate bump kernel advances it afterwards,
// every block computes the bias corrections from the pre-bump value.
extern "C" __global__ void fused_adam_kernel(
    float* __restrict__ P, const float* __restrict__ G,
    float* __restrict__ M, float* __restrict__ V, float* __restrict__ tptr,
    float lr, float b1, float b2, float eps, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const float t = tptr[0] + 1.f;
  if (i >= n) return;
  P[i] = adam_elem(P[i], G[i], &M[i], &V[i], t, lr, b1, b2, eps);
}

// separate tiny bump kernel so the ordering vs fused_adam_kernel is safe
extern "C" __global__ void adam_bump_kernel(float* __restrict__ tptr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) tptr[0] += 1.f;
}

// torch's float lerp (ATen/native/Lerp.h), with the contraction that the
// GPU build of torch.Tensor.lerp_ has: both branches are one fma.
__device__ __forceinline__ float lerp_torch(float a, float b, float w) {
  const float d = b - a;
  return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, 1.f - w, b);
}

// Twin-critic Adam step and polyak update of the matching target pools in
// one launch: blockIdx.y picks the pool, each thread does adam_elem and then
// T = lerp(T, P_new, tau). Replaces two fused_adam_kernel launches on forked
// streams and two lerp_ launches.
extern "C" __global__ void fused_adam_polyak2_kernel(AdamPolyak2Args a,
                                                     float lr, float b1,
                                                     float b2, float eps,
                                                     float tau, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  float* __restrict__ P = k ? a.P1 : a.P0;
  const float* __restrict__ G = k ? a.G1 : a.G0;
  float* __restrict__ M = k ? a.M1 : a.M0;
  float* __restrict__ V = k ? a.V1 : a.V0;
  float* __restrict__ T = k ? a.T1 : a.T0;
  const float t = (k ? a.t1 : a.t0)[0] + 1.f;
  if (i >= n) return;
  const float p = adam_elem(P[i], G[i], &M[i], &V[i], t, lr, b1, b2, eps);
  P[i] = p;
  T[i] = lerp_torch(T[i], p, tau);
}

extern "C" __global__ void adam_bump2_kernel(float* __restrict__ t0,
                                             float* __restrict__ t1) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    t0[0] += 1.f;
    t1[0] += 1.f;
  }
}
