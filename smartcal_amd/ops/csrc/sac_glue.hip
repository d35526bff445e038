// The SAC learn step's elementwise glue as single launches: critic loss and
// actor loss (forward and backward) and the replay gather. Each replaces a
// chain of torch kernels on B x 1 tensors and rounds where those kernels
// rounded, so no product and sum may contract into an fma here.

#include "common.h"

#pragma clang fp contract(off)

#define LOSS_THREADS 256

// torch.minimum on floats: a NaN operand is the result, else min.
__device__ __forceinline__ float minimum_nan(float a, float b) {
  return a != a ? a : (b != b ? b : fminf(a, b));
}

// Sum over the block in a fixed order; thread 0 holds the total.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < LOSS_THREADS / WAVE; ++w) s += red[w];
  __syncthreads();
  return s;
}

// y = r + gamma * (done ? 0 : min(q1_t, q2_t) - alpha * logp), each product
// and sum rounded on its own; loss = mean((q1-y)^2) + mean((q2-y)^2).
// One block: B is a replay batch.
extern "C" __global__ void sac_critic_loss_fwd_kernel(
    const float* __restrict__ Q1, const float* __restrict__ Q2,
    const float* __restrict__ Q1T, const float* __restrict__ Q2T,
    const float* __restrict__ LOGP, const float* __restrict__ R,
    const bool* __restrict__ DONE, const float* __restrict__ ALPHA,
    float gamma, float* __restrict__ Y, float* __restrict__ LOSS, int B) {
  __shared__ float red[LOSS_THREADS / WAVE];
  const float alpha = ALPHA[0];
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < B; i += LOSS_THREADS) {
    float t = minimum_nan(Q1T[i], Q2T[i]) - alpha * LOGP[i];
    t = DONE[i] ? 0.f : t;
    const float y = R[i] + gamma * t;
    Y[i] = y;
    const float d1 = Q1[i] - y, d2 = Q2[i] - y;
    s1 += d1 * d1;
    s2 += d2 * d2;
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) LOSS[0] = s1 / (float)B + s2 / (float)B;
}

// dq_i = norm * (q_i - y) * g with norm = float(2/B): mse_loss's backward.
extern "C" __global__ void sac_critic_loss_bwd_kernel(
    const float* __restrict__ Q1, const float* __restrict__ Q2,
    const float* __restrict__ Y, const float* __restrict__ GRAD, float norm,
    float* __restrict__ DQ1, float* __restrict__ DQ2, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float g = GRAD[0], y = Y[i];
  DQ1[i] = norm * (Q1[i] - y) * g;
  DQ2[i] = norm * (Q2[i] - y) * g;
}

// loss = mean(alpha * logp - min(q1, q2)). One block.
extern "C" __global__ void sac_actor_loss_fwd_kernel(
    const float* __restrict__ Q1, const float* __restrict__ Q2,
    const float* __restrict__ LOGP, const float* __restrict__ ALPHA,
    float* __restrict__ LOSS, int B) {
  __shared__ float red[LOSS_THREADS / WAVE];
  const float alpha = ALPHA[0];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += LOSS_THREADS)
    s += alpha * LOGP[i] - minimum_nan(Q1[i], Q2[i]);
  s = block_sum(s, red);
  if (threadIdx.x == 0) LOSS[0] = s / (float)B;
}

// c = g * inv_b (mean's backward); dlogp = c * alpha; the minimum's
// derivative sends -c to the smaller operand, halves it on a tie and sends
// it to both when neither comparison holds (a NaN row).
extern "C" __global__ void sac_actor_loss_bwd_kernel(
    const float* __restrict__ Q1, const float* __restrict__ Q2,
    const float* __restrict__ ALPHA, const float* __restrict__ GRAD,
    float inv_b, float* __restrict__ DQ1, float* __restrict__ DQ2,
    float* __restrict__ DLOGP, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float c = GRAD[0] * inv_b;
  const float q1 = Q1[i], q2 = Q2[i];
  const float d = q1 == q2 ? -c / 2.f : -c;
  DLOGP[i] = c * ALPHA[0];
  DQ1[i] = q1 > q2 ? 0.f : d;
  DQ2[i] = q1 < q2 ? 0.f : d;
}

// One replay batch in one launch: block b copies row IDX[b] of every memory
// into row b of the outputs; the reward is multiplied by scale on the way.
// IDX is not range-checked: the caller draws it with randint(0, rows).
extern "C" __global__ void replay_gather_kernel(
    const long* __restrict__ IDX, const float* __restrict__ STATE,
    const float* __restrict__ NEW_STATE, const float* __restrict__ ACTION,
    const float* __restrict__ REWARD, const bool* __restrict__ TERMINAL,
    float scale, float* __restrict__ OUT_STATE,
    float* __restrict__ OUT_NEW_STATE, float* __restrict__ OUT_ACTION,
    float* __restrict__ OUT_REWARD, bool* __restrict__ OUT_DONE, int D,
    int A) {
  const long b = blockIdx.x;
  const long r = IDX[b];
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    OUT_STATE[b * D + c] = STATE[r * D + c];
    OUT_NEW_STATE[b * D + c] = NEW_STATE[r * D + c];
  }
  for (int c = threadIdx.x; c < A; c += blockDim.x)
    OUT_ACTION[b * A + c] = ACTION[r * A + c];
  if (threadIdx.x == 0) {
    OUT_REWARD[b] = REWARD[r] * scale;
    OUT_DONE[b] = TERMINAL[r];
  }
}
