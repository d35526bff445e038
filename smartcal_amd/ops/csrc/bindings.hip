// Python bindings for the smartcal_amd HIP/CDNA4 kernels (gfx950 only).
// Explicit HIP APIs throughout — no CUDA-compat shims.

#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <algorithm>
#include <climits>
#include <tuple>

#include "common.h"

#define HMAX 7

// ---- kernel declarations (definitions in the sibling .hip files) ----
extern "C" __global__ void fused_linear_fwd_kernel(
    const float*, const float*, const float*, const float*, const float*,
    float*, float*, float*, int, int, int, int, int);
extern "C" __global__ void ln_act_bwd_kernel(const float*, const float*,
                                             const float*, const float*,
                                             const float*, float*, float*,
                                             float*, int, int, int, int,
                                             int);
extern "C" __global__ void gemm_f32_nn_kernel(const float*, const float*,
                                              float*, int, int, int);
extern "C" __global__ void gemm_f32_tn_kernel(const float*, const float*,
                                              float*, float*, int, int, int,
                                              int);
extern "C" __global__ void colsum_kernel(const float*, float*, int, int,
                                         int);
extern "C" __global__ void tanh_gauss_fwd_kernel(const float*, const float*,
                                                 const float*, float*, float*,
                                                 float*, float, int, int);
extern "C" __global__ void tanh_gauss_bwd_kernel(const float*, const float*,
                                                 const float*, const float*,
                                                 const float*, float*, float*,
                                                 float, int, int);
extern "C" __global__ void fused_adam_kernel(float*, const float*, float*,
                                             float*, float*, float, float,
                                             float, float, long);
extern "C" __global__ void adam_bump_kernel(float*);
extern "C" __global__ void tanh_gauss_head_fwd_kernel(const float*,
                                                      const float*, float*,
                                                      float*, float*, float,
                                                      float, float, int, int);
extern "C" __global__ void tanh_gauss_head_bwd_kernel(
    const float*, const float*, const float*, const float*, const float*,
    float*, float, float, float, int, int);
extern "C" __global__ void fused_adam_polyak2_kernel(AdamPolyak2Args, float,
                                                     float, float, float,
                                                     float, long);
extern "C" __global__ void adam_bump2_kernel(float*, float*);
extern "C" __global__ void sac_critic_loss_fwd_kernel(
    const float*, const float*, const float*, const float*, const float*,
    const float*, const bool*, const float*, float, float*, float*, int);
extern "C" __global__ void sac_critic_loss_bwd_kernel(const float*,
                                                      const float*,
                                                      const float*,
                                                      const float*, float,
                                                      float*, float*, int);
extern "C" __global__ void sac_actor_loss_fwd_kernel(const float*,
                                                     const float*,
                                                     const float*,
                                                     const float*, float*,
                                                     int);
extern "C" __global__ void sac_actor_loss_bwd_kernel(const float*,
                                                     const float*,
                                                     const float*,
                                                     const float*, float,
                                                     float*, float*, float*,
                                                     int);
extern "C" __global__ void replay_gather_kernel(
    const long*, const float*, const float*, const float*, const float*,
    const bool*, float, float*, float*, float*, float*, bool*, int, int);
extern "C" __global__ void enet_lbfgs_solve_kernel(
    const float*, const float*, const float*, float*, float*, float*, int*,
    int, int, int, int, int, int);
extern "C" __global__ void conv2d_k5s2_fwd_kernel(
    const float*, const float*, const float*, float*, int, int, int, int,
    int, int, int);
extern "C" __global__ void conv2d_k5s2_dx_kernel(
    const float*, const float*, float*, int, int, int, int, int, int, int);
extern "C" __global__ void conv2d_k5s2_dw_kernel(
    const float*, const float*, float*, float*, int, int, int, int, int,
    int, int);
struct c32b { float x, y; };
extern "C" __global__ void als_sweep_kernel(
    const c32b*, const c32b*, const c32b*, const int*, const int*,
    const int*, c32b*, c32b*, int, int, int, int, int, int);
extern "C" __global__ void als_sweep_w_kernel(
    const c32b*, const c32b*, const c32b*, const float*, const int*,
    const int*, const int*, c32b*, c32b*, int, int, int, int, int, int);
extern "C" __global__ void vis_residual_weights_kernel(
    const c32b*, const c32b*, const c32b*, const float*, const float*,
    const float*, const int*, const int*, const int*, c32b*, float*, float*,
    double*, int, int, int, int, int);
extern "C" __global__ void enet_influence_kernel(
    const float*, const float*, const float*, const float*, const float*,
    const int*, const float*, const float*, float*, float*, int, int, int);
extern "C" __global__ void per_sample_kernel(const float*, const float*,
                                             long*, float*, float*, int, int,
                                             float);
extern "C" __global__ void fused_linear_bf16_fwd_kernel(
    const float*, const float*, const float*, const float*, const float*,
    float*, float*, float*, int, int, int, int, int);
extern "C" __global__ void gemm_bf16_nn_kernel(const float*, const float*,
                                               float*, int, int, int);
extern "C" __global__ void gemm_bf16_tn_kernel(const float*, const float*,
                                               float*, int, int, int, int);
extern "C" __global__ void attn_fwd_kernel(const float*, const float*,
                                           const float*, float*, float*,
                                           int, int, int);
extern "C" __global__ void attn_bwd_kernel(const float*, const float*,
                                           const float*, const float*,
                                           const float*, float*, float*,
                                           float*, int, int, int);
extern "C" __global__ void cgemm_nn_bcast_kernel(const float*, const float*,
                                                 float*, int, int, int, int,
                                                 int);
extern "C" __global__ void coherency_kernel(const double*, const double*,
                                            const int*, float*, double,
                                            int, int, int);
extern "C" __global__ void shapelet_kernel(const double*, const double*,
                                           const int*, const double*,
                                           const int*, const int*, float*,
                                           double, int, int, int, long);
extern "C" __global__ void shapelet_beam_kernel(
    const double*, const double*, const int*, const double*, const int*,
    const int*, float*, double, int, int, int, long, const double*,
    const int*, const int*, int, int, int, int);
extern "C" __global__ void station_beam_kernel(const double*, const double*,
                                               double*, double, int, int,
                                               int, int);
extern "C" __global__ void coherency_beam_kernel(
    const double*, const double*, const int*, const double*, const int*,
    const int*, float*, double, int, int, int, int, int, int);
extern "C" __global__ void dft_image_kernel(const double*, const float2*,
                                            const double*, float*, double*,
                                            double, double, long, int, int,
                                            int, int);
extern "C" __global__ void dft_image_reduce_kernel(const double*, float*,
                                                   long, int);
struct c32h2 { float x, y; };
extern "C" __global__ void hessianres_kernel(
    const c32h2*, const c32h2*, const c32h2*, const int*, const int*,
    c32h2*, int, int, int, int);
extern "C" __global__ void hessianres_scale_diag_kernel(c32h2*, int, int,
                                                        int, int);
extern "C" __global__ void two_loop_kernel(const float*, const float*,
                                           const float*, float*,
                                           const float*, float, int, long,
                                           int);
extern "C" __global__ void gather_sum_kernel(const c32b*, const long*,
                                             c32b*, int, int, long, int,
                                             int);
extern "C" __global__ void per_update_kernel(float*, const long*,
                                             const float*, int, float, float,
                                             float);

namespace {

inline void check_f32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline hipStream_t stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// Read the status of the launch just issued, so that a refused launch
// raises here and does not leave its error for the next binding.
inline void check_launch(const char* kernel) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, kernel, " launch: ",
              hipGetErrorString(err));
}

inline void check_c64(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == at::kComplexFloat, name,
              " must be complex64");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// An index table the callers build: 1-D, `count` entries of `type`.
inline void check_index(const at::Tensor& t, at::ScalarType type,
                        int64_t count, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == type, name, " must be ", type);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == count, name, " must hold ",
              count, " entries, got ", t.sizes());
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> fused_linear_fwd(
    const at::Tensor& x, const at::Tensor& W,
    const c10::optional<at::Tensor>& bias,
    const c10::optional<at::Tensor>& gamma,
    const c10::optional<at::Tensor>& beta, int64_t act, bool with_ln) {
  check_f32(x, "x");
  check_f32(W, "W");
  const int B = x.size(0), K = x.size(1), N = W.size(0);
  TORCH_CHECK(W.size(1) == K, "W/K mismatch");
  TORCH_CHECK(N <= 1536, "fused_linear: N>1536 unsupported (extend NT_MAX)");
  TORCH_CHECK(!with_ln || gamma.has_value(), "LN requires gamma");
  auto y = at::empty({B, N}, x.options());
  auto zhat = with_ln ? at::empty({B, N}, x.options())
                      : at::empty({0}, x.options());
  auto rstd = with_ln ? at::empty({B}, x.options())
                      : at::empty({0}, x.options());
  dim3 grid((B + 15) / 16);
  hipLaunchKernelGGL(fused_linear_fwd_kernel, grid, dim3(512), 0, stream(),
                     x.data_ptr<float>(), W.data_ptr<float>(),
                     bias ? bias->data_ptr<float>() : nullptr,
                     gamma ? gamma->data_ptr<float>() : nullptr,
                     beta ? beta->data_ptr<float>() : nullptr,
                     y.data_ptr<float>(),
                     with_ln ? zhat.data_ptr<float>() : nullptr,
                     with_ln ? rstd.data_ptr<float>() : nullptr, B, K, N,
                     (int)act, with_ln ? 1 : 0);
  return {y, zhat, rstd};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> fused_linear_bwd_dz(
    const at::Tensor& dy, const at::Tensor& y, const at::Tensor& zhat,
    const at::Tensor& rstd, const c10::optional<at::Tensor>& gamma,
    int64_t act, bool with_ln) {
  check_f32(dy, "dy");
  const int B = dy.size(0), N = dy.size(1);
  auto dz = at::empty({B, N}, dy.options());
  auto dgamma = at::zeros({N}, dy.options());
  auto dbeta = at::zeros({N}, dy.options());
  hipLaunchKernelGGL(ln_act_bwd_kernel, dim3(B), dim3(256), 0, stream(),
                     dy.data_ptr<float>(), y.data_ptr<float>(),
                     with_ln ? zhat.data_ptr<float>() : nullptr,
                     with_ln ? rstd.data_ptr<float>() : nullptr,
                     gamma ? gamma->data_ptr<float>() : nullptr,
                     dz.data_ptr<float>(), dgamma.data_ptr<float>(),
                     dbeta.data_ptr<float>(), B, N, (int)act,
                     with_ln ? 1 : 0, N);
  return {dz, dgamma, dbeta};
}

// Argument block of mlp_chain_bf16_fwd_kernel, which keeps the plain-chain
// layout (fused_linear_bf16.hip defines the same struct for itself). The
// fp32 kernel takes the layer program ChainArgs of common.h.
struct ChainArgsBf16 {
  const float* W[4];
  const float* bias[4];
  const float* gamma[4];
  const float* beta[4];
  float* Y[4];
  float* ZHAT[4];
  float* RSTD[4];
  int dims[5];
  int act[4];
  int with_ln[4];
  int L;
  int B;
};
extern "C" __global__ void mlp_chain_fwd_kernel(ChainArgs);
extern "C" __global__ void mlp_chain_bf16_fwd_kernel(const float*,
                                                     ChainArgsBf16);

using OptTensors = std::vector<c10::optional<at::Tensor>>;

struct ChainSaved {
  std::vector<at::Tensor> ys, zhats, rstds;
};

inline int round_up_64(int v) { return (v + 63) / 64 * 64; }

// Layer l of a chain program: parameters, shape and LDS ranges. With
// `save` the per-layer y / zhat / rstd that backward needs are allocated
// and stored; `keep_y` alone allocates y (a final output).
void chain_set_layer(ChainArgs& a, int l, const at::Tensor& W,
                     const c10::optional<at::Tensor>& bias,
                     const c10::optional<at::Tensor>& gamma,
                     const c10::optional<at::Tensor>& beta, int64_t act,
                     int src, int src_off, int dst, int dst_off, bool save,
                     bool keep_y, const at::TensorOptions& opt,
                     ChainSaved& out) {
  check_f32(W, "W");
  const int N = W.size(0), K = W.size(1);
  const bool ln = gamma.has_value();
  TORCH_CHECK(!ln || beta.has_value(), "LN requires gamma and beta");
  TORCH_CHECK(K >= 1 && N >= 1 && K <= 512 && N <= 512,
              "chain widths must be in 1..512");
  TORCH_CHECK(src_off >= 0 && dst_off >= 0
              && src_off + round_up_64(K) <= CHAIN_XMAX
              && round_up_64(dst_off + N) <= CHAIN_XMAX,
              "chain layer leaves its LDS buffer");
  // a layer may read and write one buffer only in disjoint column ranges
  TORCH_CHECK(src != dst || src_off + round_up_64(K) <= dst_off
              || round_up_64(dst_off + N) <= src_off,
              "chain layer reads and writes overlapping LDS columns");
  if (bias) check_f32(*bias, "bias");
  if (ln) {
    check_f32(*gamma, "gamma");
    check_f32(*beta, "beta");
    TORCH_CHECK(gamma->numel() == N && beta->numel() == N, "LN size");
  }
  TORCH_CHECK(!bias || bias->numel() == N, "bias size");
  a.W[l] = W.data_ptr<float>();
  a.bias[l] = bias ? bias->data_ptr<float>() : nullptr;
  a.gamma[l] = ln ? gamma->data_ptr<float>() : nullptr;
  a.beta[l] = ln ? beta->data_ptr<float>() : nullptr;
  a.K[l] = K;
  a.N[l] = N;
  a.src[l] = src;
  a.src_off[l] = src_off;
  a.dst[l] = dst;
  a.dst_off[l] = dst_off;
  a.act[l] = (int)act;
  a.with_ln[l] = ln ? 1 : 0;
  const int B = a.B;
  if (save || keep_y) {
    out.ys.push_back(at::empty({B, N}, opt));
    a.Y[l] = out.ys.back().data_ptr<float>();
  }
  if (save) {
    out.zhats.push_back(ln ? at::empty({B, N}, opt) : at::empty({0}, opt));
    out.rstds.push_back(ln ? at::empty({B}, opt) : at::empty({0}, opt));
    a.ZHAT[l] = ln ? out.zhats.back().data_ptr<float>() : nullptr;
    a.RSTD[l] = ln ? out.rstds.back().data_ptr<float>() : nullptr;
  }
}

void chain_launch(const ChainArgs& args) {
  // dynamic LDS: 2 activation buffers + per-wave W subtiles (16 waves)
  // + row stats — ~139 KB of the 160 KB LDS (one block per CU; only
  // ceil(B/16) blocks exist anyway)
  const int lds_bytes =
      (2 * 16 * (CHAIN_XMAX + 1) + 16 * 16 * 65 + 16 * 16 * 2 + 16 * 2)
      * (int)sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&mlp_chain_fwd_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    attr_set = true;
  }
  if (args.B == 0) return;
  hipLaunchKernelGGL(mlp_chain_fwd_kernel, dim3((args.B + 15) / 16),
                     dim3(1024), lds_bytes, stream(), args);
}

// One kernel for a whole Linear(+LN)(+act) chain (≤4 layers, widths ≤512):
// activations ping-pong in LDS. Returns lists [y_l], [zhat_l], [rstd_l] for
// backward; with save == false (nothing will be differentiated) only the
// last layer's y is allocated and stored: ([y_last], [], []).
std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>,
           std::vector<at::Tensor>>
mlp_chain_fwd(const at::Tensor& x, const std::vector<at::Tensor>& Ws,
              const OptTensors& bs, const OptTensors& gammas,
              const OptTensors& betas, const std::vector<int64_t>& acts,
              bool bf16, bool save) {
  check_f32(x, "x");
  const int L = (int)Ws.size();
  TORCH_CHECK(L >= 1 && L <= 4, "chain supports 1..4 layers");
  TORCH_CHECK((int)bs.size() == L && (int)gammas.size() == L
              && (int)betas.size() == L && (int)acts.size() == L,
              "chain needs one entry per layer");
  TORCH_CHECK(x.dim() == 2, "x must be (B, K)");
  const int B = x.size(0);
  if (bf16) {
    ChainArgsBf16 args{};
    args.L = L;
    args.B = B;
    args.dims[0] = x.size(1);
    std::vector<at::Tensor> ys, zhats, rstds;
    for (int l = 0; l < L; ++l) {
      check_f32(Ws[l], "W");
      const int N = Ws[l].size(0);
      TORCH_CHECK(Ws[l].size(1) == args.dims[l], "chain dim mismatch");
      TORCH_CHECK(N <= 512 && args.dims[l] <= 512, "chain widths <= 512");
      args.dims[l + 1] = N;
      args.W[l] = Ws[l].data_ptr<float>();
      args.bias[l] = bs[l] ? bs[l]->data_ptr<float>() : nullptr;
      const bool ln = gammas[l].has_value();
      args.with_ln[l] = ln ? 1 : 0;
      args.gamma[l] = ln ? gammas[l]->data_ptr<float>() : nullptr;
      args.beta[l] = ln ? betas[l]->data_ptr<float>() : nullptr;
      args.act[l] = (int)acts[l];
      ys.push_back(at::empty({B, N}, x.options()));
      zhats.push_back(ln ? at::empty({B, N}, x.options())
                         : at::empty({0}, x.options()));
      rstds.push_back(ln ? at::empty({B}, x.options())
                         : at::empty({0}, x.options()));
      args.Y[l] = ys[l].data_ptr<float>();
      args.ZHAT[l] = ln ? zhats[l].data_ptr<float>() : nullptr;
      args.RSTD[l] = ln ? rstds[l].data_ptr<float>() : nullptr;
    }
    // bf16 W region: 16 waves x 16 x 72 bf16 rounded up to floats
    const int lds_bytes =
        (2 * 16 * (CHAIN_XMAX + 1) + (16 * 16 * 72 + 1) / 2 + 16 * 16 * 2
         + 16 * 2) * (int)sizeof(float);
    static bool attr_set_b = false;
    if (!attr_set_b) {
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(&mlp_chain_bf16_fwd_kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
      attr_set_b = true;
    }
    hipLaunchKernelGGL(mlp_chain_bf16_fwd_kernel, dim3((B + 15) / 16),
                       dim3(1024), lds_bytes, stream(),
                       x.data_ptr<float>(), args);
    return {ys, zhats, rstds};
  }
  ChainArgs args{};
  args.L = L;
  args.B = B;
  args.XIN[0] = x.data_ptr<float>();
  ChainSaved out;
  int K = x.size(1);
  for (int l = 0; l < L; ++l) {
    TORCH_CHECK(Ws[l].dim() == 2 && Ws[l].size(1) == K,
                "chain dim mismatch");
    chain_set_layer(args, l, Ws[l], bs[l], gammas[l], betas[l], acts[l],
                    l & 1, 0, 1 - (l & 1), 0, save, l == L - 1,
                    x.options(), out);
    K = Ws[l].size(0);
  }
  chain_launch(args);
  return {out.ys, out.zhats, out.rstds};
}

// The critic (state branch s1, s2; action branch a1, a2; linear head over
// their concatenation) as ONE chain-kernel launch. Ws/bs/gammas/betas/acts
// hold s1, s2, a1, a2, head. The branch outputs land side by side in one
// LDS buffer, which the head reads as its input. Returns q, the
// concatenated head input zcat (B, N_s2 + N_a2) and the per-layer lists of
// the four branch layers; with save == false only q is allocated and
// stored (zcat is empty, the lists too).
std::tuple<at::Tensor, at::Tensor, std::vector<at::Tensor>,
           std::vector<at::Tensor>, std::vector<at::Tensor>>
critic_fwd(const at::Tensor& state, const at::Tensor& action,
           const std::vector<at::Tensor>& Ws, const OptTensors& bs,
           const OptTensors& gammas, const OptTensors& betas,
           const std::vector<int64_t>& acts, bool save) {
  check_f32(state, "state");
  check_f32(action, "action");
  TORCH_CHECK(Ws.size() == 5 && bs.size() == 5 && gammas.size() == 5
              && betas.size() == 5 && acts.size() == 5,
              "critic_fwd takes five layers: s1, s2, a1, a2, head");
  TORCH_CHECK(state.dim() == 2 && action.dim() == 2
              && state.size(0) == action.size(0),
              "state and action must be (B, K) with one batch size");
  for (const auto& W : Ws) TORCH_CHECK(W.dim() == 2, "W must be (N, K)");
  const int B = state.size(0);
  const int Ns1 = Ws[0].size(0), Ns2 = Ws[1].size(0);
  const int Na1 = Ws[2].size(0), Na2 = Ws[3].size(0);
  TORCH_CHECK(Ws[0].size(1) == state.size(1) && Ws[1].size(1) == Ns1
              && Ws[2].size(1) == action.size(1) && Ws[3].size(1) == Na1
              && Ws[4].size(1) == Ns2 + Na2, "critic dim mismatch");
  TORCH_CHECK(Ns2 + Na2 <= 512, "critic head input <= 512");
  TORCH_CHECK(!gammas[4].has_value(), "the critic head has no LayerNorm");
  const int Kpa = round_up_64((int)action.size(1));
  ChainArgs args{};
  args.L = 5;
  args.B = B;
  args.XIN[0] = state.data_ptr<float>();
  args.XIN[2] = action.data_ptr<float>();
  ChainSaved out;
  const auto opt = state.options();
  // buffer 0 collects the head input; buffer 1 holds s1's output, then the
  // staged action (columns 0..Kpa) and a1's output behind it
  chain_set_layer(args, 0, Ws[0], bs[0], gammas[0], betas[0], acts[0],
                  0, 0, 1, 0, save, false, opt, out);
  chain_set_layer(args, 1, Ws[1], bs[1], gammas[1], betas[1], acts[1],
                  1, 0, 0, 0, save, false, opt, out);
  chain_set_layer(args, 2, Ws[2], bs[2], gammas[2], betas[2], acts[2],
                  1, 0, 1, Kpa, save, false, opt, out);
  chain_set_layer(args, 3, Ws[3], bs[3], gammas[3], betas[3], acts[3],
                  1, Kpa, 0, Ns2, save, false, opt, out);
  ChainSaved head;
  chain_set_layer(args, 4, Ws[4], bs[4], gammas[4], betas[4], acts[4],
                  0, 0, 1, 0, false, true, opt, head);
  at::Tensor zcat = at::empty({save ? B : 0, Ns2 + Na2}, opt);
  if (save) {
    args.ldc = Ns2 + Na2;
    args.YC[1] = zcat.data_ptr<float>();
    args.YC[3] = zcat.data_ptr<float>() + Ns2;
  }
  chain_launch(args);
  return {head.ys[0], zcat, out.ys, out.zhats, out.rstds};
}

at::Tensor conv2d_k5s2_fwd(const at::Tensor& x, const at::Tensor& W,
                           const c10::optional<at::Tensor>& bias) {
  check_f32(x, "x");
  check_f32(W, "W");
  TORCH_CHECK(x.dim() == 4 && W.dim() == 4,
              "conv2d_k5s2: x must be (B, Cin, H, W), weight 4-D");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), Wd = x.size(3);
  const int Cout = W.size(0);
  TORCH_CHECK(W.size(1) == Cin && W.size(2) == 5 && W.size(3) == 5,
              "conv2d_k5s2: weight must be (Cout, Cin, 5, 5)");
  // below 5 the C division would still give one window, outside the image
  TORCH_CHECK(H >= 5 && Wd >= 5, "conv2d_k5s2: the image (", H, " x ", Wd,
              ") is smaller than the 5 x 5 kernel");
  if (bias) {
    check_f32(*bias, "bias");
    TORCH_CHECK(bias->numel() == Cout, "conv2d_k5s2: bias must hold Cout");
  }
  const int OH = (H - 5) / 2 + 1, OW = (Wd - 5) / 2 + 1;
  auto y = at::empty({B, Cout, OH, OW}, x.options());
  const long total = (long)B * Cout * OH * OW;
  if (total == 0) return y;
  TORCH_CHECK(Cin >= 1, "conv2d_k5s2: no input channels");
  hipLaunchKernelGGL(conv2d_k5s2_fwd_kernel,
                     dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream(), x.data_ptr<float>(), W.data_ptr<float>(),
                     bias ? bias->data_ptr<float>() : nullptr,
                     y.data_ptr<float>(), B, Cin, H, Wd, Cout, OH, OW);
  check_launch("conv2d_k5s2_fwd_kernel");
  return y;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> conv2d_k5s2_bwd(
    const at::Tensor& dy, const at::Tensor& x, const at::Tensor& W) {
  check_f32(dy, "dy");
  check_f32(x, "x");
  check_f32(W, "W");
  TORCH_CHECK(x.dim() == 4 && W.dim() == 4 && dy.dim() == 4,
              "conv2d_k5s2_bwd: dy, x and weight must be 4-D");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), Wd = x.size(3);
  const int Cout = W.size(0);
  TORCH_CHECK(W.size(1) == Cin && W.size(2) == 5 && W.size(3) == 5,
              "conv2d_k5s2_bwd: weight must be (Cout, Cin, 5, 5)");
  TORCH_CHECK(H >= 5 && Wd >= 5, "conv2d_k5s2_bwd: the image (", H, " x ",
              Wd, ") is smaller than the 5 x 5 kernel");
  const int OH = (H - 5) / 2 + 1, OW = (Wd - 5) / 2 + 1;
  TORCH_CHECK(dy.size(0) == B && dy.size(1) == Cout && dy.size(2) == OH
              && dy.size(3) == OW, "conv2d_k5s2_bwd: dy must be (", B, ", ",
              Cout, ", ", OH, ", ", OW, "), got ", dy.sizes());
  const long totx = (long)B * Cin * H * Wd;
  const bool empty = B == 0 || Cout == 0;
  TORCH_CHECK(empty || Cin >= 1, "conv2d_k5s2_bwd: no input channels");
  // an empty batch or channel axis leaves every gradient at zero
  auto dx = empty ? at::zeros_like(x) : at::empty_like(x);
  auto dW = empty ? at::zeros_like(W) : at::empty_like(W);
  auto db = empty ? at::zeros({Cout}, x.options())
                  : at::empty({Cout}, x.options());
  if (empty) return {dx, dW, db};
  hipLaunchKernelGGL(conv2d_k5s2_dx_kernel,
                     dim3((unsigned)((totx + 255) / 256)), dim3(256), 0,
                     stream(), dy.data_ptr<float>(), W.data_ptr<float>(),
                     dx.data_ptr<float>(), B, Cin, H, Wd, Cout, OH, OW);
  check_launch("conv2d_k5s2_dx_kernel");
  hipLaunchKernelGGL(conv2d_k5s2_dw_kernel, dim3(Cout * Cin), dim3(256), 0,
                     stream(), dy.data_ptr<float>(), x.data_ptr<float>(),
                     dW.data_ptr<float>(), db.data_ptr<float>(), B, Cin, H,
                     Wd, Cout, OH, OW);
  check_launch("conv2d_k5s2_dw_kernel");
  return {dx, dW, db};
}

// Fused ALS-sweep contributions for the calibration solver: one launch
// instead of ~100 elementwise kernels per sweep (radio/solver.py). With
// weights w (F, T, B) every entry of a sample is scaled by its weight
// (als_sweep_w_kernel, the weighted instance of the same body).
std::tuple<at::Tensor, at::Tensor> als_sweep_impl(
    const char* who, const at::Tensor& C22, const at::Tensor& V22,
    const at::Tensor& J, const at::Tensor* w, const at::Tensor& p_idx,
    const at::Tensor& q_idx, const at::Tensor& t_int) {
  check_c64(C22, "C22");
  check_c64(V22, "V22");
  check_c64(J, "J");
  TORCH_CHECK(C22.dim() == 6 && C22.size(4) == 2 && C22.size(5) == 2,
              who, ": C22 must be (F, K, T, B, 2, 2), got ", C22.sizes());
  const int64_t F = C22.size(0), K = C22.size(1), T = C22.size(2),
                B = C22.size(3);
  TORCH_CHECK(K <= 8, who, " supports K <= 8");
  TORCH_CHECK(V22.dim() == 5 && V22.size(0) == F && V22.size(1) == T
              && V22.size(2) == B && V22.size(3) == 2 && V22.size(4) == 2,
              who, ": V22 must be (", F, ", ", T, ", ", B,
              ", 2, 2), got ", V22.sizes());
  TORCH_CHECK(J.dim() == 6 && J.size(0) == F && J.size(2) == K
              && J.size(4) == 2 && J.size(5) == 2,
              who, ": J must be (", F, ", Ts, ", K, ", N, 2, 2), got ",
              J.sizes());
  const int64_t Ts = J.size(1), N = J.size(3);
  if (w) {
    check_f32(*w, "w");
    TORCH_CHECK(w->dim() == 3 && w->size(0) == F && w->size(1) == T
                && w->size(2) == B, who, ": w must be (", F, ", ", T, ", ",
                B, "), got ", w->sizes());
  }
  check_index(p_idx, at::kInt, B, "p_idx");
  check_index(q_idx, at::kInt, B, "q_idx");
  check_index(t_int, at::kInt, T, "t_int");
  // entry-major layout (F, X, 2TB): kernel writes coalesce across the
  // sample axis and the gather+sum reduces along the last dim
  auto rhs_cat = at::empty({F, 2L * 2 * K, 2L * T * B}, C22.options());
  auto nm_cat = at::empty({F, 4L * K * K, 2L * T * B}, C22.options());
  const long total = (long)F * T * B;
  if (total == 0 || K == 0) return {rhs_cat, nm_cat};  // nothing to write
  TORCH_CHECK(Ts >= 1 && N >= 1, who, ": J holds no solutions");
  TORCH_CHECK(T * B <= INT_MAX / 2 && F <= INT_MAX && Ts <= INT_MAX && N <= INT_MAX
              && (total + 255) / 256 <= INT_MAX,
              who, ": too many samples");
  const dim3 grid((unsigned)((total + 255) / 256));
  const auto* Cp = reinterpret_cast<const c32b*>(C22.data_ptr());
  const auto* Vp = reinterpret_cast<const c32b*>(V22.data_ptr());
  const auto* Jp = reinterpret_cast<const c32b*>(J.data_ptr());
  auto* rhs_p = reinterpret_cast<c32b*>(rhs_cat.data_ptr());
  auto* nm_p = reinterpret_cast<c32b*>(nm_cat.data_ptr());
  if (w) {
    hipLaunchKernelGGL(als_sweep_w_kernel, grid, dim3(256), 0, stream(),
                       Cp, Vp, Jp, w->data_ptr<float>(),
                       p_idx.data_ptr<int>(), q_idx.data_ptr<int>(),
                       t_int.data_ptr<int>(), rhs_p, nm_p,
                       (int)F, (int)K, (int)T, (int)B, (int)N, (int)Ts);
    check_launch("als_sweep_w_kernel");
  } else {
    hipLaunchKernelGGL(als_sweep_kernel, grid, dim3(256), 0, stream(),
                       Cp, Vp, Jp, p_idx.data_ptr<int>(),
                       q_idx.data_ptr<int>(), t_int.data_ptr<int>(), rhs_p,
                       nm_p, (int)F, (int)K, (int)T, (int)B, (int)N, (int)Ts);
    check_launch("als_sweep_kernel");
  }
  return {rhs_cat, nm_cat};
}

std::tuple<at::Tensor, at::Tensor> als_sweep(
    const at::Tensor& C22, const at::Tensor& V22, const at::Tensor& J,
    const at::Tensor& p_idx, const at::Tensor& q_idx,
    const at::Tensor& t_int) {
  return als_sweep_impl("als_sweep", C22, V22, J, nullptr, p_idx, q_idx,
                        t_int);
}

std::tuple<at::Tensor, at::Tensor> als_sweep_w(
    const at::Tensor& C22, const at::Tensor& V22, const at::Tensor& J,
    const at::Tensor& w, const at::Tensor& p_idx, const at::Tensor& q_idx,
    const at::Tensor& t_int) {
  return als_sweep_impl("als_sweep_w", C22, V22, J, &w, p_idx, q_idx, t_int);
}

// Residual r = V - sum_k J_p C_k J_q^H, its squared norm e2, the robust
// weight w = m (nu + 8) / (nu + e2 / sigma2) and the float64 per-block
// partial sums (F, nblk, 4) of m, w e2, w and m (ln w - w), in one launch
// (robust.hip). nu and sigma2 are per-frequency device arrays.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
vis_residual_weights(const at::Tensor& C22, const at::Tensor& V22,
                     const at::Tensor& J, const at::Tensor& m,
                     const at::Tensor& nu, const at::Tensor& sigma2,
                     const at::Tensor& p_idx, const at::Tensor& q_idx,
                     const at::Tensor& t_int) {
  const char* who = "vis_residual_weights";
  check_c64(C22, "C22");
  check_c64(V22, "V22");
  check_c64(J, "J");
  check_f32(m, "m");
  check_f32(nu, "nu");
  check_f32(sigma2, "sigma2");
  TORCH_CHECK(C22.dim() == 6 && C22.size(4) == 2 && C22.size(5) == 2,
              who, ": C22 must be (F, K, T, B, 2, 2), got ", C22.sizes());
  const int64_t F = C22.size(0), K = C22.size(1), T = C22.size(2),
                B = C22.size(3);
  TORCH_CHECK(V22.dim() == 5 && V22.size(0) == F && V22.size(1) == T
              && V22.size(2) == B && V22.size(3) == 2 && V22.size(4) == 2,
              who, ": V22 must be (", F, ", ", T, ", ", B,
              ", 2, 2), got ", V22.sizes());
  TORCH_CHECK(J.dim() == 6 && J.size(0) == F && J.size(2) == K
              && J.size(4) == 2 && J.size(5) == 2,
              who, ": J must be (", F, ", Ts, ", K, ", N, 2, 2), got ",
              J.sizes());
  const int64_t Ts = J.size(1), N = J.size(3);
  TORCH_CHECK(m.dim() == 3 && m.size(0) == F && m.size(1) == T
              && m.size(2) == B, who, ": m must be (", F, ", ", T, ", ", B,
              "), got ", m.sizes());
  TORCH_CHECK(nu.dim() == 1 && nu.size(0) == F, who, ": nu must be (", F,
              ",), got ", nu.sizes());
  TORCH_CHECK(sigma2.dim() == 1 && sigma2.size(0) == F, who,
              ": sigma2 must be (", F, ",), got ", sigma2.sizes());
  check_index(p_idx, at::kInt, B, "p_idx");
  check_index(q_idx, at::kInt, B, "q_idx");
  check_index(t_int, at::kInt, T, "t_int");
  const int64_t TB = T * B, nblk = (TB + 255) / 256;
  auto r = at::empty({F, TB, 4}, C22.options());
  auto e2 = at::empty({F, T, B}, m.options());
  auto w = at::empty({F, T, B}, m.options());
  // every block writes its four sums, so nothing is zeroed beforehand
  auto part = at::empty({F, nblk, 4}, m.options().dtype(at::kDouble));
  if (F == 0 || TB == 0) return {r, e2, w, part};      // nothing to write
  TORCH_CHECK(K == 0 || (Ts >= 1 && N >= 1), who, ": J holds no solutions");
  TORCH_CHECK(F <= 65535, who, " grid limit: F = ", F);
  TORCH_CHECK(TB <= INT_MAX / 2 && K <= INT_MAX && Ts <= INT_MAX
              && N <= INT_MAX, who, ": too many samples");
  hipLaunchKernelGGL(vis_residual_weights_kernel,
                     dim3((unsigned)nblk, (unsigned)F), dim3(256), 0,
                     stream(),
                     reinterpret_cast<const c32b*>(C22.data_ptr()),
                     reinterpret_cast<const c32b*>(V22.data_ptr()),
                     reinterpret_cast<const c32b*>(J.data_ptr()),
                     m.data_ptr<float>(), nu.data_ptr<float>(),
                     sigma2.data_ptr<float>(), p_idx.data_ptr<int>(),
                     q_idx.data_ptr<int>(), t_int.data_ptr<int>(),
                     reinterpret_cast<c32b*>(r.data_ptr()),
                     e2.data_ptr<float>(), w.data_ptr<float>(),
                     part.data_ptr<double>(), (int)K, (int)T, (int)B, (int)N,
                     (int)Ts);
  check_launch("vis_residual_weights_kernel");
  return {r, e2, w, part};
}

// Direct-accumulate variant of fused_linear_bwd_dz: dgamma/dbeta are
// (pre-zeroed) flat-grad views the kernel adds its column sums into
// (fixed summation order, no atomics). Pass None for both when the sums
// are not wanted (frozen parameters): the kernel then skips them.
// Without LayerNorm (with_ln false: zhat, rstd and gamma are not read)
// this is dz = dy * act'(y).
at::Tensor fused_linear_bwd_dz_into(
    const at::Tensor& dy, const at::Tensor& y, const at::Tensor& zhat,
    const at::Tensor& rstd, const c10::optional<at::Tensor>& gamma,
    int64_t act, bool with_ln, const c10::optional<at::Tensor>& dgamma,
    const c10::optional<at::Tensor>& dbeta) {
  // dy may be a column slice of a wider row-major matrix (the critic
  // head's dX, split between the two branches): rows keep unit stride
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kFloat
              && dy.dim() == 2 && (dy.size(1) == 1 || dy.stride(1) == 1)
              && dy.stride(0) >= dy.size(1),
              "dy must be fp32 (B, N) on the GPU with unit column stride");
  check_f32(y, "y");
  const int B = dy.size(0), N = dy.size(1);
  TORCH_CHECK(y.dim() == 2 && y.size(0) == B && y.size(1) == N,
              "dy / y shape mismatch");
  auto dz = at::empty({B, N}, dy.options());
  const bool want_cols = dgamma.has_value();
  TORCH_CHECK(dbeta.has_value() == want_cols,
              "dgamma and dbeta are given together or not at all");
  if (want_cols) {
    check_f32(*dgamma, "dgamma");
    check_f32(*dbeta, "dbeta");
    TORCH_CHECK(dgamma->numel() == N && dbeta->numel() == N,
                "grad views must have N elements");
  }
  hipLaunchKernelGGL(ln_act_bwd_kernel, dim3(B), dim3(256), 0, stream(),
                     dy.data_ptr<float>(), y.data_ptr<float>(),
                     with_ln ? zhat.data_ptr<float>() : nullptr,
                     with_ln ? rstd.data_ptr<float>() : nullptr,
                     gamma ? gamma->data_ptr<float>() : nullptr,
                     dz.data_ptr<float>(),
                     want_cols ? dgamma->data_ptr<float>() : nullptr,
                     want_cols ? dbeta->data_ptr<float>() : nullptr, B, N,
                     (int)act, with_ln ? 1 : 0, (int)dy.stride(0));
  return dz;
}

at::Tensor mfma_gemm_nn(const at::Tensor& A, const at::Tensor& B) {
  check_f32(A, "A");
  check_f32(B, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "gemm_nn takes two matrices");
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K, "gemm_nn shape mismatch");
  auto C = at::empty({M, N}, A.options());
  if (M == 0 || N == 0) return C;
  dim3 grid((M + 15) / 16, (N + 63) / 64);
  hipLaunchKernelGGL(gemm_f32_nn_kernel, grid, dim3(256), 0, stream(),
                     A.data_ptr<float>(), B.data_ptr<float>(),
                     C.data_ptr<float>(), M, K, N);
  check_launch("gemm_f32_nn_kernel");
  return C;
}

std::tuple<at::Tensor, at::Tensor> mfma_gemm_tn_bias(const at::Tensor& dz,
                                                     const at::Tensor& x) {
  check_f32(dz, "dz");
  check_f32(x, "x");
  TORCH_CHECK(dz.dim() == 2 && x.dim() == 2, "gemm_tn takes two matrices");
  const int Bb = dz.size(0), N = dz.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == Bb, "gemm_tn batch mismatch");
  auto dW = at::empty({N, K}, dz.options());
  auto db = at::empty({N}, dz.options());
  if (N == 0) return {dW, db};
  if (K > 0) {
    dim3 grid((N + 15) / 16, (K + 63) / 64);
    hipLaunchKernelGGL(gemm_f32_tn_kernel, grid, dim3(256), 0, stream(),
                       dz.data_ptr<float>(), x.data_ptr<float>(),
                       dW.data_ptr<float>(), nullptr, N, Bb, K, 0);
    check_launch("gemm_f32_tn_kernel");
  }
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0,
                     stream(), dz.data_ptr<float>(), db.data_ptr<float>(),
                     Bb, N, 0);
  check_launch("colsum_kernel");
  return {dW, db};
}

// Direct-accumulate variant: dW/db are views into the (pre-zeroed) flat
// gradient pool — the kernel writes with += and the caller skips
// autograd's per-parameter zero+add kernels entirely. One launch: the
// column sums run as an extra grid row of the GEMM kernel.
void mfma_gemm_tn_bias_into(const at::Tensor& dz, const at::Tensor& x,
                            at::Tensor dW, at::Tensor db) {
  check_f32(dz, "dz");
  check_f32(x, "x");
  check_f32(dW, "dW");
  check_f32(db, "db");
  TORCH_CHECK(dz.dim() == 2 && x.dim() == 2, "gemm_tn takes two matrices");
  const int Bb = dz.size(0), N = dz.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == Bb, "gemm_tn batch mismatch");
  TORCH_CHECK(dW.numel() == (int64_t)N * K && db.numel() == N,
              "grad views must hold N*K and N elements");
  if (N == 0) return;
  dim3 grid((N + 15) / 16, (K + 63) / 64 + 1);
  hipLaunchKernelGGL(gemm_f32_tn_kernel, grid, dim3(256), 0, stream(),
                     dz.data_ptr<float>(), x.data_ptr<float>(),
                     dW.data_ptr<float>(), db.data_ptr<float>(), N, Bb, K,
                     1);
  check_launch("gemm_f32_tn_kernel");
}

// ---- bf16-compute variants (fp32 interfaces, bf16 MFMA inside) ----

std::tuple<at::Tensor, at::Tensor, at::Tensor> fused_linear_bf16_fwd(
    const at::Tensor& x, const at::Tensor& W,
    const c10::optional<at::Tensor>& bias,
    const c10::optional<at::Tensor>& gamma,
    const c10::optional<at::Tensor>& beta, int64_t act, bool with_ln) {
  check_f32(x, "x");
  check_f32(W, "W");
  const int B = x.size(0), K = x.size(1), N = W.size(0);
  TORCH_CHECK(W.size(1) == K, "W/K mismatch");
  TORCH_CHECK(N <= 1536, "fused_linear_bf16: N>1536 unsupported");
  TORCH_CHECK(!with_ln || gamma.has_value(), "LN requires gamma");
  auto y = at::empty({B, N}, x.options());
  auto zhat = with_ln ? at::empty({B, N}, x.options())
                      : at::empty({0}, x.options());
  auto rstd = with_ln ? at::empty({B}, x.options())
                      : at::empty({0}, x.options());
  dim3 grid((B + 15) / 16);
  hipLaunchKernelGGL(fused_linear_bf16_fwd_kernel, grid, dim3(512), 0,
                     stream(), x.data_ptr<float>(), W.data_ptr<float>(),
                     bias ? bias->data_ptr<float>() : nullptr,
                     gamma ? gamma->data_ptr<float>() : nullptr,
                     beta ? beta->data_ptr<float>() : nullptr,
                     y.data_ptr<float>(),
                     with_ln ? zhat.data_ptr<float>() : nullptr,
                     with_ln ? rstd.data_ptr<float>() : nullptr, B, K, N,
                     (int)act, with_ln ? 1 : 0);
  return {y, zhat, rstd};
}

at::Tensor mfma_gemm_nn_bf16(const at::Tensor& A, const at::Tensor& B) {
  check_f32(A, "A");
  check_f32(B, "B");
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K, "gemm_nn shape mismatch");
  auto C = at::empty({M, N}, A.options());
  dim3 grid((M + 15) / 16, (N + 63) / 64);
  hipLaunchKernelGGL(gemm_bf16_nn_kernel, grid, dim3(256), 0, stream(),
                     A.data_ptr<float>(), B.data_ptr<float>(),
                     C.data_ptr<float>(), M, K, N);
  return C;
}

void mfma_gemm_tn_bias_into_bf16(const at::Tensor& dz, const at::Tensor& x,
                                 at::Tensor dW, at::Tensor db) {
  check_f32(dz, "dz");
  check_f32(x, "x");
  const int Bb = dz.size(0), N = dz.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == Bb, "gemm_tn batch mismatch");
  TORCH_CHECK(dW.is_contiguous() && db.is_contiguous(),
              "grad views must be contiguous");
  dim3 grid((N + 15) / 16, (K + 63) / 64);
  hipLaunchKernelGGL(gemm_bf16_tn_kernel, grid, dim3(256), 0, stream(),
                     dz.data_ptr<float>(), x.data_ptr<float>(),
                     dW.data_ptr<float>(), N, Bb, K, 1);
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0,
                     stream(), dz.data_ptr<float>(), db.data_ptr<float>(),
                     Bb, N, 1);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> tanh_gauss_fwd(
    const at::Tensor& mu, const at::Tensor& logsigma, const at::Tensor& eps,
    double max_action) {
  check_f32(mu, "mu");
  check_f32(logsigma, "logsigma");
  check_f32(eps, "eps");
  TORCH_CHECK(mu.dim() == 2, "tanh_gauss_fwd: mu must be (B, A)");
  TORCH_CHECK(logsigma.sizes() == mu.sizes() && eps.sizes() == mu.sizes(),
              "tanh_gauss_fwd: logsigma and eps must have mu's shape");
  const int B = mu.size(0), A = mu.size(1);
  auto action = at::empty_like(mu);
  auto at_ = at::empty_like(mu);
  // a row without actions sums to log-probability 0
  auto logp = A == 0 ? at::zeros({B, 1}, mu.options())
                     : at::empty({B, 1}, mu.options());
  if (B == 0 || A == 0) return {action, logp, at_};
  hipLaunchKernelGGL(tanh_gauss_fwd_kernel, dim3(B), dim3(64), 0, stream(),
                     mu.data_ptr<float>(), logsigma.data_ptr<float>(),
                     eps.data_ptr<float>(), action.data_ptr<float>(),
                     logp.data_ptr<float>(), at_.data_ptr<float>(),
                     (float)max_action, B, A);
  check_launch("tanh_gauss_fwd_kernel");
  return {action, logp, at_};
}

std::tuple<at::Tensor, at::Tensor> tanh_gauss_bwd(
    const at::Tensor& dact, const at::Tensor& dlogp,
    const at::Tensor& logsigma, const at::Tensor& eps, const at::Tensor& at_,
    double max_action) {
  check_f32(dact, "dact");
  check_f32(dlogp, "dlogp");
  check_f32(logsigma, "logsigma");
  check_f32(eps, "eps");
  check_f32(at_, "at");
  TORCH_CHECK(dact.dim() == 2, "tanh_gauss_bwd: dact must be (B, A)");
  TORCH_CHECK(logsigma.sizes() == dact.sizes()
              && eps.sizes() == dact.sizes() && at_.sizes() == dact.sizes(),
              "tanh_gauss_bwd: logsigma, eps and at must have dact's shape");
  const int B = dact.size(0), A = dact.size(1);
  TORCH_CHECK(dlogp.numel() == B, "tanh_gauss_bwd: dlogp must hold B values");
  auto dmu = at::empty_like(dact);
  auto dls = at::empty_like(dact);
  const long n = (long)B * A;
  if (n == 0) return {dmu, dls};
  hipLaunchKernelGGL(tanh_gauss_bwd_kernel, dim3((n + 255) / 256), dim3(256),
                     0, stream(), dact.data_ptr<float>(),
                     dlogp.data_ptr<float>(), logsigma.data_ptr<float>(),
                     eps.data_ptr<float>(), at_.data_ptr<float>(),
                     dmu.data_ptr<float>(), dls.data_ptr<float>(),
                     (float)max_action, B, A);
  check_launch("tanh_gauss_bwd_kernel");
  return {dmu, dls};
}

void fused_adam(at::Tensor& p, const at::Tensor& g, at::Tensor& m,
                at::Tensor& v, at::Tensor& t_dev, double lr, double b1,
                double b2, double eps) {
  check_f32(p, "p");
  check_f32(g, "g");
  check_f32(m, "m");
  check_f32(v, "v");
  check_f32(t_dev, "t_dev");
  const long n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n,
              "fused_adam: g, m and v must hold as many values as p");
  TORCH_CHECK(t_dev.numel() == 1, "fused_adam: t_dev is one step counter");
  if (n == 0) return;  // no parameters, no step: t_dev stays too
  hipLaunchKernelGGL(fused_adam_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     stream(), p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     t_dev.data_ptr<float>(), (float)lr, (float)b1,
                     (float)b2, (float)eps, n);
  check_launch("fused_adam_kernel");
  hipLaunchKernelGGL(adam_bump_kernel, dim3(1), dim3(64), 0, stream(),
                     t_dev.data_ptr<float>());
  check_launch("adam_bump_kernel");
}

// The sampler on the actor head's raw output (B, 2A): slice, clamp and
// sample in one launch. Returns (action, logprob, tanh(z)).
std::tuple<at::Tensor, at::Tensor, at::Tensor> tanh_gauss_head_fwd(
    const at::Tensor& out, const at::Tensor& eps, double max_action,
    double lo, double hi) {
  check_f32(out, "out");
  check_f32(eps, "eps");
  TORCH_CHECK(out.dim() == 2 && out.size(1) % 2 == 0,
              "tanh_gauss_head_fwd: out must be (B, 2A)");
  const int B = out.size(0), A = out.size(1) / 2;
  TORCH_CHECK(eps.dim() == 2 && eps.size(0) == B && eps.size(1) == A,
              "tanh_gauss_head_fwd: eps must be (B, A)");
  auto action = at::empty_like(eps);
  auto at_ = at::empty_like(eps);
  // a row without actions sums to log-probability 0
  auto logp = A == 0 ? at::zeros({B, 1}, out.options())
                     : at::empty({B, 1}, out.options());
  if (B == 0 || A == 0) return {action, logp, at_};
  hipLaunchKernelGGL(tanh_gauss_head_fwd_kernel, dim3(B), dim3(64), 0,
                     stream(), out.data_ptr<float>(), eps.data_ptr<float>(),
                     action.data_ptr<float>(), logp.data_ptr<float>(),
                     at_.data_ptr<float>(), (float)max_action, (float)lo,
                     (float)hi, B, A);
  check_launch("tanh_gauss_head_fwd_kernel");
  return {action, logp, at_};
}

at::Tensor tanh_gauss_head_bwd(const at::Tensor& dact,
                               const at::Tensor& dlogp,
                               const at::Tensor& out, const at::Tensor& eps,
                               const at::Tensor& at_, double max_action,
                               double lo, double hi) {
  check_f32(dact, "dact");
  check_f32(dlogp, "dlogp");
  check_f32(out, "out");
  check_f32(eps, "eps");
  check_f32(at_, "at");
  TORCH_CHECK(dact.dim() == 2, "tanh_gauss_head_bwd: dact must be (B, A)");
  TORCH_CHECK(eps.sizes() == dact.sizes() && at_.sizes() == dact.sizes(),
              "tanh_gauss_head_bwd: eps and at must have dact's shape");
  const int B = dact.size(0), A = dact.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) == 2 * A,
              "tanh_gauss_head_bwd: out must be (B, 2A)");
  TORCH_CHECK(dlogp.numel() == B,
              "tanh_gauss_head_bwd: dlogp must hold B values");
  auto dout = at::empty_like(out);
  const long n = (long)B * A;
  if (n == 0) return dout;
  hipLaunchKernelGGL(tanh_gauss_head_bwd_kernel, dim3((n + 255) / 256),
                     dim3(256), 0, stream(), dact.data_ptr<float>(),
                     dlogp.data_ptr<float>(), out.data_ptr<float>(),
                     eps.data_ptr<float>(), at_.data_ptr<float>(),
                     dout.data_ptr<float>(), (float)max_action, (float)lo,
                     (float)hi, B, A);
  check_launch("tanh_gauss_head_bwd_kernel");
  return dout;
}

// Adam on two equal-sized pools and the polyak update of their targets in
// one launch, then one bump of both step counters.
void fused_adam_polyak2(at::Tensor& p0, const at::Tensor& g0, at::Tensor& m0,
                        at::Tensor& v0, at::Tensor& t0, at::Tensor& tgt0,
                        at::Tensor& p1, const at::Tensor& g1, at::Tensor& m1,
                        at::Tensor& v1, at::Tensor& t1, at::Tensor& tgt1,
                        double lr, double b1, double b2, double eps,
                        double tau) {
  const at::Tensor* all[] = {&p0, &g0, &m0, &v0, &tgt0,
                             &p1, &g1, &m1, &v1, &tgt1};
  const long n = p0.numel();
  for (const at::Tensor* t : all) {
    check_f32(*t, "fused_adam_polyak2 pool");
    TORCH_CHECK(t->numel() == n,
                "fused_adam_polyak2: every pool must hold as many values as "
                "p0");
  }
  check_f32(t0, "t0");
  check_f32(t1, "t1");
  TORCH_CHECK(t0.numel() == 1 && t1.numel() == 1,
              "fused_adam_polyak2: t0 and t1 are one step counter each");
  if (n == 0) return;  // no parameters, no step: the counters stay too
  AdamPolyak2Args a;
  a.P0 = p0.data_ptr<float>();
  a.P1 = p1.data_ptr<float>();
  a.G0 = g0.data_ptr<float>();
  a.G1 = g1.data_ptr<float>();
  a.M0 = m0.data_ptr<float>();
  a.M1 = m1.data_ptr<float>();
  a.V0 = v0.data_ptr<float>();
  a.V1 = v1.data_ptr<float>();
  a.t0 = t0.data_ptr<float>();
  a.t1 = t1.data_ptr<float>();
  a.T0 = tgt0.data_ptr<float>();
  a.T1 = tgt1.data_ptr<float>();
  hipLaunchKernelGGL(fused_adam_polyak2_kernel, dim3((n + 255) / 256, 2),
                     dim3(256), 0, stream(), a, (float)lr, (float)b1,
                     (float)b2, (float)eps, (float)tau, n);
  check_launch("fused_adam_polyak2_kernel");
  hipLaunchKernelGGL(adam_bump2_kernel, dim3(1), dim3(64), 0, stream(),
                     t0.data_ptr<float>(), t1.data_ptr<float>());
  check_launch("adam_bump2_kernel");
}

// A (B, 1) fp32 column of the SAC losses.
inline void check_col(const at::Tensor& t, int64_t B, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == B && t.size(1) == 1, name,
              " must be (", B, ", 1), got ", t.sizes());
}

// A 0-dim or one-element fp32 device scalar (alpha, the loss's gradient).
inline void check_scalar(const at::Tensor& t, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.numel() == 1, name, " must hold one value");
}

// Returns (loss, new_q_value).
std::tuple<at::Tensor, at::Tensor> sac_critic_loss_fwd(
    const at::Tensor& q1, const at::Tensor& q2, const at::Tensor& q1_t,
    const at::Tensor& q2_t, const at::Tensor& logp, const at::Tensor& reward,
    const at::Tensor& done, const at::Tensor& alpha, double gamma) {
  TORCH_CHECK(q1.dim() == 2 && q1.size(0) > 0,
              "sac_critic_loss_fwd: q1 must be (B, 1) with B > 0");
  const int64_t B = q1.size(0);
  check_col(q1, B, "q1");
  check_col(q2, B, "q2");
  check_col(q1_t, B, "q1_t");
  check_col(q2_t, B, "q2_t");
  check_col(logp, B, "logp");
  check_col(reward, B, "reward");
  TORCH_CHECK(done.is_cuda() && done.scalar_type() == at::kBool
              && done.is_contiguous() && done.numel() == B,
              "done must hold B contiguous bools on the GPU");
  check_scalar(alpha, "alpha");
  auto y = at::empty_like(q1);
  auto loss = at::empty({}, q1.options());
  hipLaunchKernelGGL(sac_critic_loss_fwd_kernel, dim3(1), dim3(256), 0,
                     stream(), q1.data_ptr<float>(), q2.data_ptr<float>(),
                     q1_t.data_ptr<float>(), q2_t.data_ptr<float>(),
                     logp.data_ptr<float>(), reward.data_ptr<float>(),
                     done.data_ptr<bool>(), alpha.data_ptr<float>(),
                     (float)gamma, y.data_ptr<float>(),
                     loss.data_ptr<float>(), (int)B);
  check_launch("sac_critic_loss_fwd_kernel");
  return {loss, y};
}

// Returns (dq1, dq2).
std::tuple<at::Tensor, at::Tensor> sac_critic_loss_bwd(
    const at::Tensor& q1, const at::Tensor& q2, const at::Tensor& y,
    const at::Tensor& grad) {
  TORCH_CHECK(q1.dim() == 2 && q1.size(0) > 0,
              "sac_critic_loss_bwd: q1 must be (B, 1) with B > 0");
  const int64_t B = q1.size(0);
  check_col(q1, B, "q1");
  check_col(q2, B, "q2");
  check_col(y, B, "new_q_value");
  check_scalar(grad, "grad");
  auto dq1 = at::empty_like(q1);
  auto dq2 = at::empty_like(q2);
  // mse_loss's backward scales by 2/B, formed in double and cast
  hipLaunchKernelGGL(sac_critic_loss_bwd_kernel, dim3((B + 255) / 256),
                     dim3(256), 0, stream(), q1.data_ptr<float>(),
                     q2.data_ptr<float>(), y.data_ptr<float>(),
                     grad.data_ptr<float>(), (float)(2.0 / (double)B),
                     dq1.data_ptr<float>(), dq2.data_ptr<float>(), (int)B);
  check_launch("sac_critic_loss_bwd_kernel");
  return {dq1, dq2};
}

at::Tensor sac_actor_loss_fwd(const at::Tensor& q1, const at::Tensor& q2,
                              const at::Tensor& logp,
                              const at::Tensor& alpha) {
  TORCH_CHECK(q1.dim() == 2 && q1.size(0) > 0,
              "sac_actor_loss_fwd: q1 must be (B, 1) with B > 0");
  const int64_t B = q1.size(0);
  check_col(q1, B, "q1");
  check_col(q2, B, "q2");
  check_col(logp, B, "logp");
  check_scalar(alpha, "alpha");
  auto loss = at::empty({}, q1.options());
  hipLaunchKernelGGL(sac_actor_loss_fwd_kernel, dim3(1), dim3(256), 0,
                     stream(), q1.data_ptr<float>(), q2.data_ptr<float>(),
                     logp.data_ptr<float>(), alpha.data_ptr<float>(),
                     loss.data_ptr<float>(), (int)B);
  check_launch("sac_actor_loss_fwd_kernel");
  return loss;
}

// Returns (dq1, dq2, dlogp).
std::tuple<at::Tensor, at::Tensor, at::Tensor> sac_actor_loss_bwd(
    const at::Tensor& q1, const at::Tensor& q2, const at::Tensor& alpha,
    const at::Tensor& grad) {
  TORCH_CHECK(q1.dim() == 2 && q1.size(0) > 0,
              "sac_actor_loss_bwd: q1 must be (B, 1) with B > 0");
  const int64_t B = q1.size(0);
  check_col(q1, B, "q1");
  check_col(q2, B, "q2");
  check_scalar(alpha, "alpha");
  check_scalar(grad, "grad");
  auto dq1 = at::empty_like(q1);
  auto dq2 = at::empty_like(q1);
  auto dlogp = at::empty_like(q1);
  // mean's backward divides by B as a product with the float reciprocal
  hipLaunchKernelGGL(sac_actor_loss_bwd_kernel, dim3((B + 255) / 256),
                     dim3(256), 0, stream(), q1.data_ptr<float>(),
                     q2.data_ptr<float>(), alpha.data_ptr<float>(),
                     grad.data_ptr<float>(), 1.0f / (float)B,
                     dq1.data_ptr<float>(), dq2.data_ptr<float>(),
                     dlogp.data_ptr<float>(), (int)B);
  check_launch("sac_actor_loss_bwd_kernel");
  return {dq1, dq2, dlogp};
}

// One replay batch in one launch. idx is not range-checked on the device:
// the caller draws it with randint(0, n), n <= rows, which guarantees it.
void replay_gather(const at::Tensor& idx, const at::Tensor& state_mem,
                   const at::Tensor& new_state_mem,
                   const at::Tensor& action_mem,
                   const at::Tensor& reward_mem,
                   const at::Tensor& terminal_mem, double scale,
                   at::Tensor& out_state, at::Tensor& out_new_state,
                   at::Tensor& out_action, at::Tensor& out_reward,
                   at::Tensor& out_done) {
  check_f32(state_mem, "state_mem");
  check_f32(new_state_mem, "new_state_mem");
  check_f32(action_mem, "action_mem");
  check_f32(reward_mem, "reward_mem");
  check_f32(out_state, "out_state");
  check_f32(out_new_state, "out_new_state");
  check_f32(out_action, "out_action");
  check_f32(out_reward, "out_reward");
  TORCH_CHECK(out_state.dim() >= 1, "replay_gather: out_state must be (B, D)");
  const int64_t B = out_state.size(0);
  check_index(idx, at::kLong, B, "idx");
  TORCH_CHECK(state_mem.dim() >= 1 && state_mem.size(0) > 0,
              "replay_gather: state_mem must have rows");
  const int64_t rows = state_mem.size(0);
  const int64_t D = state_mem.numel() / rows;
  const int64_t A = action_mem.numel() / rows;
  TORCH_CHECK(new_state_mem.numel() == rows * D
              && action_mem.numel() == rows * A
              && reward_mem.numel() == rows && terminal_mem.numel() == rows,
              "replay_gather: the memories must have the same number of rows");
  TORCH_CHECK(terminal_mem.is_cuda() && terminal_mem.scalar_type() == at::kBool
              && terminal_mem.is_contiguous(),
              "terminal_mem must be contiguous bools on the GPU");
  TORCH_CHECK(out_done.is_cuda() && out_done.scalar_type() == at::kBool
              && out_done.is_contiguous() && out_done.numel() == B,
              "out_done must hold B contiguous bools on the GPU");
  TORCH_CHECK(out_state.numel() == B * D && out_new_state.numel() == B * D
              && out_action.numel() == B * A && out_reward.numel() == B,
              "replay_gather: the outputs must be B rows of the memories' "
              "widths");
  if (B == 0) return;
  hipLaunchKernelGGL(replay_gather_kernel, dim3(B), dim3(256), 0, stream(),
                     (const long*)idx.data_ptr<int64_t>(),
                     state_mem.data_ptr<float>(),
                     new_state_mem.data_ptr<float>(),
                     action_mem.data_ptr<float>(),
                     reward_mem.data_ptr<float>(),
                     terminal_mem.data_ptr<bool>(), (float)scale,
                     out_state.data_ptr<float>(),
                     out_new_state.data_ptr<float>(),
                     out_action.data_ptr<float>(),
                     out_reward.data_ptr<float>(),
                     out_done.data_ptr<bool>(), (int)D, (int)A);
  check_launch("replay_gather_kernel");
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> enet_lbfgs_solve(
    const at::Tensor& A, const at::Tensor& y, const at::Tensor& rho,
    int64_t epochs, int64_t max_iter, int64_t history) {
  check_f32(A, "A");
  check_f32(y, "y");
  check_f32(rho, "rho");
  const int E = A.size(0), N = A.size(1), M = A.size(2);
  TORCH_CHECK(N <= 32 && M <= 32, "enet solver supports N,M <= 32");
  TORCH_CHECK(history <= HMAX, "history <= 7");
  auto x = at::empty({E, M}, A.options());
  auto Y = at::empty({E, (long)HMAX, M}, A.options());
  auto S = at::empty({E, (long)HMAX, M}, A.options());
  auto nh = at::empty({E}, A.options().dtype(at::kInt));
  const int lds_floats = N * M + N + 5 * M + N + 2 * HMAX * M + 2 * M
                         + 2 * HMAX + M;
  hipLaunchKernelGGL(enet_lbfgs_solve_kernel, dim3(E), dim3(64),
                     lds_floats * sizeof(float), stream(),
                     A.data_ptr<float>(), y.data_ptr<float>(),
                     rho.data_ptr<float>(), x.data_ptr<float>(),
                     Y.data_ptr<float>(), S.data_ptr<float>(),
                     nh.data_ptr<int>(), E, N, M, (int)epochs, (int)max_iter,
                     (int)history);
  return {x, Y, S, nh};
}

std::tuple<at::Tensor, at::Tensor> enet_influence(
    const at::Tensor& A, const at::Tensor& y, const at::Tensor& x,
    const at::Tensor& Y, const at::Tensor& S, const at::Tensor& nh,
    const at::Tensor& penalty, const at::Tensor& rho) {
  check_f32(A, "A");
  check_f32(rho, "rho");
  const int E = A.size(0), N = A.size(1), M = A.size(2);
  TORCH_CHECK(N <= 32 && M <= 32, "enet influence supports N,M <= 32");
  TORCH_CHECK(rho.numel() == 2 * E, "rho must be (E, 2)");
  auto EE = at::empty({E, N}, A.options());
  auto reward = at::empty({E}, A.options());
  const int lds_floats = N * M + M * N + N * N + 2 * HMAX * M + HMAX * N + N
                         + M + N + HMAX;
  hipLaunchKernelGGL(enet_influence_kernel, dim3(E), dim3(64),
                     lds_floats * sizeof(float), stream(),
                     A.data_ptr<float>(), y.data_ptr<float>(),
                     x.data_ptr<float>(), Y.data_ptr<float>(),
                     S.data_ptr<float>(), nh.data_ptr<int>(),
                     penalty.data_ptr<float>(), rho.data_ptr<float>(),
                     EE.data_ptr<float>(), reward.data_ptr<float>(),
                     E, N, M);
  return {EE, reward};
}

// PER sampling capacity: n fp32 prefix sums must fit in LDS next to the
// scan scratch and weight buffer. 32k priorities = 128 KB of the CU's
// 160 KB — covers every workload config (mem_size <= 16000); larger
// buffers take the torch scan path in python (ops/per.py).
#define PER_LDS_MAX_N 32768
#define PER_MAX_B 4096

std::tuple<at::Tensor, at::Tensor, at::Tensor> per_sample(
    const at::Tensor& priorities, const at::Tensor& u, double beta) {
  check_f32(priorities, "priorities");
  check_f32(u, "u");
  const int64_t n = priorities.numel();
  const int64_t B = u.numel();
  TORCH_CHECK(n >= 1 && n <= PER_LDS_MAX_N,
              "per_sample: n must be in [1, 32768]");
  TORCH_CHECK(B <= PER_MAX_B, "per_sample: B must be in [0, 4096]");
  auto idx = at::empty({B}, priorities.options().dtype(at::kLong));
  auto probs = at::empty({B}, priorities.options());
  auto w = at::empty({B}, priorities.options());
  if (B == 0) return {idx, probs, w};  // no draws: nothing to launch
  const int T = 256;
  const size_t lds = (size_t)(n + T + 1 + B) * sizeof(float);
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(T), lds, stream(),
                     priorities.data_ptr<float>(), u.data_ptr<float>(),
                     idx.data_ptr<long>(), probs.data_ptr<float>(),
                     w.data_ptr<float>(), (int)n, (int)B, (float)beta);
  check_launch("per_sample_kernel");
  return {idx, probs, w};
}

void per_update(at::Tensor& priorities, const at::Tensor& idx,
                const at::Tensor& td, double eps, double alpha,
                double max_priority) {
  check_f32(priorities, "priorities");
  check_f32(td, "td");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kLong
              && idx.is_contiguous(),
              "idx must be contiguous int64 on the GPU");
  const int64_t B = idx.numel();
  TORCH_CHECK(td.numel() == B, "per_update: one td error per index");
  TORCH_CHECK(B <= INT_MAX, "per_update: too many indices");
  if (B == 0) return;  // nothing to update
  TORCH_CHECK(priorities.numel() >= 1, "per_update: empty priority array");
  hipLaunchKernelGGL(per_update_kernel, dim3((unsigned)((B + 255) / 256)),
                     dim3(256), 0, stream(), priorities.data_ptr<float>(),
                     idx.data_ptr<long>(), td.data_ptr<float>(), (int)B,
                     (float)eps, (float)alpha, (float)max_priority);
  check_launch("per_update_kernel");
}

// Batched complex64 GEMM with A broadcast over `rep` consecutive batch
// elements: C[g] = A[g / rep] @ B[g]. The dsolutions hot op.
at::Tensor cgemm_nn_bcast(const at::Tensor& A, const at::Tensor& B,
                          int64_t rep) {
  check_c64(A, "A");
  check_c64(B, "B");
  TORCH_CHECK(A.dim() == 3 && B.dim() == 3,
              "cgemm: A must be (KA, M, K) and B (G, K, N), got ", A.sizes(),
              " and ", B.sizes());
  TORCH_CHECK(rep >= 1, "cgemm: rep must be at least 1, got ", rep);
  const int64_t KA = A.size(0), M = A.size(1), Kd = A.size(2);
  const int64_t G = B.size(0), N = B.size(2);
  TORCH_CHECK(B.size(1) == Kd, "cgemm K mismatch");
  TORCH_CHECK(G == KA * rep, "cgemm batch/rep mismatch");
  TORCH_CHECK(M <= INT_MAX - 64 && Kd <= INT_MAX - 32 && N <= INT_MAX - 16,
              "cgemm: matrix too large");
  // an empty sum is zero
  auto C = Kd == 0 ? at::zeros({G, M, N}, A.options())
                   : at::empty({G, M, N}, A.options());
  if (G == 0 || M == 0 || N == 0 || Kd == 0) return C;
  TORCH_CHECK((N + 15) / 16 <= 65535 && G <= 65535,
              "cgemm grid limits: N = ", N, ", G = ", G);
  dim3 grid((unsigned)((M + 63) / 64), (unsigned)((N + 15) / 16),
            (unsigned)G);
  hipLaunchKernelGGL(cgemm_nn_bcast_kernel, grid, dim3(256), 0, stream(),
                     reinterpret_cast<const float*>(A.data_ptr()),
                     reinterpret_cast<const float*>(B.data_ptr()),
                     reinterpret_cast<float*>(C.data_ptr()),
                     (int)M, (int)Kd, (int)N, (int)G, (int)rep);
  check_launch("cgemm_nn_bcast_kernel");
  return C;
}

// Fused gather + segment-sum (the ALS per-station reduction).
at::Tensor gather_sum(const at::Tensor& in, const at::Tensor& gidx) {
  check_c64(in, "in");
  TORCH_CHECK(gidx.is_cuda() && gidx.scalar_type() == at::kLong
              && gidx.is_contiguous(),
              "gidx must be contiguous int64 on the GPU");
  TORCH_CHECK(in.dim() == 3 && gidx.dim() == 2,
              "gather_sum: in must be (F, X, S) and gidx (G, Cnt), got ",
              in.sizes(), " and ", gidx.sizes());
  const int64_t F = in.size(0), X = in.size(1);
  const long S = in.size(2);
  const int64_t G = gidx.size(0), Cnt = gidx.size(1);
  const long total = (long)F * X * G;
  // an empty sum is zero
  auto out = Cnt == 0 ? at::zeros({F, X, G}, in.options())
                      : at::empty({F, X, G}, in.options());
  if (total == 0 || Cnt == 0) return out;
  TORCH_CHECK(S >= 1, "gather_sum: indices into an empty axis");
  TORCH_CHECK(F <= INT_MAX && X <= INT_MAX && G <= INT_MAX
              && Cnt <= INT_MAX && (total + 3) / 4 <= INT_MAX,
              "gather_sum: too many outputs");
  hipLaunchKernelGGL(gather_sum_kernel,
                     dim3((unsigned)((total + 3) / 4)), dim3(256), 0,
                     stream(), reinterpret_cast<const c32b*>(in.data_ptr()),
                     gidx.data_ptr<long>(),
                     reinterpret_cast<c32b*>(out.data_ptr()), (int)F, (int)X,
                     S, (int)G, (int)Cnt);
  check_launch("gather_sum_kernel");
  return out;
}

// General L-BFGS two-loop for m RHS rows in one launch (N6/N7).
at::Tensor two_loop_apply(const at::Tensor& Y, const at::Tensor& S,
                          const at::Tensor& Q, const at::Tensor& ro,
                          double gamma) {
  check_f32(Y, "Y");
  check_f32(S, "S");
  check_f32(Q, "Q");
  check_f32(ro, "ro");
  TORCH_CHECK(Y.dim() == 2 && S.dim() == 2 && Q.dim() == 2 && ro.dim() == 1,
              "two_loop: Y, S must be (h, n), Q (m, n), ro (h,)");
  const int64_t h = Y.size(0);
  const long n = Y.size(1);
  const int64_t m = Q.size(0);
  TORCH_CHECK(h <= 16, "two_loop: history <= 16");
  TORCH_CHECK(Q.size(1) == n && S.sizes() == Y.sizes(), "shape mismatch");
  TORCH_CHECK(ro.size(0) == h, "two_loop: ro must hold one entry per pair");
  auto R = at::empty_like(Q);
  if (m == 0 || n == 0) return R;  // no right-hand side: nothing to launch
  TORCH_CHECK(m <= INT_MAX, "two_loop: too many right-hand sides");
  hipLaunchKernelGGL(two_loop_kernel, dim3((unsigned)m), dim3(256), 0,
                     stream(), Y.data_ptr<float>(), S.data_ptr<float>(),
                     Q.data_ptr<float>(), R.data_ptr<float>(),
                     ro.data_ptr<float>(), (float)gamma, (int)h, n, (int)m);
  check_launch("two_loop_kernel");
  return R;
}

// Calibration Hessian assembly in one launch (N9).
at::Tensor hessianres(const at::Tensor& C, const at::Tensor& R,
                      const at::Tensor& J, const at::Tensor& p_idx,
                      const at::Tensor& q_idx, int64_t N) {
  check_c64(C, "C");
  check_c64(R, "R");
  check_c64(J, "J");
  TORCH_CHECK(N >= 2 && N <= 32768, "hessianres: N must be in [2, 32768], "
              "got ", N);
  TORCH_CHECK(C.dim() == 3 && C.size(2) == 4,
              "hessianres: C must be (K, T*B, 4), got ", C.sizes());
  const int64_t K = C.size(0);
  const int64_t S = C.size(1);
  const int64_t B = N * (N - 1) / 2;
  TORCH_CHECK(S >= 1 && S % B == 0, "hessianres: ", S,
              " samples are no positive multiple of the ", B, " baselines");
  TORCH_CHECK(S <= INT_MAX / 4, "hessianres: too many samples");
  const int64_t T = S / B;
  TORCH_CHECK((R.dim() == 2 && R.size(0) == 2 * S && R.size(1) == 2)
              || (R.dim() == 3 && R.size(0) == S && R.size(1) == 2
                  && R.size(2) == 2),
              "hessianres: R must be (2*T*B, 2) or (T*B, 2, 2), got ",
              R.sizes());
  TORCH_CHECK((J.dim() == 3 && J.size(0) == K && J.size(1) == 2 * N
               && J.size(2) == 2)
              || (J.dim() == 4 && J.size(0) == K && J.size(1) == N
                  && J.size(2) == 2 && J.size(3) == 2),
              "hessianres: J must be (K, 2N, 2) or (K, N, 2, 2), got ",
              J.sizes());
  check_index(p_idx, at::kInt, B, "p_idx");
  check_index(q_idx, at::kInt, B, "q_idx");
  TORCH_CHECK(K <= 65535, "hessianres grid limit: K = ", K);
  auto H = at::zeros({K, 4 * N, 4 * N}, C.options());
  if (K == 0) return H;
  dim3 grid((unsigned)((B + 3) / 4), (unsigned)K);
  hipLaunchKernelGGL(hessianres_kernel, grid, dim3(64), 0, stream(),
                     reinterpret_cast<const c32h2*>(C.data_ptr()),
                     reinterpret_cast<const c32h2*>(R.data_ptr()),
                     reinterpret_cast<const c32h2*>(J.data_ptr()),
                     p_idx.data_ptr<int>(), q_idx.data_ptr<int>(),
                     reinterpret_cast<c32h2*>(H.data_ptr()),
                     (int)K, (int)N, (int)B, (int)T);
  check_launch("hessianres_kernel");
  // the diagonal blocks hold unscaled sums: scale them once
  const long diag = (long)K * N * 16;
  hipLaunchKernelGGL(hessianres_scale_diag_kernel,
                     dim3((unsigned)((diag + 255) / 256)), dim3(256), 0,
                     stream(), reinterpret_cast<c32h2*>(H.data_ptr()),
                     (int)K, (int)N, (int)B, (int)T);
  check_launch("hessianres_scale_diag_kernel");
  return H;
}

namespace {

// Shared checks of the coherency bindings: uvw (T, 3) f64, the source
// table (S, 11) f64 and the cluster offsets (K+1) int32, all on the GPU.
void check_sky_tables(const at::Tensor& uvw_scaled, const at::Tensor& src,
                      const at::Tensor& off) {
  TORCH_CHECK(uvw_scaled.is_cuda()
              && uvw_scaled.scalar_type() == at::kDouble
              && uvw_scaled.is_contiguous() && uvw_scaled.dim() == 2
              && uvw_scaled.size(1) == 3, "uvw must be f64 contiguous (T, 3)");
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kDouble
              && src.is_contiguous() && src.dim() == 2 && src.size(1) == 11,
              "src table must be f64 contiguous (S, 11)");
  TORCH_CHECK(off.is_cuda() && off.scalar_type() == at::kInt
              && off.is_contiguous() && off.numel() >= 1,
              "offsets must be int32");
}

}  // namespace

// Whole-sky coherency prediction in one launch (N8).
at::Tensor coherency_predict(const at::Tensor& uvw_scaled,
                             const at::Tensor& src, const at::Tensor& off,
                             double fdelta) {
  check_sky_tables(uvw_scaled, src, off);
  const int T = uvw_scaled.size(0);
  const int K = off.numel() - 1;
  TORCH_CHECK(K <= 65535, "coherency grid limit: K = ", K);
  auto C = at::zeros({K, T, 4},
                     uvw_scaled.options().dtype(at::kComplexFloat));
  if (K == 0 || T == 0) return C;
  dim3 grid((T + 255) / 256, K);
  hipLaunchKernelGGL(coherency_kernel, grid, dim3(256), 0, stream(),
                     uvw_scaled.data_ptr<double>(), src.data_ptr<double>(),
                     off.data_ptr<int>(),
                     reinterpret_cast<float*>(C.data_ptr()), fdelta, T,
                     (int)src.size(0), K);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "coherency_kernel launch: ",
              hipGetErrorString(err));
  return C;
}

// Station array-factor table (beam.hip): E (Tt, Sall, N) complex128 for
// elements elem (Tt, N, Ne, 3) f64 meters and sources lmn (Sall, 3) f64;
// scale = 2πf/c. One launch.
at::Tensor station_beam(const at::Tensor& elem, const at::Tensor& lmn,
                        double scale) {
  TORCH_CHECK(elem.is_cuda() && elem.scalar_type() == at::kDouble
              && elem.is_contiguous() && elem.dim() == 4
              && elem.size(3) == 3,
              "elem must be f64 contiguous (Tt, N, Ne, 3) on the GPU");
  TORCH_CHECK(lmn.is_cuda() && lmn.scalar_type() == at::kDouble
              && lmn.is_contiguous() && lmn.dim() == 2 && lmn.size(1) == 3,
              "lmn must be f64 contiguous (Sall, 3) on the GPU");
  const int Tt = elem.size(0), N = elem.size(1), Ne = elem.size(2);
  const int Sall = lmn.size(0);
  TORCH_CHECK(Ne >= 1, "a station needs at least one element");
  TORCH_CHECK(Tt <= 65535 && N <= 65535, "station_beam grid limits: Tt = ",
              Tt, ", N = ", N);
  auto E = at::zeros({Tt, Sall, N},
                     elem.options().dtype(at::kComplexDouble));
  if (Tt == 0 || N == 0 || Sall == 0) return E;
  dim3 grid((Sall + 127) / 128, N, Tt);
  hipLaunchKernelGGL(station_beam_kernel, grid, dim3(128), 0, stream(),
                     elem.data_ptr<double>(), lmn.data_ptr<double>(),
                     reinterpret_cast<double*>(E.data_ptr()), scale, Tt, N,
                     Ne, Sall);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "station_beam_kernel launch: ",
              hipGetErrorString(err));
  return E;
}

namespace {

// Shared checks of the beam consumers: E (Tt, Sall, N) complex128 and the
// baseline tables p, q (B) int32 against T = Tt·B samples.
void check_beam_tables(const at::Tensor& E, const at::Tensor& p,
                       const at::Tensor& q, int64_t T) {
  TORCH_CHECK(E.is_cuda() && E.scalar_type() == at::kComplexDouble
              && E.is_contiguous() && E.dim() == 3,
              "E must be contiguous cdouble (Tt, Sall, N) on the GPU");
  for (const at::Tensor* t : {&p, &q})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt
                && t->is_contiguous() && t->dim() == 1,
                "baseline tables must be int32 (B) on the GPU");
  TORCH_CHECK(p.numel() == q.numel(), "baseline table sizes");
  const int64_t Tt = E.size(0), N = E.size(2), B = p.numel();
  TORCH_CHECK(B == N * (N - 1) / 2, "B = ", B, " baselines for N = ", N,
              " stations");
  TORCH_CHECK(T == Tt * B, "T = ", T, " samples, but Tt·B = ", Tt * B);
}

}  // namespace

// Beam-weighted whole-sky coherency prediction in one launch;
// rows of src index the source axis of E.
at::Tensor coherency_beam_predict(const at::Tensor& uvw_scaled,
                                  const at::Tensor& src,
                                  const at::Tensor& off, double fdelta,
                                  const at::Tensor& E, const at::Tensor& p,
                                  const at::Tensor& q) {
  check_sky_tables(uvw_scaled, src, off);
  const int64_t T = uvw_scaled.size(0);
  check_beam_tables(E, p, q, T);
  TORCH_CHECK(src.size(0) <= E.size(1), "E covers ", E.size(1),
              " sources, src table has ", src.size(0));
  const int K = off.numel() - 1;
  const int Tt = E.size(0), Sall = E.size(1), N = E.size(2);
  const int B = p.numel();
  TORCH_CHECK(Tt <= 65535 && K <= 65535, "coherency_beam grid limits: Tt = ",
              Tt, ", K = ", K);
  auto C = at::zeros({K, T, 4},
                     uvw_scaled.options().dtype(at::kComplexFloat));
  if (K == 0 || T == 0) return C;
  dim3 grid((B + 255) / 256, Tt, K);
  hipLaunchKernelGGL(coherency_beam_kernel, grid, dim3(256), 0, stream(),
                     uvw_scaled.data_ptr<double>(), src.data_ptr<double>(),
                     off.data_ptr<int>(),
                     reinterpret_cast<const double*>(E.data_ptr()),
                     p.data_ptr<int>(), q.data_ptr<int>(),
                     reinterpret_cast<float*>(C.data_ptr()), fdelta, B, Tt,
                     K, N, (int)src.size(0), Sall);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "coherency_beam_kernel launch: ",
              hipGetErrorString(err));
  return C;
}

// Direct-Fourier-sum image cube (dft_image.hip) in one launch: uvw (S, 3)
// f64 metres, vals (F, M, S) complex64 with weights and normalisation
// folded in, fpar (F, 2) f64 rows [f/c, cell]; image centre (lc, mc).
// Returns (F, M, npix, npix) f32. nsplit slices the sample range over
// blockIdx.z (0 = choose for occupancy); more than one slice adds a
// fixed-order reduction launch.
at::Tensor dft_image(const at::Tensor& uvw, const at::Tensor& vals,
                     const at::Tensor& fpar, int64_t npix, double lc,
                     double mc, int64_t nsplit) {
  TORCH_CHECK(uvw.is_cuda() && uvw.scalar_type() == at::kDouble
              && uvw.is_contiguous() && uvw.dim() == 2 && uvw.size(1) == 3,
              "uvw must be f64 contiguous (S, 3) on the GPU");
  TORCH_CHECK(vals.is_cuda() && vals.scalar_type() == at::kComplexFloat
              && vals.is_contiguous() && vals.dim() == 3,
              "vals must be contiguous complex64 (F, M, S) on the GPU");
  TORCH_CHECK(fpar.is_cuda() && fpar.scalar_type() == at::kDouble
              && fpar.is_contiguous() && fpar.dim() == 2
              && fpar.size(1) == 2, "fpar must be f64 contiguous (F, 2)");
  const int64_t S = uvw.size(0), F = vals.size(0), M = vals.size(1);
  TORCH_CHECK(vals.size(2) == S, "vals has ", vals.size(2),
              " samples, uvw has ", S);
  TORCH_CHECK(fpar.size(0) == F, "fpar rows = ", fpar.size(0), ", F = ", F);
  TORCH_CHECK(npix >= 1 && npix <= 16384, "npix = ", npix);
  TORCH_CHECK(F <= 65535 && M <= 65535, "dft_image grid limits: F = ", F,
              ", M = ", M);
  TORCH_CHECK(nsplit >= 0 && nsplit <= 65535, "nsplit = ", nsplit);
  auto out = at::zeros({F, M, npix, npix}, uvw.options().dtype(at::kFloat));
  if (F == 0 || M == 0 || S == 0) return out;
  const int64_t nt = (npix + 15) / 16;
  if (nsplit == 0) {
    // about 8 blocks per CU, at least one LDS chunk of samples per slice
    const int64_t want = (2048 + nt * nt * F - 1) / (nt * nt * F);
    nsplit = std::max<int64_t>(
        1, std::min<int64_t>({want, S / 256, (int64_t)64}));
  }
  at::Tensor part;
  if (nsplit > 1)
    part = at::empty({nsplit, F, M, npix, npix},
                     uvw.options().dtype(at::kDouble));
  dim3 grid((unsigned)(nt * nt), (unsigned)F, (unsigned)nsplit);
  hipLaunchKernelGGL(dft_image_kernel, grid, dim3(256), 0, stream(),
                     uvw.data_ptr<double>(),
                     reinterpret_cast<const float2*>(vals.data_ptr()),
                     fpar.data_ptr<double>(), out.data_ptr<float>(),
                     nsplit > 1 ? part.data_ptr<double>() : nullptr, lc, mc,
                     (long)S, (int)M, (int)npix, (int)F, (int)nsplit);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "dft_image_kernel launch: ",
              hipGetErrorString(err));
  if (nsplit > 1) {
    const long n = out.numel();
    hipLaunchKernelGGL(dft_image_reduce_kernel, dim3((n + 255) / 256),
                       dim3(256), 0, stream(), part.data_ptr<double>(),
                       out.data_ptr<float>(), n, (int)nsplit);
    err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "dft_image_reduce_kernel launch: ",
                hipGetErrorString(err));
  }
  return out;
}

// Shapelet sources of all clusters, added into C in one launch.
// hdr (Ns,12) f64, coff (Ns) i32 offsets into the packed coef (f64),
// clk (Kc) i32 cluster index per grid row, soff (Kc+1) i32 source ranges.
// With a gain table E (Tt, Sall, N) — station_beam, its sources
// sbase..sbase+Ns the shapelet centres in hdr order — and the baseline
// tables p, q, every source is weighted by E_p · conj(E_q).
void shapelet_predict(at::Tensor C, const at::Tensor& uvw_scaled,
                      const at::Tensor& hdr, const at::Tensor& coff,
                      const at::Tensor& coef, const at::Tensor& clk,
                      const at::Tensor& soff, double fdelta,
                      const c10::optional<at::Tensor>& E,
                      const c10::optional<at::Tensor>& p,
                      const c10::optional<at::Tensor>& q, int64_t sbase) {
  TORCH_CHECK(C.is_cuda() && C.scalar_type() == at::kComplexFloat
              && C.is_contiguous() && C.dim() == 3 && C.size(2) == 4,
              "C must be contiguous cfloat (K, T, 4) on the GPU");
  TORCH_CHECK(uvw_scaled.is_cuda()
              && uvw_scaled.scalar_type() == at::kDouble
              && uvw_scaled.is_contiguous() && uvw_scaled.dim() == 2
              && uvw_scaled.size(1) == 3, "uvw must be f64 contiguous (T, 3)");
  TORCH_CHECK(uvw_scaled.size(0) == C.size(1), "uvw / C sample count");
  TORCH_CHECK(hdr.is_cuda() && hdr.scalar_type() == at::kDouble
              && hdr.is_contiguous() && hdr.dim() == 2 && hdr.size(1) == 12,
              "hdr table must be f64 contiguous (Ns, 12)");
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kDouble
              && coef.is_contiguous(), "coef must be f64 contiguous");
  for (const at::Tensor* t : {&coff, &clk, &soff})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt
                && t->is_contiguous(), "index tables must be int32");
  const int Ns = hdr.size(0);
  const int Kc = clk.numel();
  TORCH_CHECK(coff.numel() == Ns && soff.numel() == Kc + 1,
              "index table sizes");
  const int K = C.size(0), T = C.size(1);
  const bool beam = E.has_value();
  TORCH_CHECK(p.has_value() == beam && q.has_value() == beam,
              "a gain table needs both baseline tables, and they need it");
  if (beam) {
    check_beam_tables(*E, *p, *q, T);
    TORCH_CHECK(sbase >= 0 && sbase + Ns <= E->size(1), "E covers ",
                E->size(1), " sources, shapelets need ", sbase, "..",
                sbase + Ns);
  }
  if (Kc == 0 || T == 0) return;
  dim3 grid((T + 127) / 128, Kc);
  if (beam)
    hipLaunchKernelGGL(shapelet_beam_kernel, grid, dim3(128), 0, stream(),
                       uvw_scaled.data_ptr<double>(), hdr.data_ptr<double>(),
                       coff.data_ptr<int>(), coef.data_ptr<double>(),
                       clk.data_ptr<int>(), soff.data_ptr<int>(),
                       reinterpret_cast<float*>(C.data_ptr()), fdelta, T, K,
                       Ns, (long)coef.numel(),
                       reinterpret_cast<const double*>(E->data_ptr()),
                       p->data_ptr<int>(), q->data_ptr<int>(),
                       (int)p->numel(), (int)E->size(2), (int)E->size(1),
                       (int)sbase);
  else
    hipLaunchKernelGGL(shapelet_kernel, grid, dim3(128), 0, stream(),
                       uvw_scaled.data_ptr<double>(), hdr.data_ptr<double>(),
                       coff.data_ptr<int>(), coef.data_ptr<double>(),
                       clk.data_ptr<int>(), soff.data_ptr<int>(),
                       reinterpret_cast<float*>(C.data_ptr()), fdelta, T, K,
                       Ns, (long)coef.numel());
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "shapelet_kernel launch: ",
              hipGetErrorString(err));
}

// Fused small-sequence attention: O = softmax(Q K^T / sqrt(dh)) V in one
// launch per call; A (softmax) returned for backward/inspection.
std::tuple<at::Tensor, at::Tensor> attn_fwd(const at::Tensor& Q,
                                            const at::Tensor& K,
                                            const at::Tensor& V) {
  check_f32(Q, "Q");
  check_f32(K, "K");
  check_f32(V, "V");
  TORCH_CHECK(Q.dim() == 3, "attn_fwd: Q must be (G, T, dh)");
  // one (T, dh) for all three: the kernel has no separate key length
  TORCH_CHECK(K.sizes() == Q.sizes() && V.sizes() == Q.sizes(),
              "attn_fwd: K and V must have Q's shape ", Q.sizes(), ", got ",
              K.sizes(), " and ", V.sizes(), " (python falls back)");
  const int64_t G = Q.size(0);
  const int T = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(T <= 32 && dh <= 96,
              "attn_fwd caps: T <= 32, dh <= 96 (python falls back)");
  TORCH_CHECK(G <= INT_MAX, "attn_fwd: too many groups");
  auto O = at::empty_like(Q);
  auto A = at::empty({G, T, T}, Q.options());
  if (G == 0 || T == 0) return {O, A};
  TORCH_CHECK(dh >= 1, "attn_fwd: dh must be at least 1");
  const int Tp = (T + 15) & ~15;
  const int dp = ((dh + 3) & ~3) + 1;
  const size_t lds = (size_t)(3 * Tp * dp + Tp * (Tp + 1)) * sizeof(float);
  hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)G), dim3(64), lds,
                     stream(), Q.data_ptr<float>(), K.data_ptr<float>(),
                     V.data_ptr<float>(), O.data_ptr<float>(),
                     A.data_ptr<float>(), (int)G, T, dh);
  check_launch("attn_fwd_kernel");
  return {O, A};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> attn_bwd(
    const at::Tensor& dO, const at::Tensor& A, const at::Tensor& Q,
    const at::Tensor& K, const at::Tensor& V) {
  check_f32(dO, "dO");
  check_f32(A, "A");
  check_f32(Q, "Q");
  check_f32(K, "K");
  check_f32(V, "V");
  TORCH_CHECK(Q.dim() == 3, "attn_bwd: Q must be (G, T, dh)");
  TORCH_CHECK(K.sizes() == Q.sizes() && V.sizes() == Q.sizes()
              && dO.sizes() == Q.sizes(),
              "attn_bwd: K, V and dO must have Q's shape ", Q.sizes());
  const int64_t G = Q.size(0);
  const int T = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(A.dim() == 3 && A.size(0) == G && A.size(1) == T
              && A.size(2) == T, "attn_bwd: A must be (G, T, T)");
  TORCH_CHECK(T <= 32 && dh <= 96, "attn_bwd caps: T <= 32, dh <= 96");
  TORCH_CHECK(G <= INT_MAX, "attn_bwd: too many groups");
  auto dQ = at::empty_like(Q);
  auto dK = at::empty_like(Q);
  auto dV = at::empty_like(Q);
  if (G == 0 || T == 0) return {dQ, dK, dV};
  TORCH_CHECK(dh >= 1, "attn_bwd: dh must be at least 1");
  const int Tp = (T + 15) & ~15;
  const int dp = ((dh + 3) & ~3) + 1;
  const size_t lds =
      (size_t)(4 * Tp * dp + 2 * Tp * (Tp + 1) + Tp) * sizeof(float);
  hipLaunchKernelGGL(attn_bwd_kernel, dim3((unsigned)G), dim3(64), lds,
                     stream(), dO.data_ptr<float>(), A.data_ptr<float>(),
                     Q.data_ptr<float>(), K.data_ptr<float>(),
                     V.data_ptr<float>(), dQ.data_ptr<float>(),
                     dK.data_ptr<float>(), dV.data_ptr<float>(), (int)G, T,
                     dh);
  check_launch("attn_bwd_kernel");
  return {dQ, dK, dV};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("fused_linear_fwd", &fused_linear_fwd);
  m.def("fused_linear_bwd_dz", &fused_linear_bwd_dz);
  m.def("mfma_gemm_nn", &mfma_gemm_nn);
  m.def("mfma_gemm_tn_bias", &mfma_gemm_tn_bias);
  m.def("mfma_gemm_tn_bias_into", &mfma_gemm_tn_bias_into);
  m.def("fused_linear_bwd_dz_into", &fused_linear_bwd_dz_into);
  m.def("mlp_chain_fwd", &mlp_chain_fwd, py::arg("x"), py::arg("Ws"),
        py::arg("bs"), py::arg("gammas"), py::arg("betas"), py::arg("acts"),
        py::arg("bf16") = false, py::arg("save") = true);
  m.def("critic_fwd", &critic_fwd, py::arg("state"), py::arg("action"),
        py::arg("Ws"), py::arg("bs"), py::arg("gammas"), py::arg("betas"),
        py::arg("acts"), py::arg("save") = true);
  m.def("als_sweep", &als_sweep);
  m.def("als_sweep_w", &als_sweep_w);
  m.def("vis_residual_weights", &vis_residual_weights);
  m.def("conv2d_k5s2_fwd", &conv2d_k5s2_fwd);
  m.def("conv2d_k5s2_bwd", &conv2d_k5s2_bwd);
  m.def("tanh_gauss_fwd", &tanh_gauss_fwd);
  m.def("tanh_gauss_bwd", &tanh_gauss_bwd);
  m.def("fused_adam", &fused_adam);
  m.def("tanh_gauss_head_fwd", &tanh_gauss_head_fwd);
  m.def("tanh_gauss_head_bwd", &tanh_gauss_head_bwd);
  m.def("fused_adam_polyak2", &fused_adam_polyak2);
  m.def("sac_critic_loss_fwd", &sac_critic_loss_fwd);
  m.def("sac_critic_loss_bwd", &sac_critic_loss_bwd);
  m.def("sac_actor_loss_fwd", &sac_actor_loss_fwd);
  m.def("sac_actor_loss_bwd", &sac_actor_loss_bwd);
  m.def("replay_gather", &replay_gather);
  m.def("enet_lbfgs_solve", &enet_lbfgs_solve);
  m.def("enet_influence", &enet_influence);
  m.def("per_sample", &per_sample);
  m.def("per_update", &per_update);
  m.def("fused_linear_bf16_fwd", &fused_linear_bf16_fwd);
  m.def("mfma_gemm_nn_bf16", &mfma_gemm_nn_bf16);
  m.def("mfma_gemm_tn_bias_into_bf16", &mfma_gemm_tn_bias_into_bf16);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("cgemm_nn_bcast", &cgemm_nn_bcast);
  m.def("coherency_predict", &coherency_predict);
  m.def("shapelet_predict", &shapelet_predict, py::arg("C"),
        py::arg("uvw_scaled"), py::arg("hdr"), py::arg("coff"),
        py::arg("coef"), py::arg("clk"), py::arg("soff"), py::arg("fdelta"),
        py::arg("E") = py::none(), py::arg("p") = py::none(),
        py::arg("q") = py::none(), py::arg("sbase") = 0);
  m.def("station_beam", &station_beam);
  m.def("coherency_beam_predict", &coherency_beam_predict);
  m.def("dft_image", &dft_image, py::arg("uvw"), py::arg("vals"),
        py::arg("fpar"), py::arg("npix"), py::arg("lc"), py::arg("mc"),
        py::arg("nsplit") = 0);
  m.def("hessianres", &hessianres);
  m.def("two_loop_apply", &two_loop_apply);
  m.def("gather_sum", &gather_sum);
}
