"""Fused Linear(+LayerNorm)(+ELU) — the actor/critic MLP hot op (N1).

The reference's MLP layers are ``F.elu(LayerNorm(Linear(x)))`` chains
(reference ``elasticnet/enet_sac.py:436-444`` actor, ``:382-394`` critic).
Here the whole layer is ONE CDNA4 HIP kernel on the forward path: an
MFMA(f32)-tiled GEMM with LDS-staged X/W tiles whose epilogue computes the
row mean/variance with wave ``shfl_xor`` reductions and applies the affine
LayerNorm + ELU before a single store — no separate normalisation kernel, no
extra HBM round-trip for the pre-activations (gfx950 has exact f32-input MFMA
at the f32 vector rate; there is no TF32 on CDNA4).

Backward is three kernels: (1) ELU'+LayerNorm backward with fused
dgamma/dbeta column reductions, (2) dX = dZ @ W, (3) dW = dZ^T @ X + db —
both MFMA f32 GEMMs. (1) is skipped for a head without LayerNorm and
activation (dz is dy), (2) for a first layer whose input needs no gradient.

``fused_chain`` runs a stack of layers, and ``fused_critic`` the whole
critic (two branches and the head over their concatenation), as one kernel
launch each; forwards that nothing will differentiate store only their
final output.

CPU tensors run the equivalent torch composition (also the test oracle).

CONTRACT RESTRICTION (deliberate): on the HIP path the backward
accumulates parameter gradients straight into ``.grad`` (the agents' flat
gradient pools) and returns ``None`` for the W/b/gamma/beta grad outputs.
This removes every per-parameter AccumulateGrad/zero kernel from the
learn graph, but it means ``torch.autograd.grad(loss, params)`` and
double-backward (``create_graph=True`` — e.g.
``autograd_tools.hessian_vec_prod``) are NOT supported through the HIP
fused path; influence/HVP tooling uses plain ``nn.Linear`` models, which
is what every in-repo consumer of ``autograd_tools`` does. The CPU path
has no such restriction.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ext, use_hip

ACT_NONE = 0
ACT_ELU = 1
ACT_RELU = 2
ACT_TANH = 3

_ACT_CODES = {"none": ACT_NONE, "elu": ACT_ELU, "relu": ACT_RELU,
              "tanh": ACT_TANH}

# Process-wide compute dtype for the fused-linear family ("fp32" | "bf16").
# bf16 keeps fp32 master weights, fp32 tensors and fp32 LayerNorm/epilogue;
# only the GEMM multiplies run on the bf16 MFMA pipe
# (v_mfma_f32_16x16x32_bf16, fp32 accumulate) — BASELINE config 2.
_COMPUTE_DTYPE = "fp32"


def set_compute_dtype(dtype: str) -> None:
    global _COMPUTE_DTYPE
    assert dtype in ("fp32", "bf16"), dtype
    _COMPUTE_DTYPE = dtype


def get_compute_dtype() -> str:
    return _COMPUTE_DTYPE


def _grad_view(p: torch.Tensor) -> torch.Tensor:
    """The tensor the kernels accumulate this parameter's gradient into.

    Agents bind each parameter's .grad to a slice of one flat pool
    (``utils.flatten.FlatParams``), so the backward kernels can write
    with += directly — no per-parameter autograd zero/add kernels in the
    learn graph. Standalone tensors (tests) get a zeroed .grad created
    on first use, which matches autograd's accumulate semantics.
    """
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def _needs_graph(*tensors) -> bool:
    """True iff autograd will record an op over these inputs. When it
    will not, the forward bindings skip every tensor only backward reads."""
    return torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in tensors)


def _layers_backward(dy, x, ys, zhats, rstds, params, acts, wants,
                     need_dx: bool, bf16: bool):
    """Backward of a stack of fused layers, last layer first.

    ``params`` is [W, b, gamma, beta] per layer (gamma None: no
    LayerNorm), ``wants[l]`` whether layer l's parameter gradients are
    accumulated (False: frozen). Returns d/dx, or None when ``need_dx`` is
    False — the first layer's dX GEMM is then not launched at all.
    ``dy`` may be a column slice of a wider contiguous matrix (the
    backward-dz kernel takes a row stride).
    """
    e = ext()
    for l in range(len(acts) - 1, -1, -1):
        if not need_dx and not any(wants[:l + 1]):
            # nothing below consumes a gradient (frozen layers under an
            # input without grad): no kernel at all
            return None
        W, b, g, be = params[4 * l:4 * l + 4]
        if g is not None:
            # grads not wanted (frozen params): no dgamma/dbeta sums
            dz = e.fused_linear_bwd_dz_into(
                dy, ys[l], zhats[l], rstds[l], g, acts[l], True,
                _grad_view(g) if wants[l] else None,
                _grad_view(be) if wants[l] else None)
        elif acts[l] == ACT_NONE:
            # no LayerNorm, no activation: identity, no kernel
            dz = dy.contiguous()
        else:
            dz = e.fused_linear_bwd_dz_into(
                dy, ys[l], zhats[l], rstds[l], None, acts[l], False,
                None, None)
        if wants[l]:
            # dW = dz^T @ x and db = col-sum(dz), accumulated straight
            # into the flat gradient pool by the kernel
            x_l = x if l == 0 else ys[l - 1]
            if bf16:
                e.mfma_gemm_tn_bias_into_bf16(dz, x_l, _grad_view(W),
                                              _grad_view(b))
            else:
                e.mfma_gemm_tn_bias_into(dz, x_l, _grad_view(W),
                                         _grad_view(b))
        if l == 0 and not need_dx:
            return None
        # (B,N) @ (N,K) -> (B,K)
        dy = e.mfma_gemm_nn_bf16(dz, W) if bf16 else e.mfma_gemm_nn(dz, W)
    return dy


class _FusedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, gamma, beta, act_code: int, with_ln: bool):
        bf16 = _COMPUTE_DTYPE == "bf16"
        fwd = ext().fused_linear_bf16_fwd if bf16 \
            else ext().fused_linear_fwd
        y, zhat, rstd = fwd(x, W, b, gamma, beta, act_code, with_ln)
        ctx.save_for_backward(x, zhat, rstd, y)
        # python refs to the parameter objects for direct grad
        # accumulation (not part of the autograd graph)
        ctx.param_refs = (W, b, gamma if with_ln else None,
                          beta if with_ln else None)
        ctx.act_code = act_code
        ctx.bf16 = bf16
        return y

    @staticmethod
    def backward(ctx, dy):
        x, zhat, rstd, y = ctx.saved_tensors
        dx = _layers_backward(
            dy.contiguous(), x, (y,), (zhat,), (rstd,), ctx.param_refs,
            (ctx.act_code,), (ctx.needs_input_grad[1],),
            ctx.needs_input_grad[0], ctx.bf16)
        return dx, None, None, None, None, None, None


def fused_linear(x: torch.Tensor, W: torch.Tensor,
                 b: Optional[torch.Tensor] = None,
                 gamma: Optional[torch.Tensor] = None,
                 beta: Optional[torch.Tensor] = None,
                 act: str = "none") -> torch.Tensor:
    """y = act(LayerNorm(x @ W.T + b; gamma, beta)).

    LayerNorm is applied iff gamma is not None. ``x``: (B, K) or (K,);
    ``W``: (N, K). fp32.
    """
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    with_ln = gamma is not None
    act_code = _ACT_CODES[act]
    if use_hip(x):
        y = _FusedLinearFn.apply(x.contiguous(), W, b, gamma, beta,
                                 act_code, with_ln)
    else:
        z = F.linear(x, W, b)
        if with_ln:
            z = F.layer_norm(z, (W.shape[0],), gamma, beta)
        if act == "elu":
            z = F.elu(z)
        elif act == "relu":
            z = F.relu(z)
        elif act == "tanh":
            z = torch.tanh(z)
        y = z
    return y.squeeze(0) if squeeze else y


class FusedLinear(torch.nn.Module):
    """Linear(+LayerNorm)(+activation) module over the fused kernel.

    Weight/bias init follows the reference's fan-based uniform init
    (``enet_sac.py:18-22``: sc = 1/sqrt(weight.size(0)) unless given).
    """

    def __init__(self, in_features: int, out_features: int,
                 ln: bool = True, act: str = "elu",
                 init_scale: Optional[float] = None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.act = act
        sc = init_scale if init_scale is not None else 1.0 / (out_features ** 0.5)
        self.weight = torch.nn.Parameter(
            torch.empty(out_features, in_features).uniform_(-sc, sc))
        self.bias = torch.nn.Parameter(
            torch.empty(out_features).uniform_(-sc, sc))
        if ln:
            self.ln_weight = torch.nn.Parameter(torch.ones(out_features))
            self.ln_bias = torch.nn.Parameter(torch.zeros(out_features))
        else:
            self.register_parameter("ln_weight", None)
            self.register_parameter("ln_bias", None)

    def forward(self, x):
        return fused_linear(x, self.weight, self.bias,
                            self.ln_weight, self.ln_bias, self.act)

    def extra_repr(self):
        return (f"in={self.in_features}, out={self.out_features}, "
                f"ln={self.ln_weight is not None}, act={self.act}")


def _split_params(params, L):
    return ([params[4 * l + 0] for l in range(L)],
            [params[4 * l + 1] for l in range(L)],
            [params[4 * l + 2] for l in range(L)],
            [params[4 * l + 3] for l in range(L)])


def _layer_params(layers):
    params = []
    for m in layers:
        params += [m.weight, m.bias, m.ln_weight, m.ln_bias]
    return params


class _FusedChainFn(torch.autograd.Function):
    """Whole-chain forward (one kernel) with per-layer direct-accumulate
    backward. flat params layout: [W, b, gamma, beta] per layer (gamma and
    beta None for a layer without LayerNorm)."""

    @staticmethod
    def forward(ctx, x, acts, *params):
        L = len(acts)
        Ws, bs, gs, bes = _split_params(params, L)
        bf16 = _COMPUTE_DTYPE == "bf16"
        ys, zhats, rstds = ext().mlp_chain_fwd(
            x, Ws, bs, gs, bes, [int(a) for a in acts], bf16)
        ctx.save_for_backward(x, *ys, *zhats, *rstds)
        ctx.param_refs = params
        ctx.acts = acts
        ctx.L = L
        ctx.bf16 = bf16
        return ys[-1]

    @staticmethod
    def backward(ctx, dy):
        L = ctx.L
        saved = ctx.saved_tensors
        dx = _layers_backward(
            dy.contiguous(), saved[0], saved[1:1 + L],
            saved[1 + L:1 + 2 * L], saved[1 + 2 * L:1 + 3 * L],
            ctx.param_refs, ctx.acts,
            [ctx.needs_input_grad[2 + 4 * l] for l in range(L)],
            ctx.needs_input_grad[0], ctx.bf16)
        return (dx, None) + (None,) * (4 * L)


def fused_chain(x: torch.Tensor, layers) -> torch.Tensor:
    """Run a stack of FusedLinear layers as ONE kernel on GPU (activations
    stay in LDS between layers); CPU falls back to the per-layer path.
    Every layer but the last has LayerNorm; the last may be a plain head
    (fp32 compute only)."""
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    if use_hip(x) and 2 <= len(layers) <= 4 \
            and all(m.ln_weight is not None for m in layers[:-1]) \
            and (layers[-1].ln_weight is not None
                 or _COMPUTE_DTYPE == "fp32"):
        acts = tuple(_ACT_CODES[m.act] for m in layers)
        params = _layer_params(layers)
        x = x.contiguous()
        if _COMPUTE_DTYPE == "fp32" and not _needs_graph(x, *params):
            # nothing to differentiate: only the output is stored
            Ws, bs, gs, bes = _split_params(params, len(layers))
            ys, _, _ = ext().mlp_chain_fwd(x, Ws, bs, gs, bes, list(acts),
                                           False, False)
            y = ys[0]
        else:
            y = _FusedChainFn.apply(x, acts, *params)
    else:
        y = x
        for m in layers:
            y = m(y)
    return y.squeeze(0) if squeeze else y


class _FusedCriticFn(torch.autograd.Function):
    """Critic forward as one kernel: state branch (s1, s2), action branch
    (a1, a2) and the head over their concatenation. Backward runs the
    per-layer kernels of the composed critic, accumulating parameter
    gradients into the flat pools. params: [W, b, gamma, beta] for s1, s2,
    a1, a2, head (the head has no LayerNorm: gamma and beta None)."""

    @staticmethod
    def forward(ctx, state, action, acts, *params):
        Ws, bs, gs, bes = _split_params(params, 5)
        q, zcat, ys, zhats, rstds = ext().critic_fwd(
            state, action, Ws, bs, gs, bes, [int(a) for a in acts], True)
        ctx.save_for_backward(state, action, zcat, q, *ys, *zhats, *rstds)
        ctx.param_refs = params
        ctx.acts = acts
        return q

    @staticmethod
    def backward(ctx, dq):
        saved = ctx.saved_tensors
        state, action, zcat, q = saved[:4]
        ys, zhats, rstds = saved[4:8], saved[8:12], saved[12:16]
        params, acts = ctx.param_refs, ctx.acts
        wants = [ctx.needs_input_grad[3 + 4 * l] for l in range(5)]
        empty = zhats[0].new_empty(0)
        dz = _layers_backward(dq.contiguous(), zcat, (q,), (empty,),
                              (empty,), params[16:20], acts[4:5],
                              wants[4:5], True, False)
        # the two branches read their column ranges of the head's dX in
        # place (no copies as after a torch.cat)
        ns = ys[1].shape[1]
        dstate = _layers_backward(
            dz[:, :ns], state, ys[0:2], zhats[0:2], rstds[0:2],
            params[0:8], acts[0:2], wants[0:2], ctx.needs_input_grad[0],
            False)
        daction = _layers_backward(
            dz[:, ns:], action, ys[2:4], zhats[2:4], rstds[2:4],
            params[8:16], acts[2:4], wants[2:4], ctx.needs_input_grad[1],
            False)
        return (dstate, daction, None) + (None,) * 20


def fused_critic(state: torch.Tensor, action: torch.Tensor,
                 layers) -> torch.Tensor:
    """q = head(cat(s2(s1(state)), a2(a1(action)))) for the FusedLinear
    layers (s1, s2, a1, a2, head) in ONE kernel. HIP fp32 path only: the
    caller composes the layers itself on CPU or with bf16 compute."""
    assert use_hip(state) and _COMPUTE_DTYPE == "fp32"
    squeeze = state.dim() == 1
    if squeeze:
        state = state.unsqueeze(0)
        action = action.unsqueeze(0)
    acts = tuple(_ACT_CODES[m.act] for m in layers)
    params = _layer_params(layers)
    state = state.contiguous()
    action = action.contiguous()
    if not _needs_graph(state, action, *params):
        Ws, bs, gs, bes = _split_params(params, 5)
        q = ext().critic_fwd(state, action, Ws, bs, gs, bes, list(acts),
                             False)[0]
    else:
        q = _FusedCriticFn.apply(state, action, acts, *params)
    return q.squeeze(0) if squeeze else q
