"""The agent-side HIP kernels (per.hip, elementwise.hip, attention.hip,
conv2d.hip, gemm_f32.hip) against the float64 oracles of
test_agent_kernel_oracles.py, at their edge shapes (GPU).

Each comparison prints ``ratio <family> <case> <output> <error / bound>``
before it asserts ``<= 1``; docs/TESTING.md records the worst per family.
"""

import numpy as np
import pytest
import torch

from test_agent_kernel_oracles import (
    ADAM_HYPERS, ADAM_SIZES, ATTN_CASES, ATTN_KINDS, CONV_CASES,
    GEMM_NN_CASES, GEMM_TN_CASES, PER_CASES, PER_KINDS, TG_CASES,
    TG_MAX_ACTIONS, U32, adam_eager, adam_inputs, adam_oracle,
    attention_eager, attention_inputs, attention_lengths, attention_oracle,
    conv_inputs, conv_lengths, conv_oracle, f64, gemm_nn_inputs,
    gemm_nn_oracle, gemm_tn_inputs, gemm_tn_oracle, per_delta, per_draws,
    per_index_oracle, per_priorities, per_probs_oracle, per_update_inputs,
    per_update_oracle, per_weights_oracle, per_window_check, product_ratio,
    record, rule_ratio, tanh_gauss_eager, tanh_gauss_inputs,
    tanh_gauss_oracle)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import smartcal_amd.ops as ops
    from smartcal_amd.ops import attention as attn_ops
    from smartcal_amd.ops import per as per_ops
    from smartcal_amd.ops.conv import conv2d_k5s2
    DEV = torch.device("cuda:0")
else:
    DEV = None


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_hip(), "HIP extension must be loaded on a GPU box"


def hold(family, case, figures):
    """Print every (output, ratio) of one case, then assert all <= 1."""
    for name, ratio in figures:
        print(f"ratio {family} {case} {name} {ratio:.4g}")
        record(family, ratio)
    bad = [(name, ratio) for name, ratio in figures if not ratio <= 1.0]
    assert not bad, (family, case, bad)


def by_rule(got, eager, oracle, L):
    return rule_ratio(got, eager, oracle, L)[0]


def gpu(*ts):
    out = tuple(t.to(DEV).contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


# ---------------------------------------------------------------- PER ----

@pytest.mark.parametrize("kind", PER_KINDS)
@pytest.mark.parametrize("n,B", PER_CASES)
def test_per_sample_against_oracles(n, B, kind):
    beta = 0.62
    pri = per_priorities(kind, n, n + B)
    u = per_draws(B, n + B)
    idx_g, probs_g, w_g = ops.ext().per_sample(
        torch.from_numpy(pri).to(DEV), torch.from_numpy(u).to(DEV), beta)
    torch.cuda.synchronize()
    assert idx_g.shape == probs_g.shape == w_g.shape == (B,)
    assert idx_g.dtype == torch.int64
    idx = idx_g.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < n
    # indices: bit for bit the emulated scan, and inside the float64
    # windows whatever the scan order
    outside, away, inside = per_window_check(pri, u, idx)
    print(f"per windows n={n} B={B} {kind}: outside {outside} away {away} "
          f"inside-and-different {inside}")
    assert outside == 0 and away == 0
    assert np.array_equal(idx, per_index_oracle(pri, u))
    # probabilities: PRI[j] / total, off by the rounding of the total only
    ref = per_probs_oracle(pri, idx)
    assert (ref > 0).all()
    rel = np.abs(f64(probs_g) - ref) / ref
    # weights: tolerance rule against importance_weights in fp32
    pri_t = torch.from_numpy(pri)
    eager_w = per_ops.importance_weights(
        pri_t[torch.from_numpy(idx)] / pri_t.sum(), n, beta)
    w64 = per_weights_oracle(pri, idx, beta)
    hold("per_sample", f"n={n},B={B},{kind}",
         [("probs", rel.max() / per_delta(n, 1.0)),
          ("w", by_rule(w_g, eager_w, w64, 1))])
    w = w_g.cpu().numpy()
    assert w.max() == 1.0 and (w > 0).all()
    if kind == "one":
        assert (idx == n // 2).all()
        assert (probs_g.cpu().numpy() == 1.0).all() and (w == 1.0).all()


@pytest.mark.parametrize("alpha", [0.6, 1.0])
@pytest.mark.parametrize("B", [1, 257])
def test_per_update_against_oracle(B, alpha):
    pri, idx, td = per_update_inputs(B)
    got = torch.from_numpy(pri.copy()).to(DEV)
    per_ops.update_priorities(got, torch.from_numpy(idx).to(DEV),
                              torch.from_numpy(td).to(DEV), 0.01, alpha, 1.0)
    eager = torch.from_numpy(pri.copy())
    per_ops.update_priorities(eager, torch.from_numpy(idx),
                              torch.from_numpy(td), 0.01, alpha, 1.0)
    ref = per_update_oracle(pri, idx, td, 0.01, alpha, 1.0)
    hold("per_update", f"B={B},alpha={alpha}",
         [("pri", by_rule(got, eager, ref, 1))])
    untouched = np.setdiff1d(np.arange(len(pri)), idx)
    assert np.array_equal(got.cpu().numpy()[untouched], pri[untouched])


def test_per_bindings_reject_bad_arguments():
    e = ops.ext()
    pri = torch.rand(64, device=DEV)
    u = torch.rand(8, device=DEV)
    with pytest.raises(RuntimeError):
        e.per_sample(pri.double(), u, 0.5)
    with pytest.raises(RuntimeError):
        e.per_sample(torch.rand(32769, device=DEV), u, 0.5)
    with pytest.raises(RuntimeError):
        e.per_sample(pri, torch.rand(4097, device=DEV), 0.5)
    idx = torch.arange(8, device=DEV)
    with pytest.raises(RuntimeError):
        e.per_update(pri, idx, torch.rand(7, device=DEV), 0.01, 0.6, 1.0)
    with pytest.raises(RuntimeError):
        e.per_update(pri, idx.int(), u, 0.01, 0.6, 1.0)
    with pytest.raises(RuntimeError):
        e.per_update(pri, idx.cpu(), u, 0.01, 0.6, 1.0)


# ------------------------------------------------------- tanh-Gaussian ----

def tanh_gauss_gpu(mu, ls, eps, max_action, dact, dlogp):
    mu_g = mu.to(DEV).requires_grad_(True)
    ls_g = ls.to(DEV).requires_grad_(True)
    a, lp = ops.tanh_gauss_sample(mu_g, ls_g, max_action, True,
                                  eps.to(DEV))
    ((a * dact.to(DEV)).sum() + (lp * dlogp.to(DEV)).sum()).backward()
    return a.detach(), lp.detach(), mu_g.grad, ls_g.grad


@pytest.mark.parametrize("max_action", TG_MAX_ACTIONS)
@pytest.mark.parametrize("B,A", TG_CASES)
def test_tanh_gauss_against_oracle(B, A, max_action):
    mu, ls, eps, dact, dlogp = tanh_gauss_inputs(B, A, 100 * B + A)
    ref = tanh_gauss_oracle(mu, ls, eps, max_action, dact, dlogp)
    eager = tanh_gauss_eager(mu, ls, eps, max_action, dact, dlogp)
    got = tanh_gauss_gpu(mu, ls, eps, max_action, dact, dlogp)
    assert got[0].shape == (B, A) and got[1].shape == (B, 1)
    hold("tanh_gauss", f"B={B},A={A},M={max_action}",
         [(name, by_rule(g, e, r, L)) for name, g, e, r, L in zip(
             ("action", "logp", "dmu", "dlogsigma"), got, eager, ref,
             (1, A, 1, 1))])


@pytest.mark.parametrize("max_action", TG_MAX_ACTIONS)
def test_tanh_gauss_saturated(max_action):
    """z = +-12: tanh is 1 to fp32, 1 - at^2 is off by at most one ulp of 1
    against the 1e-6 guard, so each term of logp by 2^-23 / 1e-6 * M."""
    B, A = 4, 70
    g = torch.Generator().manual_seed(1)
    mu = torch.full((B, A), 12.0)
    mu[:, ::2] = -12.0
    ls = torch.randn(B, A, generator=g) - 1.0
    eps = torch.zeros(B, A)
    dact = torch.randn(B, A, generator=g)
    dlogp = torch.randn(B, 1, generator=g)
    a, lp, dmu, dls = tanh_gauss_gpu(mu, ls, eps, max_action, dact, dlogp)
    a64, lp64 = tanh_gauss_oracle(mu, ls, eps, max_action)
    for t in (a, lp, dmu, dls):
        assert bool(torch.isfinite(t).all())
    assert float(a.abs().max()) <= max_action
    err = np.abs(f64(lp) - lp64).max()
    bound = A * 2.0 ** -23 / 1e-6 * max_action
    print(f"tanh_gauss saturated M={max_action}: logp error {err:.4g} "
          f"bound {bound:.4g}")
    assert err <= bound


def test_tanh_gauss_without_reparameterization():
    mu, ls, eps, _, _ = gpu(*tanh_gauss_inputs(7, 130, 3))
    mu.requires_grad_(True)
    a0, lp0 = ops.tanh_gauss_sample(mu, ls, 2.5, True, eps)
    a1, lp1 = ops.tanh_gauss_sample(mu, ls, 2.5, False, eps)
    assert a0.requires_grad and not a1.requires_grad
    assert not lp1.requires_grad
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1)


def test_tanh_gauss_wrapper_input_hygiene():
    mu, ls, eps, _, _ = gpu(*tanh_gauss_inputs(6, 65, 11))
    a0, lp0 = ops.tanh_gauss_sample(mu, ls, 2.5, True, eps)
    eps_t = eps.t().contiguous().t()
    assert not eps_t.is_contiguous() and torch.equal(eps_t, eps)
    a1, lp1 = ops.tanh_gauss_sample(mu, ls, 2.5, True, eps_t)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1)
    a2, lp2 = ops.tanh_gauss_sample(mu, ls, 2.5, True, eps.double())
    assert torch.equal(a0, a2) and torch.equal(lp0, lp2)
    a3, lp3 = ops.tanh_gauss_sample(mu[2], ls[2], 2.5, True, eps[2])
    assert torch.equal(a3.reshape(-1), a0[2])
    assert torch.equal(lp3.reshape(-1), lp0[2])
    # a transposed mu / logsigma too
    mu_t, ls_t = mu.t().contiguous().t(), ls.t().contiguous().t()
    a4, lp4 = ops.tanh_gauss_sample(mu_t, ls_t, 2.5, True, eps)
    assert torch.equal(a0, a4) and torch.equal(lp0, lp4)


def test_tanh_gauss_bindings_reject_bad_arguments():
    e = ops.ext()
    mu, ls, eps, dact, dlogp = gpu(*tanh_gauss_inputs(4, 6, 2))
    for bad in [(mu, ls.double(), eps), (mu, ls, eps.double()),
                (mu, ls, eps.t()), (mu, ls[:, :5], eps),
                (mu, ls, eps[:3]), (mu[0], ls[0], eps[0]),
                (mu, ls, eps.cpu())]:
        with pytest.raises(RuntimeError):
            e.tanh_gauss_fwd(*bad, 1.0)
    _, _, at = e.tanh_gauss_fwd(mu, ls, eps, 1.0)
    for bad in [(dact, dlogp.double(), ls, eps, at),
                (dact, dlogp, ls, eps, at.double()),
                (dact, dlogp[:3], ls, eps, at),
                (dact, dlogp, ls, eps[:, :5], at),
                (dact, dlogp, ls, eps, at[:3]),
                (dact, dlogp, ls.t(), eps, at)]:
        with pytest.raises(RuntimeError):
            e.tanh_gauss_bwd(*bad, 1.0)


# ---------------------------------------------------------------- Adam ----

@pytest.mark.parametrize("resumed", [False, True])
@pytest.mark.parametrize("hypers", ADAM_HYPERS)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_fused_adam_against_oracle(n, hypers, resumed):
    """p, m and v after 3 steps from zero state, or 5 from t = 1000.

    The oracle takes the fp32 values of the hyper-parameters, as the kernel
    does (adam_oracle). Against a float64 Adam at the double values v is
    off by |(1 - fl(beta2)) - (1 - beta2)| / (1 - beta2) of itself, 1.3e-5
    at beta2 = 0.999: the kernel is the exact Adam of beta2 = fl(beta2)."""
    steps = 5 if resumed else 3
    p, m, v, t0, grads = adam_inputs(n, resumed, steps, n)
    ref = adam_oracle(p, m, v, t0, grads, hypers)
    eager = adam_eager(p, m, v, t0, grads, hypers)
    p_g, m_g, v_g = gpu(p.clone(), m.clone(), v.clone())
    t_dev = torch.full((1,), float(t0), device=DEV)
    for k, g in enumerate(grads):
        ops.ext().fused_adam(p_g, g.to(DEV), m_g, v_g, t_dev, *hypers)
        assert float(t_dev) == t0 + k + 1.0
    hold("fused_adam", f"n={n},hypers={hypers},resumed={resumed}",
         [(name, by_rule(g, e, r, 1)) for name, g, e, r in zip(
             "pmv", (p_g, m_g, v_g), eager[:3], ref)])
    # the zero gradient entries left p alone from zero state
    if not resumed:
        assert torch.equal(p_g.cpu()[::7], p[::7])


def test_fused_adam_step_with_weight_decay():
    """FusedAdam.step() on the GPU against its CPU branch."""
    hypers, wd = ADAM_HYPERS[0], 0.01
    p, m, v, t0, grads = adam_inputs(1000, True, 4, 5)
    ref = adam_oracle(p, m, v, t0, grads, hypers, wd)
    eager = adam_eager(p, m, v, t0, grads, hypers, wd)
    got = adam_eager(p, m, v, t0, grads, hypers, wd, device=DEV)
    assert float(got[3]) == t0 + 4.0
    hold("fused_adam", "step,weight_decay",
         [(name, by_rule(g, e, r, 1)) for name, g, e, r in zip(
             "pmv", got[:3], eager[:3], ref)])


def test_fused_adam_rejects_bad_arguments():
    p, g, m, v = (torch.zeros(10, device=DEV) for _ in range(4))
    t_dev = torch.zeros(1, device=DEV)
    hy = ADAM_HYPERS[0]
    for bad in [(p, g.double(), m, v, t_dev), (p, g[:9], m, v, t_dev),
                (p, g, m[::2], v, t_dev), (p, g, m, v.cpu(), t_dev),
                (p, g, m, v, torch.zeros(2, device=DEV)),
                (p, g, m, v, t_dev.double())]:
        with pytest.raises(RuntimeError):
            ops.ext().fused_adam(*bad, *hy)
    assert float(t_dev) == 0.0


# ----------------------------------------------------------- attention ----

def attention_gpu(q, k, v, do):
    q, k, v = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o, a = attn_ops.scaled_dot_product(q, k, v)
    (o * do.to(DEV)).sum().backward()
    return o.detach(), a.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("kind", ATTN_KINDS)
@pytest.mark.parametrize("G,T,dh", ATTN_CASES)
def test_attention_against_oracle(G, T, dh, kind, monkeypatch):
    q, k, v, do = attention_inputs(G, T, dh, kind, 7 * T + dh)
    ref = attention_oracle(q, k, v, do)
    eager = attention_eager(q, k, v, do)
    calls = []
    for name in ("attn_fwd", "attn_bwd"):
        fn = getattr(ops.ext(), name)
        monkeypatch.setattr(
            ops.ext(), name,
            lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1])
    got = attention_gpu(q, k, v, do)
    assert calls == ["attn_fwd", "attn_bwd"]
    assert got[0].shape == (G, T, dh) and got[1].shape == (G, T, T)
    hold("attention", f"G={G},T={T},dh={dh},{kind}",
         [(name, by_rule(g, e, r, L)) for name, g, e, r, L in zip(
             ("O", "A", "dQ", "dK", "dV"), got, eager, ref,
             attention_lengths(T, dh))])
    if kind == "ties":   # equal logits: every weight is 1/T as fp32 has it
        row = got[1][:, T // 2].cpu()
        assert torch.equal(row, torch.full((G, T), 1.0 / T))


@pytest.mark.parametrize("T,dh", [(15, 4), (17, 33)])
def test_attention_through_wrapper_noncontiguous(T, dh):
    """Leading dims (2, 3) from a transpose, as a multi-head layer makes
    them."""
    g = torch.Generator().manual_seed(T)
    q, k, v, do = (torch.randn(2, T, 3, dh, generator=g).transpose(1, 2)
                   for _ in range(4))
    assert not q.is_contiguous()
    flat = [t.contiguous().reshape(6, T, dh) for t in (q, k, v, do)]
    ref = attention_oracle(*flat)
    eager = attention_eager(*flat)
    got = attention_gpu(q, k, v, do)
    assert got[0].shape == (2, 3, T, dh) and got[1].shape == (2, 3, T, T)
    assert got[2].shape == (2, 3, T, dh)
    hold("attention", f"wrapper,T={T},dh={dh}",
         [(name, by_rule(g_.reshape(r.shape), e, r, L))
          for name, g_, e, r, L in zip(("O", "A", "dQ", "dK", "dV"), got,
                                       eager, ref,
                                       attention_lengths(T, dh))])


def test_attention_key_length_of_its_own_falls_back(monkeypatch):
    """T_k = 2 T_q: the element counts divide evenly, and the kernel has
    one T. The wrapper must hand this to _torch_sdp."""
    def no_kernel(*a):
        raise AssertionError("attn_fwd reached with mismatched shapes")
    monkeypatch.setattr(ops.ext(), "attn_fwd", no_kernel)
    g = torch.Generator().manual_seed(4)
    q = torch.randn(2, 3, 8, 16, generator=g).to(DEV)
    k = torch.randn(2, 3, 16, 16, generator=g).to(DEV)
    v = torch.randn(2, 3, 16, 16, generator=g).to(DEV)
    o, a = attn_ops.scaled_dot_product(q, k, v)
    o_ref, a_ref = attn_ops._torch_sdp(q, k, v)
    assert o.shape == (2, 3, 8, 16) and a.shape == (2, 3, 8, 16)
    assert torch.equal(o, o_ref) and torch.equal(a, a_ref)
    O, A = attention_oracle(q.reshape(6, 8, 16), k.reshape(6, 16, 16),
                            v.reshape(6, 16, 16))
    assert np.abs(f64(o).reshape(6, 8, 16) - O).max() <= 64 * U32
    # broadcast leading dims fall back too
    o2, _ = attn_ops.scaled_dot_product(q, k[:1, :, :8], v[:1, :, :8])
    assert o2.shape == (2, 3, 8, 16)


def test_attention_map_gradient_raises():
    q, k, v, _ = gpu(*attention_inputs(2, 5, 4, "randn", 1))
    q.requires_grad_(True)
    _, a = attn_ops.scaled_dot_product(q, k, v)
    with pytest.raises(RuntimeError, match="attention map"):
        a.sum().backward()


def test_attention_bindings_reject_bad_arguments():
    e = ops.ext()
    q, k, v, do = gpu(*attention_inputs(2, 8, 16, "randn", 2))
    k2 = torch.randn(2, 16, 16, device=DEV)
    big_t = torch.randn(2, 33, 16, device=DEV)
    big_d = torch.randn(2, 8, 97, device=DEV)
    for bad in [(q, k2, v), (q, k, k2), (q.double(), k, v),
                (q, k.transpose(1, 2), v), (big_t, big_t, big_t),
                (big_d, big_d, big_d), (q[0], k[0], v[0])]:
        with pytest.raises(RuntimeError):
            e.attn_fwd(*bad)
    _, a = e.attn_fwd(q, k, v)
    a33 = torch.rand(2, 33, 33, device=DEV)
    for bad in [(do, a, q.double(), k, v), (do, a, q, k.cpu(), v),
                (do, a, q, k, v.transpose(1, 2)), (do, a, q, k2, v),
                (do[:, :4], a, q, k, v), (do, a[:, :4], q, k, v),
                (do, a[:1], q, k, v), (do.double(), a, q, k, v),
                (big_t, a33, big_t, big_t, big_t)]:
        with pytest.raises(RuntimeError):
            e.attn_bwd(*bad)


# --------------------------------------------------------- convolution ----

@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,Cin,Cout,H,W", CONV_CASES)
def test_conv2d_k5s2_against_oracle(B, Cin, Cout, H, W, with_bias):
    x, w, b, dy = conv_inputs(B, Cin, Cout, H, W, H * W + Cin)
    b = b if with_bias else None
    ref, absref = conv_oracle(x, w, b, dy)
    x_g = x.to(DEV).requires_grad_(True)
    w_g = w.to(DEV).requires_grad_(True)
    b_g = b.to(DEV).requires_grad_(True) if with_bias else None
    y = conv2d_k5s2(x_g, w_g, b_g)
    dy_g = dy.transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
    assert dy_g.is_contiguous() == dy.is_contiguous()
    leaves = (x_g, w_g) + ((b_g,) if with_bias else ())
    grads = torch.autograd.grad(y, leaves, dy_g)
    got = (y.detach(),) + tuple(grads)
    assert y.shape == ref[0].shape
    hold("conv2d_k5s2", f"{(B, Cin, Cout, H, W)},bias={with_bias}",
         [(name, product_ratio(g, r, a, L)) for name, g, r, a, L in zip(
             ("y", "dx", "dW", "db"), got, ref, absref,
             conv_lengths(B, Cin, Cout, H, W))])
    dx = grads[0]
    if H % 2 == 0:   # the last row and column belong to no window
        assert float(dx[:, :, -1, :].abs().max()) == 0.0
    if W % 2 == 0:
        assert float(dx[:, :, :, -1].abs().max()) == 0.0


def test_conv2d_k5s2_rejects_bad_shapes():
    e = ops.ext()
    w = torch.randn(2, 1, 5, 5, device=DEV)
    for H, W in [(4, 9), (9, 4), (4, 4)]:
        with pytest.raises(RuntimeError):
            conv2d_k5s2(torch.randn(1, 1, H, W, device=DEV), w)
    x = torch.randn(2, 1, 12, 12, device=DEV)
    with pytest.raises(RuntimeError):
        e.conv2d_k5s2_fwd(x, torch.randn(2, 3, 5, 5, device=DEV), None)
    with pytest.raises(RuntimeError):
        e.conv2d_k5s2_fwd(x, w, torch.randn(3, device=DEV))
    for shape in [(2, 2, 5, 4), (2, 2, 4, 5), (2, 1, 4, 4), (1, 2, 4, 4),
                  (2, 2, 16)]:
        with pytest.raises(RuntimeError):
            e.conv2d_k5s2_bwd(torch.randn(*shape, device=DEV), x, w)
    with pytest.raises(RuntimeError):
        e.conv2d_k5s2_bwd(torch.randn(1, 2, 1, 1, device=DEV),
                          torch.randn(1, 1, 4, 4, device=DEV), w)


# ----------------------------------------------------------------- GEMM ---

@pytest.mark.parametrize("M,K,N", GEMM_NN_CASES)
def test_mfma_gemm_nn_against_oracle(M, K, N):
    A, B = gemm_nn_inputs(M, K, N, M + K + N)
    C64, absC = gemm_nn_oracle(A, B)
    C = ops.ext().mfma_gemm_nn(*gpu(A, B))
    assert C.shape == (M, N)
    hold("gemm_f32_nn", f"{(M, K, N)}",
         [("C", product_ratio(C, C64, absC, K))])


@pytest.mark.parametrize("Bb,N,K", GEMM_TN_CASES)
def test_mfma_gemm_tn_bias_against_oracle(Bb, N, K):
    dz, x, dW0, db0 = gemm_tn_inputs(Bb, N, K, Bb + N + K)
    (dW64, db64), (aW, ab) = gemm_tn_oracle(dz, x)
    dz_g, x_g = gpu(dz, x)
    dW, db = ops.ext().mfma_gemm_tn_bias(dz_g, x_g)
    assert dW.shape == (N, K) and db.shape == (N,)
    figures = [("dW", product_ratio(dW, dW64, aW, Bb)),
               ("db", product_ratio(db, db64, ab, Bb))]
    # the accumulating form, onto gradients that are not zero
    (dW64, db64), (aW, ab) = gemm_tn_oracle(dz, x, dW0, db0)
    dW_g, db_g = gpu(dW0.clone(), db0.clone())
    ops.ext().mfma_gemm_tn_bias_into(dz_g, x_g, dW_g, db_g)
    figures += [("dW_into", product_ratio(dW_g, dW64, aW, Bb + 1)),
                ("db_into", product_ratio(db_g, db64, ab, Bb + 1))]
    hold("gemm_f32_tn", f"{(Bb, N, K)}", figures)


def test_gemm_bindings_reject_bad_arguments():
    e = ops.ext()
    A = torch.randn(4, 8, device=DEV)
    for bad in [(A, torch.randn(7, 3, device=DEV)), (A, A.double()),
                (A, torch.randn(3, 8, device=DEV).t()), (A[0], A.t())]:
        with pytest.raises(RuntimeError):
            e.mfma_gemm_nn(*bad)
    with pytest.raises(RuntimeError):
        e.mfma_gemm_tn_bias(A, torch.randn(5, 3, device=DEV))
    with pytest.raises(RuntimeError):
        e.mfma_gemm_tn_bias_into(A, A, torch.zeros(8, 7, device=DEV),
                                 torch.zeros(8, device=DEV))


# ------------------------------------------------------ launch hygiene ----

def _follow_up_gemm():
    A, B = gemm_nn_inputs(17, 65, 65, 9)
    C = ops.ext().mfma_gemm_nn(*gpu(A, B))
    torch.cuda.synchronize()
    C64, absC = gemm_nn_oracle(A, B)
    assert product_ratio(C, C64, absC, 65) <= 1.0


def _follow_up_per_update():
    pri, idx, td = per_update_inputs(257)
    got = torch.from_numpy(pri.copy()).to(DEV)
    ops.ext().per_update(got, torch.from_numpy(idx).to(DEV),
                         torch.from_numpy(td).reshape(-1).to(DEV), 0.01,
                         0.6, 1.0)
    torch.cuda.synchronize()
    ref = per_update_oracle(pri, idx, td, 0.01, 0.6, 1.0)
    assert np.abs(f64(got) - ref).max() <= 8 * U32


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device=DEV, dtype=dtype)


def _empty_per_sample(e):
    idx, probs, w = e.per_sample(torch.rand(9, device=DEV), _z(0), 0.5)
    assert idx.shape == probs.shape == w.shape == (0,)
    assert idx.dtype == torch.int64


def _empty_per_update(e):
    pri = torch.rand(9, device=DEV)
    keep = pri.clone()
    e.per_update(pri, _z(0, dtype=torch.long), _z(0), 0.01, 0.6, 1.0)
    assert torch.equal(pri, keep)


def _empty_tanh_fwd(e):
    a, lp, at = e.tanh_gauss_fwd(_z(0, 3), _z(0, 3), _z(0, 3), 1.0)
    assert a.shape == at.shape == (0, 3) and lp.shape == (0, 1)
    a, lp, at = e.tanh_gauss_fwd(_z(4, 0), _z(4, 0), _z(4, 0), 1.0)
    assert a.shape == (4, 0) and torch.equal(lp, _z(4, 1))


def _empty_tanh_bwd(e):
    dmu, dls = e.tanh_gauss_bwd(_z(0, 3), _z(0, 1), _z(0, 3), _z(0, 3),
                                _z(0, 3), 1.0)
    assert dmu.shape == dls.shape == (0, 3)


def _empty_adam(e):
    t_dev = torch.full((1,), 3.0, device=DEV)
    e.fused_adam(_z(0), _z(0), _z(0), _z(0), t_dev, *ADAM_HYPERS[0])
    assert float(t_dev) == 3.0


def _empty_attn_fwd(e):
    o, a = e.attn_fwd(_z(0, 5, 4), _z(0, 5, 4), _z(0, 5, 4))
    assert o.shape == (0, 5, 4) and a.shape == (0, 5, 5)
    o, a = attn_ops.scaled_dot_product(_z(2, 0, 5, 4), _z(2, 0, 5, 4),
                                       _z(2, 0, 5, 4))
    assert o.shape == (2, 0, 5, 4) and a.shape == (2, 0, 5, 5)


def _empty_attn_bwd(e):
    grads = e.attn_bwd(_z(0, 5, 4), _z(0, 5, 5), _z(0, 5, 4), _z(0, 5, 4),
                       _z(0, 5, 4))
    assert all(g.shape == (0, 5, 4) for g in grads)


def _empty_conv_fwd(e):
    y = e.conv2d_k5s2_fwd(_z(0, 3, 12, 17), _z(5, 3, 5, 5), None)
    assert y.shape == (0, 5, 4, 7)
    y = e.conv2d_k5s2_fwd(_z(2, 3, 12, 17), _z(0, 3, 5, 5), None)
    assert y.shape == (2, 0, 4, 7)


def _empty_conv_bwd(e):
    w = torch.randn(5, 3, 5, 5, device=DEV)
    dx, dW, db = e.conv2d_k5s2_bwd(_z(0, 5, 4, 7), _z(0, 3, 12, 17), w)
    assert dx.shape == (0, 3, 12, 17)
    assert torch.equal(dW, torch.zeros_like(w)) and torch.equal(db, _z(5))
    x = torch.randn(2, 3, 12, 17, device=DEV)
    dx, dW, db = e.conv2d_k5s2_bwd(_z(2, 0, 4, 7), x, _z(0, 3, 5, 5))
    assert torch.equal(dx, torch.zeros_like(x))
    assert dW.shape == (0, 3, 5, 5) and db.shape == (0,)


def _empty_gemm_nn(e):
    assert e.mfma_gemm_nn(_z(0, 8), _z(8, 5)).shape == (0, 5)
    assert e.mfma_gemm_nn(_z(4, 8), _z(8, 0)).shape == (4, 0)
    # an empty sum is zero
    assert torch.equal(e.mfma_gemm_nn(_z(4, 0), _z(0, 5)), _z(4, 5))


def _empty_gemm_tn(e):
    dW, db = e.mfma_gemm_tn_bias(_z(6, 0), _z(6, 8))
    assert dW.shape == (0, 8) and db.shape == (0,)
    dz = torch.randn(6, 3, device=DEV)
    dW, db = e.mfma_gemm_tn_bias(dz, _z(6, 0))
    assert dW.shape == (3, 0)
    assert np.abs(f64(db) - f64(dz).sum(0)).max() <= 8 * U32 * 6
    dW, db = e.mfma_gemm_tn_bias(_z(0, 3), _z(0, 8))
    assert torch.equal(dW, _z(3, 8)) and torch.equal(db, _z(3))


def _empty_gemm_tn_into(e):
    e.mfma_gemm_tn_bias_into(_z(6, 0), _z(6, 8), _z(0, 8), _z(0))
    dW, db = torch.ones(3, 8, device=DEV), torch.ones(3, device=DEV)
    e.mfma_gemm_tn_bias_into(_z(0, 3), _z(0, 8), dW, db)
    assert torch.equal(dW, torch.ones(3, 8, device=DEV))
    assert torch.equal(db, torch.ones(3, device=DEV))


EMPTY_CALLS = [_empty_per_sample, _empty_per_update, _empty_tanh_fwd,
               _empty_tanh_bwd, _empty_adam, _empty_attn_fwd,
               _empty_attn_bwd, _empty_conv_fwd, _empty_conv_bwd,
               _empty_gemm_nn, _empty_gemm_tn, _empty_gemm_tn_into]


@pytest.mark.parametrize("empty", EMPTY_CALLS, ids=lambda f: f.__name__[7:])
def test_empty_call_launches_nothing_and_leaves_no_error(empty):
    """An empty call returns its correctly shaped or unchanged result, and
    the next binding, another one, runs and is right: no zero-block launch
    left its error behind."""
    empty(ops.ext())
    torch.cuda.synchronize()
    if "gemm" in empty.__name__:
        _follow_up_per_update()
    else:
        _follow_up_gemm()
