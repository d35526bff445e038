"""Float64 oracles of the agent-side kernels (prioritized replay,
tanh-Gaussian sampling, fused Adam, fused attention, k5/s2 convolution,
fp32 GEMMs), the tolerance rule that ties a kernel to them, and the tests
that validate the oracles on the CPU. test_gpu_agent_kernels.py imports
the oracles and the case lists from here and holds the kernels to them.

Tolerance rule (``rule_ratio``): every oracle is float64 evaluated on the
fp32 inputs; a kernel's largest error against it may be at most four times
the largest error of the project's own fp32 eager path on the same inputs,
plus a floor of L * 2^-24 * max|oracle| (L the reduction length, 1 for an
elementwise op). GEMM and convolution use the per-element bound
``(L + 2) * 2^-24 * (|A| . |B|)`` instead (``product_ratio``), which any
correct fp32 summation order meets and a dropped, doubled or misplaced
term does not.
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from smartcal_amd.ops import attention as attn_ops
from smartcal_amd.ops import per as per_ops
from smartcal_amd.ops.conv import conv2d_k5s2
from smartcal_amd.ops.sampling import tanh_gauss_sample
from smartcal_amd.utils.flatten import FlatParams, FusedAdam

U32 = 2.0 ** -24          # unit roundoff of fp32
RATIOS = {}               # kernel family -> worst error / bound seen


def record(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))
    return ratio


def f64(t):
    """numpy float64 copy of a tensor or array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def rule_ratio(got, eager, oracle, L):
    """kernel error / (4 * eager error + L * 2^-24 * max|oracle|), and the
    three figures it is made of."""
    got, eager, oracle = f64(got), f64(eager), f64(oracle)
    assert got.shape == oracle.shape == eager.shape, (got.shape,
                                                      eager.shape,
                                                      oracle.shape)
    if oracle.size == 0:
        return 0.0, 0.0, 0.0, 0.0
    err = float(np.max(np.abs(got - oracle)))
    err_eager = float(np.max(np.abs(eager - oracle)))
    bound = 4.0 * err_eager + L * U32 * float(np.max(np.abs(oracle)))
    if bound == 0.0:
        return (0.0 if err == 0.0 else math.inf), err, err_eager, bound
    return err / bound, err, err_eager, bound


def product_ratio(got, oracle, absprod, L):
    """max over elements of |got - oracle| / ((L + 2) 2^-24 absprod)."""
    got, oracle, absprod = f64(got), f64(oracle), f64(absprod)
    assert got.shape == oracle.shape == absprod.shape, (got.shape,
                                                        oracle.shape)
    if oracle.size == 0:
        return 0.0
    err = np.abs(got - oracle)
    bound = (L + 2) * U32 * absprod
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0),
                     np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


# ---------------------------------------------------------------- PER ----

PER_CASES = [(1, 8), (255, 7), (256, 256), (257, 64), (4099, 256),
             (16000, 256), (32768, 1), (32768, 4096)]
PER_KINDS = ["integer", "real", "equal", "one"]
PER_THREADS = 256


def per_priorities(kind, n, seed):
    """fp32 priority array of one of the four classes."""
    rng = np.random.default_rng(seed)
    if kind == "integer":     # exact partial sums, zero-priority runs
        pri = rng.integers(1, 11, n).astype(np.float32)
        pri[rng.random(n) < 0.2] = 0.0
    elif kind == "real":      # what update_priorities writes
        td = rng.standard_normal(n).astype(np.float32) * np.float32(2)
        pri = np.minimum(np.abs(td) + np.float32(0.01),
                         np.float32(1)) ** np.float32(0.6)
        pri = pri.astype(np.float32)
        pri[rng.random(n) < 0.2] = 0.0
        run = n // 16
        if run:               # a leading and a trailing run of zeros
            pri[:run] = 0.0
            pri[-run:] = 0.0
    elif kind == "equal":
        pri = np.full(n, 0.37, dtype=np.float32)
    elif kind == "one":
        pri = np.zeros(n, dtype=np.float32)
        pri[n // 2] = 0.37
    else:
        raise ValueError(kind)
    if not pri.any():
        pri[n // 2] = 1.0
    return pri


def per_draws(B, seed):
    """fp32 uniforms in [2^-24, 1)."""
    rng = np.random.default_rng(seed + 7919)
    u = rng.random(B).astype(np.float32)
    return np.clip(u, np.float32(U32), np.float32(1.0 - U32))


def per_scan_emulation(pri):
    """fp32 emulation of per_sample_kernel's three-phase scan: (inclusive
    prefix sums, total). 256 contiguous chunks of ceil(n/256) entries are
    summed sequentially, the chunk totals exclusive-scanned sequentially,
    the offsets added back."""
    pri = np.asarray(pri, dtype=np.float32)
    n = pri.shape[0]
    c = -(-n // PER_THREADS)
    pad = np.zeros(PER_THREADS * c, dtype=np.float32)
    pad[:n] = pri
    within = np.cumsum(pad.reshape(PER_THREADS, c), axis=1,
                       dtype=np.float32)
    incl = np.cumsum(within[:, -1], dtype=np.float32)
    off = np.concatenate([np.zeros(1, np.float32), incl[:-1]])
    pref = (within + off[:, None]).astype(np.float32).reshape(-1)[:n]
    return pref, np.float32(incl[-1])


def per_index_oracle(pri, u):
    """Indices the kernel must return bit for bit: adds and one multiply
    only, so fp32 numpy reproduces them."""
    pref, total = per_scan_emulation(pri)
    B = u.shape[0]
    seg = np.float32(total / np.float32(B))
    target = ((np.arange(B, dtype=np.float32) + u.astype(np.float32))
              * seg).astype(np.float32)
    idx = np.searchsorted(pref, target, side="left")
    return np.minimum(idx, pri.shape[0] - 1).astype(np.int64)


def per_delta(n, total):
    """Summation-error bound of the scan: a prefix sum passes through at
    most ceil(n/256) + 256 adds, the target through four more roundings."""
    return (-(-n // PER_THREADS) + 260) * U32 * float(total)


def per_window_check(pri, u, idx):
    """(draws outside their delta-window, draws away from every window
    that differ from the float64 index, draws inside a window that
    differ)."""
    pri64 = f64(pri)
    n, B = pri64.shape[0], u.shape[0]
    cdf = np.cumsum(pri64)
    total = cdf[-1]
    delta = per_delta(n, total)
    target = (np.arange(B, dtype=np.float64) + f64(u)) * (total / B)
    idx = np.asarray(idx, dtype=np.int64)
    lower = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    outside = ~((lower - delta < target) & (target <= cdf[idx] + delta))
    j64 = np.minimum(np.searchsorted(cdf, target, side="left"), n - 1)
    lower64 = np.where(j64 > 0, cdf[np.maximum(j64 - 1, 0)], 0.0)
    near = (cdf[j64] - target <= delta) | (target - lower64 <= delta)
    differ = idx != j64
    return (int(outside.sum()), int((differ & ~near).sum()),
            int((differ & near).sum()))


def per_probs_oracle(pri, idx):
    pri64 = f64(pri)
    return pri64[np.asarray(idx)] / pri64.sum()


def per_weights_oracle(pri, idx, beta):
    n = len(pri)
    w = np.maximum(n * per_probs_oracle(pri, idx), 1e-12) ** (-beta)
    return w / w.max()


def per_update_oracle(pri, idx, td, eps, alpha, maxp):
    """float64 min(|td| + eps, maxp)^alpha on the fp32 inputs; the scalars
    reach the kernel as floats."""
    out = f64(pri).copy()
    eps, alpha, maxp = (float(np.float32(v)) for v in (eps, alpha, maxp))
    out[np.asarray(idx)] = np.minimum(np.abs(f64(td).reshape(-1)) + eps,
                                      maxp) ** alpha
    return out


@pytest.mark.parametrize("kind", PER_KINDS)
@pytest.mark.parametrize("n,B", PER_CASES)
def test_per_emulation_lies_in_float64_windows(n, B, kind):
    pri = per_priorities(kind, n, n + B)
    u = per_draws(B, n + B)
    assert u.min() >= np.float32(U32) and u.max() < 1.0
    idx = per_index_oracle(pri, u)
    outside, away, inside = per_window_check(pri, u, idx)
    assert outside == 0 and away == 0, (outside, away, inside)
    assert (pri[idx] > 0).all()       # a zero priority is never drawn
    if kind == "one":
        assert (idx == n // 2).all()


@pytest.mark.parametrize("kind", PER_KINDS)
@pytest.mark.parametrize("n,B", PER_CASES)
def test_per_eager_path_against_oracle(n, B, kind):
    """The torch composition: indices inside the same windows (its cumsum
    order differs from the kernel's), probabilities to the rounding of the
    total, weights close to float64."""
    pri = per_priorities(kind, n, n + B)
    u = per_draws(B, n + B)
    idx, probs = per_ops._torch_stratified(torch.from_numpy(pri), B,
                                           torch.from_numpy(u))
    outside, away, _ = per_window_check(pri, u, idx.numpy())
    assert outside == 0 and away == 0
    ref = per_probs_oracle(pri, idx.numpy())
    rel = np.abs(f64(probs) - ref) / ref
    assert rel.max() <= per_delta(n, 1.0)
    w = per_ops.importance_weights(probs, n, 0.62)
    w64 = per_weights_oracle(pri, idx.numpy(), 0.62)
    assert np.abs(f64(w) - w64).max() <= 32 * U32


def test_per_prefix_differencing_loses_the_probability():
    """Why the kernel reads PRI[j] for the probability: differencing two
    fp32 prefix sums of the emulated scan is wrong in the third digit at
    the workload's buffer size."""
    n = 16000
    pri = per_priorities("real", n, 1)
    pref, total = per_scan_emulation(pri)
    j = np.flatnonzero(pri > 0)
    diff = (pref[j] - np.where(j > 0, pref[np.maximum(j - 1, 0)],
                               np.float32(0))) / total
    ref = f64(pri)[j] / f64(pri).sum()
    rel_diff = np.abs(f64(diff) - ref) / ref
    rel_read = np.abs(f64(pri[j] / total) - ref) / ref
    assert rel_diff.max() > 1e-4
    assert rel_read.max() <= per_delta(n, 1.0)


@pytest.mark.parametrize("alpha", [0.6, 1.0])
@pytest.mark.parametrize("B", [1, 257])
def test_per_update_eager_against_oracle(B, alpha):
    pri, idx, td = per_update_inputs(B)
    got = torch.from_numpy(pri.copy())
    per_ops.update_priorities(got, torch.from_numpy(idx),
                              torch.from_numpy(td), 0.01, alpha, 1.0)
    ref = per_update_oracle(pri, idx, td, 0.01, alpha, 1.0)
    assert np.abs(f64(got) - ref).max() <= 8 * U32
    untouched = np.setdiff1d(np.arange(len(pri)), idx)
    assert np.array_equal(got.numpy()[untouched], pri[untouched])
    assert ref[idx].max() == 1.0          # the clip is reached ...
    if B > 4:
        assert ref[idx].min() < 1.0       # ... and not by every entry


def per_update_inputs(B):
    """(priorities (600,), idx (B,), td (B, 1)): negative td, |td| + eps on
    both sides of max_priority = 1, duplicate indices with one td."""
    rng = np.random.default_rng(B)
    pri = (rng.random(600) + 0.1).astype(np.float32)
    idx = rng.permutation(600)[:B].astype(np.int64)
    td = (rng.standard_normal((B, 1)) * 1.2).astype(np.float32)
    td[0, 0] = -2.5                       # clipped
    if B > 4:
        td[1, 0] = -0.3                   # below the clip
        td[2, 0] = 0.99                   # |td| + eps == 1.0 to rounding
        idx[3], td[3, 0] = idx[1], td[1, 0]   # duplicate, same td
        idx[4], td[4, 0] = idx[0], td[0, 0]
    return pri, idx, td


# ------------------------------------------------------- tanh-Gaussian ----

TG_CASES = [(1, 1), (5, 2), (3, 63), (3, 64), (3, 65), (2, 128), (7, 130)]
TG_MAX_ACTIONS = [1.0, 2.5, 0.5]
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def tanh_gauss_inputs(B, A, seed, zmax=3.0):
    """fp32 (mu, logsigma, eps, dact, dlogp) with |mu + sigma eps| <= zmax,
    kept by clamping mu."""
    g = torch.Generator().manual_seed(seed)
    logsigma = torch.randn(B, A, generator=g) * 0.5 - 1.0
    eps = torch.randn(B, A, generator=g)
    se = (logsigma.double().exp() * eps.double()).float()
    mu = torch.randn(B, A, generator=g)
    margin = 1e-3
    mu = torch.minimum(torch.maximum(mu, -zmax + margin - se),
                       zmax - margin - se)
    dact = torch.randn(B, A, generator=g)
    dlogp = torch.randn(B, 1, generator=g)
    z = mu.double() + logsigma.double().exp() * eps.double()
    assert float(z.abs().max()) <= zmax
    return mu, logsigma, eps, dact, dlogp


def tanh_gauss_oracle(mu, logsigma, eps, max_action, dact=None, dlogp=None):
    """float64 action, logp and, given upstream gradients, dmu, dlogsigma
    from the closed forms (no autograd)."""
    mu, ls, e = f64(mu), f64(logsigma), f64(eps)
    M = float(max_action)
    sig = np.exp(ls)
    at = np.tanh(mu + sig * e)
    one_m = 1.0 - at * at
    D = M * one_m + 1e-6
    action = M * at
    logp = (-0.5 * e * e - ls - _LOG_SQRT_2PI - np.log(D)).sum(
        1, keepdims=True)
    if dact is None:
        return action, logp
    da, dl = f64(dact), f64(dlogp).reshape(-1, 1)
    dz = da * M * one_m + dl * (2.0 * M * at * one_m / D)
    return action, logp, dz, dz * sig * e - dl


def tanh_gauss_eager(mu, logsigma, eps, max_action, dact, dlogp):
    """The wrapper's CPU branch in fp32, gradients by autograd."""
    mu = mu.detach().cpu().clone().requires_grad_(True)
    ls = logsigma.detach().cpu().clone().requires_grad_(True)
    a, lp = tanh_gauss_sample(mu, ls, max_action, True, eps.cpu())
    ((a * dact.cpu()).sum() + (lp * dlogp.cpu()).sum()).backward()
    return a.detach(), lp.detach(), mu.grad, ls.grad


@pytest.mark.parametrize("max_action", TG_MAX_ACTIONS)
@pytest.mark.parametrize("B,A", TG_CASES)
def test_tanh_gauss_oracle_against_eager(B, A, max_action):
    mu, ls, eps, dact, dlogp = tanh_gauss_inputs(B, A, 100 * B + A)
    ref = tanh_gauss_oracle(mu, ls, eps, max_action, dact, dlogp)
    got = tanh_gauss_eager(mu, ls, eps, max_action, dact, dlogp)
    # 1 - tanh^2 >= 0.0099 on |z| <= 3: one ulp of tanh is amplified by at
    # most 2 / 0.0099 in log(1 - tanh^2) and its derivative
    amp = 2.0 / 0.0099
    for name, g, r, L in zip(("action", "logp", "dmu", "dlogsigma"), got,
                             ref, (1, A, 1, 1)):
        err = np.abs(f64(g) - r).max()
        scale = max(np.abs(r).max(), 1.0)
        assert err <= 16 * L * amp * U32 * scale, (name, err)


def test_tanh_gauss_oracle_gradient_is_the_float64_autograd_one():
    mu, ls, eps, dact, dlogp = tanh_gauss_inputs(4, 9, 5)
    ref = tanh_gauss_oracle(mu, ls, eps, 2.5, dact, dlogp)
    got = tanh_gauss_eager(mu.double(), ls.double(), eps.double(), 2.5,
                           dact.double(), dlogp.double())
    for g, r in zip(got, ref):
        assert np.abs(f64(g) - r).max() <= 1e-10


def test_tanh_gauss_wrapper_input_hygiene_cpu():
    """float64 or transposed noise and 1-D rows give the values of the
    plain fp32 2-D call (the CPU branch)."""
    mu, ls, eps, _, _ = tanh_gauss_inputs(6, 5, 11)
    a0, lp0 = tanh_gauss_sample(mu, ls, 2.5, True, eps)
    a1, lp1 = tanh_gauss_sample(mu, ls, 2.5, True, eps.double())
    assert a1.dtype == torch.float32 and lp1.dtype == torch.float32
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1)
    eps_t = eps.t().contiguous().t()
    assert not eps_t.is_contiguous()
    a2, lp2 = tanh_gauss_sample(mu, ls, 2.5, True, eps_t)
    assert torch.equal(a0, a2) and torch.equal(lp0, lp2)
    a3, lp3 = tanh_gauss_sample(mu[2], ls[2], 2.5, True, eps[2])
    a4, lp4 = tanh_gauss_sample(mu[2:3], ls[2:3], 2.5, True, eps[2:3])
    assert torch.equal(a3.reshape(-1), a4.reshape(-1))
    assert torch.equal(lp3.reshape(-1), lp4.reshape(-1))
    a5, lp5 = tanh_gauss_sample(mu, ls, 2.5, False, eps)
    assert torch.equal(a0, a5) and torch.equal(lp0, lp5)


# ---------------------------------------------------------------- Adam ----

ADAM_SIZES = [1, 255, 256, 257, 10001]
ADAM_HYPERS = [(1e-3, 0.9, 0.999, 1e-8), (3e-4, 0.5, 0.9, 1e-3)]


def adam_inputs(n, resumed, steps, seed):
    """(p, m, v, t0, [g_1..g_steps]) in fp32; every seventh gradient entry
    is zero; a resumed state starts at t = 1000 with random m, positive v."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grads = []
    for _ in range(steps):
        gr = torch.randn(n, generator=g)
        gr[::7] = 0.0
        grads.append(gr)
    if resumed:
        m = torch.randn(n, generator=g) * 0.1
        v = torch.rand(n, generator=g) * 0.5 + 1e-3
        t0 = 1000
    else:
        m, v, t0 = torch.zeros(n), torch.zeros(n), 0
    return p, m, v, t0, grads


def adam_oracle(p, m, v, t0, grads, hypers, weight_decay=0.0):
    """float64 Adam on the fp32 inputs. The hyper-parameters are inputs
    too: the kernel receives them as floats, so the oracle takes their
    fp32 values (beta2 = 0.999 is 0.99900001287 there, and 1 - beta2
    differs from 0.001 by 1.3e-5 of itself)."""
    lr, b1, b2, eps = (float(np.float32(h)) for h in hypers)
    wd = float(np.float32(weight_decay))
    p, m, v = f64(p).copy(), f64(m).copy(), f64(v).copy()
    for k, g in enumerate(grads):
        t = t0 + k + 1
        g = f64(g) + wd * p
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - lr * (m / (1.0 - b1 ** t)) / (
            np.sqrt(v / (1.0 - b2 ** t)) + eps)
    return p, m, v


class _Pool(torch.nn.Module):
    def __init__(self, p):
        super().__init__()
        self.w = torch.nn.Parameter(p.clone())


def adam_eager(p, m, v, t0, grads, hypers, weight_decay=0.0, device="cpu"):
    """FusedAdam.step() of utils/flatten.py (its CPU branch on the CPU, the
    kernel on a GPU): (p, m, v, t_dev)."""
    lr, b1, b2, eps = hypers
    fp = FlatParams(_Pool(p).to(device))
    opt = FusedAdam(fp, lr, (b1, b2), eps, weight_decay)
    opt.load_state_dict({"step": t0, "m": m.to(device), "v": v.to(device)})
    for g in grads:
        fp.flat_grad.copy_(g)
        opt.step()
    return fp.flat.detach(), opt.m, opt.v, opt.t_dev


@pytest.mark.parametrize("resumed", [False, True])
@pytest.mark.parametrize("hypers", ADAM_HYPERS)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_oracle_against_eager(n, hypers, resumed):
    steps = 5 if resumed else 3
    p, m, v, t0, grads = adam_inputs(n, resumed, steps, n)
    ref = adam_oracle(p, m, v, t0, grads, hypers)
    got = adam_eager(p, m, v, t0, grads, hypers)
    # the eager path forms 1 - beta in double, the oracle from the fp32
    # beta: m and v may differ by that much of themselves, p far less
    d1 = abs((1 - hypers[1]) - (1 - float(np.float32(hypers[1]))))
    d2 = abs((1 - hypers[2]) - (1 - float(np.float32(hypers[2]))))
    tols = (16 * U32, d1 / (1 - hypers[1]) + 16 * U32,
            d2 / (1 - hypers[2]) + 16 * U32)
    for name, g, r, tol in zip("pmv", got[:3], ref, tols):
        scale = max(np.abs(r).max(), 1e-30)
        assert np.abs(f64(g) - r).max() <= steps * tol * scale, name
    assert float(got[3]) == t0


# ----------------------------------------------------------- attention ----

ATTN_CASES = [(4, 1, 1), (3, 15, 4), (2, 16, 96), (2, 31, 95), (5, 32, 3),
              (8, 17, 33), (6, 8, 66), (12, 12, 16), (2, 32, 96), (3, 5, 7),
              (1, 17, 20)]
ATTN_KINDS = ["randn", "peaked", "shifted", "ties"]


def attention_inputs(G, T, dh, kind, seed):
    """fp32 (q, k, v, do)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(G, T, dh, generator=g)
    k = torch.randn(G, T, dh, generator=g)
    v = torch.randn(G, T, dh, generator=g)
    do = torch.randn(G, T, dh, generator=g)
    if kind == "peaked":
        q, k = 4 * q, 4 * k
    elif kind == "shifted":   # every logit near +80: the max is subtracted
        a = math.sqrt(80.0 * math.sqrt(dh))
        q, k = 0.3 * q, 0.3 * k
        q[..., 0] = a
        k[..., 0] = a
    elif kind == "ties":      # one row of exactly equal logits
        q[:, T // 2, :] = 0.0
    return q, k, v, do


def attention_oracle(q, k, v, do=None):
    """float64 (O, A) and, given dO, (dQ, dK, dV) from the closed forms."""
    q, k, v = f64(q), f64(k), f64(v)
    s = 1.0 / math.sqrt(q.shape[-1])
    S = np.einsum("gid,gjd->gij", q, k) * s
    E = np.exp(S - S.max(-1, keepdims=True))
    A = E / E.sum(-1, keepdims=True)
    O = np.einsum("gij,gjd->gid", A, v)
    if do is None:
        return O, A
    do = f64(do)
    dV = np.einsum("gij,gid->gjd", A, do)
    dA = np.einsum("gid,gjd->gij", do, v)
    dS = A * (dA - (dA * A).sum(-1, keepdims=True))
    dQ = np.einsum("gij,gjd->gid", dS, k) * s
    dK = np.einsum("gij,gid->gjd", dS, q) * s
    return O, A, dQ, dK, dV


def attention_eager(q, k, v, do):
    """_torch_sdp in fp32 on the CPU, gradients by autograd."""
    q, k, v = (t.detach().cpu().clone().requires_grad_(True)
               for t in (q, k, v))
    o, a = attn_ops._torch_sdp(q, k, v)
    (o * do.cpu()).sum().backward()
    return o.detach(), a.detach(), q.grad, k.grad, v.grad


def attention_lengths(T, dh):
    """Reduction lengths of (O, A, dQ, dK, dV): each output is a chain of
    a dh-long and a T-long sum whose errors add, the map A a dh-long one."""
    return (T + dh, dh, T + dh, T + dh, T + dh)


@pytest.mark.parametrize("kind", ATTN_KINDS)
@pytest.mark.parametrize("G,T,dh", ATTN_CASES)
def test_attention_oracle_against_eager(G, T, dh, kind):
    q, k, v, do = attention_inputs(G, T, dh, kind, 7 * T + dh)
    ref = attention_oracle(q, k, v, do)
    got = attention_eager(q, k, v, do)
    if kind == "ties":
        assert np.array_equal(ref[1][:, T // 2], np.full((G, T), 1.0 / T))
    # logits up to |s|: exp(s) carries |s| ulps, so does every output
    cond = max(float(np.abs(np.einsum("gid,gjd->gij", f64(q), f64(k)))
                     .max()) / math.sqrt(dh), 1.0)
    for g, r, L in zip(got, ref, attention_lengths(T, dh)):
        scale = max(np.abs(r).max(), 1.0)
        assert np.abs(f64(g) - r).max() <= 16 * L * cond * U32 * scale


def test_attention_wrapper_fallbacks_cpu():
    """Off the GPU the wrapper is _torch_sdp, for a key length of its own
    too; a gradient into the map is an ordinary autograd one there."""
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, 3, 5, 4, generator=g)
    k = torch.randn(2, 3, 10, 4, generator=g)
    v = torch.randn(2, 3, 10, 4, generator=g)
    o, a = attn_ops.scaled_dot_product(q, k, v)
    o_ref, a_ref = attn_ops._torch_sdp(q, k, v)
    assert o.shape == (2, 3, 5, 4) and a.shape == (2, 3, 5, 10)
    assert torch.equal(o, o_ref) and torch.equal(a, a_ref)
    O, A = attention_oracle(q.reshape(6, 5, 4), k.reshape(6, 10, 4),
                            v.reshape(6, 10, 4))
    assert np.abs(f64(o).reshape(6, 5, 4) - O).max() <= 64 * U32


# --------------------------------------------------------- convolution ----

CONV_CASES = [(1, 1, 1, 5, 5), (2, 1, 16, 12, 12), (2, 3, 5, 12, 17),
              (1, 16, 32, 6, 31), (3, 32, 32, 13, 13), (1, 1, 16, 128, 128)]


def conv_inputs(B, Cin, Cout, H, W, seed):
    """fp32 (x, weight, bias, dy); dy is a non-contiguous view."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 5, 5, generator=g) / math.sqrt(25 * Cin)
    b = torch.randn(Cout, generator=g)
    OH, OW = (H - 5) // 2 + 1, (W - 5) // 2 + 1
    dy = torch.randn(B, Cout, OW, OH, generator=g).transpose(2, 3)
    if OH > 1 and OW > 1:
        assert not dy.is_contiguous()
    return x, w, b, dy


def conv_oracle(x, w, b, dy):
    """float64 (y, dx, dW, db) and the matching sums of absolute products
    (|bias| included in y's), by float64 F.conv2d and its autograd: with
    every operand replaced by its absolute value each gradient is exactly
    the sum of absolute products."""
    outs = []
    for absolute in (False, True):
        xs, ws, dys = (t.detach().cpu().double() for t in (x, w, dy))
        bs = None if b is None else b.detach().cpu().double()
        if absolute:
            xs, ws, dys = xs.abs(), ws.abs(), dys.abs()
            bs = None if bs is None else bs.abs()
        xs.requires_grad_(True)
        ws.requires_grad_(True)
        y = F.conv2d(xs, ws, bs, stride=2)
        dx, dw = torch.autograd.grad(y, (xs, ws), dys)
        outs.append((y.detach(), dx, dw, dys.sum((0, 2, 3))))
    return outs[0], outs[1]


def conv_lengths(B, Cin, Cout, H, W):
    OH, OW = (H - 5) // 2 + 1, (W - 5) // 2 + 1
    return (25 * Cin, 9 * Cout, B * OH * OW, B * OH * OW)


def conv_naive(x, w, b):
    """Loop transcription of the k5/s2 definition, float64."""
    x, w = f64(x), f64(w)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    OH, OW = (H - 5) // 2 + 1, (W - 5) // 2 + 1
    y = np.zeros((B, Cout, OH, OW))
    for oy in range(OH):
        for ox in range(OW):
            patch = x[:, :, 2 * oy:2 * oy + 5, 2 * ox:2 * ox + 5]
            y[:, :, oy, ox] = np.einsum("bcij,ocij->bo", patch, w)
    return y if b is None else y + f64(b)[None, :, None, None]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,Cin,Cout,H,W", CONV_CASES[:5])
def test_conv_oracle_against_eager_and_loops(B, Cin, Cout, H, W, with_bias):
    x, w, b, dy = conv_inputs(B, Cin, Cout, H, W, H * W + Cin)
    b = b if with_bias else None
    ref, absref = conv_oracle(x, w, b, dy)
    assert np.abs(f64(ref[0]) - conv_naive(x, w, b)).max() <= 1e-12
    xs = x.clone().requires_grad_(True)
    ws = w.clone().requires_grad_(True)
    y = conv2d_k5s2(xs, ws, b)
    dx, dw = torch.autograd.grad(y, (xs, ws), dy)
    got = (y.detach(), dx, dw, dy.sum((0, 2, 3)))
    for g, r, a, L in zip(got, ref, absref, conv_lengths(B, Cin, Cout, H,
                                                         W)):
        assert product_ratio(g, r, a, L) <= 1.0
    if H % 2 == 0:   # the last row belongs to no window
        assert float(ref[1][:, :, -1, :].abs().max()) == 0.0
    if W % 2 == 0:
        assert float(ref[1][:, :, :, -1].abs().max()) == 0.0


def test_conv_rejects_small_images_cpu():
    w = torch.randn(2, 1, 5, 5)
    for H, W in [(4, 9), (9, 4)]:
        with pytest.raises(RuntimeError):
            conv2d_k5s2(torch.randn(1, 1, H, W), w)


# ----------------------------------------------------------------- GEMM ---

GEMM_NN_CASES = [(1, 1, 1), (16, 64, 64), (17, 65, 65), (3, 63, 15),
                 (5, 129, 1), (64, 128, 420), (33, 200, 513)]
GEMM_TN_CASES = [(1, 1, 1), (33, 17, 65), (32, 64, 64), (257, 5, 129),
                 (64, 512, 420)]


def gemm_nn_inputs(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)


def gemm_tn_inputs(Bb, N, K, seed):
    """(dz (Bb, N), x (Bb, K), dW0 (N, K), db0 (N,))."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Bb, N, generator=g), torch.randn(Bb, K, generator=g),
            torch.randn(N, K, generator=g), torch.randn(N, generator=g))


def gemm_nn_oracle(A, B):
    A, B = f64(A), f64(B)
    return A @ B, np.abs(A) @ np.abs(B)


def gemm_tn_oracle(dz, x, dW0=None, db0=None):
    """float64 (dW, db) = (dz^T x, column sums of dz), added to dW0 / db0
    if given, and the sums of absolute values behind each element."""
    dz, x = f64(dz), f64(x)
    dW, db = dz.T @ x, dz.sum(0)
    aW, ab = np.abs(dz).T @ np.abs(x), np.abs(dz).sum(0)
    if dW0 is not None:
        dW, db = dW + f64(dW0), db + f64(db0)
        aW, ab = aW + np.abs(f64(dW0)), ab + np.abs(f64(db0))
    return (dW, db), (aW, ab)


@pytest.mark.parametrize("M,K,N", GEMM_NN_CASES)
def test_gemm_nn_oracle_against_eager(M, K, N):
    A, B = gemm_nn_inputs(M, K, N, M + K + N)
    C64, absC = gemm_nn_oracle(A, B)
    assert product_ratio(torch.matmul(A, B), C64, absC, K) <= 1.0
    # a dropped term is caught: leave out the last slice of the sum
    if K > 1:
        short = torch.matmul(A[:, :-1], B[:-1])
        assert product_ratio(short, C64, absC, K) > 1.0


@pytest.mark.parametrize("Bb,N,K", GEMM_TN_CASES)
def test_gemm_tn_oracle_against_eager(Bb, N, K):
    dz, x, dW0, db0 = gemm_tn_inputs(Bb, N, K, Bb + N + K)
    (dW, db), (aW, ab) = gemm_tn_oracle(dz, x)
    assert product_ratio(torch.matmul(dz.t(), x), dW, aW, Bb) <= 1.0
    assert product_ratio(dz.sum(0), db, ab, Bb) <= 1.0
    (dW, db), (aW, ab) = gemm_tn_oracle(dz, x, dW0, db0)
    assert product_ratio(dW0 + torch.matmul(dz.t(), x), dW, aW,
                         Bb + 1) <= 1.0
    assert product_ratio(db0 + dz.sum(0), db, ab, Bb + 1) <= 1.0


def test_rule_ratio_figures():
    oracle = np.array([1.0, -2.0])
    ratio, err, err_eager, bound = rule_ratio(
        oracle + [0.0, 3e-7], oracle + [1e-7, 0.0], oracle, 3)
    assert err == pytest.approx(3e-7) and err_eager == pytest.approx(1e-7)
    assert bound == pytest.approx(4e-7 + 3 * U32 * 2.0)
    assert ratio == pytest.approx(err / bound)
    assert rule_ratio(np.zeros(0), np.zeros(0), np.zeros(0), 1)[0] == 0.0
