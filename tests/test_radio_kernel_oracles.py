"""Float64 / complex128 oracles of the kernels behind the calibration
solver and the influence map (als_sweep.hip, gather_sum.hip,
hessianres.hip, two_loop.hip, cgemm.hip), their case lists and input
builders, and the tests that validate the oracles against the project's
eager fp32 paths on the CPU. test_gpu_radio_kernels.py imports all of it
and holds the kernels to the same bounds.

The two rules of test_agent_kernel_oracles.py apply unchanged. Sums of
products (the als_sweep outputs, gather_sum, hessianres, cgemm) use
``product_ratio``: per element, |error| <= (L + 2) 2^-24 * (sum of the
absolute values of the real products behind it), L the number of real
terms. Real and imaginary parts are held separately. The sum of absolute
products comes from the same oracle loops run in the arithmetic of
absolute values (``split_abs``): a complex number a + ib becomes the pair
(|a|, |b|), a product of two pairs (r1 r2 + i1 i2, r1 i2 + i1 r2), a
conjugate or a sign changes nothing. That arithmetic is the split-complex
one; it is componentwise in u = r + i, v = r - i, so the loops run twice
on real inputs. The two-loop recursion and the full sweep pass through
divisions or a solve and use ``rule_ratio``.

No oracle builds the solver's gather plan, a permuted layout or an index
tensor of the code under test: they loop over samples and stations and
place every entry by index arithmetic written out here.
"""

import functools

import numpy as np
import pytest
import torch

from smartcal_amd import autograd_tools as at_
from smartcal_amd.radio import hessian as hs
from smartcal_amd.radio import solver as rs

from test_agent_kernel_oracles import (U32, f64, product_ratio, record,
                                       rule_ratio)

__all__ = ["U32", "f64", "product_ratio", "record", "rule_ratio"]


def c128(t):
    """numpy complex128 copy of a tensor or array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.complex128)


def herm(x):
    return np.conj(np.swapaxes(x, -1, -2))


def split_abs(fn, *zs):
    """(sum of |real products| behind the real part, behind the imaginary
    part) of every output of ``fn``, a multilinear function without signs
    of the complex arrays ``zs``: fn on u = |re| + |im| and on
    v = |re| - |im|, recombined."""
    zs = [c128(z) for z in zs]
    U = fn(*[np.abs(z.real) + np.abs(z.imag) for z in zs])
    V = fn(*[np.abs(z.real) - np.abs(z.imag) for z in zs])
    if isinstance(U, tuple):
        return tuple((0.5 * (u + v), 0.5 * (u - v)) for u, v in zip(U, V))
    return 0.5 * (U + V), 0.5 * (U - V)


def complex_product_ratios(got, oracle, absparts, L):
    """product_ratio of the real and of the imaginary part."""
    got, oracle = c128(got), c128(oracle)
    return (product_ratio(got.real, oracle.real, absparts[0], L),
            product_ratio(got.imag, oracle.imag, absparts[1], L))


def crandn(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen),
                         torch.randn(*shape, generator=gen))


def gauss_int(rng, *shape):
    """complex64 Gaussian integers with |re|, |im| <= 3."""
    z = rng.integers(-3, 4, shape) + 1j * rng.integers(-3, 4, shape)
    return torch.from_numpy(z.astype(np.complex64))


def baselines(N):
    """(p, q) of the B = N (N - 1) / 2 baselines, p < q lexicographic."""
    pq = [(p, q) for p in range(N - 1) for q in range(p + 1, N)]
    return (np.array([p for p, _ in pq], dtype=np.int64),
            np.array([q for _, q in pq], dtype=np.int64))


# ------------------------------------------------- ALS contributions ----

# (F, K, N, Ts, Tdelta); the last has F T B = 294 samples, across the
# 256-thread block
ALS_CASES = [(1, 1, 2, 1, 1), (2, 3, 7, 2, 3), (1, 8, 7, 2, 3),
             (1, 2, 7, 1, 7), (2, 8, 3, 3, 2), (2, 2, 7, 1, 7)]


def als_inputs(F, K, N, Ts, Tdelta, seed):
    """complex64 (V22 (F,T,B,2,2), C22 (F,K,T,B,2,2), J (F,Ts,K,N,2,2)) and
    int64 (p_idx, q_idx, t_int). J is the identity plus a random matrix
    of its own per frequency, interval, direction and station."""
    g = torch.Generator().manual_seed(seed)
    B, T = N * (N - 1) // 2, Ts * Tdelta
    C22 = crandn(g, F, K, T, B, 2, 2)
    V22 = crandn(g, F, T, B, 2, 2)
    J = 0.4 * crandn(g, F, Ts, K, N, 2, 2)
    J[..., 0, 0] += 1.0
    J[..., 1, 1] += 1.0
    p, q = baselines(N)
    t_int = np.minimum(np.arange(T) // Tdelta, Ts - 1)
    return (V22, C22, J, torch.from_numpy(p), torch.from_numpy(q),
            torch.from_numpy(t_int))


def _als_contrib_loops(V22, C22, J, p_idx, q_idx, t_int):
    F, K, T, B = C22.shape[:4]
    TB, K2 = T * B, 2 * K
    dtype = np.result_type(C22, np.float64)
    rhs = np.zeros((F, 2 * K2, 2 * TB), dtype=dtype)
    nm = np.zeros((F, K2 * K2, 2 * TB), dtype=dtype)
    for f in range(F):
        for t in range(T):
            ti = int(t_int[t])
            for b in range(B):
                p, q = int(p_idx[b]), int(q_idx[b])
                V = V22[f, t, b]
                Wp = np.concatenate([C22[f, k, t, b] @ herm(J[f, ti, k, q])
                                     for k in range(K)])        # (2K, 2)
                Wq = np.concatenate([herm(C22[f, k, t, b])
                                     @ herm(J[f, ti, k, p])
                                     for k in range(K)])
                col = t * B + b
                for side, Vs, W in ((0, V, Wp), (1, herm(V), Wq)):
                    r = Vs @ herm(W)                            # (2, 2K)
                    n = W @ herm(W)                             # (2K, 2K)
                    for i in range(2):
                        for c in range(K2):
                            rhs[f, i * K2 + c, side * TB + col] = r[i, c]
                    for a in range(K2):
                        for c in range(K2):
                            nm[f, a * K2 + c, side * TB + col] = n[a, c]
    return rhs, nm


def als_contrib_oracle(V22, C22, J, p_idx, q_idx, t_int):
    """complex128 (rhs_cat (F, 2·2K, 2TB), nm_cat (F, 4K², 2TB)) and, for
    each, the (real, imaginary) sums of absolute products.

    Per sample (f, t, b) with stations (p, q) and interval ti:
    W_p = [C_k J_q^kH]_k, W_q = [C_k^H J_p^kH]_k (2K x 2), rhs_p = V W_p^H,
    rhs_q = V^H W_q^H, nm = W W^H; entry (i, c) of rhs at row i·2K + c,
    entry (a, c) of nm at row a·2K + c, the p side in column t·B + b, the
    q side in column T·B + t·B + b."""
    idx = [np.asarray(t) for t in (p_idx, q_idx, t_int)]
    out = _als_contrib_loops(c128(V22), c128(C22), c128(J), *idx)
    absout = split_abs(lambda v, c, j: _als_contrib_loops(v, c, j, *idx),
                       V22, C22, J)
    return out, absout


# real terms behind one entry: rhs is 2 (t) x 2 (m) complex products of
# three factors, four real terms each; nm 2 x 2 x 2 products of four
# factors, eight real terms each
ALS_L = {"rhs": 16, "nm": 64}


def als_contrib_eager(V22, C22, J, p_idx, q_idx, t_int):
    return rs._als_contributions_torch(V22, C22, J, p_idx, q_idx, t_int)


def als_contrib_figures(got, oracle, absout):
    figs = []
    for name, g, o, a in zip(("rhs", "nm"), got, oracle, absout):
        re, im = complex_product_ratios(g, o, a, ALS_L[name])
        figs += [(name + ".re", re), (name + ".im", im)]
    return figs


@pytest.mark.parametrize("F,K,N,Ts,Tdelta", ALS_CASES)
def test_als_contrib_oracle_against_eager(F, K, N, Ts, Tdelta):
    args = als_inputs(F, K, N, Ts, Tdelta, 11 * K + N)
    oracle, absout = als_contrib_oracle(*args)
    got = als_contrib_eager(*args)
    assert got[0].shape == oracle[0].shape and got[1].shape == oracle[1].shape
    for name, ratio in als_contrib_figures(got, oracle, absout):
        assert ratio <= 1.0, (name, ratio)


def test_als_contrib_bound_rejects_swapped_stations_and_intervals():
    V22, C22, J, p, q, t_int = als_inputs(2, 3, 7, 2, 3, 40)
    oracle, absout = als_contrib_oracle(V22, C22, J, p, q, t_int)
    for bad in [(V22, C22, J, q, p, t_int),                 # p and q swapped
                (V22, C22, J, p, q, 1 - t_int),             # wrong interval
                (V22, C22, J.flip(0), p, q, t_int),         # wrong frequency
                (V22, C22, J.flip(2), p, q, t_int)]:        # wrong direction
        figs = dict(als_contrib_figures(als_contrib_eager(*bad), oracle,
                                        absout))
        assert min(figs["rhs.re"], figs["nm.re"]) > 1.0, figs
    # one normal-matrix entry of one sample put into its transposed place
    rhs, nm = (t.clone() for t in als_contrib_eager(V22, C22, J, p, q, t_int))
    nm[1, 1 * 6 + 4, 17], nm[1, 4 * 6 + 1, 17] = \
        nm[1, 4 * 6 + 1, 17].clone(), nm[1, 1 * 6 + 4, 17].clone()
    figs = dict(als_contrib_figures((rhs, nm), oracle, absout))
    assert figs["nm.im"] > 1.0 and figs["rhs.re"] <= 1.0


# ------------------------------------------------------ the full sweep ----

# (F, K, N, Ts, Tdelta, prox); Tdelta (N - 1) >= K + 2 or a prox term with
# rho >= 1 keeps the 2K x 2K normal matrices well conditioned
SWEEP_CASES = [(2, 3, 7, 2, 3, False), (1, 8, 7, 2, 3, True),
               (1, 1, 2, 1, 4, True)]
SWEEP_COUNTS = [1, 2]


def sweep_inputs(F, K, N, Ts, Tdelta, prox, seed):
    """als_inputs plus (rho (K,) fp32, distinct and >= 1, prox target
    (F,Ts,K,N,2,2) or None)."""
    V22, C22, J, p, q, t_int = als_inputs(F, K, N, Ts, Tdelta, seed)
    g = torch.Generator().manual_seed(seed + 1)
    rho = 1.0 + 0.5 * torch.arange(K, dtype=torch.float32) \
        + 0.25 * torch.rand(K, generator=g)
    target = None
    if prox:
        target = 0.4 * crandn(g, F, Ts, K, N, 2, 2)
        target[..., 0, 0] += 1.0
        target[..., 1, 1] += 1.0
    return V22, C22, J, rho, target, p, q


def sweep_oracle(V22, C22, J, rho, target, N, Tdelta, n_sweeps,
                 lambda_reg=1e-6):
    """complex128 J after n_sweeps ALS sweeps: for every (frequency,
    interval, station) the normal matrix and right-hand side are summed
    over the samples whose baseline holds the station, the prox term and
    lambda_reg added, G = rhs nm^-1 solved and J <- J/2 + G/2 for all
    stations at once. Timeslot t belongs to interval min(t // Tdelta,
    Ts - 1)."""
    V22, C22, J = c128(V22), c128(C22), c128(J).copy()
    rho = f64(rho)
    target = None if target is None else c128(target)
    F, K, T, B = C22.shape[:4]
    Ts = J.shape[1]
    lam = float(np.float32(lambda_reg))
    pq = [(p, q) for p in range(N - 1) for q in range(p + 1, N)]
    assert len(pq) == B
    for _ in range(n_sweeps):
        Jn = np.empty_like(J)
        for f in range(F):
            for ti in range(Ts):
                slots = [t for t in range(T)
                         if min(t // Tdelta, Ts - 1) == ti]
                for n in range(N):
                    nm = np.zeros((2 * K, 2 * K), dtype=np.complex128)
                    rhs = np.zeros((2, 2 * K), dtype=np.complex128)
                    for t in slots:
                        for b, (p, q) in enumerate(pq):
                            if n == p:
                                W = np.concatenate(
                                    [C22[f, k, t, b] @ herm(J[f, ti, k, q])
                                     for k in range(K)])
                                Vs = V22[f, t, b]
                            elif n == q:
                                W = np.concatenate(
                                    [herm(C22[f, k, t, b])
                                     @ herm(J[f, ti, k, p])
                                     for k in range(K)])
                                Vs = herm(V22[f, t, b])
                            else:
                                continue
                            rhs += Vs @ herm(W)
                            nm += W @ herm(W)
                    if target is not None:
                        for k in range(K):
                            nm[2 * k, 2 * k] += rho[k]
                            nm[2 * k + 1, 2 * k + 1] += rho[k]
                            rhs[:, 2 * k:2 * k + 2] += \
                                rho[k] * target[f, ti, k, n]
                    nm += lam * np.eye(2 * K)
                    G = np.linalg.solve(nm.T, rhs.T).T
                    for k in range(K):
                        Jn[f, ti, k, n] = G[:, 2 * k:2 * k + 2]
        J = 0.5 * J + 0.5 * Jn
    return J


def sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, n_sweeps,
              device="cpu"):
    """_solve_sweeps on ``device`` (the torch path on the CPU, the kernels
    on a GPU for K <= 8)."""
    mv = lambda t: None if t is None else t.to(device)
    Jw = J.clone().to(device)
    rs._solve_sweeps(mv(V22), mv(C22), Jw, mv(rho), mv(target), mv(p),
                     mv(q), N, Tdelta, n_sweeps)
    return Jw


def sweep_length(K, N, Tdelta):
    """2K unknowns per row times the Cnt = Tdelta (N - 1) contributions."""
    return 2 * K * Tdelta * (N - 1)


def complex_rule(got, eager, oracle, L):
    """rule_ratio of the real and imaginary parts stacked."""
    st = lambda z: np.stack([c128(z).real, c128(z).imag])
    return rule_ratio(st(got), st(eager), st(oracle), L)


@functools.lru_cache(maxsize=None)
def sweep_reference(case, n_sweeps):
    """(inputs, oracle J) of one case and sweep count, computed once and
    shared; nothing writes to either."""
    F, K, N, Ts, Tdelta, prox = case
    inp = sweep_inputs(F, K, N, Ts, Tdelta, prox, 5 * K + N)
    V22, C22, J, rho, target, p, q = inp
    return inp, sweep_oracle(V22, C22, J, rho, target, N, Tdelta, n_sweeps)


@pytest.mark.parametrize("n_sweeps", SWEEP_COUNTS)
@pytest.mark.parametrize("F,K,N,Ts,Tdelta,prox", SWEEP_CASES)
def test_sweep_oracle_against_eager(F, K, N, Ts, Tdelta, prox, n_sweeps):
    inp, ref = sweep_reference((F, K, N, Ts, Tdelta, prox), n_sweeps)
    V22, C22, J, rho, target, p, q = inp
    got = sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, n_sweeps)
    _, err, err_eager, _ = complex_rule(got, got, ref,
                                        sweep_length(K, N, Tdelta))
    # the rule's eager term must stay small, or it bounds nothing
    assert err_eager <= 1e-5 * np.abs(ref).max(), err_eager
    assert np.abs(ref - c128(J)).max() > 0.05      # the sweep moved J


def test_sweep_bound_rejects_wrong_interval_and_dropped_sample():
    inp, ref = sweep_reference((2, 3, 7, 2, 3, False), 1)
    V22, C22, J, rho, target, p, q = inp
    good = sweep_run(V22, C22, J, rho, target, p, q, 7, 3, 1)
    L = sweep_length(3, 7, 3)
    # the two intervals' solutions exchanged
    assert complex_rule(good.flip(1), good, ref, L)[0] > 1.0
    # one sample of 126 per frequency left out of the sums
    V2, C2 = V22.clone(), C22.clone()
    V2[:, 4, 9] = 0
    C2[:, :, 4, 9] = 0
    bad = sweep_run(V2, C2, J, rho, target, p, q, 7, 3, 1)
    assert complex_rule(bad, good, ref, L)[0] > 1.0
    assert complex_rule(good, good, ref, L)[0] <= 0.25


def test_solve_sweeps_rejects_a_longer_last_interval():
    """T = 7 with Ts = 2 intervals of Tdelta = 3: the gather plan's
    reshape succeeds (Cnt = 21) and cuts the contributions at the wrong
    places; against sweep_oracle the result was off by 0.19 of its
    maximum. It raises now, before any work."""
    N, K, Ts, Tdelta, T = 7, 3, 2, 3, 7
    B = N * (N - 1) // 2
    g = torch.Generator().manual_seed(0)
    V22, C22 = crandn(g, 1, T, B, 2, 2), crandn(g, 1, K, T, B, 2, 2)
    J = crandn(g, 1, Ts, K, N, 2, 2)
    keep = J.clone()
    p, q = (torch.from_numpy(a) for a in baselines(N))
    with pytest.raises(ValueError, match="7 timeslots"):
        rs._solve_sweeps(V22, C22, J, torch.ones(K), None, p, q, N, Tdelta,
                         1)
    assert torch.equal(J, keep)


def test_solve_sweeps_six_timeslots_match_the_loop_oracle():
    N, K, Ts, Tdelta, T = 7, 3, 2, 3, 6
    V22, C22, J, p, q, _ = als_inputs(1, K, N, Ts, Tdelta, 3)
    assert V22.shape[1] == T
    ref = sweep_oracle(V22, C22, J, torch.ones(K), None, N, Tdelta, 1)
    got = sweep_run(V22, C22, J, torch.ones(K), None, p, q, N, Tdelta, 1)
    assert np.abs(c128(got) - ref).max() <= 1e-6 * np.abs(ref).max()
    # and in complex128 the plan and the loops agree to rounding
    got = sweep_run(V22.to(torch.complex128), C22.to(torch.complex128),
                    J.to(torch.complex128), torch.ones(K).double(), None,
                    p, q, N, Tdelta, 1)
    assert np.abs(c128(got) - ref).max() <= 1e-12 * np.abs(ref).max()


# ---------------------------------------------------------- gather_sum ----

# (F, X, S, G, Cnt, duplicate indices)
GATHER_CASES = [(1, 1, 1, 1, 1, False), (1, 5, 40, 1, 63, False),
                (1, 1, 300, 7, 64, False), (2, 3, 300, 5, 65, False),
                (3, 24, 4000, 50, 80, False), (1, 2, 500, 3, 200, True)]


def gather_inputs(F, X, S, G, Cnt, dup, seed, integer=False):
    """(in (F, X, S) complex64, gidx (G, Cnt) int64). Without duplicates
    the indices are distinct where S allows; with them each row repeats
    its first index five times and two rows share a quarter."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    inp = gauss_int(rng, F, X, S) if integer else crandn(g, F, X, S)
    if G * Cnt <= S:
        gidx = rng.permutation(S)[:G * Cnt].reshape(G, Cnt)
    else:
        gidx = rng.integers(0, S, (G, Cnt))
    if dup:
        gidx[:, 1:6] = gidx[:, :1]
        gidx[-1, Cnt // 2:3 * Cnt // 4] = gidx[0, Cnt // 2:3 * Cnt // 4]
    return inp, torch.from_numpy(gidx.astype(np.int64))


def gather_oracle(inp, gidx):
    """complex128 out[f, x, g] = sum_c in[f, x, gidx[g, c]] and the
    (real, imaginary) sums of absolute values."""
    z, gi = c128(inp), np.asarray(gidx)
    G, Cnt = gi.shape
    out = np.zeros(z.shape[:2] + (G,), dtype=np.complex128)
    are = np.zeros(out.shape)
    aim = np.zeros(out.shape)
    for g in range(G):
        for c in range(Cnt):
            col = z[:, :, gi[g, c]]
            out[:, :, g] += col
            are[:, :, g] += np.abs(col.real)
            aim[:, :, g] += np.abs(col.imag)
    return out, (are, aim)


def gather_eager(inp, gidx):
    """The torch composition of _solve_sweeps."""
    F, X = inp.shape[:2]
    G, Cnt = gidx.shape
    return inp[:, :, gidx.reshape(-1)].reshape(F, X, G, Cnt).sum(dim=3)


def solver_plan(N, Ts, Tdelta):
    """The (Ts N, Cnt) gather plan _solve_sweeps builds."""
    p, q = (torch.from_numpy(a) for a in baselines(N))
    t_int = torch.arange(Ts * Tdelta) // Tdelta
    return rs._gather_plan(t_int, p, q, N, Ts)


@pytest.mark.parametrize("F,X,S,G,Cnt,dup", GATHER_CASES)
def test_gather_oracle_against_eager(F, X, S, G, Cnt, dup):
    inp, gidx = gather_inputs(F, X, S, G, Cnt, dup, S + Cnt)
    if dup:
        assert len(np.unique(gidx[0].numpy())) < Cnt
    out, absparts = gather_oracle(inp, gidx)
    got = gather_eager(inp, gidx)
    assert max(complex_product_ratios(got, out, absparts, Cnt)) <= 1.0
    # a dropped term is caught
    if Cnt > 1:
        short = gather_eager(inp, gidx[:, :-1].contiguous())
        assert max(complex_product_ratios(short, out, absparts, Cnt)) > 1.0
    # integer inputs: every fp32 sum is exact
    inp, gidx = gather_inputs(F, X, S, G, Cnt, dup, S + Cnt, integer=True)
    out, _ = gather_oracle(inp, gidx)
    assert torch.equal(gather_eager(inp, gidx),
                       torch.from_numpy(out.astype(np.complex64)))


def test_solver_plan_gives_every_station_its_samples():
    """Row ti·N + n of the plan holds the Tdelta (N - 1) columns of
    cat([p side, q side]) whose sample has station n in interval ti."""
    N, Ts, Tdelta = 7, 2, 3
    B, T = 21, 6
    plan = solver_plan(N, Ts, Tdelta).numpy()
    assert plan.shape == (Ts * N, Tdelta * (N - 1))
    p, q = baselines(N)
    for ti in range(Ts):
        for n in range(N):
            want = [side * T * B + t * B + b
                    for side, st in ((0, p), (1, q))
                    for t in range(ti * Tdelta, (ti + 1) * Tdelta)
                    for b in range(B) if st[b] == n]
            assert sorted(plan[ti * N + n].tolist()) == sorted(want)


# ---------------------------------------------------------- hessianres ----

# (N, T, K): B = 1, 3, 10, 15 and 36 baselines in blocks of four
HESS_CASES = [(2, 1, 1), (2, 4, 2), (3, 1, 2), (5, 3, 1), (6, 3, 3),
              (9, 2, 1)]


def hess_inputs(N, T, K, seed, integer=False):
    """complex64 (R (2 T B, 2), C (K, T B, 4), J (K, 2N, 2))."""
    S = N * (N - 1) // 2 * T
    if integer:
        rng = np.random.default_rng(seed)
        return (gauss_int(rng, 2 * S, 2), gauss_int(rng, K, S, 4),
                gauss_int(rng, K, 2 * N, 2))
    g = torch.Generator().manual_seed(seed)
    return crandn(g, 2 * S, 2), crandn(g, K, S, 4), crandn(g, K, 2 * N, 2)


def _hess_loops(R, C, J, N, sign=-1.0):
    """The quadruple loop of test_radio_hessian._oracle_hessianres in the
    dtype of its inputs: (off + mirror blocks, diag-p terms, diag-q terms),
    each (K, 4N, 4N), already divided by B T."""
    K, S = C.shape[0], C.shape[1]
    B = N * (N - 1) // 2
    T = S // B
    dtype = np.result_type(C, np.float64)
    Hoff = np.zeros((K, 4 * N, 4 * N), dtype=dtype)
    Hp, Hq = np.zeros_like(Hoff), np.zeros_like(Hoff)
    for k in range(K):
        ck = 0
        for _ in range(T):
            for p in range(N - 1):
                for q in range(p + 1, N):
                    Res = R[2 * ck:2 * ck + 2, :]
                    Ci = C[k, ck, :].reshape((2, 2), order="F")
                    Imp = np.kron(sign * np.conj(Ci), Res)
                    Hoff[k, 4 * p:4 * p + 4, 4 * q:4 * q + 4] += Imp
                    Hoff[k, 4 * q:4 * q + 4, 4 * p:4 * p + 4] += herm(Imp)
                    R1 = Ci @ herm(J[k, 2 * q:2 * q + 2, :])
                    Hp[k, 4 * p:4 * p + 4, 4 * p:4 * p + 4] += \
                        np.kron((R1 @ herm(R1)).T, np.eye(2))
                    R2 = J[k, 2 * p:2 * p + 2, :] @ Ci
                    Hq[k, 4 * q:4 * q + 4, 4 * q:4 * q + 4] += \
                        np.kron((herm(R2) @ R2).T, np.eye(2))
                    ck += 1
    return Hoff / (B * T), Hp / (B * T), Hq / (B * T)


def hess_oracle(R, C, J, N):
    """complex128 H (K, 4N, 4N) and the (real, imaginary) sums of absolute
    products of its off + mirror part and of its diagonal part."""
    Hoff, Hp, Hq = _hess_loops(c128(R), c128(C), c128(J), N)
    aoff, ap, aq = split_abs(lambda r, c, j: _hess_loops(r, c, j, N, 1.0),
                             R, C, J)
    adiag = (ap[0] + aq[0], ap[1] + aq[1])
    return Hoff + Hp + Hq, aoff, adiag


def hess_lengths(N, T):
    """Real terms behind one entry. An off or mirror entry sums T complex
    products conj(Ci) Res: L = 2 T, and the two roundings of the 1/(B T)
    scale are the + 2 of the bound. A diagonal entry sums, over the
    (N - 1) T samples of its station, (Ci G Ci^H)[j][i] =
    sum_{m,n} Ci[j][m] G[m][n] conj(Ci[i][n]) with G[m][n] =
    sum_r conj(J[r][m]) J[r][n]: 2·2·2 complex products of four factors,
    eight real terms each, 64 per sample. A term passes through three
    multiplications where the bound's + 2 allows for one and the scale,
    so L = 64 (N - 1) T + 2."""
    return 2 * T, 64 * (N - 1) * T + 2


def hess_masks(N):
    """Boolean (4N, 4N) masks of the block kinds: off (p < q), mirror,
    diag, and the diagonal blocks that hold p-side terms only (station 0)
    and q-side terms only (station N - 1)."""
    blk = np.arange(4 * N) // 4
    r, c = blk[:, None], blk[None, :]
    return {"off": r < c, "mirror": r > c, "diag": r == c,
            "diag-p": (r == c) & (r == 0),
            "diag-q": (r == c) & (r == N - 1)}


def hess_figures(got, H, aoff, adiag, N, T):
    """(block kind, worst of the real and imaginary ratio) per kind."""
    got = c128(got)
    Loff, Ldiag = hess_lengths(N, T)
    figs = []
    for kind, mask in hess_masks(N).items():
        a, L = (adiag, Ldiag) if kind.startswith("diag") else (aoff, Loff)
        m = np.broadcast_to(mask, H.shape)
        figs.append((kind, max(complex_product_ratios(
            got[m], H[m], (a[0][m], a[1][m]), L))))
    return figs


def hess_structure_ok(H, N):
    """The (q, p) block is the exact conjugate transpose of the (p, q)
    block, and the diagonal-block entries (i, a), (j, c) with a != c are
    exactly zero."""
    H = H.detach().cpu()
    K = H.shape[0]
    Hb = H.reshape(K, N, 4, N, 4)
    off = ~torch.eye(N, dtype=torch.bool)
    mir = Hb.permute(0, 3, 4, 1, 2).conj().resolve_conj()
    mirror_ok = torch.equal(Hb.permute(0, 1, 3, 2, 4)[:, off],
                            mir.permute(0, 1, 3, 2, 4)[:, off])
    D = torch.stack([Hb[:, n, :, n, :] for n in range(N)], 1)
    D = D.reshape(K, N, 2, 2, 2, 2)                  # (i, a, j, c)
    zero_ok = bool((D[:, :, :, 0, :, 1] == 0).all()
                   and (D[:, :, :, 1, :, 0] == 0).all())
    return mirror_ok, zero_ok


@pytest.mark.parametrize("N,T,K", HESS_CASES)
def test_hessianres_oracle_against_eager(N, T, K):
    R, C, J = hess_inputs(N, T, K, 100 * N + T)
    H, aoff, adiag = hess_oracle(R, C, J, N)
    got = hs.hessianres(R, C, J, N)
    for kind, ratio in hess_figures(got, H, aoff, adiag, N, T):
        assert ratio <= 1.0, (kind, ratio)
    assert hess_structure_ok(got, N) == (True, True)
    # the oracle has the structure too, and its absolute sums bound it
    Hoff, Hp, Hq = _hess_loops(c128(R), c128(C), c128(J), N)
    assert np.abs(Hoff.real).max() <= aoff[0].max() * (1 + 1e-12)
    assert (np.abs((Hp + Hq).imag) <= adiag[1] * (1 + 1e-12) + 1e-300).all()


def test_hessianres_bound_sees_an_off_block_error_the_max_norm_misses():
    """A transposed off block, a timeslot left out of one off block and a
    p-side term counted on the q side are rejected by the per-kind bound;
    so is an error of 3e-6 of max|H| in one off entry, which a max-norm
    over the whole H at 1e-5 accepts (the diagonal blocks set max|H|)."""
    N, T, K = 6, 3, 3
    R, C, J = hess_inputs(N, T, K, 100 * N + T)
    H, aoff, adiag = hess_oracle(R, C, J, N)
    good = hs.hessianres(R, C, J, N)
    fig = lambda Hx: dict(hess_figures(Hx, H, aoff, adiag, N, T))
    # transposed block (1, 4)
    bad = good.clone()
    bad[0, 4:8, 16:20] = good[0, 4:8, 16:20].mT
    assert fig(bad)["off"] > 1.0 and fig(bad)["mirror"] <= 1.0
    assert hess_structure_ok(bad, N)[0] is False
    # a dropped timeslot: R of sample (t = 1, b = 3) zeroed
    R2 = R.clone()
    R2[2 * (15 + 3):2 * (15 + 3) + 2] = 0
    f = fig(hs.hessianres(R2, C, J, N))
    assert f["off"] > 1.0 and f["mirror"] > 1.0 and f["diag"] <= 1.0
    # a small error in one off entry
    bad = good.clone()
    delta = 3e-6 * float(good.abs().max())
    bad[1, 2, 21] += delta
    assert float((bad - good).abs().max() / good.abs().max()) < 1e-5
    assert fig(bad)["off"] > 1.0
    # a p-side term counted on the q side
    bad = good.clone()
    bad[:, :4, :4], bad[:, -4:, -4:] = good[:, -4:, -4:], good[:, :4, :4]
    assert fig(bad)["diag-p"] > 1.0 and fig(bad)["diag-q"] > 1.0


@pytest.mark.parametrize("N,T", [(2, 1), (2, 4), (5, 3)])
def test_hessianres_eager_on_integers(N, T):
    """Gaussian-integer inputs: every sum is exact, so at N = 2 (B T a
    power of two) H is exact and elsewhere within the roundings of the
    1/(B T) scale."""
    R, C, J = hess_inputs(N, T, 2, N + T, integer=True)
    H = hess_oracle(R, C, J, N)[0]
    got = hs.hessianres(R, C, J, N)
    if N == 2:
        assert torch.equal(got, torch.from_numpy(H.astype(np.complex64)))
    else:
        assert max(r for _, r in hess_integer_figures(got, H, N)) <= 1.0


def hess_integer_figures(got, H, N):
    """Per block kind, the worst |error| / (2·2^-24 |H|) over the real and
    imaginary parts of its entries; infinite where an exact zero is
    missed."""
    d = c128(got) - H
    figs = []
    for kind in ("off", "mirror", "diag"):
        m = np.broadcast_to(hess_masks(N)[kind], H.shape)
        worst = 0.0
        for err, ref in ((np.abs(d.real[m]), np.abs(H.real[m])),
                         (np.abs(d.imag[m]), np.abs(H.imag[m]))):
            bound = 2 * U32 * ref
            ratio = np.where(bound > 0,
                             err / np.where(bound > 0, bound, 1.0),
                             np.where(err > 0, np.inf, 0.0))
            worst = max(worst, float(ratio.max()))
        figs.append((kind, worst))
    return figs


# ------------------------------------------------------------ two-loop ----

# (h, n, m)
TWO_LOOP_CASES = [(1, 1, 1), (2, 63, 2), (7, 20, 20), (16, 255, 2),
                  (16, 256, 1), (5, 257, 3), (3, 4097, 2)]


def two_loop_inputs(h, n, m, seed):
    """fp32 (Y (h, n), S (h, n), Q (m, n) rows, ro (h,), gamma) of a
    positive-definite history: Y = S diag(d) + (S U) U^T, d in [0.5, 4],
    so that y·s > 0, ro = 1 / (y·s) is O(1) and so is the result.
    ro and gamma = y·s / y·y of the newest pair are formed in float64
    from the fp32 Y and S."""
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(h, n, generator=g)
    d = 0.5 + 3.5 * torch.rand(n, generator=g)
    U = torch.randn(n, 3, generator=g) / max(n, 1) ** 0.5
    Y = (S.double() * d.double()
         + (S.double() @ U.double()) @ U.double().t()).float()
    Q = torch.randn(m, n, generator=g)
    ys = (Y.double() * S.double()).sum(1)
    assert h == 0 or float(ys.min()) > 0
    ro = (1.0 / ys).float()
    gamma = float(ys[-1] / (Y[-1].double() ** 2).sum()) if h else 1.0
    return Y, S, Q, ro, gamma


def two_loop_oracle(Y, S, Q, ro, gamma):
    """Textbook two-loop recursion in float64 on the rows of Q with ro
    given: ro[i] = 0 drops pair i. gamma reaches the kernel as a float."""
    Y, S, ro = f64(Y), f64(S), f64(ro)
    gamma = float(np.float32(gamma))
    h = Y.shape[0]
    q = f64(Q).copy()
    al = np.zeros((h, q.shape[0]))
    for i in range(h - 1, -1, -1):
        al[i] = (q @ S[i]) * ro[i]
        q -= np.outer(al[i], Y[i])
    r = gamma * q
    for i in range(h):
        be = (r @ Y[i]) * ro[i]
        r += np.outer(al[i] - be, S[i])
    return r


def two_loop_eager(Y, S, Q):
    """inv_hessian_mult_mat's CPU composition on the rows of Q; it forms
    ro and gamma itself in fp32."""
    return at_.inv_hessian_mult_mat(Y.cpu(), S.cpu(),
                                    Q.cpu().t().contiguous()).t()


def two_loop_length(h):
    """Elementwise updates an entry goes through: h in each loop, the
    copy and the scale."""
    return 2 * h + 2


@pytest.mark.parametrize("h,n,m", TWO_LOOP_CASES)
def test_two_loop_oracle_against_eager(h, n, m):
    Y, S, Q, ro, gamma = two_loop_inputs(h, n, m, 31 * h + n)
    ref = two_loop_oracle(Y, S, Q, ro, gamma)
    got = two_loop_eager(Y, S, Q)
    assert got.shape == (m, n)
    _, _, err_eager, _ = rule_ratio(got, got, ref, two_loop_length(h))
    scale = np.abs(ref).max()
    assert 1e-3 < scale < 1e3
    assert err_eager <= 1e-5 * scale, (err_eager, scale)


def test_two_loop_zero_ro_drops_the_pair():
    Y, S, Q, ro, gamma = two_loop_inputs(7, 20, 20, 5)
    keep = [0, 2, 3, 5, 6]
    ro_f = ro.clone()
    ro_f[[1, 4]] = 0.0
    ref = two_loop_oracle(Y, S, Q, ro_f, gamma)
    only = two_loop_oracle(Y[keep], S[keep], Q, ro[keep], gamma)
    assert np.array_equal(ref, only)
    full = two_loop_oracle(Y, S, Q, ro, gamma)
    assert np.abs(full - ref).max() > 1e-2 * np.abs(ref).max()
    # and the eager path on the remaining pairs is the oracle's
    got = two_loop_eager(Y[keep], S[keep], Q)
    assert rule_ratio(got, got, ref, 12)[2] <= 1e-5 * np.abs(ref).max()


def test_two_loop_bound_rejects_a_wrong_coefficient():
    """A wrong al[i], a wrong sign in the second loop and a wrong gamma
    each miss the rule by orders of magnitude on a positive-definite
    history. On independent randn Y and S, as the older GPU test draws
    them, the result's maximum is 1e2 to 1e12 and its 1e-4 of that
    maximum lets all three pass."""
    h, n, m = 7, 20, 20
    Y, S, Q, ro, gamma = two_loop_inputs(h, n, m, 31 * h + n)
    ref = two_loop_oracle(Y, S, Q, ro, gamma)
    eager = two_loop_eager(Y, S, Q)
    L = two_loop_length(h)
    assert rule_ratio(eager, eager, ref, L)[0] <= 0.25
    ro_bad = ro.clone()
    ro_bad[3] *= 1.01                                   # al[3], be[3]
    assert rule_ratio(two_loop_oracle(Y, S, Q, ro_bad, gamma), eager, ref,
                      L)[0] > 100
    assert rule_ratio(two_loop_oracle(Y, S, Q, ro, 1.001 * gamma), eager,
                      ref, L)[0] > 100
    Yd, Sd, qd = f64(Y), f64(S), f64(Q).copy()
    al = np.zeros((h, m))
    for i in range(h - 1, -1, -1):
        al[i] = (qd @ Sd[i]) * f64(ro)[i]
        qd -= np.outer(al[i], Yd[i])
    r = float(np.float32(gamma)) * qd
    for i in range(h):
        r += np.outer(al[i] + (r @ Yd[i]) * f64(ro)[i], Sd[i])   # sign
    assert rule_ratio(r, eager, ref, L)[0] > 100


# --------------------------------------------------------------- cgemm ----

# (KA, rep, M, Kd, N)
CGEMM_CASES = [(1, 1, 1, 1, 1), (2, 2, 63, 31, 15), (1, 1, 64, 32, 16),
               (3, 8, 65, 33, 17), (2, 8, 68, 68, 130), (1, 2, 17, 100, 1)]


def cgemm_inputs(KA, rep, M, Kd, N, seed, integer=False):
    """complex64 (A (KA, M, Kd), B (KA rep, Kd, N)); every A block is its
    own."""
    if integer:
        rng = np.random.default_rng(seed)
        return gauss_int(rng, KA, M, Kd), gauss_int(rng, KA * rep, Kd, N)
    g = torch.Generator().manual_seed(seed)
    return crandn(g, KA, M, Kd), crandn(g, KA * rep, Kd, N)


def cgemm_oracle(A, B, rep):
    """complex128 C[g] = A[g // rep] @ B[g] and the (real, imaginary) sums
    of absolute products; L = 2 Kd real terms each."""
    A = np.repeat(c128(A), rep, axis=0)
    B = c128(B)
    ar, ai, br, bi = (np.abs(x) for x in (A.real, A.imag, B.real, B.imag))
    return A @ B, (ar @ br + ai @ bi, ar @ bi + ai @ br)


def cgemm_eager(A, B, rep):
    return torch.repeat_interleave(A, rep, dim=0) @ B


@pytest.mark.parametrize("KA,rep,M,Kd,N", CGEMM_CASES)
def test_cgemm_oracle_against_eager(KA, rep, M, Kd, N):
    A, B = cgemm_inputs(KA, rep, M, Kd, N, M + Kd + N)
    C, absparts = cgemm_oracle(A, B, rep)
    got = cgemm_eager(A, B, rep)
    assert got.shape == (KA * rep, M, N)
    assert max(complex_product_ratios(got, C, absparts, 2 * Kd)) <= 1.0
    # the split-complex run gives the same absolute sums
    sa = split_abs(lambda a, b: np.repeat(a, rep, axis=0) @ b, A, B)
    assert np.allclose(sa[0], absparts[0], rtol=1e-12, atol=1e-12)
    assert np.allclose(sa[1], absparts[1], rtol=1e-12, atol=1e-12)
    # integer inputs: exact
    A, B = cgemm_inputs(KA, rep, M, Kd, N, M + Kd + N, integer=True)
    C = cgemm_oracle(A, B, rep)[0]
    assert torch.equal(cgemm_eager(A, B, rep),
                       torch.from_numpy(C.astype(np.complex64)))


def test_cgemm_bound_rejects_the_wrong_A_block_and_a_dropped_term():
    KA, rep, M, Kd, N = 3, 8, 65, 33, 17
    A, B = cgemm_inputs(KA, rep, M, Kd, N, M + Kd + N)
    C, absparts = cgemm_oracle(A, B, rep)
    # g % KA in place of g // rep
    wrong = A[torch.arange(KA * rep) % KA] @ B
    assert min(complex_product_ratios(wrong, C, absparts, 2 * Kd)) > 1.0
    short = cgemm_eager(A[:, :, :-1], B[:, :-1], rep)
    assert min(complex_product_ratios(short, C, absparts, 2 * Kd)) > 1.0
