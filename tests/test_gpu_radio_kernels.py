"""The HIP kernels behind the calibration solver and the influence map
(als_sweep.hip, gather_sum.hip, hessianres.hip, two_loop.hip, cgemm.hip)
against the complex128 / float64 oracles of test_radio_kernel_oracles.py,
at their edge shapes (GPU).

Each comparison prints ``ratio <family> <case> <output> <error / bound>``
before it asserts ``<= 1``; docs/TESTING.md records the worst per family.
Index arguments (gidx, p_idx, q_idx, t_int) are only ever the ones the
callers build: out-of-range values are not checked by the bindings and
not fed to them here.
"""

import numpy as np
import pytest
import torch

from test_radio_kernel_oracles import (
    ALS_CASES, CGEMM_CASES, GATHER_CASES, HESS_CASES, SWEEP_CASES,
    SWEEP_COUNTS, TWO_LOOP_CASES, als_contrib_figures, als_contrib_oracle,
    als_inputs, cgemm_inputs, cgemm_oracle, complex_product_ratios,
    complex_rule, gather_inputs, gather_oracle, hess_figures, hess_inputs,
    hess_integer_figures, hess_oracle, hess_structure_ok, record, rule_ratio,
    solver_plan, sweep_inputs, sweep_length, sweep_oracle, sweep_reference,
    sweep_run, two_loop_eager, two_loop_inputs, two_loop_length,
    two_loop_oracle)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import smartcal_amd.ops as ops
    from smartcal_amd import autograd_tools as at_
    from smartcal_amd.radio import hessian as hs
    from smartcal_amd.radio import solver as rs
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


def gpu(*ts):
    out = tuple(t.to(DEV).contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


def c64(a):
    return torch.from_numpy(np.asarray(a).astype(np.complex64))


def spy_on(monkeypatch, *names):
    """Count the calls of the named bindings."""
    calls = []
    for name in names:
        fn = getattr(ops.ext(), name)
        monkeypatch.setattr(
            ops.ext(), name,
            lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1])
    return calls


def forbid(monkeypatch, name):
    def reached(*a):
        raise AssertionError(name + " reached")
    monkeypatch.setattr(ops.ext(), name, reached)


# ----------------------------------------------------------- als_sweep ----

def als_binding_args(V22, C22, J, p, q, t_int):
    """The binding's argument order and index types."""
    return gpu(C22, V22, J, p.int(), q.int(), t_int.int())


@pytest.mark.parametrize("F,K,N,Ts,Tdelta", ALS_CASES)
def test_als_sweep_against_oracle(F, K, N, Ts, Tdelta):
    args = als_inputs(F, K, N, Ts, Tdelta, 11 * K + N)
    oracle, absout = als_contrib_oracle(*args)
    rhs, nm = ops.ext().als_sweep(*als_binding_args(*args))
    torch.cuda.synchronize()
    assert rhs.shape == oracle[0].shape and nm.shape == oracle[1].shape
    hold("als_sweep", f"{(F, K, N, Ts, Tdelta)}",
         als_contrib_figures((rhs, nm), oracle, absout))


@pytest.mark.parametrize("n_sweeps", SWEEP_COUNTS)
@pytest.mark.parametrize("F,K,N,Ts,Tdelta,prox", SWEEP_CASES)
def test_solve_sweeps_against_oracle(F, K, N, Ts, Tdelta, prox, n_sweeps,
                                     monkeypatch):
    inp, ref = sweep_reference((F, K, N, Ts, Tdelta, prox), n_sweeps)
    V22, C22, J, rho, target, p, q = inp
    eager = sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, n_sweeps)
    calls = spy_on(monkeypatch, "als_sweep", "gather_sum")
    got = sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, n_sweeps,
                    device=DEV)
    assert calls == ["als_sweep", "gather_sum", "gather_sum"] * n_sweeps
    ratio, _, err_eager, _ = complex_rule(got, eager, ref,
                                          sweep_length(K, N, Tdelta))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("solve_sweeps", f"{(F, K, N, Ts, Tdelta)},prox={prox},"
         f"sweeps={n_sweeps}", [("J", ratio)])


def test_als_sweep_nine_directions_take_the_torch_path(monkeypatch):
    """K = 9 is past the kernel's register arrays: the binding raises, and
    _solve_sweeps on the GPU runs the torch composition, which is held to
    the oracle like the kernels."""
    F, K, N, Ts, Tdelta = 1, 9, 7, 1, 3
    args = als_inputs(F, K, N, Ts, Tdelta, 11 * K + N)
    with pytest.raises(RuntimeError, match="K <= 8"):
        ops.ext().als_sweep(*als_binding_args(*args))
    V22, C22, J, rho, target, p, q = sweep_inputs(F, K, N, Ts, Tdelta,
                                                  False, 5 * K + N)
    ref = sweep_oracle(V22, C22, J, rho, target, N, Tdelta, 1)
    eager = sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, 1)
    forbid(monkeypatch, "als_sweep")
    forbid(monkeypatch, "gather_sum")
    got = sweep_run(V22, C22, J, rho, target, p, q, N, Tdelta, 1,
                    device=DEV)
    ratio, _, err_eager, _ = complex_rule(got, eager, ref,
                                          sweep_length(K, N, Tdelta))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("solve_sweeps", "K=9,torch path", [("J", ratio)])


def test_solve_sweeps_rejects_a_longer_last_interval_on_the_gpu():
    N, K, Ts, Tdelta, T = 7, 3, 2, 3, 7
    V22, C22, J, p, q, _ = als_inputs(1, K, N, 1, T, 1)
    J = J.expand(1, Ts, K, N, 2, 2).contiguous()
    with pytest.raises(ValueError, match="7 timeslots"):
        rs._solve_sweeps(*gpu(V22, C22, J, torch.ones(K)), None,
                         *gpu(p, q), N, Tdelta, 1)


# ---------------------------------------------------------- gather_sum ----

@pytest.mark.parametrize("F,X,S,G,Cnt,dup", GATHER_CASES)
def test_gather_sum_against_oracle(F, X, S, G, Cnt, dup):
    inp, gidx = gather_inputs(F, X, S, G, Cnt, dup, S + Cnt)
    out, absparts = gather_oracle(inp, gidx)
    got = ops.ext().gather_sum(*gpu(inp, gidx))
    assert got.shape == (F, X, G)
    re, im = complex_product_ratios(got, out, absparts, Cnt)
    hold("gather_sum", f"{(F, X, S, G, Cnt)}", [("re", re), ("im", im)])
    # Gaussian integers: every fp32 sum is exact
    inp, gidx = gather_inputs(F, X, S, G, Cnt, dup, S + Cnt, integer=True)
    got = ops.ext().gather_sum(*gpu(inp, gidx))
    assert torch.equal(got.cpu(), c64(gather_oracle(inp, gidx)[0]))


def test_gather_sum_on_the_solver_plan():
    N, Ts, Tdelta = 7, 2, 3
    plan = solver_plan(N, Ts, Tdelta)
    S = 2 * Ts * Tdelta * (N * (N - 1) // 2)
    assert plan.shape == (Ts * N, Tdelta * (N - 1))
    assert sorted(plan.reshape(-1).tolist()) == list(range(S))
    inp, _ = gather_inputs(2, 5, S, 1, 1, False, 3)
    out, absparts = gather_oracle(inp, plan)
    got = ops.ext().gather_sum(*gpu(inp, plan))
    re, im = complex_product_ratios(got, out, absparts, plan.shape[1])
    hold("gather_sum", "solver plan N=7,Ts=2,Tdelta=3",
         [("re", re), ("im", im)])
    inp, _ = gather_inputs(2, 5, S, 1, 1, False, 3, integer=True)
    got = ops.ext().gather_sum(*gpu(inp, plan))
    assert torch.equal(got.cpu(), c64(gather_oracle(inp, plan)[0]))


# ---------------------------------------------------------- hessianres ----

def hessianres_gpu(R, C, J, N):
    p, q = hs.baseline_pq(N, DEV)
    return ops.ext().hessianres(*gpu(C, R, J), p.int().contiguous(),
                                q.int().contiguous(), N)


@pytest.mark.parametrize("N,T,K", HESS_CASES)
def test_hessianres_against_oracle(N, T, K, monkeypatch):
    R, C, J = hess_inputs(N, T, K, 100 * N + T)
    H, aoff, adiag = hess_oracle(R, C, J, N)
    got = hessianres_gpu(R, C, J, N)
    assert got.shape == (K, 4 * N, 4 * N)
    hold("hessianres", f"{(N, T, K)}",
         hess_figures(got, H, aoff, adiag, N, T))
    assert hess_structure_ok(got, N) == (True, True)
    # the wrapper reaches the same kernel with the same arguments
    calls = spy_on(monkeypatch, "hessianres")
    via = hs.hessianres(*gpu(R, C, J), N)
    assert calls == ["hessianres"]
    # the diagonal blocks are summed by atomics in any order
    figs = hess_figures(via, H, aoff, adiag, N, T)
    assert max(r for _, r in figs) <= 1.0
    off = ~torch.eye(N, dtype=torch.bool).repeat_interleave(4, 0) \
        .repeat_interleave(4, 1)
    assert torch.equal(via.cpu()[:, off], got.cpu()[:, off])


@pytest.mark.parametrize("N,T", [(2, 1), (2, 4), (5, 3)])
def test_hessianres_on_integers(N, T):
    """Gaussian-integer inputs, every sum exact: bit for bit the oracle
    at N = 2, where B T is a power of two; at B T = 30 within the two
    roundings of inv = 1 / (B T) and of the product by it, each block
    kind on its own.

    With each baseline's partial sum scaled by inv before its atomicAdd,
    as the kernel first had it, a diagonal entry went through up to
    N + 1 = 6 roundings and missed this bound at (5, 3): error / bound
    2.91, against 0.82 for the off and mirror blocks. The diagonal blocks
    now accumulate unscaled and are scaled once."""
    R, C, J = hess_inputs(N, T, 2, N + T, integer=True)
    H = hess_oracle(R, C, J, N)[0]
    got = hessianres_gpu(R, C, J, N)
    if N == 2:
        assert torch.equal(got.cpu(), c64(H))
    else:
        hold("hessianres", f"integers {(N, T)}",
             hess_integer_figures(got, H, N))
    assert hess_structure_ok(got, N) == (True, True)


# ------------------------------------------------------------ two-loop ----

@pytest.mark.parametrize("h,n,m", TWO_LOOP_CASES)
def test_two_loop_against_oracle(h, n, m):
    Y, S, Q, ro, gamma = two_loop_inputs(h, n, m, 31 * h + n)
    ref = two_loop_oracle(Y, S, Q, ro, gamma)
    eager = two_loop_eager(Y, S, Q)
    got = ops.ext().two_loop_apply(*gpu(Y, S, Q, ro), gamma)
    assert got.shape == (m, n)
    ratio, _, err_eager, _ = rule_ratio(got, eager, ref, two_loop_length(h))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("two_loop", f"{(h, n, m)}", [("R", ratio)])


def test_two_loop_filtered_pairs():
    """ro[1] = ro[4] = 0 through the binding, against the oracle and the
    eager path on the five remaining pairs."""
    h, n, m = 7, 20, 20
    Y, S, Q, ro, gamma = two_loop_inputs(h, n, m, 5)
    keep = [0, 2, 3, 5, 6]
    ro_f = ro.clone()
    ro_f[[1, 4]] = 0.0
    ref = two_loop_oracle(Y[keep], S[keep], Q, ro[keep], gamma)
    eager = two_loop_eager(Y[keep], S[keep], Q)
    got = ops.ext().two_loop_apply(*gpu(Y, S, Q, ro_f), gamma)
    ratio, _, err_eager, _ = rule_ratio(got, eager, ref, two_loop_length(h))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("two_loop", "(7, 20, 20),pairs 1 and 4 filtered", [("R", ratio)])


def test_two_loop_without_history_scales_by_gamma():
    _, _, Q, _, _ = two_loop_inputs(7, 20, 20, 5)
    empty = torch.zeros(0, 20)
    got = ops.ext().two_loop_apply(*gpu(empty, empty, Q, torch.zeros(0)),
                                   0.37)
    assert torch.equal(got.cpu(), Q * np.float32(0.37))


class _History:
    """What inv_hessian_mult reads of an L-BFGS optimizer."""

    def __init__(self, Y, S):
        self.pairs = {"old_dirs": list(Y), "old_stps": list(S)}

    def state_dict(self):
        return {"state": {0: self.pairs}}


def _wrapper_oracle(Y, S, Q):
    """ro and gamma as the wrappers form them, in float64."""
    ys = (Y.double() * S.double()).sum(1)
    gamma = float(ys[-1] / (Y[-1].double() ** 2).sum())
    Y64, S64, Q64 = (t.double().numpy() for t in (Y, S, Q))
    h = Y.shape[0]
    ro = 1.0 / ys.numpy()
    q = Q64.copy()
    al = np.zeros((h, q.shape[0]))
    for i in range(h - 1, -1, -1):
        al[i] = (q @ S64[i]) * ro[i]
        q -= np.outer(al[i], Y64[i])
    r = gamma * q
    for i in range(h):
        r += np.outer(al[i] - (r @ Y64[i]) * ro[i], S64[i])
    return r


def test_two_loop_through_the_wrappers(monkeypatch):
    h, n, m = 7, 20, 20
    Y, S, Q, _, _ = two_loop_inputs(h, n, m, 31 * h + n)
    ref = _wrapper_oracle(Y, S, Q)
    eager = two_loop_eager(Y, S, Q)
    calls = spy_on(monkeypatch, "two_loop_apply")
    got = at_.inv_hessian_mult_mat(*gpu(Y, S, Q.t().contiguous()))
    assert got.shape == (n, m) and calls == ["two_loop_apply"]
    figures = [("mat", rule_ratio(got.t(), eager, ref,
                                  two_loop_length(h))[0])]
    # one vector through the optimizer-history form; q is scratch and
    # holds the result afterwards
    Yg, Sg = gpu(Y, S)
    q = Q[3].clone().to(DEV)
    r = at_.inv_hessian_mult(_History(Yg, Sg), q)
    assert calls == ["two_loop_apply"] * 2 and torch.equal(q, r)
    eager_v = at_.inv_hessian_mult(_History(Y, S), Q[3].clone())
    figures.append(("vec", rule_ratio(r, eager_v, ref[3],
                                      two_loop_length(h))[0]))
    hold("two_loop", "(7, 20, 20),wrappers", figures)


def test_two_loop_seventeen_pairs_fall_back(monkeypatch):
    h, n, m = 17, 40, 3
    Y, S, Q, ro, gamma = two_loop_inputs(h, n, m, 9)
    with pytest.raises(RuntimeError, match="history"):
        ops.ext().two_loop_apply(*gpu(Y, S, Q, ro), gamma)
    ref = _wrapper_oracle(Y, S, Q)
    eager = two_loop_eager(Y, S, Q)
    forbid(monkeypatch, "two_loop_apply")
    got = at_.inv_hessian_mult_mat(*gpu(Y, S, Q.t().contiguous()))
    ratio, _, err_eager, _ = rule_ratio(got.t(), eager, ref,
                                        two_loop_length(h))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("two_loop", "(17, 40, 3),torch path", [("R", ratio)])


# --------------------------------------------------------------- cgemm ----

@pytest.mark.parametrize("KA,rep,M,Kd,N", CGEMM_CASES)
def test_cgemm_against_oracle(KA, rep, M, Kd, N):
    A, B = cgemm_inputs(KA, rep, M, Kd, N, M + Kd + N)
    C, absparts = cgemm_oracle(A, B, rep)
    got = ops.ext().cgemm_nn_bcast(*gpu(A, B), rep)
    assert got.shape == (KA * rep, M, N)
    re, im = complex_product_ratios(got, C, absparts, 2 * Kd)
    hold("cgemm", f"{(KA, rep, M, Kd, N)}", [("re", re), ("im", im)])
    # Gaussian integers: exact
    A, B = cgemm_inputs(KA, rep, M, Kd, N, M + Kd + N, integer=True)
    got = ops.ext().cgemm_nn_bcast(*gpu(A, B), rep)
    assert torch.equal(got.cpu(), c64(cgemm_oracle(A, B, rep)[0]))


# ------------------------------------------------------ launch hygiene ----

def _follow_up_cgemm():
    A, B = cgemm_inputs(3, 8, 65, 33, 17, 1, integer=True)
    got = ops.ext().cgemm_nn_bcast(*gpu(A, B), 8)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c64(cgemm_oracle(A, B, 8)[0]))


def _follow_up_gather():
    inp, gidx = gather_inputs(2, 3, 300, 5, 65, False, 1, integer=True)
    got = ops.ext().gather_sum(*gpu(inp, gidx))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c64(gather_oracle(inp, gidx)[0]))


def _zc(*shape):
    return torch.zeros(*shape, device=DEV, dtype=torch.complex64)


def _zf(*shape):
    return torch.zeros(*shape, device=DEV)


def _zi(n, dtype=torch.int32):
    return torch.zeros(n, device=DEV, dtype=dtype)


def _empty_als_sweep(e):
    # T = 0
    rhs, nm = e.als_sweep(_zc(2, 3, 0, 21, 2, 2), _zc(2, 0, 21, 2, 2),
                          _zc(2, 1, 3, 7, 2, 2), _zi(21), _zi(21), _zi(0))
    assert rhs.shape == (2, 12, 0) and nm.shape == (2, 36, 0)
    # no frequency, no direction
    rhs, nm = e.als_sweep(_zc(0, 3, 2, 21, 2, 2), _zc(0, 2, 21, 2, 2),
                          _zc(0, 1, 3, 7, 2, 2), _zi(21), _zi(21), _zi(2))
    assert rhs.shape == (0, 12, 84) and nm.shape == (0, 36, 84)
    rhs, nm = e.als_sweep(_zc(1, 0, 2, 21, 2, 2), _zc(1, 2, 21, 2, 2),
                          _zc(1, 1, 0, 7, 2, 2), _zi(21), _zi(21), _zi(2))
    assert rhs.shape == (1, 0, 84) and nm.shape == (1, 0, 84)


def _empty_cgemm(e):
    assert e.cgemm_nn_bcast(_zc(2, 0, 5), _zc(4, 5, 3), 2).shape == (4, 0, 3)
    assert e.cgemm_nn_bcast(_zc(2, 6, 5), _zc(4, 5, 0), 2).shape == (4, 6, 0)
    assert e.cgemm_nn_bcast(_zc(0, 6, 5), _zc(0, 5, 3), 2).shape == (0, 6, 3)
    # an empty sum is zero
    assert torch.equal(e.cgemm_nn_bcast(_zc(2, 6, 0), _zc(4, 0, 3), 2),
                       _zc(4, 6, 3))


def _empty_gather_sum(e):
    gidx = _zi(12, torch.int64).reshape(3, 4)
    assert e.gather_sum(_zc(0, 5, 9), gidx).shape == (0, 5, 3)
    assert e.gather_sum(_zc(2, 0, 9), gidx).shape == (2, 0, 3)
    assert e.gather_sum(_zc(2, 5, 9), gidx[:0]).shape == (2, 5, 0)
    ones = torch.ones(2, 5, 9, device=DEV, dtype=torch.complex64)
    assert torch.equal(e.gather_sum(ones, gidx[:, :0].contiguous()),
                       _zc(2, 5, 3))


def _empty_two_loop(e):
    Y, S, ro = _zf(3, 8), _zf(3, 8), _zf(3)
    assert e.two_loop_apply(Y, S, _zf(0, 8), ro, 1.0).shape == (0, 8)
    assert e.two_loop_apply(_zf(3, 0), _zf(3, 0), _zf(4, 0), ro,
                            1.0).shape == (4, 0)


def _empty_hessianres(e):
    H = e.hessianres(_zc(0, 6, 4), _zc(12, 2), _zc(0, 6, 2), _zi(3), _zi(3),
                     3)
    assert H.shape == (0, 12, 12)


EMPTY_CALLS = [_empty_als_sweep, _empty_cgemm, _empty_gather_sum,
               _empty_two_loop, _empty_hessianres]


@pytest.mark.parametrize("empty", EMPTY_CALLS, ids=lambda f: f.__name__[7:])
def test_empty_call_launches_nothing_and_leaves_no_error(empty):
    """An empty call returns its correctly shaped result, and the next
    binding, another one, runs and is right: no zero-block launch left
    its error behind."""
    empty(ops.ext())
    torch.cuda.synchronize()
    if "cgemm" in empty.__name__:
        _follow_up_gather()
    else:
        _follow_up_cgemm()


def _noncontiguous(t):
    """Same shape and values, strides doubled."""
    out = torch.stack([t, t], dim=-1)[..., 0]
    assert not out.is_contiguous() and out.shape == t.shape
    return out


def _other_dtype(t):
    return t.to({torch.complex64: torch.complex128,
                 torch.float32: torch.float64, torch.int32: torch.int64,
                 torch.int64: torch.int32}[t.dtype])


def _rejects(fn, good, tail, shapes):
    """fn(*good, *tail) runs; with any one tensor of ``good`` in another
    dtype, on the CPU, non-contiguous or in one of its wrong ``shapes`` it
    raises RuntimeError."""
    fn(*good, *tail)
    for i, t in enumerate(good):
        variants = [_other_dtype(t), t.cpu(), _noncontiguous(t)]
        variants += [cut(t).contiguous() for cut in shapes[i]]
        for v in variants:
            bad = list(good)
            bad[i] = v
            with pytest.raises(RuntimeError):
                fn(*bad, *tail)


def test_als_sweep_rejects_bad_arguments():
    good = als_binding_args(*als_inputs(2, 3, 7, 2, 3, 1))
    _rejects(ops.ext().als_sweep, good, (), [
        [lambda t: t[:, :, :, :-1], lambda t: t[:, :, :-1], lambda t: t[0],
         lambda t: t[..., :1]],
        [lambda t: t[:, :-1], lambda t: t[:1], lambda t: t[0]],
        [lambda t: t[:1], lambda t: t[:, :, :-1], lambda t: t[0]],
        [lambda t: t[:-1], lambda t: t.reshape(3, 7)],
        [lambda t: t[:-1]],
        [lambda t: t[:-1]]])
    _follow_up_cgemm()


def test_cgemm_rejects_bad_arguments():
    e = ops.ext()
    good = gpu(*cgemm_inputs(2, 2, 17, 9, 5, 1))
    _rejects(e.cgemm_nn_bcast, good, (2,), [
        [lambda t: t[:, :, :-1], lambda t: t[:1], lambda t: t[0]],
        [lambda t: t[:-1], lambda t: t[:, :-1], lambda t: t[0]]])
    for rep in (0, -2, 3):
        with pytest.raises(RuntimeError):
            e.cgemm_nn_bcast(*good, rep)
    with pytest.raises(RuntimeError, match="grid"):
        e.cgemm_nn_bcast(_zc(1, 1, 1), _zc(65536, 1, 1), 65536)
    _follow_up_gather()


def test_gather_sum_rejects_bad_arguments():
    good = gpu(*gather_inputs(2, 3, 300, 5, 65, False, 1))
    _rejects(ops.ext().gather_sum, good, (), [
        [lambda t: t[0], lambda t: t[None]],
        [lambda t: t[0], lambda t: t[None]]])
    _follow_up_cgemm()


def test_two_loop_rejects_bad_arguments():
    Y, S, Q, ro, gamma = two_loop_inputs(5, 40, 3, 1)
    _rejects(ops.ext().two_loop_apply, gpu(Y, S, Q, ro), (gamma,), [
        [lambda t: t[:-1], lambda t: t[:, :-1], lambda t: t[0]],
        [lambda t: t[:-1], lambda t: t[:, :-1], lambda t: t[0]],
        [lambda t: t[:, :-1], lambda t: t[0]],
        [lambda t: t[:-1], lambda t: t[:, None]]])
    _follow_up_cgemm()


def test_hessianres_rejects_bad_arguments():
    e = ops.ext()
    N, T, K = 5, 3, 2
    R, C, J = hess_inputs(N, T, K, 1)
    p, q = hs.baseline_pq(N, DEV)
    good = gpu(C, R, J) + (p.int().contiguous(), q.int().contiguous())
    _rejects(e.hessianres, good, (N,), [
        [lambda t: t[:, :-1], lambda t: t[..., :3], lambda t: t[0]],
        [lambda t: t[:-2], lambda t: t[:, :1], lambda t: t.reshape(-1)],
        [lambda t: t[:1], lambda t: t[:, :-2], lambda t: t[0]],
        [lambda t: t[:-1]],
        [lambda t: t[:-1]]])
    # N < 2 (B = 0 was a division by zero on the host), no sample, a
    # sample count that is no multiple of B
    for n_bad in (1, 0, -3):
        with pytest.raises(RuntimeError):
            e.hessianres(_zc(K, 30, 4), _zc(60, 2), _zc(K, 2 * max(n_bad, 0),
                                                       2),
                         _zi(0), _zi(0), n_bad)
    with pytest.raises(RuntimeError):
        e.hessianres(_zc(K, 0, 4), _zc(0, 2), good[2], good[3], good[4], N)
    with pytest.raises(RuntimeError):
        e.hessianres(_zc(K, 25, 4), _zc(50, 2), good[2], good[3], good[4], N)
    with pytest.raises(RuntimeError, match="grid"):
        e.hessianres(_zc(65536, 1, 4), _zc(2, 2), _zc(65536, 4, 2), _zi(1),
                     _zi(1), 2)
    _follow_up_cgemm()
