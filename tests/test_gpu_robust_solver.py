"""The weighted ALS sweep and the residual/weights kernel (als_sweep.hip,
robust.hip) against the complex128 / float64 oracles of
test_robust_solver.py, and weights, flags, the uv cut and the robust noise
model through `calibrate` and `CalibEnv` on the GPU.

Each comparison prints ``ratio <family> <case> <output> <error / bound>``
before it asserts ``<= 1``; docs/TESTING.md records the worst per family.
Index arguments are only ever the ones the callers build.
"""

import numpy as np
import pytest
import torch

from test_radio_kernel_oracles import (
    ALS_CASES, SWEEP_CASES, SWEEP_COUNTS, als_inputs, cgemm_inputs,
    cgemm_oracle, complex_rule, sweep_length)
from test_robust_solver import (
    RW_CASES, E2E_SEEDS, als_contrib_w_figures, als_w_reference,
    calib_env_default_unchanged, calib_env_robust_steps, e2e_hold, hold,
    power_of_two_identity, rw_figures, rw_inputs, rw_reference,
    rw_sum_ratio, station_without_weight_keeps_its_jones, sweep_w_reference,
    sweep_w_run, unit_weight_identity, uv_cut_weights)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import smartcal_amd.ops as ops
    from smartcal_amd.radio import solver as rs
    DEV = torch.device("cuda:0")
else:
    DEV = None


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_hip(), "HIP extension must be loaded on a GPU box"


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


# --------------------------------------------------------- als_sweep_w ----

def als_w_binding(V22, C22, J, w, p, q, t_int):
    """The weighted binding in the oracle's argument order."""
    return ops.ext().als_sweep_w(*gpu(C22, V22, J, w, p.int(), q.int(),
                                      t_int.int()))


def als_binding(V22, C22, J, p, q, t_int):
    return ops.ext().als_sweep(*gpu(C22, V22, J, p.int(), q.int(),
                                    t_int.int()))


@pytest.mark.parametrize("case", ALS_CASES, ids=str)
def test_als_sweep_w_against_oracle(case):
    args, w, oracle, absout = als_w_reference(case)
    rhs, nm = als_w_binding(*args[:3], w, *args[3:])
    torch.cuda.synchronize()
    assert rhs.shape == oracle[0].shape and nm.shape == oracle[1].shape
    hold("als_sweep_w", f"{case}",
         als_contrib_w_figures((rhs, nm), oracle, absout))


@pytest.mark.parametrize("case", ALS_CASES, ids=str)
def test_als_sweep_w_identities(case):
    assert unit_weight_identity(als_w_binding, als_binding, case)
    assert power_of_two_identity(als_w_binding, als_binding, case)


@pytest.mark.parametrize("n_sweeps", SWEEP_COUNTS)
@pytest.mark.parametrize("case", SWEEP_CASES, ids=str)
def test_weighted_solve_sweeps_against_oracle(case, n_sweeps, monkeypatch):
    F, K, N, Ts, Tdelta, prox = case
    inp, w, ref = sweep_w_reference(case, n_sweeps)
    V22, C22, J, rho, target, p, q = inp
    eager = sweep_w_run(V22, C22, J, rho, target, w, p, q, N, Tdelta,
                        n_sweeps)
    calls = spy_on(monkeypatch, "als_sweep", "als_sweep_w", "gather_sum")
    got = sweep_w_run(V22, C22, J, rho, target, w, p, q, N, Tdelta,
                      n_sweeps, device=DEV)
    assert calls == ["als_sweep_w", "gather_sum", "gather_sum"] * n_sweeps
    ratio, _, err_eager, _ = complex_rule(got, eager, ref,
                                          sweep_length(K, N, Tdelta))
    assert err_eager <= 1e-5 * np.abs(ref).max()
    hold("solve_sweeps_w", f"{case},sweeps={n_sweeps}", [("J", ratio)])


def test_station_without_weight_keeps_its_jones_on_the_gpu():
    station_without_weight_keeps_its_jones(DEV)


# ------------------------------------------------ vis_residual_weights ----

def rw_binding(V22, C22, J, m, nu, sigma2, p, q, t_int):
    return ops.ext().vis_residual_weights(
        *gpu(C22, V22, J, m, nu, sigma2, p.int(), q.int(), t_int.int()))


@pytest.mark.parametrize("case", RW_CASES, ids=str)
def test_vis_residual_weights_against_oracle(case):
    F, K, N, Ts, Tdelta = case
    inp, oracle = rw_reference(case)
    V22, C22, J, m, nu, sigma2, p, q, t_int = inp
    r, e2, w, part = rw_binding(*inp)
    torch.cuda.synchronize()
    TB = Ts * Tdelta * (N * (N - 1) // 2)
    assert r.shape == (F, TB, 4) and r.dtype == torch.complex64
    assert e2.shape == w.shape == m.shape and w.dtype == torch.float32
    assert part.shape == (F, -(-TB // 256), 4)
    assert part.dtype == torch.float64
    figs = rw_figures(r, e2, w, oracle, m, nu, sigma2, K)
    figs.append(("sums", rw_sum_ratio(part.sum(dim=1), m, e2, w)))
    hold("vis_residual_weights", f"{case}", figs)
    # the order of the reduction is fixed: the same bits again
    again = rw_binding(*inp)
    torch.cuda.synchronize()
    for a, b in zip((r, e2, w, part), again):
        assert torch.equal(a, b)
    # and the solver's wrapper reaches the kernel and sums its partials
    via = rs._residual_weights(*gpu(C22, V22, J, m, nu, sigma2, p, q, t_int))
    assert torch.equal(via[0], r) and torch.equal(via[2], w)
    assert torch.equal(via[3], part.sum(dim=1))


# ------------------------------------------------------ launch hygiene ----

def _follow_up_cgemm():
    A, B = cgemm_inputs(3, 8, 65, 33, 17, 1, integer=True)
    got = ops.ext().cgemm_nn_bcast(*gpu(A, B), 8)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c64(cgemm_oracle(A, B, 8)[0]))


def _zc(*shape):
    return torch.zeros(*shape, device=DEV, dtype=torch.complex64)


def _zf(*shape):
    return torch.zeros(*shape, device=DEV)


def _zi(n):
    return torch.zeros(n, device=DEV, dtype=torch.int32)


def _empty_als_sweep_w(e):
    # T = 0
    rhs, nm = e.als_sweep_w(_zc(2, 3, 0, 21, 2, 2), _zc(2, 0, 21, 2, 2),
                            _zc(2, 1, 3, 7, 2, 2), _zf(2, 0, 21), _zi(21),
                            _zi(21), _zi(0))
    assert rhs.shape == (2, 12, 0) and nm.shape == (2, 36, 0)
    # no frequency, no direction
    rhs, nm = e.als_sweep_w(_zc(0, 3, 2, 21, 2, 2), _zc(0, 2, 21, 2, 2),
                            _zc(0, 1, 3, 7, 2, 2), _zf(0, 2, 21), _zi(21),
                            _zi(21), _zi(2))
    assert rhs.shape == (0, 12, 84) and nm.shape == (0, 36, 84)
    rhs, nm = e.als_sweep_w(_zc(1, 0, 2, 21, 2, 2), _zc(1, 2, 21, 2, 2),
                            _zc(1, 1, 0, 7, 2, 2), _zf(1, 2, 21), _zi(21),
                            _zi(21), _zi(2))
    assert rhs.shape == (1, 0, 84) and nm.shape == (1, 0, 84)


def _empty_vis_residual_weights(e):
    # T = 0
    r, e2, w, part = e.vis_residual_weights(
        _zc(2, 3, 0, 21, 2, 2), _zc(2, 0, 21, 2, 2), _zc(2, 1, 3, 7, 2, 2),
        _zf(2, 0, 21), _zf(2), _zf(2), _zi(21), _zi(21), _zi(0))
    assert r.shape == (2, 0, 4) and e2.shape == w.shape == (2, 0, 21)
    assert part.shape == (2, 0, 4) and part.dtype == torch.float64
    # no frequency
    r, e2, w, part = e.vis_residual_weights(
        _zc(0, 3, 2, 21, 2, 2), _zc(0, 2, 21, 2, 2), _zc(0, 1, 3, 7, 2, 2),
        _zf(0, 2, 21), _zf(0), _zf(0), _zi(21), _zi(21), _zi(2))
    assert r.shape == (0, 42, 4) and e2.shape == w.shape == (0, 2, 21)
    assert part.shape == (0, 1, 4)
    # no direction: the model is zero and the residual is the data
    V = torch.ones(1, 2, 21, 2, 2, device=DEV, dtype=torch.complex64)
    r, e2, w, part = e.vis_residual_weights(
        _zc(1, 0, 2, 21, 2, 2), V, _zc(1, 1, 0, 7, 2, 2),
        torch.ones(1, 2, 21, device=DEV), torch.full((1,), 2.0, device=DEV),
        torch.ones(1, device=DEV), _zi(21), _zi(21), _zi(2))
    assert torch.equal(r, V.reshape(1, 42, 4))
    assert torch.equal(e2, torch.full((1, 2, 21), 4.0, device=DEV))
    assert torch.equal(w, torch.full((1, 2, 21), 10.0 / 6.0, device=DEV))
    assert part.shape == (1, 1, 4) and float(part[0, 0, 0]) == 42.0


@pytest.mark.parametrize("empty", [_empty_als_sweep_w,
                                   _empty_vis_residual_weights],
                         ids=lambda f: f.__name__[7:])
def test_empty_call_launches_nothing_and_leaves_no_error(empty):
    empty(ops.ext())
    torch.cuda.synchronize()
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


def _rejects(fn, good, shapes):
    """fn(*good) runs; with any one tensor of ``good`` in another dtype,
    on the CPU, non-contiguous or in one of its wrong ``shapes`` it raises
    RuntimeError."""
    fn(*good)
    for i, t in enumerate(good):
        variants = [_other_dtype(t), t.cpu(), _noncontiguous(t)]
        variants += [cut(t).contiguous() for cut in shapes[i]]
        for v in variants:
            bad = list(good)
            bad[i] = v
            with pytest.raises(RuntimeError):
                fn(*bad)


_C22_CUTS = [lambda t: t[:, :, :, :-1], lambda t: t[:, :, :-1],
             lambda t: t[0], lambda t: t[..., :1]]
_V22_CUTS = [lambda t: t[:, :-1], lambda t: t[:1], lambda t: t[0]]
_J_CUTS = [lambda t: t[:1], lambda t: t[:, :, :-1], lambda t: t[0]]
_W_CUTS = [lambda t: t[:, :-1], lambda t: t[:1], lambda t: t[0],
           lambda t: t[..., :-1]]
_F_CUTS = [lambda t: t[:-1], lambda t: t[:, None]]
_P_CUTS = [lambda t: t[:-1], lambda t: t.reshape(3, 7)]


def test_als_sweep_w_rejects_bad_arguments():
    V22, C22, J, p, q, t_int = als_inputs(2, 3, 7, 2, 3, 1)
    w = torch.ones(V22.shape[:3])
    good = gpu(C22, V22, J, w, p.int(), q.int(), t_int.int())
    _rejects(ops.ext().als_sweep_w, good, [
        _C22_CUTS, _V22_CUTS, _J_CUTS, _W_CUTS, _P_CUTS,
        [lambda t: t[:-1]], [lambda t: t[:-1]]])
    args = als_inputs(1, 9, 7, 1, 3, 2)
    with pytest.raises(RuntimeError, match="K <= 8"):
        als_w_binding(*args[:3], torch.ones(args[0].shape[:3]), *args[3:])
    _follow_up_cgemm()


def test_vis_residual_weights_rejects_bad_arguments():
    V22, C22, J, m, nu, sigma2, p, q, t_int = rw_inputs(2, 3, 7, 2, 3, 1)
    good = gpu(C22, V22, J, m, nu, sigma2, p.int(), q.int(), t_int.int())
    _rejects(ops.ext().vis_residual_weights, good, [
        _C22_CUTS, _V22_CUTS, _J_CUTS, _W_CUTS, _F_CUTS, _F_CUTS, _P_CUTS,
        [lambda t: t[:-1]], [lambda t: t[:-1]]])
    _follow_up_cgemm()


# ------------------------------------------------------------ end to end ----

@pytest.mark.parametrize("seed", E2E_SEEDS)
def test_robust_and_flags_recover_the_clean_solution_on_the_gpu(seed):
    e2e_hold(seed, DEV)


def test_calibrate_launches_the_weighted_kernels(monkeypatch):
    """robust=True: every sweep is als_sweep_w, and the residual/weights
    kernel runs once for the first sigma2, once before every n_sweeps of
    the initial sweeps, once per ADMM iteration (every robust_every-th)
    and once for the final residual. The default call reaches neither."""
    from test_robust_solver import e2e_scenario
    vis, bad, mask, sky, cs, rho, C = e2e_scenario(0, DEV)
    calls = spy_on(monkeypatch, "als_sweep", "als_sweep_w",
                   "vis_residual_weights")
    rs.calibrate(bad, sky, cs, rho, C_cache=C, admm_iter=3, n_sweeps=2,
                 init_sweeps=4, robust=True)
    round_ = ["vis_residual_weights", "als_sweep_w", "als_sweep_w"]
    assert calls == ["vis_residual_weights"] + round_ * 2 + round_ * 3 \
        + ["vis_residual_weights"]
    del calls[:]
    rs.calibrate(bad, sky, cs, rho, C_cache=C, admm_iter=3, n_sweeps=2,
                 init_sweeps=4, robust=True, robust_every=2)
    assert calls.count("vis_residual_weights") == 1 + 2 + 2 + 1
    assert calls.count("als_sweep_w") == 10
    del calls[:]
    # flags without the robust model: weighted sweeps, one final launch
    from dataclasses import replace
    rs.calibrate(replace(bad, flags=mask), sky, cs, rho, C_cache=C,
                 admm_iter=3, n_sweeps=2, init_sweeps=4)
    assert calls == ["als_sweep_w"] * 10 + ["vis_residual_weights"]
    del calls[:]
    rs.calibrate(bad, sky, cs, rho, C_cache=C, admm_iter=3, n_sweeps=2,
                 init_sweeps=4)
    assert calls == ["als_sweep"] * 10


def test_uv_cut_gives_zero_and_one_weights_on_the_gpu():
    uv_cut_weights(DEV)


def test_calib_env_robust_with_rfi_resets_and_steps_on_the_gpu():
    calib_env_robust_steps(DEV)


def test_calib_env_default_is_unchanged_on_the_gpu():
    calib_env_default_unchanged(DEV, exact_image=False)
