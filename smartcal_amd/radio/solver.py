"""Direction-dependent calibration solver with consensus ADMM.

The in-repo replacement for the external ``sagecal_gpu`` /
``mpirun sagecal-mpi_gpu`` binaries the reference shells out to
(`calibration/docal.sh:12`, `demixing_rl/demixingenv.py:129`,
SURVEY.md §2.2 N13/N14). MI355X-first design:

* **J-step** — joint full-Jones alternating least squares: fixing all
  other stations, each station's stacked per-direction Jones
  G_p = [J¹_p … J^K_p] (2×2K) has a closed-form solution from 2K×2K
  normal equations. All stations, solution intervals and frequencies are
  solved as ONE batched ``torch.linalg.solve`` per sweep (GEMM-shaped
  work), with 0.5 averaging damping à la StefCal. The ADMM proximal term
  ρ_k‖J^k − B_f Z^k + Y^k/ρ_k‖² enters the normal equations exactly.
* **Z-step** — consensus polynomial over frequency (`-P` order, ordinary
  or Bernstein basis as `consensus_poly`, `calibration_tools.py:551-585`):
  closed-form per direction via the (Ne×Ne) pinv, with federated-averaging
  spatial regularization α. When ``torch.distributed`` is initialized the
  per-frequency partial sums are combined with ONE flat all_reduce (RCCL
  over xGMI); single-process mode sums locally over its frequencies.
* **Y-step** — dual ascent.

Interfaces are in-memory tensors (`radio.sim.VisData`); solutions are
returned in the reference's J layout (K, 2N·Ts, 2) so the influence
pipeline (`radio.influence`) and text writers consume them directly.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from .consensus import bpoly
from .hessian import baseline_pq
from .coherency import predict_coherencies_uvw
from .sim import VisData, apply_jones

__all__ = ["CalSolution", "calibrate"]


@dataclass
class CalSolution:
    J: torch.Tensor          # (Nf_local, K, Ts, N, 2, 2) complex64
    Z: torch.Tensor          # (K, Ne, Ts, N, 2, 2) complex64 (global)
    residual: torch.Tensor   # (Nf_local, S, 4) complex64 = data − model
    freqs: np.ndarray        # local frequencies
    rho: np.ndarray          # per-direction spectral rho used
    # set when weights, flags, a uv cut or the robust model are in use:
    weights: torch.Tensor | None = None   # (Nf_local, S) final weights
    nu: torch.Tensor | None = None        # (Nf_local,) Student's-t ν
    sigma2: torch.Tensor | None = None    # (Nf_local,) noise variance

    def J_ref_layout(self, fi: int) -> torch.Tensor:
        """J for local freq fi in the reference layout (K, 2N·Ts, 2)
        (`calibration_tools.py:105-119`)."""
        K = self.J.shape[1]
        return self.J[fi].reshape(K, -1, 2)


def _poly_basis(freqs: np.ndarray, f_all: np.ndarray, f0: float, Ne: int,
                polytype: int) -> np.ndarray:
    """Rows of the frequency polynomial basis for ``freqs``, defined over
    the global frequency set ``f_all`` (Bernstein normalization needs the
    global min/max, as in `consensus_poly`)."""
    if polytype == 0:
        B = np.zeros((len(freqs), Ne))
        B[:, 0] = 1.0
        ff = (freqs - f0) / f0
        for cj in range(1, Ne):
            B[:, cj] = ff ** cj
    else:
        lo, hi = f_all.min(), f_all.max()
        ff = (freqs - lo) / (hi - lo) if hi > lo else np.zeros_like(freqs)
        B = bpoly(ff, Ne - 1).astype(np.float64)
    return B


def _als_contributions_torch(data22, C22, J, p_idx, q_idx, t_int):
    """Per-sample normal-equation contributions of one ALS sweep, the
    torch composition of ops/csrc/als_sweep.hip: (rhs_cat (F, 2·2K, 2TB),
    nm_cat (F, 2K·2K, 2TB)), the p-side samples in columns [0, TB), the
    q-side ones in [TB, 2TB)."""
    F, T, Bn = data22.shape[0], data22.shape[1], data22.shape[2]
    K = C22.shape[1]
    # A^k for p-side rows: A = C_pq (J^k_q)^H ; for q-side rows:
    # A' = C_pq^H (J^k_p)^H  (from V_pq^H = Σ J^k_q C^H J_p^H)
    Jt = J[:, t_int]                               # (F,T,K,N,2,2)
    Jq = Jt[:, :, :, q_idx]                        # (F,T,K,B,2,2)
    Jp = Jt[:, :, :, p_idx]
    Cp = C22.permute(0, 2, 3, 1, 4, 5)             # (F,T,B,K,2,2)
    # elementwise small-complex products (radio.small_complex):
    # batched 2×2 / k=2 shapes are pathological for rocBLAS
    from .small_complex import mm2H, Hmm2, abH_k2
    A_p = mm2H(Cp, Jq.permute(0, 1, 3, 2, 4, 5))   # (F,T,B,K,2,2)
    A_q = Hmm2(Cp, Jp.permute(0, 1, 3, 2, 4, 5).conj().mT)
    V = data22                                      # (F,T,B,2,2)
    # per (station, interval): normal matrix (2K,2K), rhs (2,2K)
    # W = A stacked over k → (2K,2); contribs V·W^H and W·W^H
    Wp = A_p.reshape(F, T, Bn, 2 * K, 2)
    Wq = A_q.reshape(F, T, Bn, 2 * K, 2)
    rhs_p = abH_k2(V, Wp)                           # (F,T,B,2,2K)
    rhs_q = abH_k2(V.mH, Wq)
    nm_p = abH_k2(Wp, Wp)                           # (F,T,B,2K,2K)
    nm_q = abH_k2(Wq, Wq)
    rhs_cat = torch.cat(
        [rhs_p.reshape(F, T * Bn, 2 * 2 * K),
         rhs_q.reshape(F, T * Bn, 2 * 2 * K)], dim=1) \
        .permute(0, 2, 1)
    nm_cat = torch.cat(
        [nm_p.reshape(F, T * Bn, 2 * K * 2 * K),
         nm_q.reshape(F, T * Bn, 2 * K * 2 * K)], dim=1) \
        .permute(0, 2, 1)
    return rhs_cat, nm_cat


def _als_contributions_torch_w(data22, C22, J, w, p_idx, q_idx, t_int):
    """`_als_contributions_torch` for the weighted cost Σ_s w_s ‖V_s − …‖²,
    w (F, T, B) ≥ 0: every entry of a sample times its weight, the torch
    composition of als_sweep_w_kernel."""
    rhs_cat, nm_cat = _als_contributions_torch(data22, C22, J, p_idx, q_idx,
                                               t_int)
    F = w.shape[0]
    w2 = torch.cat([w.reshape(F, 1, -1)] * 2, dim=2)       # (F, 1, 2TB)
    return rhs_cat * w2, nm_cat * w2


def _residual_weights_torch(C22, data22, J, m, nu, sigma2, p_idx, q_idx,
                            t_int):
    """The torch composition of ops/csrc/robust.hip: residual r (F, S, 4)
    of the model Σ_k J_p C_k J_q^H, e² (F, T, B) the squared norm of its
    8 real components, the Student's-t weight
    w = m (ν + 8) / (ν + e²/σ²) and the float64 sums (F, 4) of m, w e², w
    and m (ln w − w), the last over the samples with m > 0."""
    from .small_complex import mm2, mm2H
    F, T, Bn = data22.shape[0], data22.shape[1], data22.shape[2]
    Jt = J[:, t_int]                               # (F,T,K,N,2,2)
    Jp = Jt[:, :, :, p_idx]                        # (F,T,K,B,2,2)
    Jq = Jt[:, :, :, q_idx]
    Cp = C22.permute(0, 2, 1, 3, 4, 5)             # (F,T,K,B,2,2)
    r = data22 - mm2H(mm2(Jp, Cp), Jq).sum(dim=2)  # (F,T,B,2,2)
    e2 = torch.view_as_real(r).square().sum(dim=(3, 4, 5))
    nu_, s2_ = nu.view(F, 1, 1), sigma2.view(F, 1, 1)
    w = m * ((nu_ + 8.0) / (nu_ + e2 / s2_))
    md, wd = m.double(), w.double()
    live = (m > 0) & (w > 0)
    lw = torch.where(live, md * (torch.log(torch.where(live, wd, 1.0)) - wd),
                     0.0)
    sums = torch.stack([md.sum((1, 2)), (wd * e2.double()).sum((1, 2)),
                        wd.sum((1, 2)), lw.sum((1, 2))], dim=1)
    return r.reshape(F, T * Bn, 4), e2, w, sums


def _residual_weights(C22, data22, J, m, nu, sigma2, p_idx, q_idx, t_int):
    """(r, e², w, sums (F, 4) float64): one launch of
    vis_residual_weights_kernel plus the sum over its per-block partials
    on a GPU, `_residual_weights_torch` on the CPU."""
    if data22.device.type != "cuda":
        return _residual_weights_torch(C22, data22, J, m, nu, sigma2,
                                       p_idx, q_idx, t_int)
    from ..ops import ext
    r, e2, w, part = ext().vis_residual_weights(
        C22.contiguous(), data22.contiguous(), J.contiguous(),
        m.contiguous(), nu.contiguous(), sigma2.contiguous(),
        p_idx.to(torch.int32).contiguous(),
        q_idx.to(torch.int32).contiguous(),
        t_int.to(torch.int32).contiguous())
    return r, e2, w, part.sum(dim=1)


def _unweighted_stations(w, gidx, Ts, N):
    """(F, Ts, 1, N, 1, 1) bool: the (frequency, interval, station) whose
    samples all have weight 0. It changes only with the weights, so the
    callers form it once per weight update."""
    F = w.shape[0]
    w2 = torch.cat([w.reshape(F, -1)] * 2, dim=1)           # (F, 2TB)
    tot = w2[:, gidx.reshape(-1)].reshape(F, Ts * N, -1).sum(dim=2)
    return (tot == 0).reshape(F, Ts, 1, N, 1, 1)


def _gather_plan(t_int, p_idx, q_idx, N, Ts):
    """Gather plan (Ts·N, Cnt) for the per-(interval, station) reduction:
    station n of interval ti receives exactly Cnt = Tdelta·(N−1)
    contributions (as the p side or the q side of a baseline).
    Precomputing the gather indices into cat([p-side, q-side]) turns four
    slow complex index_add_ scatters per sweep into two coalesced
    gather+sum passes."""
    T, Bn = t_int.shape[0], p_idx.shape[0]
    flat_p = (t_int.view(T, 1) * N + p_idx.view(1, Bn)).reshape(-1)
    flat_q = (t_int.view(T, 1) * N + q_idx.view(1, Bn)).reshape(-1)
    both = torch.cat([flat_p, flat_q])              # (2·T·B,)
    order = torch.argsort(both, stable=True)
    Cnt = T * Bn * 2 // (Ts * N)                    # = Tdelta·(N−1)
    return order.reshape(Ts * N, Cnt)               # (Ts·N, Cnt)


def _solve_sweeps(data22, C22, J, rho_t, prox_target, p_idx, q_idx, N,
                  Tdelta, n_sweeps, lambda_reg=1e-6, w=None, unweighted=None):
    """In-place alternating-LS sweeps for J (F?,Ts,K,N,2,2).

    data22: (F,T,B,2,2); C22: (F,K,T,B,2,2); rho_t: (K,) float;
    prox_target: (F,Ts,K,N,2,2) or None — the ADMM prox point
    (B_f Z − Y/ρ).
    w: (F,T,B) float sample weights ≥ 0 of the cost Σ_s w_s ‖V_s − …‖², or
    None for the plain sum of squares. Without a prox term a (frequency,
    interval, station) whose samples all have weight 0 has no equations
    and keeps its J; ``unweighted`` is that mask
    (`_unweighted_stations`), formed here once per call when not given.
    With a prox term its equations are the prox term alone.
    """
    F, T, Bn = data22.shape[0], data22.shape[1], data22.shape[2]
    K = C22.shape[1]
    Ts = J.shape[1]
    if T != Ts * Tdelta:
        # the gather plan below gives every (interval, station) the same
        # number of contributions; a longer last interval would be cut at
        # the wrong places and solved wrongly without any sign of it
        raise ValueError(
            f"_solve_sweeps: {T} timeslots are not {Ts} solution intervals "
            f"of {Tdelta}")
    dev = data22.device
    t_int = (torch.arange(T, device=dev) // Tdelta).clamp_(max=Ts - 1)
    eyeK = torch.eye(2 * K, dtype=data22.dtype, device=dev)
    gidx = _gather_plan(t_int, p_idx, q_idx, N, Ts)
    Cnt = gidx.shape[1]
    use_kernel = dev.type == "cuda" and K <= 8
    if use_kernel:
        from ..ops import ext
        p32 = p_idx.to(torch.int32).contiguous()
        q32 = q_idx.to(torch.int32).contiguous()
        t32 = t_int.to(torch.int32).contiguous()
        C22c = C22.contiguous()
        wc = None if w is None else w.contiguous()
    if w is not None and prox_target is None and unweighted is None:
        unweighted = _unweighted_stations(w, gidx, Ts, N)
    for _ in range(n_sweeps):
        if use_kernel and w is not None:
            rhs_cat, nm_cat = ext().als_sweep_w(
                C22c, data22.contiguous(), J.contiguous(), wc, p32, q32,
                t32)
        elif w is not None:
            rhs_cat, nm_cat = _als_contributions_torch_w(
                data22, C22, J, w, p_idx, q_idx, t_int)
        elif use_kernel:
            # fused HIP kernel: all per-sample Jones products +
            # normal-equation contributions in ONE launch (the env step
            # is dispatch-bound; see ops/csrc/als_sweep.hip). Output is
            # entry-major (F, X, 2TB) for coalesced writes.
            rhs_cat, nm_cat = ext().als_sweep(
                C22c, data22.contiguous(), J.contiguous(), p32, q32, t32)
        else:
            rhs_cat, nm_cat = _als_contributions_torch(
                data22, C22, J, p_idx, q_idx, t_int)
        # reduce into (F,Ts,N,…) by interval and station via the
        # precomputed gather plan (see above); cat layout is (F, X, 2TB)
        if use_kernel:
            # fused gather+segment-sum (ops/csrc/gather_sum.hip): the
            # torch composition below materializes the full gathered
            # copy (~260 MB/sweep at LOFAR scale) before reducing
            from ..ops import ext as _ext
            gc = gidx.contiguous()
            rhs = _ext().gather_sum(rhs_cat.contiguous(), gc) \
                .permute(0, 2, 1).reshape(F, Ts, N, 2, 2 * K)
            nm = _ext().gather_sum(nm_cat.contiguous(), gc) \
                .permute(0, 2, 1).reshape(F, Ts, N, 2 * K, 2 * K)
        else:
            rhs = rhs_cat[:, :, gidx.reshape(-1)] \
                .reshape(F, 2 * 2 * K, Ts * N, Cnt).sum(dim=3) \
                .permute(0, 2, 1).reshape(F, Ts, N, 2, 2 * K)
            nm = nm_cat[:, :, gidx.reshape(-1)] \
                .reshape(F, 2 * K * 2 * K, Ts * N, Cnt).sum(dim=3) \
                .permute(0, 2, 1).reshape(F, Ts, N, 2 * K, 2 * K)
        # ADMM prox: + diag(ρ_k I2) and + ρ_k F^k on the rhs
        if prox_target is not None:
            rho_blocks = torch.kron(
                torch.diag(rho_t.to(nm.real.dtype)),
                torch.eye(2, device=dev)).to(nm.dtype)
            nm = nm + rho_blocks
            # prox rhs: (F,Ts,K,N,2,2) → (F,Ts,N,2,2K) with ρ_k weights
            pt = prox_target * rho_t.view(1, 1, K, 1, 1, 1)
            rhs = rhs + pt.permute(0, 1, 3, 4, 2, 5).reshape(
                F, Ts, N, 2, 2 * K)
        nm = nm + lambda_reg * eyeK
        # solve G (2,2K): G nm = rhs → nm^T G^T = rhs^T
        G = torch.linalg.solve(nm.mT, rhs.mT).mT            # (F,Ts,N,2,2K)
        Jnew = G.reshape(F, Ts, N, 2, K, 2).permute(0, 1, 4, 2, 3, 5)
        if w is not None and prox_target is None:
            # no equations: today's algebra would give G = 0 and halve J
            Jnew = torch.where(unweighted, J, Jnew)
        J.copy_(0.5 * J + 0.5 * Jnew)
    return J


_C_LIGHT = 299792458.0


def _prior_weights(vis, weights, uvmin, uvmax):
    """Prior weights m (Nf, T, B) float32: ``weights`` times 0 on flagged
    samples times the uv cut; None when none of the three is given."""
    if weights is None and vis.flags is None and uvmin is None \
            and uvmax is None:
        return None
    dev = vis.data.device
    Nf, S = vis.data.shape[0], vis.data.shape[1]
    m = torch.ones((Nf, S), dtype=torch.float32, device=dev)
    if weights is not None:
        wt = torch.as_tensor(weights, dtype=torch.float32, device=dev)
        if wt.shape not in ((Nf, S), (S,)):
            raise ValueError(f"calibrate: weights must be ({Nf}, {S}) or "
                             f"({S},), got {tuple(wt.shape)}")
        m = m * wt
    if vis.flags is not None:
        if vis.flags.shape != (Nf, S):
            raise ValueError(f"calibrate: flags must be ({Nf}, {S}), got "
                             f"{tuple(vis.flags.shape)}")
        m = m * (~vis.flags.to(dev, torch.bool)).to(torch.float32)
    if uvmin is not None or uvmax is not None:
        uvlen = torch.linalg.vector_norm(vis.uvw[:, :2].double(), dim=1)
        fs = torch.as_tensor(np.asarray(vis.freqs, np.float64), device=dev)
        lam = uvlen.view(1, S) * (fs.view(Nf, 1) / _C_LIGHT)  # wavelengths
        keep = torch.ones_like(lam, dtype=torch.bool)
        if uvmin is not None:
            keep &= lam >= float(uvmin)
        if uvmax is not None:
            keep &= lam <= float(uvmax)
        m = m * keep.to(torch.float32)
    return m.reshape(Nf, vis.n_time, vis.B).contiguous()


def _sigma2(num, sum_m):
    """σ² = num / (8 Σ m) per frequency as float32, kept positive so that
    a frequency without any weight divides by no zero."""
    return (num / (8.0 * sum_m).clamp(min=1e-300)).clamp(min=1e-30).float()


def _nu_update(nu, sums, nu_grid):
    """ν per frequency: the point of ``nu_grid`` that minimises
    |ψ((ν_old+8)/2) − ln((ν_old+8)/2) − ψ(ν/2) + ln(ν/2)
     + Σ m (ln w − w)/Σ m + 1|, the ν equation of the Student's-t EM
    update with 8 real components per sample."""
    a = (nu.double() + 8.0) / 2.0
    const = torch.special.digamma(a) - torch.log(a) \
        + sums[:, 3] / sums[:, 0].clamp(min=1e-300) + 1.0       # (F,)
    g = nu_grid / 2.0
    val = (const.view(-1, 1) - torch.special.digamma(g).view(1, -1)
           + torch.log(g).view(1, -1)).abs()
    return nu_grid[val.argmin(dim=1)].float()


def calibrate(vis: VisData, sky, clusters, rho_spectral,
              admm_iter: int = 10, poly_order: int = 2, polytype: int = 1,
              alpha: float = 0.0, n_sweeps: int = 3, init_sweeps: int = 6,
              smear_bw: float | None = 180e3,
              C_cache: torch.Tensor | None = None,
              freq_group: "dist.ProcessGroup | None" = None,
              beam=None, weights: torch.Tensor | None = None,
              uvmin: float | None = None, uvmax: float | None = None,
              robust: bool = False, nulow: float = 2.0,
              nuhigh: float = 30.0, robust_every: int = 1) -> CalSolution:
    """Consensus-ADMM direction-dependent calibration of ``vis``.

    rho_spectral: (K,) ADMM regularization per direction (the env action);
    admm_iter: ADMM iterations (the reference's ``-A``);
    poly_order: consensus polynomial terms (``-P``);
    alpha: federated-averaging / spatial regularization (``-X`` style);
    beam: `radio.array.StationBeam` for the model coherencies predicted
    here (ignored with ``C_cache``); None calibrates without a beam.

    Sample weights (all opt-in; without them the cost is the plain sum of
    squares and nothing below runs). The prior weight m of a sample is
    ``weights`` ((Nf, S) or (S,), ≥ 0) times 0 where ``vis.flags`` is set
    times the uv cut: 0 where |(u, v)|·f/c lies outside
    [``uvmin``, ``uvmax``] wavelengths (sagecal's ``-x``), per frequency.
    ``robust`` adds SAGECal's Student's-t noise model (``-L nulow`` and the
    upper bound ``nuhigh``): before every ``n_sweeps`` of the initial
    sweeps and before the J-step of every ``robust_every``-th ADMM
    iteration the weights become w = m (ν + 8)/(ν + e²/σ²) from the
    current residual, σ² ← Σ w e² / (8 Σ m), and ν moves to the point of
    a 30-point grid on [nulow, nuhigh] that best solves the ν equation of
    the EM update; they start from σ² = Σ m e² / (8 Σ m) at the initial J
    and ν = nulow. All of it is per frequency and stays on the device, so
    frequency shards remain independent. The solution then carries the
    final ``weights``, and ``nu`` and ``sigma2`` when robust.

    When torch.distributed is initialized, each rank is expected to hold
    a disjoint frequency shard in ``vis``; the Z-step all_reduces the
    basis-projected partial sums (one flat RCCL all_reduce per ADMM
    iteration over xGMI).
    """
    dev = vis.data.device
    N, B, Ts, Tdelta = vis.N, vis.B, vis.Ts, vis.Tdelta
    T = vis.n_time
    K = len(clusters)
    Nf = len(vis.freqs)
    Ne = poly_order
    p_idx, q_idx = baseline_pq(N, dev)
    rho_t = torch.as_tensor(np.asarray(rho_spectral, np.float32), device=dev)

    # model coherencies per local frequency (cacheable across env steps)
    if C_cache is None:
        C = torch.stack([
            predict_coherencies_uvw(sky, clusters, vis.uvw, float(f),
                                    vis.ra0, vis.dec0, smear_bw=smear_bw,
                                    beam=beam)
            for f in vis.freqs])                            # (Nf,K,S,4)
    else:
        C = C_cache
    # row-major 2×2 physical convention throughout the solver (matches
    # apply_jones; see sim.apply_jones note)
    C22 = C.reshape(Nf, K, T, B, 2, 2)
    data22 = vis.data.reshape(Nf, T, B, 2, 2)

    # prior weights m (Nf,T,B): None on the default path
    m = _prior_weights(vis, weights, uvmin, uvmax)
    if robust and m is None:
        m = torch.ones((Nf, T, B), dtype=torch.float32, device=dev)
    w = m                                 # weights of the J-step
    if m is not None:
        t_int = (torch.arange(T, device=dev) // Tdelta).clamp_(max=Ts - 1)
        one_f = torch.ones(Nf, dtype=torch.float32, device=dev)
        rw_args = (p_idx, q_idx, t_int)
    nu = sigma2 = None

    # distributed frequency-shard info
    distributed = dist.is_available() and dist.is_initialized() \
        and dist.get_world_size(freq_group) > 1
    if distributed:
        all_freqs = [None] * dist.get_world_size(freq_group)
        dist.all_gather_object(all_freqs, list(vis.freqs), group=freq_group)
        f_all = np.sort(np.concatenate([np.asarray(f) for f in all_freqs]))
    else:
        f_all = np.asarray(vis.freqs)
    f0 = float(np.mean(f_all))
    Bf = _poly_basis(np.asarray(vis.freqs), f_all, f0, Ne, polytype)
    Bf_t = torch.as_tensor(Bf, dtype=torch.float32, device=dev)
    # global Gram matrix of the basis
    Ball = _poly_basis(f_all, f_all, f0, Ne, polytype)
    Gram = Ball.T @ Ball                                     # (Ne,Ne)

    # init J with identity and a few unconstrained sweeps
    J = torch.zeros((Nf, Ts, K, N, 2, 2), dtype=torch.complex64, device=dev)
    J[..., 0, 0] = 1.0
    J[..., 1, 1] = 1.0
    if not robust:
        _solve_sweeps(data22, C22, J, rho_t, None, p_idx, q_idx, N, Tdelta,
                      init_sweeps, w=w)
    else:
        # The robust model starts at the initial J: σ² of the
        # prior-weighted residual there, ν at its lower bound, and a
        # weight update before every n_sweeps of the initial sweeps.
        # Initial sweeps on the prior weights alone fit the outliers, and
        # from there the later reweighting does not always find its way
        # back (docs/TESTING.md, robust calibration).
        nu = torch.full((Nf,), float(nulow), dtype=torch.float32, device=dev)
        nu_grid = torch.linspace(float(nulow), float(nuhigh), 30,
                                 dtype=torch.float64, device=dev)
        _, e2, _, sums = _residual_weights(C22, data22, J, m, nu, one_f,
                                           *rw_args)
        sigma2 = _sigma2((m.double() * e2.double()).sum(dim=(1, 2)),
                         sums[:, 0])

        def robust_update():
            # E-step of the Student's-t model, per frequency, on device
            _, _, w_new, sums = _residual_weights(C22, data22, J, m, nu,
                                                  sigma2, *rw_args)
            return (w_new, _sigma2(sums[:, 1], sums[:, 0]),
                    _nu_update(nu, sums, nu_grid))

        step = max(n_sweeps, 1)
        for done in range(0, init_sweeps, step):
            w, sigma2, nu = robust_update()
            _solve_sweeps(data22, C22, J, rho_t, None, p_idx, q_idx, N,
                          Tdelta, min(step, init_sweeps - done), w=w)

    Y = torch.zeros_like(J)                                  # scaled dual
    Z = torch.zeros((K, Ne, Ts, N, 2, 2), dtype=torch.complex64, device=dev)
    rho_k = rho_t.view(1, 1, K, 1, 1, 1)

    for it in range(admm_iter):
        # ---- Z-step: per direction closed form over all freqs ----------
        # partial sum: Σ_f b_f ⊗ ρ (J_f + Y_f/ρ)  → (Ne,K,Ts,N,2,2)
        JY = J + Y / rho_k.clamp(min=1e-12)
        part = torch.einsum('fe,ftknab->ektnab',
                            Bf_t.to(torch.complex64), JY)
        if distributed:
            dist.all_reduce(part, group=freq_group)
        # weight by rho (same for all freqs) and solve (ρ Gram + αI) Z = part
        M = torch.as_tensor(Gram, dtype=torch.complex64, device=dev)
        rhoZ = rho_t.view(K, 1, 1, 1, 1, 1).to(torch.complex64)
        A = (M.unsqueeze(0) * rhoZ.view(K, 1, 1)
             + alpha * torch.eye(Ne, dtype=torch.complex64, device=dev))
        rhs = part.permute(1, 0, 2, 3, 4, 5).reshape(K, Ne, -1) \
            * rhoZ.view(K, 1, 1)
        # inv+GEMM: complex batched trsm is broken for wide RHS on this
        # ROCm build (see radio.hessian.dsolutions_r note); Ne is tiny
        Z = (torch.linalg.inv(A) @ rhs).reshape(K, Ne, Ts, N, 2, 2)
        # ---- J-step with prox toward B_f Z − Y/ρ -----------------------
        BZ = torch.einsum('fe,ektnab->ftknab', Bf_t.to(torch.complex64),
                          Z.permute(1, 0, 2, 3, 4, 5))      # (F,Ts,K,N,2,2)
        prox = BZ - Y / rho_k.clamp(min=1e-12)
        if robust and it % robust_every == 0:
            w, sigma2, nu = robust_update()
        _solve_sweeps(data22, C22, J, rho_t, prox, p_idx, q_idx, N, Tdelta,
                      n_sweeps, w=w)
        # ---- dual ascent ----------------------------------------------
        Y = Y + rho_k.to(torch.complex64) * (J - BZ)

    # residual = data − model(J)
    w_out = None
    if m is None:
        res = torch.empty_like(vis.data)
        for fi in range(Nf):
            model = apply_jones(C[fi], J[fi].permute(1, 0, 2, 3, 4), N,
                                Tdelta)
            res[fi] = vis.data[fi] - model
    else:
        # one launch for all frequencies; with the robust model it also
        # gives the weights that go with the final J
        res, _, w_out, _ = _residual_weights(
            C22, data22, J, m, nu if robust else one_f,
            sigma2 if robust else one_f, *rw_args)
        w_out = (w_out if robust else m).reshape(Nf, T * B)
    return CalSolution(J=J.permute(0, 2, 1, 3, 4, 5).contiguous(), Z=Z,
                       residual=res, freqs=np.asarray(vis.freqs),
                       rho=np.asarray(rho_spectral, np.float32),
                       weights=w_out, nu=nu, sigma2=sigma2)
