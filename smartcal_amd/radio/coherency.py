"""Coherency (model visibility) prediction.

Replaces `calibration_tools.py:215-464` (`skytocoherencies[_torch|_uvw]`),
which loops over sources in Python. Here the whole prediction is one
batched tensor expression per cluster: ``phase = uvw_scaled @ lmn^T``
(a GEMM shape the GPU likes), fused with the complex exponential, flux
scaling, bandwidth-smearing sinc and the Gaussian-source envelope.

Convention: sample axis T = baselines × timeslots in the same ordering as
the visibility data; output C is (K, T, 4) complex64 with XX = YY = Stokes-I
coherency, XY = YX = 0, exactly like the reference.

Shapelet sources (names that are keys of ``sky.shapelets``) are kept out
of the point/Gaussian tables and added on top: a source centred at
(l0, m0, n0c) contributes ``G = smear(φ0) · e^{iφ0} · F(u, v)`` with
φ0 = u·l0 + v·m0 + w·n0c, F the closed-form transform of
`radio.shapelet.shapelet_uv` and smear the point-source sinc at φ0, as
``XX += (sI+sQ)·G, YY += (sI−sQ)·G, XY = YX += sU·G`` (Stokes at the
prediction frequency; V, RM and within-source w variation ignored).

Station beam (``beam=``, a `radio.array.StationBeam`): the array factor
of station p towards source s at timeslot t, steered at the phase centre,
``E[t,p,s] = (1/Ne)·Σ_e exp(+i·2πf/c·(u_e·l_s + v_e·m_s + w_e·n_s))``,
weights every source term of baseline (p, q) by ``E[t,p,s]·conj(E[t,q,s])``
— the station is the average of its elements. A shapelet source takes
the beam at its centre, on all four correlations.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from .array import StationBeam
from .hessian import baseline_pq
from .sky import SkyModel, ClusterSet
from .shapelet import MAX_N0

C_LIGHT = 2.99792458e8

__all__ = ["predict_coherencies", "predict_coherencies_uvw", "array_factor"]


def _cluster_source_tensors(sky: SkyModel, cluster, ra0, dec0, freq, device):
    """Gather per-source tensors for one cluster at ``freq`` (point and
    Gaussian sources; shapelet sources go through `_shapelet_tables`)."""
    idx = sky.index
    sel = np.asarray([idx[n] for n in cluster.names
                      if n not in sky.shapelets], dtype=np.int64)
    l, m, n = sky.lmn(ra0, dec0)
    lmn = np.stack([l[sel], m[sel], n[sel]], axis=1)          # (S,3)
    flux = sky.flux_at(freq)[sel]                              # (S,)
    t = lambda a, dt=torch.float32: torch.as_tensor(
        np.ascontiguousarray(a), dtype=dt, device=device)
    return (t(lmn, torch.float64), t(flux, torch.float64),
            t(sky.eX[sel], torch.float64), t(sky.eY[sel], torch.float64),
            t(sky.eP[sel], torch.float64),
            torch.as_tensor(sky.gaussian[sel], device=device))


def _shapelet_tables(sky: SkyModel, clusters: ClusterSet, ra0, dec0, freq):
    """Per-source tables of all shapelet sources, grouped by cluster, or
    None when no cluster holds one. Both prediction paths consume these.

    → (hdr (Ns,12) f64, coff (Ns,) i32, coef f64 packed, clk (Kc,) i32,
    soff (Kc+1,) i32); hdr row = [l0, m0, n0c, sI_f, sQ_f, sU_f, β·a, β·b,
    cosθ, sinθ, 2πβab, n0]; coff the source's offset into coef; clk the
    cluster index of each group and soff its source range."""
    if not sky.shapelets:
        return None
    idx = sky.index
    groups = [(k, [idx[n] for n in cl.names if n in sky.shapelets])
              for k, cl in enumerate(clusters)]
    groups = [(k, sel) for k, sel in groups if sel]
    if not groups:
        return None
    l, m, n = sky.lmn(ra0, dec0)
    hdr, coff, coef, clk, soff = [], [], [], [], [0]
    ncoef = 0
    for k, sel in groups:
        stokes = sky.shapelet_stokes_at(freq, sel)
        for si, st in zip(sel, stokes):
            mdl = sky.shapelets[sky.names[si]]
            if not 1 <= mdl.n0 <= MAX_N0:
                raise ValueError(
                    f"shapelet source {sky.names[si]}: n0 = {mdl.n0} "
                    f"outside the supported range 1..{MAX_N0}")
            c = np.asarray(mdl.coeff, np.float64).reshape(-1)
            if c.size != mdl.n0 * mdl.n0:
                raise ValueError(
                    f"shapelet source {sky.names[si]}: {c.size} "
                    f"coefficients for n0 = {mdl.n0}")
            hdr.append([l[si], m[si], n[si], st[0], st[1], st[2],
                        mdl.beta * mdl.a, mdl.beta * mdl.b,
                        math.cos(mdl.theta), math.sin(mdl.theta),
                        2.0 * math.pi * mdl.beta * mdl.a * mdl.b, mdl.n0])
            coff.append(ncoef)
            coef.append(c)
            ncoef += c.size
        clk.append(k)
        soff.append(len(hdr))
    return (np.asarray(hdr, np.float64), np.asarray(coff, np.int32),
            np.concatenate(coef), np.asarray(clk, np.int32),
            np.asarray(soff, np.int32))


def _hermite_functions(n0: int, t: torch.Tensor) -> torch.Tensor:
    """ψ_0..ψ_{n0−1}(t) → (n0, T) f64; torch twin of
    `radio.shapelet.hermite_functions` (same normalised recurrence)."""
    rows = [math.pi ** -0.25 * torch.exp(-0.5 * t * t)]
    if n0 > 1:
        rows.append(math.sqrt(2.0) * t * rows[0])
    for n in range(1, n0 - 1):
        rows.append(t * math.sqrt(2.0 / (n + 1)) * rows[n]
                    - math.sqrt(n / (n + 1)) * rows[n - 1])
    return torch.stack(rows)


def array_factor(beam: StationBeam, lmn: torch.Tensor,
                 freq: float) -> torch.Tensor:
    """Array-factor table E (Tt, N, S) complex128 towards directions
    ``lmn`` (S, 3) f64 (third component n − 1, as `SkyModel.lmn`), on the
    device of ``lmn`` — vectorised f64 torch, the oracle of beam.hip."""
    elem = torch.as_tensor(beam.elem_uvw, dtype=torch.float64,
                           device=lmn.device) \
        * (2.0 * math.pi / C_LIGHT * freq)                   # (Tt,N,Ne,3)
    Tt, N, Ne = elem.shape[:3]
    S = lmn.shape[0]
    E = torch.empty((Tt, N, S), dtype=torch.complex128, device=lmn.device)
    step = max(1, (1 << 22) // max(1, Tt * N * Ne))          # bound memory
    for s0 in range(0, S, step):
        ph = elem @ lmn[s0:s0 + step].T                      # (Tt,N,Ne,s)
        E[:, :, s0:s0 + step] = torch.polar(torch.ones_like(ph),
                                            ph).mean(dim=2)
    return E


def _beam_gain(E: torch.Tensor, p_idx, q_idx) -> torch.Tensor:
    """E (Tt, N, s) → per-sample gain E_p·conj(E_q), (Tt·B, s)."""
    g = E[:, p_idx] * E[:, q_idx].conj()                     # (Tt,B,s)
    return g.reshape(-1, g.shape[2])


def _add_shapelets_torch(C, u, v, w, tables, fdelta, beam=None, freq=None):
    """Vectorised f64 composition of the shapelet contribution, added
    into C in place — the CPU path and the oracle of shapelet.hip. With
    ``beam`` every source is weighted by the array factors at its centre."""
    hdr, coff, coef, clk, soff = tables
    if beam is not None:
        p_idx, q_idx = baseline_pq(beam.n_stations, u.device)
        gain = _beam_gain(
            array_factor(beam, torch.as_tensor(
                np.ascontiguousarray(hdr[:, 0:3]), device=u.device), freq),
            p_idx, q_idx)                                    # (T,Ns)
    for g, k in enumerate(clk):
        acc = torch.zeros((3, u.shape[0]), dtype=torch.complex128,
                          device=u.device)          # XX, YY, XY(=YX)
        for s in range(soff[g], soff[g + 1]):
            (l0, m0, n0c, sI, sQ, sU, ba, bb, ct, st, norm,
             n0) = hdr[s].tolist()
            n0 = int(n0)
            pu = _hermite_functions(n0, ba * (ct * u + st * v))
            pv = _hermite_functions(n0, bb * (-st * u + ct * v))
            ij = np.arange(n0)
            cij = coef[coff[s]:coff[s] + n0 * n0].reshape(n0, n0) \
                * 1j ** ((ij[:, None] + ij[None, :]) % 4)
            cij = torch.as_tensor(cij, dtype=torch.complex128,
                                  device=u.device)
            F = (pu * (cij @ pv.to(torch.complex128))).sum(dim=0)
            ph = u * l0 + v * m0 + w * n0c
            amp = torch.full_like(ph, norm)
            if fdelta:
                amp = amp * torch.abs(torch.sinc(ph * (0.5 * fdelta / math.pi)))
            G = torch.polar(amp, ph) * F
            if beam is not None:
                G = G * gain[:, s]
            acc[0] += (sI + sQ) * G
            acc[1] += (sI - sQ) * G
            acc[2] += sU * G
        Ck = C[int(k)].to(torch.complex128)
        Ck[:, 0] += acc[0]
        Ck[:, 3] += acc[1]
        Ck[:, 1] += acc[2]
        Ck[:, 2] += acc[2]
        C[int(k)] = Ck.to(torch.complex64)


def predict_coherencies_uvw(sky: SkyModel, clusters: ClusterSet,
                            uvw: torch.Tensor, freq: float,
                            ra0: float, dec0: float,
                            smear_bw: float | None = None,
                            chunk: int = 512,
                            beam: StationBeam | None = None) -> torch.Tensor:
    """Predict C (K, T, 4) complex64 for raw uvw (T, 3) in meters.

    ``smear_bw``: channel bandwidth in Hz for the sinc smearing factor
    (the reference hardcodes 180e3 in `calibration_tools.py:380`); None
    disables smearing (matching `skytocoherencies[_torch]`).
    Gaussian sources (name 'G…') get the projected-envelope treatment of
    `calibration_tools.py:424-448`; shapelet sources (module docstring)
    are added on top, with mode order n0 ≤ 32 (ValueError beyond).
    ``beam``: weight every source by the station array factors (module
    docstring); samples must then be ordered s = t·B + b with (p_b, q_b)
    of `radio.hessian.baseline_pq`, T = Tt·N(N−1)/2 (ValueError if not).
    """
    device = uvw.device
    T = uvw.shape[0]
    if beam is not None:
        Tt, N = beam.n_time, beam.n_stations
        if T != Tt * (N * (N - 1) // 2):
            raise ValueError(
                f"uvw has T = {T} samples, the beam needs Tt·N(N−1)/2 = "
                f"{Tt * (N * (N - 1) // 2)} (Tt = {Tt}, N = {N})")
    scale = 2.0 * math.pi / C_LIGHT * freq
    u = uvw[:, 0].double() * scale
    v = uvw[:, 1].double() * scale
    w = uvw[:, 2].double() * scale
    fdelta = (smear_bw / freq) if smear_bw is not None else 0.0   # 0 = off
    shp = _shapelet_tables(sky, clusters, ra0, dec0, freq)

    from ..ops import use_hip
    if use_hip(uvw.float() if uvw.is_cuda else uvw):
        # ONE kernel launch for the whole sky (ops/csrc/coherency.hip),
        # one more for all shapelet sources (ops/csrc/shapelet.hip);
        # the torch composition below is the CPU oracle
        uvw_scaled = torch.stack((u, v, w), dim=1).contiguous()
        return _predict_hip(sky, clusters, uvw_scaled, freq, ra0, dec0,
                            fdelta, shp, beam)

    K = len(clusters)
    C = torch.zeros((K, T, 4), dtype=torch.complex64, device=device)
    if beam is not None:
        p_idx, q_idx = baseline_pq(beam.n_stations, device)
    src, off = _source_table(sky, clusters, device, freq, ra0, dec0)
    off = off.tolist()
    u1, v1, w1 = u.unsqueeze(1), v.unsqueeze(1), w.unsqueeze(1)
    for ck in range(K):
        rows = src[off[ck]:off[ck + 1]]
        acc = torch.zeros(T, dtype=torch.complex128, device=device)
        if beam is not None:
            E = array_factor(beam, rows[:, 0:3].contiguous(), freq)  # (Tt,N,S)
        for s0 in range(0, rows.shape[0], chunk):
            r = rows[s0:s0 + chunk]
            # (T,s) phase — GEMM shape
            ph = u1 * r[:, 0] + v1 * r[:, 1] + w1 * r[:, 2]
            amp = r[:, 3].expand(T, r.shape[0]).clone()
            if fdelta:
                amp = amp * torch.abs(torch.sinc(ph * (0.5 * fdelta / math.pi)))
            gi = torch.nonzero(r[:, 4], as_tuple=True)[0]
            if gi.numel():
                # Gaussian envelope from the six coefficients of the row
                uut = u1 * r[gi, 5] + v1 * r[gi, 6] + w1 * r[gi, 7]
                vvt = u1 * r[gi, 8] + v1 * r[gi, 9] + w1 * r[gi, 10]
                amp[:, gi] = amp[:, gi] * (0.5 * math.pi
                                           * torch.exp(-(uut * uut + vvt * vvt)))
            term = torch.polar(amp, ph)
            if beam is not None:
                term = term * _beam_gain(E[:, :, s0:s0 + chunk], p_idx, q_idx)
            acc = acc + term.sum(dim=1)
        C[ck, :, 0] = acc.to(torch.complex64)
        C[ck, :, 3] = C[ck, :, 0]
    if shp is not None:
        _add_shapelets_torch(C, u, v, w, shp, fdelta, beam, freq)
    return C


def _predict_hip(sky, clusters, uvw_scaled, freq, ra0, dec0, fdelta,
                 shp=None, beam=None):
    """Build the per-source table and run the HIP kernels: one launch
    predicts the point/Gaussian coherencies, one more adds the shapelet
    sources of ``shp`` (`_shapelet_tables`). With ``beam``, one launch
    first builds E for all point/Gaussian rows and all shapelet centres
    (ops/csrc/beam.hip) and both predictions are weighted by it."""
    from ..ops import ext

    device = uvw_scaled.device
    src, off = _source_table(sky, clusters, device, freq, ra0, dec0)
    gain = ()
    if beam is not None:
        lmn = src[:, 0:3]
        if shp is not None:
            lmn = torch.cat((lmn, torch.as_tensor(
                np.ascontiguousarray(shp[0][:, 0:3]), device=device)))
        elem = torch.as_tensor(beam.elem_uvw, dtype=torch.float64,
                               device=device).contiguous()
        E = ext().station_beam(elem, lmn.contiguous(),
                               2.0 * math.pi / C_LIGHT * freq)
        p_idx, q_idx = (i.to(torch.int32)
                        for i in baseline_pq(beam.n_stations, device))
        # shapelet centres follow the src.shape[0] rows of the table in E
        gain = (E, p_idx, q_idx, src.shape[0])
        C = ext().coherency_beam_predict(uvw_scaled, src, off, float(fdelta),
                                         *gain[:3])
    else:
        C = ext().coherency_predict(uvw_scaled, src, off, float(fdelta))
    if shp is not None:
        ext().shapelet_predict(
            C, uvw_scaled, *(torch.as_tensor(a, device=device) for a in shp),
            float(fdelta), *gain)
    return C


def _gaussian_coeffs(lmn, eX2, eY2, eP):
    """Projected envelope of Gaussian sources (`calibration_tools.py:
    424-448`) → (gu (S, 3), gv (S, 3)). The projection of uv onto the
    source tangent plane and the position-angle rotation are linear in
    (u, v, w), so ``uut = gu·(u, v, w)``, ``vvt = gv·(u, v, w)`` and the
    envelope is π/2 · exp(−(uut² + vvt²)). Note: lmn[:, 2] is (n − 1) as
    returned by radectolm; the reference takes acos of that value directly
    (`calibration_tools.py:425`)."""
    ll, mm, nn = lmn[:, 0], lmn[:, 1], lmn[:, 2]
    phi = -torch.acos(torch.clamp(nn, -1.0, 1.0))
    xi = -torch.atan2(-ll, mm)
    cxi, sxi = torch.cos(xi), torch.sin(xi)
    cphi, sphi = torch.cos(phi), torch.sin(phi)
    cpa, spa = torch.cos(eP), torch.sin(eP)
    # uup = (cxi)u + (-cphi sxi)v + (sphi sxi)w; vvp likewise
    up = torch.stack((cxi, -cphi * sxi, sphi * sxi), dim=1)
    vp = torch.stack((sxi, cphi * cxi, -sphi * cxi), dim=1)
    return (2.0 * eX2[:, None] * (cpa[:, None] * up - spa[:, None] * vp),
            2.0 * eY2[:, None] * (spa[:, None] * up + cpa[:, None] * vp))


def _source_table(sky, clusters, device, freq, ra0, dec0):
    """→ (src (Stot, 11) f64, off (K+1,) i32): the rows
    [l, m, n, flux, gflag, gu1, gv1, gw1, gu2, gv2, gw2] of both
    prediction paths (see ops/csrc/sky_term.h) for all clusters, and the
    clusters' offsets into them."""
    rows = []
    offs = [0]
    for cluster in clusters:
        lmn, flux, eX2, eY2, eP, gflag = _cluster_source_tensors(
            sky, cluster, ra0, dec0, freq, device)
        S = lmn.shape[0]
        tab = torch.zeros(S, 11, dtype=torch.float64, device=device)
        tab[:, 0:3] = lmn
        tab[:, 3] = flux
        g = gflag.to(torch.bool)
        if bool(g.any()):
            gi = torch.nonzero(g, as_tuple=True)[0]
            tab[gi, 4] = 1.0
            tab[gi, 5:8], tab[gi, 8:11] = _gaussian_coeffs(
                lmn[gi], eX2[gi], eY2[gi], eP[gi])
        rows.append(tab)
        offs.append(offs[-1] + S)
    src = torch.cat(rows).contiguous() if rows else torch.zeros(
        0, 11, dtype=torch.float64, device=device)
    off = torch.tensor(offs, dtype=torch.int32, device=device)
    return src, off


def predict_coherencies(sky: SkyModel, clusters: ClusterSet,
                        uvw: torch.Tensor, freq: float, ra0: float,
                        dec0: float) -> torch.Tensor:
    """No-smearing variant matching `skytocoherencies_torch`
    (`calibration_tools.py:298-368`)."""
    return predict_coherencies_uvw(sky, clusters, uvw, freq, ra0, dec0,
                                   smear_bw=None)
