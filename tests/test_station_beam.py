"""Station array-factor beam: closed form, the station-equals-mean-of-its-
elements identity, prediction vs a per-sample loop transcription, the
beamless path, the rotation helpers and the public surface (CPU)."""

import math
import warnings

import numpy as np
import pytest
import torch

from smartcal_amd.radio import array as arr, sim, sky as rsky
from smartcal_amd.radio.coherency import (C_LIGHT, array_factor,
                                          predict_coherencies_uvw)
from smartcal_amd.radio.hessian import baseline_pq

from test_scripts import _run
from test_shapelet_predict import (DEC0, FREQ, RA0, _psi_scalar,
                                   make_test_sky)


# --------------------------------------------------------------------------
# shared scenario and oracles (also used by test_gpu_beam.py)
# --------------------------------------------------------------------------

def make_geometry(N, Ne, Tt=3, seed=5, span=150.0):
    """N stations within ±span m, Ne elements within 15 m of each, Tt
    timeslots one hour apart → (layout, beam, uvw (Tt·B, 3) f64 tensor)."""
    rng = np.random.default_rng(seed)
    enu = (rng.random((N, 3)) * 2 - 1) * [span, span, 2.0]
    layout = arr.StationLayout(enu)
    elem = arr.station_elements(N, Ne, rng)
    times = np.arange(Tt) * 3600.0
    beam = arr.station_beam(layout, elem, RA0, DEC0, times)
    uvw = arr.uvw_synthesis(layout, RA0, DEC0, times).reshape(-1, 3)
    return layout, beam, torch.as_tensor(uvw, dtype=torch.float64)


def point_sky():
    """The three point sources of `make_test_sky`, one cluster."""
    sky, _ = make_test_sky()
    keep = [0, 1, 2]
    sub = rsky.SkyModel.from_arrays(
        [sky.names[i] for i in keep], sky.ra[keep], sky.dec[keep],
        sky.sI[keep], sky.sP[keep], sky.f0[keep])
    return sub, rsky.ClusterSet([rsky.ClusterDef(1, 1, list(sub.names))])


def _spectral_factor(sky, s, freq):
    fr = math.log(freq / sky.f0[s])
    return math.exp(sky.sP[s, 0] * fr + sky.sP[s, 1] * fr ** 2
                    + sky.sP[s, 2] * fr ** 3)


def beam_loop_oracle(sky, clusters, uvw, freq, smear_bw, beam):
    """Per-sample, per-source, per-element python transcription of the
    beam-weighted coherency formulas → (K, T, 4) complex128; ``beam`` None
    gives the beamless prediction."""
    scale = 2.0 * math.pi / C_LIGHT * freq
    uvw = uvw.double().numpy() * scale
    l, m, n = sky.lmn(RA0, DEC0)
    idx = sky.index
    if beam is not None:
        Tt, N, Ne = beam.elem_uvw.shape[:3]
        pq = [(p, q) for p in range(N) for q in range(p + 1, N)]
        B = len(pq)
        assert uvw.shape[0] == Tt * B

    def E(t, p, s):
        acc = 0j
        for ue, ve, we in beam.elem_uvw[t, p]:
            ph = scale * (ue * l[s] + ve * m[s] + we * n[s])
            acc += complex(math.cos(ph), math.sin(ph))
        return acc / Ne

    out = np.zeros((len(clusters), uvw.shape[0], 4), np.complex128)
    for k, cl in enumerate(clusters):
        for nm in cl.names:
            s = idx[nm]
            fac = _spectral_factor(sky, s, freq)
            for i, (u, v, w) in enumerate(uvw):
                ph = u * l[s] + v * m[s] + w * n[s]
                term = complex(math.cos(ph), math.sin(ph))
                if smear_bw is not None:
                    x = ph * 0.5 * smear_bw / freq
                    term *= 1.0 if x == 0 else abs(math.sin(x) / x)
                if beam is not None:
                    t, b = divmod(i, B)
                    p, q = pq[b]
                    term *= E(t, p, s) * E(t, q, s).conjugate()
                if nm in sky.shapelets:
                    mdl = sky.shapelets[nm]
                    ct, st = math.cos(mdl.theta), math.sin(mdl.theta)
                    pu = _psi_scalar(mdl.n0, mdl.beta * mdl.a
                                     * (ct * u + st * v))
                    pv = _psi_scalar(mdl.n0, mdl.beta * mdl.b
                                     * (-st * u + ct * v))
                    F = 0j
                    for a in range(mdl.n0):
                        for c in range(mdl.n0):
                            F += mdl.coeff[a * mdl.n0 + c] * 1j ** (a + c) \
                                * pu[a] * pv[c]
                    G = term * F * 2.0 * math.pi * mdl.beta * mdl.a * mdl.b
                    fI, fQ, fU = (sky.sI[s] * fac, sky.sQ[s] * fac,
                                  sky.sU[s] * fac)
                    out[k, i, 0] += (fI + fQ) * G
                    out[k, i, 3] += (fI - fQ) * G
                    out[k, i, 1] += fU * G
                    out[k, i, 2] += fU * G
                    continue
                amp = sky.sI[s] * fac
                if sky.gaussian[s]:
                    # projected-envelope of the Gaussian source, as in
                    # `predict_coherencies_uvw` (acos of n − 1, like the
                    # reference)
                    phi = -math.acos(min(max(n[s], -1.0), 1.0))
                    xi = -math.atan2(-l[s], m[s])
                    cxi, sxi = math.cos(xi), math.sin(xi)
                    cphi, sphi = math.cos(phi), math.sin(phi)
                    uup = u * cxi - v * cphi * sxi + w * sphi * sxi
                    vvp = u * sxi + v * cphi * cxi - w * sphi * cxi
                    cpa, spa = math.cos(sky.eP[s]), math.sin(sky.eP[s])
                    uut = 2.0 * sky.eX[s] * (cpa * uup - spa * vvp)
                    vvt = 2.0 * sky.eY[s] * (spa * uup + cpa * vvp)
                    amp *= 0.5 * math.pi * math.exp(-(uut * uut + vvt * vvt))
                out[k, i, 0] += amp * term
                out[k, i, 3] += amp * term
    return out


def beam_numpy_oracle(sky, clusters, uvw, freq, smear_bw, beam):
    """Vectorised f64 numpy oracle for skies of point sources only →
    (K, T, 4) complex128."""
    assert not sky.shapelets and not sky.gaussian.any()
    scale = 2.0 * math.pi / C_LIGHT * freq
    uvw = uvw.double().numpy() * scale
    lmn = np.stack(sky.lmn(RA0, DEC0), axis=1)                # (S,3)
    Tt, N, Ne = beam.elem_uvw.shape[:3]
    E = np.exp(1j * scale * np.einsum("tpec,sc->tpse", beam.elem_uvw,
                                      lmn)).mean(axis=3)      # (Tt,N,S)
    p, q = np.triu_indices(N, k=1)
    gain = (E[:, p] * E[:, q].conj()).reshape(uvw.shape[0], -1)
    ph = uvw @ lmn.T                                          # (T,S)
    term = sky.flux_at(freq) * np.exp(1j * ph) * gain
    if smear_bw is not None:
        term = term * np.abs(np.sinc(ph * 0.5 * smear_bw / freq / math.pi))
    idx = sky.index
    out = np.zeros((len(clusters), uvw.shape[0], 4), np.complex128)
    for k, cl in enumerate(clusters):
        out[k, :, 0] = term[:, [idx[nm] for nm in cl.names]].sum(axis=1)
        out[k, :, 3] = out[k, :, 0]
    return out


def rel_err(out, ref):
    return float(np.abs(out - ref).max() / np.abs(ref).max())


def table(beam, sky, freq=FREQ):
    lmn = torch.as_tensor(np.stack(sky.lmn(RA0, DEC0), axis=1))
    return array_factor(beam, lmn, freq).numpy()


# --------------------------------------------------------------------------
# 1. array factor basics
# --------------------------------------------------------------------------

def test_array_factor_closed_form_and_bounds():
    d, Tt = 20.0, 3
    elem = np.zeros((Tt, 1, 2, 3))
    elem[:, 0, 0, 0] = d / 2
    elem[:, 0, 1, 0] = -d / 2
    sky, _ = make_test_sky()
    l = sky.lmn(RA0, DEC0)[0]
    E = table(arr.StationBeam(elem), sky)
    assert E.shape == (Tt, 1, len(sky))
    ref = np.cos(math.pi * FREQ / C_LIGHT * d * l)
    assert np.abs(E - ref[None, None, :]).max() < 1e-12
    assert np.abs(ref).min() < 0.9            # the beam is not all ones

    _, beam, _ = make_geometry(4, 7)
    centre = rsky.SkyModel.from_arrays(["P0"], [RA0], [DEC0], [1.0], [0.0],
                                       150e6)
    assert np.array_equal(table(beam, centre), np.ones((3, 4, 1)))
    E = table(beam, sky)
    assert np.abs(E).max() <= 1.0 + 1e-12
    assert np.abs(E).min() < 0.95


# --------------------------------------------------------------------------
# 2. a station is the mean of its elements (the sign convention)
# --------------------------------------------------------------------------

def test_station_equals_mean_of_its_elements():
    N, Ne, Tt = 4, 7, 3
    _, beam, uvw = make_geometry(N, Ne, Tt)
    sky, clusters = point_sky()
    C = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                beam=beam).to(torch.complex128)
    p, q = (i.numpy() for i in baseline_pq(N))
    B = len(p)
    el = torch.as_tensor(beam.elem_uvw)                  # (Tt,N,Ne,3)
    mean = torch.zeros_like(C)
    for e in range(Ne):
        for f in range(Ne):
            off = (el[:, p, e] - el[:, q, f]).reshape(Tt * B, 3)
            mean += predict_coherencies_uvw(
                sky, clusters, uvw + off, FREQ, RA0, DEC0
            ).to(torch.complex128) / (Ne * Ne)
    err = float((C - mean).abs().max() / mean.abs().max())
    print(f"station vs mean over element pairs: {err:.3e}")
    assert err < 1e-5, err
    plain = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0)
    assert float((C - plain).abs().max()) > 0.1 * float(plain.abs().max())


# --------------------------------------------------------------------------
# 3. prediction vs the per-sample loop transcription
# --------------------------------------------------------------------------

@pytest.mark.parametrize("smear_bw", [None, 180e3])
def test_beam_predict_matches_loop_oracle(smear_bw):
    sky, clusters = make_test_sky()
    _, beam, uvw = make_geometry(4, 7, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        C = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                    smear_bw=smear_bw, beam=beam)
    assert C.shape == (2, 18, 4) and C.dtype == torch.complex64
    assert bool(torch.isfinite(torch.view_as_real(C)).all())
    out = C.to(torch.complex128).numpy()
    ref = beam_loop_oracle(sky, clusters, uvw, FREQ, smear_bw, beam)
    for k in range(2):
        err = rel_err(out[k], ref[k])
        print(f"smear={smear_bw} cluster {k}: rel err {err:.3e}")
        assert err < 1e-5, (k, err)
    assert np.array_equal(out[:, :, 1], out[:, :, 2])
    assert np.abs(out[:, :, 1]).max() > 0
    # the beam is a visible share of the result and moves with time
    plain = beam_loop_oracle(sky, clusters, uvw, FREQ, smear_bw, None)
    beamless = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                       smear_bw=smear_bw)
    for k in range(2):
        assert rel_err(beamless[k].to(torch.complex128).numpy(),
                       plain[k]) < 1e-5
    share = np.abs(ref - plain).max() / np.abs(plain).max()
    E = table(beam, sky)
    drift = np.abs(E[0] - E[2]).max()
    print(f"beam vs beamless {share:.3f}, max|E[0]-E[2]| {drift:.3f}")
    assert share > 0.1
    assert drift > 0.05


# --------------------------------------------------------------------------
# 4. one element at the station centre is no beam
# --------------------------------------------------------------------------

@pytest.mark.parametrize("smear_bw", [None, 180e3])
def test_single_element_at_origin_is_beamless(smear_bw):
    sky, clusters = make_test_sky()
    _, _, uvw = make_geometry(4, 7, 3)
    beam = arr.StationBeam(np.zeros((3, 4, 1, 3)))
    C = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                smear_bw=smear_bw, beam=beam)
    plain = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                    smear_bw=smear_bw)
    assert float((C - plain).abs().max()) < 1e-6 * float(plain.abs().max())


# --------------------------------------------------------------------------
# 5. beam=None is today's call; shape errors
# --------------------------------------------------------------------------

def test_beam_none_and_shape_errors():
    sky, clusters = make_test_sky()
    _, beam, uvw = make_geometry(4, 7, 3)
    for smear in (None, 180e3):
        a = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                    smear_bw=smear)
        b = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                    smear_bw=smear, beam=None)
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="17.*18"):          # wrong T
        predict_coherencies_uvw(sky, clusters, uvw[:17], FREQ, RA0, DEC0,
                                beam=beam)
    _, beam5, _ = make_geometry(5, 7, 3)
    with pytest.raises(ValueError, match="18.*30"):          # wrong N
        predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                beam=beam5)
    layout, _, _ = make_geometry(4, 7, 3)
    with pytest.raises(ValueError):
        arr.station_beam(layout, np.zeros((5, 7, 3)), RA0, DEC0,
                         np.arange(3.0))


# --------------------------------------------------------------------------
# 6. the factored-out rotations leave uvw synthesis bit-identical
# --------------------------------------------------------------------------

def _baselines_xyz_literal(layout):
    lat = layout.latitude
    e, n, u = layout.enu[:, 0], layout.enu[:, 1], layout.enu[:, 2]
    x = -math.sin(lat) * n + math.cos(lat) * u
    y = e
    z = math.cos(lat) * n + math.sin(lat) * u
    xyz = np.stack([x, y, z], axis=1)
    pi, qi = np.triu_indices(xyz.shape[0], k=1)
    return xyz[pi] - xyz[qi]


def _uvw_synthesis_literal(layout, ra0, dec0, times_s, ha0=0.0):
    Lxyz = _baselines_xyz_literal(layout)
    H = ha0 + arr.EARTH_OMEGA * np.asarray(times_s, np.float64) - ra0
    sH, cH = np.sin(H), np.cos(H)
    sd, cd = math.sin(dec0), math.cos(dec0)
    zero = np.zeros_like(sH)
    ru = np.stack([sH, cH, zero], axis=1)
    rv = np.stack([-sd * cH, sd * sH, np.full_like(sH, cd)], axis=1)
    rw = np.stack([cd * cH, -cd * sH, np.full_like(sH, sd)], axis=1)
    return np.stack([ru @ Lxyz.T, rv @ Lxyz.T, rw @ Lxyz.T], axis=2)


def test_rotation_helpers_keep_uvw_bit_identical():
    layout = arr.lofar_like_layout(13, np.random.default_rng(3))
    times = np.arange(7) * 10.0
    assert np.array_equal(layout.baselines_xyz(),
                          _baselines_xyz_literal(layout))
    for ha0 in (0.0, 0.7):
        assert np.array_equal(
            arr.uvw_synthesis(layout, RA0, DEC0, times, ha0),
            _uvw_synthesis_literal(layout, RA0, DEC0, times, ha0))
    # an element at the station's own offset from station 0 rotates to
    # the baseline's uvw: both share the two rotations
    elem = (layout.enu - layout.enu[0])[None].repeat(13, axis=0)
    beam = arr.station_beam(layout, elem, RA0, DEC0, times)
    assert beam.elem_uvw.shape == (7, 13, 13, 3)
    uvw = arr.uvw_synthesis(layout, RA0, DEC0, times)      # (7,B,3), p<q
    np.testing.assert_allclose(beam.elem_uvw[:, 0, 1:], -uvw[:, :12],
                               rtol=0, atol=1e-8)
    elem = arr.station_elements(13, 48, np.random.default_rng(0))
    assert elem.shape == (13, 48, 3) and not elem[:, :, 2].any()
    r = np.hypot(elem[:, :, 0], elem[:, :, 1])
    assert r.max() <= 15.0
    np.testing.assert_allclose(np.sort(r, axis=1), np.sort(r[:1], axis=1)
                               .repeat(13, axis=0), atol=1e-9)
    assert np.abs(elem[0] - elem[1]).max() > 1.0           # own rotation


# --------------------------------------------------------------------------
# 7. simulated observation
# --------------------------------------------------------------------------

def test_simulate_observation_with_beam():
    sc = sim.make_calibration_sky(3, np.random.default_rng(7), diffuse=True,
                                  diffuse_beta=0.02)
    layout = arr.lofar_like_layout(8, np.random.default_rng(1))
    elem = arr.station_elements(8, 12, np.random.default_rng(4))
    freqs = np.linspace(140e6, 160e6, 2)
    vis = [sim.simulate_observation(layout, sc[0], sc[1], freqs, sc[6],
                                    sc[7], 1, 4,
                                    rng=np.random.default_rng(2),
                                    torch_seed=0, **kw)
           for kw in ({}, {"beam_elements": elem})]
    assert vis[0].beam is None
    assert vis[1].beam is not None
    assert vis[1].beam.elem_uvw.shape == (4, 8, 12, 3)
    assert np.array_equal(vis[0].J_true, vis[1].J_true)
    for v in vis:
        assert bool(torch.isfinite(torch.view_as_real(v.model)).all())
        assert bool(torch.isfinite(torch.view_as_real(v.data)).all())
    d = float((vis[1].model - vis[0].model).abs().max())
    assert d > 1e-2 * float(vis[0].model.abs().max())


# --------------------------------------------------------------------------
# 8. CalibEnv
# --------------------------------------------------------------------------

def test_calibenv_station_beam_cpu():
    from smartcal_amd.envs.calib import CalibEnv
    kw = dict(M=3, N_stations=8, Nf=2, Ts=1, Tdelta=4, Ninf=32,
              device="cpu", seed=0)
    env = CalibEnv(station_beam=True, beam_elements=12, **kw)
    obs = env.reset()
    assert env._scenario["vis"].beam.elem_uvw.shape == (4, 8, 12, 3)
    assert np.isfinite(obs["img"]).all() and np.isfinite(obs["sky"]).all()
    obs, reward, done, _ = env.step(np.zeros(6, np.float32))
    assert np.isfinite(obs["img"]).all() and np.isfinite(obs["sky"]).all()
    assert math.isfinite(reward)

    first = [CalibEnv(**kw2).reset()
             for kw2 in (kw, dict(kw, station_beam=False))]
    assert first[0].keys() == first[1].keys()
    for key in first[0]:
        assert np.array_equal(first[0][key], first[1][key])
    assert not np.array_equal(first[0]["img"], CalibEnv(
        station_beam=True, beam_elements=12, **kw).reset()["img"])


# --------------------------------------------------------------------------
# 9. pipeline CLI
# --------------------------------------------------------------------------

def test_calibration_pipeline_beam_tiny(tmp_path):
    r = _run("scripts/calibration/pipeline.py", "--K", "2", "--stations",
             "8", "--nf", "2", "--ts", "1", "--tdelta", "4", "--admm", "2",
             "--poly", "2", "--beam", "--beam-elements", "6", cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "data_img.npy").exists()
