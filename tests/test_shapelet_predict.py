"""Shapelet (diffuse-sky) sources: closed-form transform vs brute-force
quadrature, numerical stability, coherency prediction vs a per-sample
loop transcription, sky generation and the public surface (CPU)."""

import math
import warnings

import numpy as np
import pytest
import torch

from smartcal_amd.radio import array as arr, sim, sky as rsky
from smartcal_amd.radio.coherency import C_LIGHT, predict_coherencies_uvw
from smartcal_amd.radio.coords import lmtoradec
from smartcal_amd.radio.shapelet import (
    ShapeletModel, generate_random_shapelet_model, hermite_functions,
    load_shapelet_model, parse_shapelet_model, shapelet_image, shapelet_uv)

RA0, DEC0 = 0.3, 0.9
FREQ = 150e6


# --------------------------------------------------------------------------
# 1. closed form vs quadrature of the image-domain model
# --------------------------------------------------------------------------

@pytest.mark.parametrize("n0", [1, 4, 5])
@pytest.mark.parametrize("abt", [(1.0, 1.0, 0.0), (1.0, 1.0, math.pi / 2),
                                 (1.3, 0.7, 0.4)])
def test_shapelet_uv_matches_quadrature(n0, abt):
    rng = np.random.default_rng(10 * n0 + int(10 * abt[2]))
    beta = 0.02
    mdl = ShapeletModel(n0, beta, rng.standard_normal(n0 * n0), *abt)
    half = 10 * beta * max(mdl.a, mdl.b)
    g = np.linspace(-half, half, 301)
    h = g[1] - g[0]
    X, Y = np.meshgrid(g, g, indexing="ij")
    img = shapelet_image(mdl, X.ravel(), Y.ravel())
    uv = np.concatenate([(rng.random((24, 2)) * 2 - 1) * 5 / beta,
                         np.zeros((1, 2))])
    quad = np.asarray([
        np.sum(img * np.exp(1j * (u * X.ravel() + v * Y.ravel()))) * h * h
        for u, v in uv])
    F = shapelet_uv(mdl, uv[:, 0], uv[:, 1])
    err = np.abs(F - quad).max() / np.abs(quad).max()
    print(f"n0={n0} abt={abt}: rel err {err:.3e}")
    assert err < 1e-9, err


# --------------------------------------------------------------------------
# 2. stability of the recurrence on long baselines
# --------------------------------------------------------------------------

def test_hermite_recurrence_is_stable():
    t = np.asarray([0.0, 1.0, 6.0, 40.0, 300.0, 3000.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        psi = hermite_functions(20, t)
        psi_neg = hermite_functions(20, -t)
        beta = 0.1
        rng = np.random.default_rng(0)
        mdl = ShapeletModel(19, beta, rng.standard_normal(19 * 19))
        Fu = shapelet_uv(mdl, t / beta, np.zeros_like(t))
        Fv = shapelet_uv(mdl, np.zeros_like(t), -t / beta)
    assert np.isfinite(psi).all() and np.isfinite(psi_neg).all()
    assert (psi[:, t >= 40] == 0).all() and (psi_neg[:, t >= 40] == 0).all()
    assert psi[19, 2] != 0.0                      # ψ_19(6)
    assert np.isfinite(Fu).all() and np.isfinite(Fv).all()
    assert (Fu[t >= 40] == 0).all() and (Fv[t >= 40] == 0).all()
    assert (Fu[t < 40] != 0).all()


# --------------------------------------------------------------------------
# shared scenario: 2 clusters, point + Gaussian + shapelet sources
# --------------------------------------------------------------------------

def make_test_sky(n0_a=(4, 7), n0_b=5, beta=0.01, seed=3):
    """Cluster A: 3 points, 1 Gaussian, two off-centre shapelets of
    different n0; cluster B: one shapelet with sI = 0, sQ ≠ 0 and a
    non-trivial (a, b, θ)."""
    rng = np.random.default_rng(seed)
    names = ["P0", "P1", "P2", "G0", "SA1", "SA2", "SB1"]
    l = np.asarray([0.02, -0.03, 0.01, 0.015, 0.01, -0.012, 0.008])
    m = np.asarray([-0.01, 0.02, 0.03, -0.02, 0.011, 0.009, -0.01])
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    # shapelet fluxes ~1/(2πβ²) larger, so that their visibilities are
    # of the order of the point sources' (F carries a factor 2πβ²)
    sI = [1.0, 2.0, 0.5, 3.0, 100.0, 50.0, 0.0]
    sQ = [0.0, 0.0, 0.0, 0.0, 25.0, -20.0, 75.0]
    sU = [0.0, 0.0, 0.0, 0.0, 15.0, 10.0, 35.0]
    sP = np.zeros((7, 3))
    sP[:, 0] = [-0.7, -0.5, 0.2, -0.8, -0.1, -0.3, -0.1]
    sP[:, 1] = [0.0, 0.1, 0.0, 0.0, 0.05, 0.0, 0.02]
    eX = [0, 0, 0, 0.002, 0, 0, 0]
    eY = [0, 0, 0, 0.001, 0, 0, 0]
    eP = [0, 0, 0, 0.5, 0, 0, 0]
    shp = {
        "SA1": ShapeletModel(n0_a[0], beta,
                             rng.standard_normal(n0_a[0] ** 2)),
        "SA2": ShapeletModel(n0_a[1], 0.8 * beta,
                             rng.standard_normal(n0_a[1] ** 2),
                             1.2, 0.8, 0.3),
        "SB1": ShapeletModel(n0_b, beta, rng.standard_normal(n0_b ** 2),
                             1.3, 0.7, 0.4),
    }
    sky = rsky.SkyModel.from_arrays(names, ra, dec, sI, sP, 140e6, eX, eY,
                                    eP, sQ=sQ, sU=sU, shapelets=shp)
    clusters = rsky.ClusterSet([
        rsky.ClusterDef(1, 1, names[:6]), rsky.ClusterDef(2, 1, ["SB1"])])
    return sky, clusters


def make_uvw(T, seed=4, span=300.0):
    rng = np.random.default_rng(seed)
    uvw = (rng.random((T, 3)) * 2 - 1) * [span, span, span / 10]
    return torch.as_tensor(uvw, dtype=torch.float32)


def without_shapelets(sky, clusters):
    """The same sky and clusters with every shapelet source removed."""
    keep = [i for i, n in enumerate(sky.names) if n not in sky.shapelets]
    sub = rsky.SkyModel.from_arrays(
        [sky.names[i] for i in keep], sky.ra[keep], sky.dec[keep],
        sky.sI[keep], sky.sP[keep], sky.f0[keep], sky.eX[keep],
        sky.eY[keep], sky.eP[keep], sky.gaussian[keep])
    cl = rsky.ClusterSet([
        rsky.ClusterDef(c.cid, c.hybrid,
                        [n for n in c.names if n not in sky.shapelets])
        for c in clusters])
    return sub, cl


def _psi_scalar(n0, t):
    p = [math.pi ** -0.25 * math.exp(-0.5 * t * t)]
    if n0 > 1:
        p.append(math.sqrt(2.0) * t * p[0])
    for n in range(1, n0 - 1):
        p.append(t * math.sqrt(2.0 / (n + 1)) * p[n]
                 - math.sqrt(n / (n + 1)) * p[n - 1])
    return p


def shapelet_loop_oracle(sky, clusters, uvw, freq, smear_bw):
    """Per-sample, per-mode python transcription of the shapelet
    coherency formulas → (K, T, 4) complex128 (shapelet part only)."""
    scale = 2.0 * math.pi / C_LIGHT * freq
    uvw = uvw.double().numpy() * scale
    l, m, n = sky.lmn(RA0, DEC0)
    idx = sky.index
    out = np.zeros((len(clusters), uvw.shape[0], 4), np.complex128)
    for k, cl in enumerate(clusters):
        for nm in cl.names:
            if nm not in sky.shapelets:
                continue
            s = idx[nm]
            mdl = sky.shapelets[nm]
            fr = math.log(freq / sky.f0[s])
            fac = math.exp(sky.sP[s, 0] * fr + sky.sP[s, 1] * fr ** 2
                           + sky.sP[s, 2] * fr ** 3)
            fI, fQ, fU = sky.sI[s] * fac, sky.sQ[s] * fac, sky.sU[s] * fac
            ct, st = math.cos(mdl.theta), math.sin(mdl.theta)
            for t, (u, v, w) in enumerate(uvw):
                up = ct * u + st * v
                vp = -st * u + ct * v
                pu = _psi_scalar(mdl.n0, mdl.beta * mdl.a * up)
                pv = _psi_scalar(mdl.n0, mdl.beta * mdl.b * vp)
                F = 0j
                for i in range(mdl.n0):
                    for j in range(mdl.n0):
                        F += mdl.coeff[i * mdl.n0 + j] * 1j ** (i + j) \
                            * pu[i] * pv[j]
                F *= 2.0 * math.pi * mdl.beta * mdl.a * mdl.b
                ph = u * l[s] + v * m[s] + w * n[s]
                sm = 1.0
                if smear_bw is not None:
                    x = ph * 0.5 * smear_bw / freq
                    sm = 1.0 if x == 0 else abs(math.sin(x) / x)
                G = sm * complex(math.cos(ph), math.sin(ph)) * F
                out[k, t, 0] += (fI + fQ) * G
                out[k, t, 3] += (fI - fQ) * G
                out[k, t, 1] += fU * G
                out[k, t, 2] += fU * G
    return out


def reference_prediction(sky, clusters, uvw, freq, smear_bw):
    """Point/Gaussian part from the (separately oracle-tested) prediction
    of the sky without its shapelet sources, plus the shapelet loop
    oracle."""
    sub, cl = without_shapelets(sky, clusters)
    base = predict_coherencies_uvw(sub, cl, uvw, freq, RA0, DEC0,
                                   smear_bw=smear_bw)
    return base.to(torch.complex128).numpy() \
        + shapelet_loop_oracle(sky, clusters, uvw, freq, smear_bw)


# --------------------------------------------------------------------------
# 3. prediction vs the loop transcription
# --------------------------------------------------------------------------

@pytest.mark.parametrize("smear_bw", [None, 180e3])
def test_predict_matches_loop_oracle(smear_bw):
    sky, clusters = make_test_sky()
    uvw = make_uvw(300)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        C = predict_coherencies_uvw(sky, clusters, uvw, FREQ, RA0, DEC0,
                                    smear_bw=smear_bw)
    assert C.shape == (2, 300, 4) and C.dtype == torch.complex64
    assert bool(torch.isfinite(torch.view_as_real(C)).all())
    ref = reference_prediction(sky, clusters, uvw, FREQ, smear_bw)
    out = C.to(torch.complex128).numpy()
    for k in range(2):
        err = np.abs(out[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(f"smear={smear_bw} cluster {k}: rel err {err:.3e}")
        assert err < 1e-5, (k, err)
    # Q ≠ 0 splits XX from YY; XY = YX = sU·G is non-zero
    assert np.abs(out[1, :, 0] - out[1, :, 3]).max() \
        > 0.1 * np.abs(out[1]).max()
    assert np.array_equal(out[:, :, 1], out[:, :, 2])
    assert np.abs(out[:, :, 1]).max() > 0
    # the shapelet term is a visible share of the total, not rounding
    base = ref - shapelet_loop_oracle(sky, clusters, uvw, FREQ, smear_bw)
    assert np.abs(ref[0] - base[0]).max() > 0.1 * np.abs(base[0]).max()


# --------------------------------------------------------------------------
# 4. skies without shapelets are untouched
# --------------------------------------------------------------------------

def test_no_shapelet_sky_unchanged():
    names = ["P0", "P1", "G0", "S0"]
    l = np.asarray([0.02, -0.03, 0.015, 0.01])
    m = np.asarray([-0.01, 0.02, -0.02, 0.011])
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    sI, sP = [1.0, 2.0, 3.0, 1.5], [-0.7, -0.5, -0.8, -0.1]
    eX, eY, eP = [0, 0, 0.002, 0], [0, 0, 0.001, 0], [0, 0, 0.5, 0]
    old = rsky.SkyModel.from_arrays(names, ra, dec, sI, sP, 140e6, eX, eY,
                                    eP)
    new = rsky.SkyModel.from_arrays(names, ra, dec, sI, sP, 140e6, eX, eY,
                                    eP, sQ=np.zeros(4), sU=np.zeros(4),
                                    shapelets={})
    # 'S…' without an attached model is a point source
    pt = rsky.SkyModel.from_arrays(["P0", "P1", "G0", "P9"], ra, dec, sI,
                                   sP, 140e6, eX, eY, eP)
    assert old.shapelets == {} and not old.is_shapelet.any()
    uvw = make_uvw(100)
    for smear in (None, 180e3):
        outs = []
        for s in (old, new, pt):
            cl = rsky.ClusterSet([rsky.ClusterDef(1, 1, s.names[:2]),
                                  rsky.ClusterDef(2, 1, s.names[2:])])
            outs.append(predict_coherencies_uvw(s, cl, uvw, FREQ, RA0, DEC0,
                                                smear_bw=smear))
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[0], outs[2])
        assert bool((outs[0][:, :, 1:3] == 0).all())


# --------------------------------------------------------------------------
# 5. diffuse component of the calibration scenario
# --------------------------------------------------------------------------

DIFFUSE = ("SLSIRandom", "SLSQRandom", "SLSURandom")


def test_make_calibration_sky_diffuse():
    K = 3
    plain = sim.make_calibration_sky(K, np.random.default_rng(7))
    diff = sim.make_calibration_sky(K, np.random.default_rng(7),
                                    diffuse=True, diffuse_beta=0.02)
    assert len(diff) == len(plain) == 8
    sky0, sky1 = plain[0], diff[0]
    cs_sim, cs_cal = diff[1], diff[3]
    n = len(sky0)
    assert sky1.names == sky0.names + list(DIFFUSE)
    assert set(sky1.shapelets) == set(DIFFUSE)
    assert not sky0.shapelets
    for nm in DIFFUSE:
        assert nm in cs_sim[len(cs_sim) - 1].names
        assert all(nm not in c.names for c in cs_cal)
        assert all(nm not in c.names for c in list(cs_sim)[:-1])
        assert sky1.shapelets[nm].beta == 0.02
    for f in ("ra", "dec", "sI", "sP", "f0", "eX", "eY", "eP", "gaussian"):
        assert np.array_equal(getattr(sky1, f)[:n], getattr(sky0, f))
    assert np.array_equal(diff[4], plain[4])
    assert np.array_equal(diff[5], plain[5])
    assert [c.names for c in cs_cal] == [c.names for c in plain[3]]
    assert np.array_equal(sky1.sI[n:], [250.0, 0, 0])
    assert np.array_equal(sky1.sQ[n:], [0, 250.0, 0])
    assert np.array_equal(sky1.sU[n:], [0, 0, 250.0])
    assert np.array_equal(sky1.sP[n:, 0], [-0.1] * 3)
    assert not (sky1.sQ[:n].any() or sky1.sU[:n].any())
    # three independent draws; without the override β is the model's own
    own = sim.make_calibration_sky(K, np.random.default_rng(7),
                                   diffuse=True, diffuse_flux=10.0)[0]
    betas = [own.shapelets[nm].beta for nm in DIFFUSE]
    assert len(set(betas)) == 3 and all(b != 0.02 for b in betas)
    assert own.sI[n] == 10.0

    layout = arr.lofar_like_layout(8, np.random.default_rng(1))
    freqs = np.linspace(140e6, 160e6, 2)
    vis = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for sc in (plain, diff):
            vis.append(sim.simulate_observation(
                layout, sc[0], sc[1], freqs, sc[6], sc[7], 1, 4,
                rng=np.random.default_rng(2), torch_seed=0))
    for v in vis:
        assert bool(torch.isfinite(torch.view_as_real(v.model)).all())
        assert bool(torch.isfinite(torch.view_as_real(v.data)).all())
    d = (vis[1].model - vis[0].model).abs().max()
    assert float(d) > 1e-3 * float(vis[0].model.abs().max())


# --------------------------------------------------------------------------
# 6. sky text keeps Q and U
# --------------------------------------------------------------------------

def test_sky_text_round_trip_keeps_qu():
    sky, _ = make_test_sky()
    text = rsky.write_sky_text(sky)
    back = rsky.parse_sky_text(text)
    np.testing.assert_allclose(back.sQ, sky.sQ, rtol=1e-5)
    np.testing.assert_allclose(back.sU, sky.sU, rtol=1e-5)
    np.testing.assert_allclose(back.sI, sky.sI, rtol=1e-5)
    assert back.shapelets == {}
    # Q = U = 0: the line is what it has always been
    from smartcal_amd.radio.coords import rad_to_ra, rad_to_dec
    sub, _ = without_shapelets(sky, rsky.ClusterSet([]))
    lines = rsky.write_sky_text(sub).splitlines()
    assert lines[0] == \
        "## name h m s d m s sI sQ sU sV sp1 sp2 sp3 RM eX eY eP f0"
    for i, nm in enumerate(sub.names):
        h, m, s = rad_to_ra(float(sub.ra[i]))
        d, dm, ds = rad_to_dec(float(sub.dec[i]))
        sp = sub.sP[i]
        assert lines[1 + i] == (
            f"{nm} {h} {m} {s:.6f} {d} {dm} {ds:.6f} {sub.sI[i]:.6g} 0 0 0 "
            f"{sp[0]:.6g} {sp[1]:.6g} {sp[2]:.6g} 0 {sub.eX[i]:.6g} "
            f"{sub.eY[i]:.6g} {sub.eP[i]:.6g} {sub.f0[i]:.6g}")


def test_load_shapelet_model_parses_trailer():
    text, n0, beta, coeff = generate_random_shapelet_model(
        np.random.default_rng(5))
    mdl = load_shapelet_model(text)
    assert (mdl.n0, mdl.beta) == (n0, beta)
    np.testing.assert_array_equal(mdl.coeff, coeff)
    assert (mdl.a, mdl.b, mdl.theta) == (1.0, 1.0, math.pi / 2)
    bare = "\n".join(l for l in text.splitlines() if not l.startswith("L"))
    mdl = load_shapelet_model(bare + "\n")
    assert (mdl.a, mdl.b, mdl.theta) == (1.0, 1.0, 0.0)
    custom = load_shapelet_model(bare + "\nL 1.5 0.5 0.25\n")
    assert (custom.a, custom.b, custom.theta) == (1.5, 0.5, 0.25)
    assert len(parse_shapelet_model(text)) == 4


# --------------------------------------------------------------------------
# 7. public surface
# --------------------------------------------------------------------------

def test_calibenv_diffuse_sky_cpu():
    from smartcal_amd.envs.calib import CalibEnv
    env = CalibEnv(M=3, N_stations=8, Nf=2, Ts=1, Tdelta=4, Ninf=32,
                   diffuse_sky=True, diffuse_beta=0.02, device="cpu",
                   seed=0)
    obs = env.reset()
    assert set(env._scenario["sky"].shapelets) == set(DIFFUSE)
    assert np.isfinite(obs["img"]).all() and np.isfinite(obs["sky"]).all()
    obs, reward, done, _ = env.step(np.zeros(6, np.float32))
    assert np.isfinite(obs["img"]).all() and np.isfinite(obs["sky"]).all()
    assert math.isfinite(reward)


# --------------------------------------------------------------------------
# 8. mode-order cap
# --------------------------------------------------------------------------

def test_n0_above_cap_raises():
    sky, clusters = make_test_sky(n0_b=33)
    with pytest.raises(ValueError, match="n0"):
        predict_coherencies_uvw(sky, clusters, make_uvw(10), FREQ, RA0,
                                DEC0)
