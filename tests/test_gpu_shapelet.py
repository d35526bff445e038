"""shapelet_kernel (ops/csrc/shapelet.hip) vs the eager torch composition
and a numpy oracle built on `shapelet_uv`; long baselines, cluster
layouts, the no-shapelet path and the simulated observation (GPU)."""

import math
import os

import numpy as np
import pytest
import torch

from smartcal_amd.radio import array as arr, sim, sky as rsky
from smartcal_amd.radio import coherency
from smartcal_amd.radio.coherency import C_LIGHT, predict_coherencies_uvw
from smartcal_amd.radio.coords import lmtoradec
from smartcal_amd.radio.shapelet import ShapeletModel, shapelet_uv

from test_shapelet_predict import (DEC0, FREQ, RA0, make_test_sky, make_uvw,
                                   without_shapelets)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]


def predict_gpu(sky, clusters, uvw, smear_bw, eager=False, freq=FREQ):
    if eager:
        os.environ["SMARTCAL_FORCE_EAGER"] = "1"
    try:
        return predict_coherencies_uvw(sky, clusters, uvw.cuda(), freq, RA0,
                                       DEC0, smear_bw=smear_bw)
    finally:
        if eager:
            del os.environ["SMARTCAL_FORCE_EAGER"]


def shapelet_numpy_oracle(sky, clusters, uvw, freq, smear_bw):
    """Shapelet part of the coherencies, (K, T, 4) complex128, from
    `shapelet_uv` (numpy f64)."""
    uvw = uvw.double().numpy() * (2.0 * math.pi / C_LIGHT * freq)
    u, v, w = uvw.T
    l, m, n = sky.lmn(RA0, DEC0)
    idx = sky.index
    out = np.zeros((len(clusters), uvw.shape[0], 4), np.complex128)
    for k, cl in enumerate(clusters):
        for nm in cl.names:
            if nm not in sky.shapelets:
                continue
            s = idx[nm]
            fr = math.log(freq / sky.f0[s])
            fac = math.exp(sky.sP[s, 0] * fr + sky.sP[s, 1] * fr ** 2
                           + sky.sP[s, 2] * fr ** 3)
            ph = u * l[s] + v * m[s] + w * n[s]
            G = np.exp(1j * ph) * shapelet_uv(sky.shapelets[nm], u, v)
            if smear_bw is not None:
                # np.sinc(x) = sin(πx)/(πx)
                G = G * np.abs(np.sinc(ph * 0.5 * smear_bw / freq / math.pi))
            out[k, :, 0] += (sky.sI[s] + sky.sQ[s]) * fac * G
            out[k, :, 3] += (sky.sI[s] - sky.sQ[s]) * fac * G
            out[k, :, 1] += sky.sU[s] * fac * G
            out[k, :, 2] += sky.sU[s] * fac * G
    return out


def rel_err(out, ref):
    return float(np.abs(out - ref).max() / np.abs(ref).max())


# 1. kernel vs eager composition and vs the numpy oracle -------------------

@pytest.mark.parametrize("T", [45, 300, 1000])
@pytest.mark.parametrize("n0", [1, 2, 7, 19, 32])
def test_shapelet_kernel_matches_oracles(n0, T, monkeypatch):
    from smartcal_amd.ops import ext
    sky, clusters = make_test_sky(n0_a=(4, n0), n0_b=n0)
    sub, sub_cl = without_shapelets(sky, clusters)
    uvw = make_uvw(T)
    launches = []
    kernel = ext().shapelet_predict
    monkeypatch.setattr(ext(), "shapelet_predict",
                        lambda *a: (launches.append(1), kernel(*a))[1])
    for smear in (None, 180e3):
        launches.clear()
        out = predict_gpu(sky, clusters, uvw, smear)
        # one launch covers all shapelet sources of all clusters
        assert len(launches) == 1
        assert out.shape == (2, T, 4) and out.dtype == torch.complex64
        assert bool(torch.isfinite(torch.view_as_real(out)).all())
        out = out.cpu().to(torch.complex128).numpy()
        eager = predict_gpu(sky, clusters, uvw, smear, eager=True)
        assert len(launches) == 1                  # eager: no kernel
        eager = eager.cpu().to(torch.complex128).numpy()
        base = predict_gpu(sub, sub_cl, uvw, smear)
        ref = base.cpu().to(torch.complex128).numpy() \
            + shapelet_numpy_oracle(sky, clusters, uvw, FREQ, smear)
        for k in range(2):
            e_eager, e_np = rel_err(out[k], eager[k]), rel_err(out[k], ref[k])
            print(f"n0={n0} T={T} smear={smear} k={k}: vs eager "
                  f"{e_eager:.3e}, vs numpy {e_np:.3e}")
            assert e_eager < 1e-5, (smear, k, e_eager)
            assert e_np < 1e-5, (smear, k, e_np)
        assert np.array_equal(out[:, :, 1], out[:, :, 2])
        assert np.abs(out[1, :, 0] - out[1, :, 3]).max() > 0


# 2. long baselines --------------------------------------------------------

def test_shapelet_kernel_long_baselines():
    beta = 0.1
    rng = np.random.default_rng(11)
    names = ["P0", "P1", "G0", "SL"]
    l = np.asarray([0.02, -0.03, 0.015, 0.0])
    m = np.asarray([-0.01, 0.02, -0.02, 0.0])
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    sky = rsky.SkyModel.from_arrays(
        names, ra, dec, [1.0, 2.0, 3.0, 5.0], [-0.7, -0.5, -0.8, -0.1], 140e6,
        [0, 0, 0.002, 0], [0, 0, 0.001, 0], [0, 0, 0.5, 0],
        sQ=[0, 0, 0, 2.0], sU=[0, 0, 0, 1.0],
        shapelets={"SL": ShapeletModel(19, beta,
                                       rng.standard_normal(19 * 19))})
    clusters = rsky.ClusterSet([rsky.ClusterDef(1, 1, names)])
    T = 600
    uvw = (rng.random((T, 3)) * 2 - 1)
    uvw[:300] *= 100e3                 # up to ±100 km
    uvw[300:] *= [150.0, 150.0, 15.0]  # |βu| within the support
    uvw[-1] = 0.0
    uvw = torch.as_tensor(uvw, dtype=torch.float32)
    sub, sub_cl = without_shapelets(sky, clusters)
    for smear in (None, 180e3):
        out = predict_gpu(sky, clusters, uvw, smear).cpu()
        base = predict_gpu(sub, sub_cl, uvw, smear).cpu()
        assert bool(torch.isfinite(torch.view_as_real(out)).all())
        bu = beta * uvw.double().numpy() * (2.0 * math.pi / C_LIGHT * FREQ)
        far = (np.abs(bu[:, 0]) > 40) | (np.abs(bu[:, 1]) > 40)
        assert far.sum() > 250 and (~far).sum() > 100
        far_t = torch.as_tensor(far)
        assert torch.equal(out[:, far_t], base[:, far_t])
        near = out[:, ~far_t] - base[:, ~far_t]
        assert float(near.abs().max()) > 1e-3
        ref = base.to(torch.complex128).numpy() \
            + shapelet_numpy_oracle(sky, clusters, uvw, FREQ, smear)
        assert rel_err(out.to(torch.complex128).numpy(), ref) < 1e-5


# 3. cluster layouts -------------------------------------------------------

def test_shapelet_cluster_layouts_sum_of_single_sources():
    rng = np.random.default_rng(12)
    beta = 0.01
    names = ["P0", "P1", "G0", "S1", "S2", "S3", "S4"]
    l = np.asarray([0.02, -0.03, 0.015, 0.0, 0.01, -0.01, 0.005])
    m = np.asarray([-0.01, 0.02, -0.02, 0.0, 0.012, 0.008, -0.006])
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    n0s = {"S1": 3, "S2": 8, "S3": 19, "S4": 5}
    shp = {nm: ShapeletModel(n0, beta, rng.standard_normal(n0 * n0),
                             1.0 + 0.1 * i, 1.0 - 0.1 * i, 0.3 * i)
           for i, (nm, n0) in enumerate(n0s.items())}
    sky = rsky.SkyModel.from_arrays(
        names, ra, dec, [1.0, 2.0, 3.0, 80.0, 60.0, 0.0, 40.0],
        [-0.7, -0.5, -0.8, -0.1, -0.2, -0.1, 0.1], 140e6,
        [0, 0, 0.002, 0, 0, 0, 0], [0, 0, 0.001, 0, 0, 0, 0],
        [0, 0, 0.5, 0, 0, 0, 0], sQ=[0, 0, 0, 10.0, -20.0, 50.0, 5.0],
        sU=[0, 0, 0, 5.0, 8.0, -30.0, 0.0], shapelets=shp)
    layout = [["S1", "S2", "S3"], ["P0", "P1"], ["G0", "S4"]]
    clusters = rsky.ClusterSet([rsky.ClusterDef(i + 1, 1, nm)
                                for i, nm in enumerate(layout)])
    uvw = make_uvw(300)
    sub, sub_cl = without_shapelets(sky, clusters)
    for smear in (None, 180e3):
        out = predict_gpu(sky, clusters, uvw, smear).cpu()
        base = predict_gpu(sub, sub_cl, uvw, smear).cpu()
        assert bool((base[0] == 0).all())
        assert torch.equal(out[1], base[1])        # cluster with none
        total = base.to(torch.complex128)
        for nm in n0s:
            only = rsky.ClusterSet([
                rsky.ClusterDef(c.cid, 1, [n for n in c.names if n == nm])
                for c in clusters])
            total += predict_gpu(sky, only, uvw, smear).cpu() \
                .to(torch.complex128)
        out = out.to(torch.complex128).numpy()
        for k in (0, 2):
            assert rel_err(out[k], total[k].numpy()) < 1e-5
        assert np.abs(out[0]).max() > 0


# 4. no-shapelet sky -------------------------------------------------------

def test_no_shapelet_sky_skips_the_kernel(monkeypatch):
    from smartcal_amd.ops import ext
    sky, clusters = make_test_sky()
    sub, sub_cl = without_shapelets(sky, clusters)
    uvw = make_uvw(300)

    def boom(*a, **k):
        raise AssertionError("shapelet_predict launched without shapelets")

    monkeypatch.setattr(ext(), "shapelet_predict", boom, raising=False)
    scale = 2.0 * math.pi / C_LIGHT * FREQ
    for smear in (None, 180e3):
        out = predict_gpu(sub, sub_cl, uvw, smear)
        ref = coherency._predict_hip(
            sub, sub_cl, (uvw.cuda().double() * scale).contiguous(), FREQ,
            RA0, DEC0, (smear / FREQ) if smear is not None else 0.0)
        assert torch.equal(out, ref)


# 5. simulated observation -------------------------------------------------

def test_simulate_observation_diffuse_gpu_matches_cpu():
    sc = sim.make_calibration_sky(3, np.random.default_rng(7), diffuse=True,
                                  diffuse_beta=0.02)
    layout = arr.lofar_like_layout(10, np.random.default_rng(1))
    freqs = np.linspace(140e6, 160e6, 2)
    vis = [sim.simulate_observation(layout, sc[0], sc[1], freqs, sc[6],
                                    sc[7], 1, 4, device=dev,
                                    rng=np.random.default_rng(2),
                                    torch_seed=0)
           for dev in ("cpu", "cuda")]
    cpu, gpu = vis[0].model, vis[1].model.cpu()
    assert bool(torch.isfinite(torch.view_as_real(gpu)).all())
    err = float((gpu - cpu).abs().max() / cpu.abs().max())
    print(f"simulate_observation model gpu vs cpu: {err:.3e}")
    assert err < 1e-4, err
