"""station_beam_kernel / coherency_beam_kernel / shapelet_beam_kernel
(ops/csrc/beam.hip, shapelet.hip) vs the eager torch composition and the
numpy oracles; tile edges, the beamless path and the simulated observation
(GPU)."""

import os

import numpy as np
import pytest
import torch

from smartcal_amd.radio import array as arr, sim, sky as rsky
from smartcal_amd.radio.coherency import predict_coherencies_uvw
from smartcal_amd.radio.coords import lmtoradec

from test_shapelet_predict import DEC0, FREQ, RA0, make_test_sky
from test_station_beam import (beam_loop_oracle, beam_numpy_oracle,
                               make_geometry, rel_err)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

BEAM_KERNELS = ("station_beam", "coherency_beam_predict")


def predict_gpu(sky, clusters, uvw, smear_bw, beam=None, eager=False):
    if eager:
        os.environ["SMARTCAL_FORCE_EAGER"] = "1"
    try:
        kw = {} if beam is None else {"beam": beam}
        return predict_coherencies_uvw(sky, clusters, uvw.cuda(), FREQ, RA0,
                                       DEC0, smear_bw=smear_bw, **kw)
    finally:
        if eager:
            del os.environ["SMARTCAL_FORCE_EAGER"]


def to_np(C):
    return C.cpu().to(torch.complex128).numpy()


# 1. kernels vs eager composition and vs the loop oracle -------------------

@pytest.mark.parametrize("smear_bw", [None, 180e3])
def test_beam_kernels_match_oracles(smear_bw, monkeypatch):
    from smartcal_amd.ops import ext
    sky, clusters = make_test_sky()
    _, beam, uvw = make_geometry(5, 7, 3)
    launches = []
    for name in BEAM_KERNELS + ("shapelet_predict",):
        kernel = getattr(ext(), name)
        monkeypatch.setattr(
            ext(), name,
            lambda *a, _n=name, _k=kernel: (launches.append(_n), _k(*a))[1])
    out = predict_gpu(sky, clusters, uvw, smear_bw, beam)
    # one launch each: E for the whole sky, point/Gaussian, shapelets
    assert sorted(launches) == sorted(BEAM_KERNELS + ("shapelet_predict",))
    assert out.shape == (2, 30, 4) and out.dtype == torch.complex64
    assert bool(torch.isfinite(torch.view_as_real(out)).all())
    out = to_np(out)
    eager = to_np(predict_gpu(sky, clusters, uvw, smear_bw, beam,
                              eager=True))
    assert len(launches) == 3                      # eager: no kernel
    ref = beam_loop_oracle(sky, clusters, uvw, FREQ, smear_bw, beam)
    for k in range(2):
        e_eager, e_np = rel_err(out[k], eager[k]), rel_err(out[k], ref[k])
        print(f"smear={smear_bw} k={k}: vs eager {e_eager:.3e}, "
              f"vs loop oracle {e_np:.3e}")
        assert e_eager < 1e-5, (k, e_eager)
        assert e_np < 1e-5, (k, e_np)
    assert np.array_equal(out[:, :, 1], out[:, :, 2])
    plain = to_np(predict_gpu(sky, clusters, uvw, smear_bw))
    assert np.abs(out - plain).max() > 0.1 * np.abs(plain).max()


# 2. tile edges ------------------------------------------------------------

@pytest.mark.parametrize("Ne", [1, 96])
def test_beam_kernel_tile_edges(Ne):
    N, Tt = 24, 2                     # B = 276 = one full 256 block + 20
    rng = np.random.default_rng(13)
    S = 132                           # 130 crosses the 128-source chunk
    l = (rng.random(S) * 2 - 1) * 0.03
    m = (rng.random(S) * 2 - 1) * 0.03
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    names = [f"P{i}" for i in range(S)]
    sky = rsky.SkyModel.from_arrays(names, ra, dec, 0.5 + rng.random(S),
                                    -rng.random(S), 140e6)
    clusters = rsky.ClusterSet([rsky.ClusterDef(1, 1, names[:130]),
                                rsky.ClusterDef(2, 1, names[130:])])
    _, beam, uvw = make_geometry(N, Ne, Tt, seed=6)
    if Ne == 1:
        beam = arr.StationBeam(np.zeros((Tt, N, 1, 3)))
    assert uvw.shape[0] == Tt * 276
    for smear in (None, 180e3):
        out = predict_gpu(sky, clusters, uvw, smear, beam)
        assert out.shape == (2, Tt * 276, 4)
        ref = beam_numpy_oracle(sky, clusters, uvw, FREQ, smear, beam)
        for k in range(2):
            err = rel_err(to_np(out[k]), ref[k])
            print(f"Ne={Ne} smear={smear} k={k}: vs numpy {err:.3e}")
            assert err < 1e-5, (smear, k, err)
        assert bool((out[:, :, 1:3] == 0).all())
        assert torch.equal(out[:, :, 0], out[:, :, 3])
        if Ne == 1:
            plain = predict_gpu(sky, clusters, uvw, smear)
            for k in range(2):
                d = float((out[k] - plain[k]).abs().max())
                assert d < 1e-6 * float(plain[k].abs().max()), (smear, k, d)


# 3. beamless prediction never launches the new kernels --------------------

def test_beamless_prediction_skips_the_beam_kernels(monkeypatch):
    from smartcal_amd.ops import ext
    sky, clusters = make_test_sky()
    _, _, uvw = make_geometry(5, 7, 3)
    before = [predict_gpu(sky, clusters, uvw, smear)
              for smear in (None, 180e3)]

    def boom(*a, **k):
        raise AssertionError("beam kernel launched without a beam")

    for name in BEAM_KERNELS:
        monkeypatch.setattr(ext(), name, boom, raising=False)
    kernel = ext().shapelet_predict
    monkeypatch.setattr(
        ext(), "shapelet_predict",
        lambda *a: (len(a) == 8 or boom(), kernel(*a))[1])
    for smear, ref in zip((None, 180e3), before):
        assert torch.equal(predict_gpu(sky, clusters, uvw, smear), ref)
        assert torch.equal(
            predict_coherencies_uvw(sky, clusters, uvw.cuda(), FREQ, RA0,
                                    DEC0, smear_bw=smear, beam=None), ref)


# 4. simulated observation -------------------------------------------------

def test_simulate_observation_beam_gpu_matches_cpu():
    sc = sim.make_calibration_sky(3, np.random.default_rng(7), diffuse=True,
                                  diffuse_beta=0.02)
    layout = arr.lofar_like_layout(8, np.random.default_rng(1))
    elem = arr.station_elements(8, 12, np.random.default_rng(4))
    freqs = np.linspace(140e6, 160e6, 2)
    vis = [sim.simulate_observation(layout, sc[0], sc[1], freqs, sc[6],
                                    sc[7], 1, 4, device=dev,
                                    rng=np.random.default_rng(2),
                                    torch_seed=0, beam_elements=elem)
           for dev in ("cpu", "cuda")]
    cpu, gpu = vis[0].model, vis[1].model.cpu()
    assert bool(torch.isfinite(torch.view_as_real(gpu)).all())
    err = float((gpu - cpu).abs().max() / cpu.abs().max())
    print(f"simulate_observation beam model gpu vs cpu: {err:.3e}")
    assert err < 1e-4, err
    assert np.array_equal(vis[0].J_true, vis[1].J_true)
