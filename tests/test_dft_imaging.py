"""Exact direct-Fourier-sum imager (radio/imaging.py dft_image*): the torch
path against a float64 numpy oracle of the definition, the prediction
round trip with and without the w-term, agreement with the gridder where
the gridder is exact, uniform weighting, and the env / CLI wiring (CPU)."""

import math

import numpy as np
import pytest
import torch

from smartcal_amd.envs.calib import CalibEnv
from smartcal_amd.envs.demix import DemixingEnv
from smartcal_amd.envs.demix_fuzzy import FuzzyDemixingEnv
from smartcal_amd.radio import array as arr, imaging, sky as rsky
from smartcal_amd.radio.coherency import predict_coherencies_uvw
from smartcal_amd.radio.coords import radectolm
from smartcal_amd.radio.imaging import (C_LIGHT, dft_image, dft_image_cube,
                                        dft_psf, dirty_image)

from test_scripts import _run

FREQ = 150e6


# --------------------------------------------------------------------------
# shared scenario and oracle (also used by test_gpu_dft_imaging.py)
# --------------------------------------------------------------------------

def rel_err(out, ref):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(out - ref).max() / np.abs(ref).max())


def make_samples(S, M=None, F=None, seed=0, span=1500.0, dtype=torch.float32):
    """S samples within ±span m (w a tenth of that) and complex64 values of
    shape (S,), (M, S) or (F, M, S)."""
    rng = np.random.default_rng(seed)
    uvw = (rng.random((S, 3)) * 2 - 1) * [span, span, 0.1 * span]
    shape = tuple(n for n in (F, M) if n is not None) + (S,)
    vals = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return (torch.as_tensor(uvw, dtype=dtype),
            torch.as_tensor(vals, dtype=torch.complex64))


def auto_fov(uvw, freq, npix):
    """`dirty_image`'s fov=None rule, in float64."""
    uv = np.abs(np.asarray(uvw, np.float64)[:, :2])
    umax = uv.max() * freq / C_LIGHT if uv.size else 0.0
    return (npix // 2 - 1) / max(umax, 1.0)


def uniform_oracle(u, v, du, g):
    """g_s / count(cell_s) by a python loop over a dict of folded cells."""
    cells = []
    for us, vs in zip(u, v):
        iu, iv = int(np.round(us / du)), int(np.round(vs / du))
        if iu < 0 or (iu == 0 and iv < 0):
            iu, iv = -iu, -iv
        cells.append((iu, iv))
    count = {}
    for c, gs in zip(cells, g):
        if gs != 0:
            count[c] = count.get(c, 0) + 1
    return np.array([gs / count[c] if gs != 0 else 0.0
                     for c, gs in zip(cells, g)])


def dft_oracle(uvw, values, freq, npix, fov=None, center=(0.0, 0.0),
               wterm=True, weighting="natural", weights=None):
    """Float64 numpy evaluation of the definition, one map (S,) or (M, S)
    at one frequency → (npix, npix) or (M, npix, npix)."""
    if fov is None:
        fov = auto_fov(uvw, freq, npix)
    uvw = np.asarray(uvw, np.float64) * (freq / C_LIGHT)
    V = np.asarray(values, np.complex128)
    single = V.ndim == 1
    V = np.atleast_2d(V)
    S = uvw.shape[0]
    cell = fov / npix
    g = np.ones(S) if weights is None else np.asarray(weights, np.float64)
    if weighting == "uniform":
        g = uniform_oracle(uvw[:, 0], uvw[:, 1], 1.0 / fov, g)
    ax = (np.arange(npix) - npix // 2) * cell
    l = center[0] + ax[None, :]                        # [y, x]
    m = center[1] + ax[:, None]
    r2 = l * l + m * m
    sky = r2 <= 1.0
    n = np.sqrt(np.where(sky, 1.0 - r2, 0.0))
    out = np.zeros((V.shape[0], npix, npix))
    for s in range(S):
        ph = uvw[s, 0] * l + uvw[s, 1] * m
        if wterm:
            ph = ph + uvw[s, 2] * (n - 1.0)
        e = np.exp(-2j * np.pi * ph)
        for j in range(V.shape[0]):
            out[j] += g[s] * (V[j, s] * e).real
    out = out / g.sum() * sky
    return out[0] if single else out


def round_trip_scene():
    """8 LOFAR-like stations, 4 snapshots 600 s apart, 150 MHz, one 2.5 Jy
    source at (0.36, 0.85) against phase centre (0.3, 0.9) → (uvw f64,
    predicted Stokes-I visibilities, (l, m) of the source)."""
    ra0, dec0 = 0.3, 0.9
    layout = arr.lofar_like_layout(8, np.random.default_rng(0))
    uvw = arr.uvw_synthesis(layout, ra0, dec0,
                            np.arange(4) * 600.0).reshape(-1, 3)
    uvw = torch.as_tensor(uvw, dtype=torch.float64)
    sky = rsky.SkyModel.from_arrays(["A"], np.array([0.36]),
                                    np.array([0.85]), np.array([2.5]),
                                    np.zeros(1), FREQ)
    cs = rsky.ClusterSet([rsky.ClusterDef(1, 1, ["A"])])
    C = predict_coherencies_uvw(sky, cs, uvw, FREQ, ra0, dec0)
    l, m, _ = radectolm(0.36, 0.85, ra0, dec0)
    return uvw, 0.5 * (C[0][:, 0] + C[0][:, 3]), (float(l), float(m))


# --------------------------------------------------------------------------
# 1. torch path vs oracle
# --------------------------------------------------------------------------

NPIX, S0 = 24, 300

CASES = {
    "natural": dict(),
    # span: ±30 wavelengths over cells of 3.3, so most cells are shared
    "uniform": dict(weighting="uniform", fov=0.3, span=60.0),
    "weights": dict(weights="zeros"),
    "uniform_weights": dict(weighting="uniform", weights="zeros", fov=0.3,
                            span=60.0),
    "no_wterm": dict(wterm=False),
    "shifted": dict(center=(0.12, -0.2), fov=0.2),
    "auto_fov": dict(fov=None),
}


def _weights(S, seed=3):
    rng = np.random.default_rng(seed)
    w = rng.random(S) + 0.5
    w[rng.random(S) < 0.2] = 0.0
    return torch.as_tensor(w, dtype=torch.float32)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_path_matches_oracle(case, M):
    kw = dict(fov=0.25)
    kw.update(CASES[case])
    if isinstance(kw.get("weights"), str):
        kw["weights"] = _weights(S0)
    uvw, vals = make_samples(S0, M=M, seed=1, span=kw.pop("span", 1500.0))
    if kw.get("weighting") == "uniform":
        nat = dict(kw, weighting="natural")
        assert rel_err(dft_oracle(uvw, vals, FREQ, NPIX, **nat),
                       dft_oracle(uvw, vals, FREQ, NPIX, **kw)) > 1e-2
    out = dft_image(uvw, vals, FREQ, NPIX, **kw)
    assert out.shape == (M, NPIX, NPIX) and out.dtype == torch.float32
    ref = dft_oracle(uvw, vals, FREQ, NPIX, **kw)
    err = rel_err(out, ref)
    print(f"{case} M={M}: vs oracle {err:.3e}")
    assert err < 1e-6, err
    # a single map is the first map of the stack
    one = dft_image(uvw, vals[0], FREQ, NPIX, **kw)
    assert one.shape == (NPIX, NPIX)
    assert torch.equal(one, out[0])


def test_cube_matches_oracle_per_frequency():
    freqs = np.array([120e6, 150e6, 180e6])
    uvw, vals = make_samples(S0, M=2, F=3, seed=2)
    cube = dft_image_cube(uvw, vals, freqs, NPIX)          # fov=None
    assert cube.shape == (3, 2, NPIX, NPIX)
    assert cube.dtype == torch.float32
    fovs = [auto_fov(uvw, f, NPIX) for f in freqs]
    assert fovs[0] > fovs[1] > fovs[2]                     # axes differ
    for fi, f in enumerate(freqs):
        ref = dft_oracle(uvw, vals[fi], f, NPIX, fov=fovs[fi])
        err = rel_err(cube[fi], ref)
        print(f"cube f={f:.3g}: vs oracle {err:.3e}")
        assert err < 1e-6, err
        # the field is the gridder's: same cell as dirty_image's rule
        assert torch.equal(cube[fi], dft_image(uvw, vals[fi], f, NPIX))


def test_off_sky_pixels_are_zero_and_psf_peaks_at_one():
    uvw, _ = make_samples(50, seed=4)
    psf = dft_psf(uvw, FREQ, NPIX, fov=2.5)
    ax = (np.arange(NPIX) - NPIX // 2) * (2.5 / NPIX)
    off = (ax[None, :] ** 2 + ax[:, None] ** 2) > 1.0
    assert off.any() and (~off).any()
    assert bool((psf.numpy()[off] == 0).all())
    assert abs(float(psf[NPIX // 2, NPIX // 2]) - 1.0) < 1e-6
    assert float(psf.max()) <= 1.0 + 1e-6
    assert rel_err(psf, dft_oracle(uvw, np.ones(50), FREQ, NPIX,
                                   fov=2.5)) < 1e-6


def test_argument_checks():
    uvw, vals = make_samples(10, M=2, F=2)
    with pytest.raises(ValueError):
        dft_image_cube(uvw, vals, [FREQ], NPIX)
    with pytest.raises(ValueError):
        dft_image(uvw, vals[0], FREQ, NPIX, weighting="briggs")
    with pytest.raises(ValueError):
        dft_image(uvw, vals[0], FREQ, NPIX, weights=torch.ones(9))


# --------------------------------------------------------------------------
# 2. prediction round trip
# --------------------------------------------------------------------------

def test_prediction_round_trip_needs_the_wterm():
    uvw, V, (l, m) = round_trip_scene()
    img = dft_image(uvw, V, FREQ, NPIX, 0.02, center=(l, m))
    c = NPIX // 2
    peak = float(img[c, c])
    print(f"round trip: centre {peak:.6f}, max {float(img.max()):.6f}")
    assert abs(peak - 2.5) < 1e-5 * 2.5
    assert float(img.max()) == peak
    flat = dft_image(uvw, V, FREQ, NPIX, 0.02, center=(l, m), wterm=False)
    print(f"without the w-term: centre {float(flat[c, c]):.4f}")
    assert float(flat[c, c]) < 0.5 * 2.5


# --------------------------------------------------------------------------
# 3. agreement with the gridder where the gridder is exact
# --------------------------------------------------------------------------

def test_matches_gridder_on_grid_points():
    npix, fov, S = 32, 0.1, 300
    rng = np.random.default_rng(5)
    du_m = (1.0 / fov) * C_LIGHT / FREQ            # one uv cell in meters
    cells = rng.integers(-(npix // 2 - 1), npix // 2, (S, 2))
    uvw = torch.as_tensor(
        np.concatenate([cells * du_m, np.zeros((S, 1))], axis=1),
        dtype=torch.float64)
    _, V = make_samples(S, seed=6)
    grid = dirty_image(uvw, V, FREQ, npix, fov)
    dft = dft_image(uvw, V.conj(), FREQ, npix, fov, wterm=False)
    err = rel_err(grid, dft)
    print(f"gridder vs dft on grid points: {err:.3e}")
    assert err < 1e-5, err


# --------------------------------------------------------------------------
# 4. uniform weighting
# --------------------------------------------------------------------------

def _cells_to_uvw(cells, fov):
    du_m = (1.0 / fov) * C_LIGHT / FREQ
    cells = np.asarray(cells, np.float64)
    return torch.as_tensor(
        np.concatenate([cells * du_m, np.zeros((len(cells), 1))], axis=1),
        dtype=torch.float64)


def test_uniform_counts_fold_conjugates_and_skip_flagged():
    fov = 0.1
    # rows 0, 1: r and −r; rows 2, 3, 4: one cell, row 4 flagged; row 5
    # alone; rows 6, 7: (0, 3) and (0, −3)
    cells = [(4, -7), (-4, 7), (2, 2), (2, 2), (2, 2), (-9, 1), (0, 3),
             (0, -3)]
    uvw = _cells_to_uvw(cells, fov)
    # inside the cell, not on its centre
    uvw[:, :2] += 0.2 * (1.0 / fov) * C_LIGHT / FREQ * torch.tensor(
        [[1, -1], [-1, 1], [1, 1], [-1, 1], [0, 0], [1, 0], [0, 1], [0, -1]])
    w = torch.tensor([1.0, 2.0, 3.0, 1.0, 0.0, 5.0, 1.0, 1.0])
    scale = FREQ / C_LIGHT
    g = imaging._uniform_weights(uvw[:, 0] * scale, uvw[:, 1] * scale,
                                 1.0 / fov, w.double())
    expect = [0.5, 1.0, 1.5, 0.5, 0.0, 5.0, 0.5, 0.5]
    assert np.allclose(g.numpy(), expect, rtol=0, atol=1e-15)
    assert np.allclose(uniform_oracle((uvw[:, 0] * scale).numpy(),
                                      (uvw[:, 1] * scale).numpy(),
                                      1.0 / fov, w.numpy()), expect)
    # … and the image is the natural one with those weights
    _, V = make_samples(8, seed=7)
    uni = dft_image(uvw, V, FREQ, NPIX, fov, weighting="uniform", weights=w)
    nat = dft_image(uvw, V, FREQ, NPIX, fov, weights=g)
    assert rel_err(uni, nat) < 1e-6
    assert rel_err(uni, dft_oracle(uvw, V, FREQ, NPIX, fov,
                                   weighting="uniform", weights=w)) < 1e-6
    assert rel_err(uni, dft_image(uvw, V, FREQ, NPIX, fov, weights=w)) > 1e-2


def test_uniform_equals_natural_when_cells_are_distinct():
    fov = 0.1
    cells = [(i, 2 * i - 7) for i in range(1, 12)]
    uvw = _cells_to_uvw(cells, fov)
    _, V = make_samples(len(cells), M=2, seed=8)
    w = _weights(len(cells), seed=9)
    for weights in (None, w):
        uni = dft_image(uvw, V, FREQ, NPIX, fov, weighting="uniform",
                        weights=weights)
        nat = dft_image(uvw, V, FREQ, NPIX, fov, weights=weights)
        assert torch.equal(uni, nat)


# --------------------------------------------------------------------------
# 5. envs and CLI
# --------------------------------------------------------------------------

def _boom(*a, **k):
    raise AssertionError("dft imager called with imager='grid'")


CALIB_KW = dict(M=3, N_stations=6, Nf=2, Ts=1, Tdelta=4, Ninf=16,
                admm_iter=2, poly_order=2, device="cpu", inf_nfreq=1, seed=0)
DEMIX_KW = dict(K=3, Nf=2, Ninf=16, Tdelta=4, Ts=1, provide_influence=True,
                N_stations=6, device="cpu")


def test_calib_env_dft_imager(monkeypatch):
    env = CalibEnv(imager="dft", **CALIB_KW)
    obs = env.reset()
    assert obs["img"].shape == (1, 16, 16) and obs["sky"].shape == (4, 7)
    assert np.isfinite(obs["img"]).all() and np.isfinite(obs["sky"]).all()
    obs2, reward, done, _ = env.step(np.zeros(6, np.float32))
    assert obs2["img"].shape == (1, 16, 16)
    assert np.isfinite(obs2["img"]).all() and math.isfinite(reward)
    assert np.abs(obs2["img"]).max() > 0
    # the default imager is the gridder, same draws, other map
    grid = CalibEnv(**CALIB_KW)
    assert grid.imager == "grid"
    for name in ("dft_image", "dft_image_cube", "dft_psf"):
        monkeypatch.setattr(imaging, name, _boom)
    first = grid.reset()
    assert np.array_equal(first["sky"], obs["sky"])
    assert not np.array_equal(first["img"], obs["img"])
    grid.step(np.zeros(6, np.float32))
    with pytest.raises(ValueError):
        CalibEnv(imager="excon", **CALIB_KW)


def test_calib_env_dft_imager_options():
    narrow = CalibEnv(imager="dft", image_fov=0.05, image_wterm=False,
                      **CALIB_KW).reset()
    auto = CalibEnv(imager="dft", **CALIB_KW).reset()
    assert np.isfinite(narrow["img"]).all()
    assert not np.array_equal(narrow["img"], auto["img"])


@pytest.mark.parametrize("cls", [DemixingEnv, FuzzyDemixingEnv])
def test_demixing_envs_dft_imager(cls, monkeypatch):
    env = cls(imager="dft", seed=2, **DEMIX_KW)
    obs = env.reset()
    assert obs["infmap"].shape[-2:] == (16, 16)
    assert np.isfinite(obs["infmap"]).all()
    assert np.isfinite(obs["metadata"]).all()
    out = env.step(np.zeros(env.action_space.shape, np.float32))
    assert out[0]["infmap"].shape[-2:] == (16, 16)
    assert np.isfinite(out[0]["infmap"]).all()
    assert np.abs(out[0]["infmap"]).max() > 0
    grid = cls(seed=2, **DEMIX_KW)
    assert grid.imager == "grid"
    for name in ("dft_image", "dft_image_cube", "dft_psf"):
        monkeypatch.setattr(imaging, name, _boom)
    first = grid.reset()
    assert np.array_equal(first["metadata"], obs["metadata"])
    grid.step(np.zeros(grid.action_space.shape, np.float32))


def test_bench_imager_help(tmp_path):
    r = _run("scripts/calibration/bench_imager.py", "--help", cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]


def test_calibration_pipeline_dft_tiny(tmp_path):
    r = _run("scripts/calibration/pipeline.py", "--K", "2", "--stations",
             "8", "--nf", "2", "--ts", "1", "--tdelta", "4", "--admm", "2",
             "--poly", "2", "--imager", "dft", cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("data_img.npy", "res_img.npy", "influenceI.npy"):
        img = np.load(tmp_path / name)
        assert img.shape == (128, 128) and np.isfinite(img).all()
