"""Record tests/golden/sky_predict_golden.npz: the outputs of the
sky-prediction kernels (coherency, station beam, shapelet) for one fixed
seeded scenario.

Run on the GPU from a checkout whose kernels are trusted (the commit before
a change to them); tests/test_gpu_sky_golden.py then demands that the
current kernels reproduce every recorded output bit for bit. The fixture
holds a SHA-256 of the input bytes (source table, offsets, the five
shapelet tables, the scaled uvw), so a change of the table build cannot go
unnoticed, a SHA-256 of every output and of the station-beam table E, and
the output arrays themselves so that a failure can be sized.

Scenario (library calls only):
  cluster 1: 130 point / Gaussian sources — crosses the 128-row LDS chunk;
             every third one is a Gaussian, row 129 included;
  cluster 2: two point sources and two shapelets, n0 = 4 and 7;
  cluster 3: one shapelet with sI = 0, sQ ≠ 0 — its point table is empty;
  24 stations (B = 276 = one 256-lane tile + 20), 2 timeslots (T = 552),
  7 elements per station.
Cases: beam ∈ {none, beam} × smearing ∈ {off, 180 kHz}.

    python scripts/record_sky_golden.py [--root CHECKOUT] [--out FILE]
"""

import argparse
import hashlib
import math
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent.parent

SEED = 20240911
RA0, DEC0 = 0.3, 0.9
FREQ = 150e6
N_STATIONS, N_TIME, N_ELEM = 24, 2, 7
CASES = [("plain", False, None), ("plain_smear", False, 180e3),
         ("beam", True, None), ("beam_smear", True, 180e3)]
MAX_BYTES = 160_000       # above this, only the smear-on arrays are kept


def make_scenario():
    """→ (sky, clusters, beam, uvw (T, 3) f64 CPU tensor)."""
    from smartcal_amd.radio import array as arr, sky as rsky
    from smartcal_amd.radio.coords import lmtoradec
    from smartcal_amd.radio.shapelet import ShapeletModel

    rng = np.random.default_rng(SEED)
    n1 = 130
    names = [f"G{i}" if i % 3 == 0 else f"P{i}" for i in range(n1)]
    names += ["Q0", "Q1", "SA1", "SA2", "SB1"]
    S = len(names)
    l = (rng.random(S) * 2 - 1) * 0.03
    m = (rng.random(S) * 2 - 1) * 0.03
    ra, dec = lmtoradec(l, m, RA0, DEC0)
    gauss = np.asarray([nm.startswith("G") for nm in names])
    sI = 0.5 + rng.random(S)
    sI[n1 + 2:] = [100.0, 50.0, 0.0]
    sQ, sU = np.zeros(S), np.zeros(S)
    sQ[n1 + 2:] = [25.0, -20.0, 75.0]
    sU[n1 + 2:] = [15.0, 10.0, 35.0]
    sP = np.zeros((S, 3))
    sP[:, 0] = -rng.random(S)
    sP[:, 1] = 0.1 * rng.random(S)
    eX = np.where(gauss, 0.001 + 0.002 * rng.random(S), 0.0)
    eY = np.where(gauss, 0.0005 + 0.001 * rng.random(S), 0.0)
    eP = np.where(gauss, rng.random(S) * math.pi, 0.0)
    beta = 0.01
    shp = {
        "SA1": ShapeletModel(4, beta, rng.standard_normal(16)),
        "SA2": ShapeletModel(7, 0.8 * beta, rng.standard_normal(49),
                             1.2, 0.8, 0.3),
        "SB1": ShapeletModel(5, beta, rng.standard_normal(25), 1.3, 0.7, 0.4),
    }
    sky = rsky.SkyModel.from_arrays(names, ra, dec, sI, sP, 140e6, eX, eY, eP,
                                    sQ=sQ, sU=sU, shapelets=shp)
    clusters = rsky.ClusterSet([
        rsky.ClusterDef(1, 1, names[:n1]),
        rsky.ClusterDef(2, 1, names[n1:n1 + 4]),
        rsky.ClusterDef(3, 1, ["SB1"])])

    enu = (rng.random((N_STATIONS, 3)) * 2 - 1) * [150.0, 150.0, 2.0]
    layout = arr.StationLayout(enu)
    elem = arr.station_elements(N_STATIONS, N_ELEM, rng)
    times = np.arange(N_TIME) * 3600.0
    beam = arr.station_beam(layout, elem, RA0, DEC0, times)
    uvw = arr.uvw_synthesis(layout, RA0, DEC0, times).reshape(-1, 3)
    return sky, clusters, beam, torch.as_tensor(uvw, dtype=torch.float64)


def kernel_inputs(sky, clusters, uvw, dev):
    """The tables that `predict_coherencies_uvw` hands to the kernels →
    (src, off, the five shapelet tables, uvw_scaled), as CPU numpy."""
    from smartcal_amd.radio import coherency

    src, off = coherency._source_table(sky, clusters, dev, FREQ, RA0, DEC0)
    shp = coherency._shapelet_tables(sky, clusters, RA0, DEC0, FREQ)
    scale = 2.0 * math.pi / coherency.C_LIGHT * FREQ
    uvw = uvw.to(dev)
    uvw_scaled = torch.stack([uvw[:, i].double() * scale for i in range(3)],
                             dim=1).contiguous()
    return (src.cpu().numpy(), off.cpu().numpy(), *shp,
            uvw_scaled.cpu().numpy())


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def beam_table(ext, beam, inputs, dev):
    """E (Tt, Sall, N) complex128 of station_beam for the point/Gaussian
    rows followed by the shapelet centres, as the beam prediction builds
    it."""
    from smartcal_amd.radio import coherency

    src, hdr = inputs[0], inputs[2]
    lmn = torch.as_tensor(np.concatenate((src[:, 0:3], hdr[:, 0:3])),
                          device=dev).contiguous()
    elem = torch.as_tensor(beam.elem_uvw, dtype=torch.float64,
                           device=dev).contiguous()
    return ext.station_beam(elem, lmn,
                            2.0 * math.pi / coherency.C_LIGHT * FREQ)


def run_case(sky, clusters, beam, uvw, dev, with_beam, smear_bw):
    from smartcal_amd.radio.coherency import predict_coherencies_uvw

    kw = {"beam": beam} if with_beam else {}
    return predict_coherencies_uvw(sky, clusters, uvw.to(dev), FREQ, RA0,
                                   DEC0, smear_bw=smear_bw, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE),
                    help="checkout whose built extension records the golden")
    ap.add_argument("--out", default=str(HERE / "tests" / "golden"
                                         / "sky_predict_golden.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import smartcal_amd.ops as ops
    dev = torch.device("cuda:0")
    sky, clusters, beam, uvw = make_scenario()
    inputs = kernel_inputs(sky, clusters, uvw, dev)
    out = {"inputs/sha256": np.array(digest(*inputs))}
    E = beam_table(ops.ext(), beam, inputs, dev)
    out["E/sha256"] = np.array(digest(E.cpu().numpy()))
    arrays = {}
    for name, with_beam, smear_bw in CASES:
        C = run_case(sky, clusters, beam, uvw, dev, with_beam,
                     smear_bw).cpu().numpy()
        out[f"{name}/sha256"] = np.array(digest(C))
        arrays[f"{name}/C"] = C
    np.savez_compressed(a.out, **out, **arrays)
    if Path(a.out).stat().st_size > MAX_BYTES:
        np.savez_compressed(a.out, **out, **{
            k: v for k, v in arrays.items() if k.endswith("_smear/C")})
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes from",
          Path(ops.__file__).resolve().parent)


if __name__ == "__main__":
    main()
