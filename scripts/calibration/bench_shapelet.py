"""Time shapelet prediction: shapelet_kernel vs the eager torch
composition (`SMARTCAL_FORCE_EAGER=1` path) of the same call.

Workload: three n0 = 19 shapelet sources in one cluster, T = 37 820
samples (62 stations, 20 timeslots), one frequency. Device events, after
warm-up, median of ``--repeats`` runs. Prints one JSON line.
"""

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from smartcal_amd.ops import ext
from smartcal_amd.radio import array as arr
from smartcal_amd.radio import coherency
from smartcal_amd.radio.shapelet import ShapeletModel
from smartcal_amd.radio.sky import ClusterDef, ClusterSet, SkyModel


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", default=62, type=int)
    ap.add_argument("--timeslots", default=20, type=int)
    ap.add_argument("--n0", default=19, type=int)
    ap.add_argument("--beta", default=0.01, type=float)
    ap.add_argument("--warmup", default=10, type=int)
    ap.add_argument("--repeats", default=100, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    rng = np.random.default_rng(0)
    ra0, dec0, freq, smear = 0.0, math.pi / 2.2, 150e6, 180e3
    layout = arr.lofar_like_layout(args.stations, rng)
    uvw_t = arr.uvw_synthesis(layout, ra0, dec0,
                              np.arange(args.timeslots) * 10.0)
    uvw = torch.as_tensor(uvw_t.reshape(-1, 3), dtype=torch.float32,
                          device="cuda")
    names = ["SLSI", "SLSQ", "SLSU"]
    shp = {nm: ShapeletModel(args.n0, args.beta,
                             rng.standard_normal(args.n0 ** 2), 1.0, 1.0,
                             math.pi / 2) for nm in names}
    sky = SkyModel.from_arrays(names, [ra0] * 3, [dec0] * 3, [250.0, 0, 0],
                               [-0.1] * 3, 150e6, sQ=[0, 250.0, 0],
                               sU=[0, 0, 250.0], shapelets=shp)
    clusters = ClusterSet([ClusterDef(1, 1, names)])

    # the shapelet step alone, on tables already built and uploaded
    tables = coherency._shapelet_tables(sky, clusters, ra0, dec0, freq)
    dev_tables = [torch.as_tensor(a, device="cuda") for a in tables]
    scale = 2.0 * math.pi / coherency.C_LIGHT * freq
    uvw_s = (uvw.double() * scale).contiguous()
    u, v, w = uvw_s[:, 0], uvw_s[:, 1], uvw_s[:, 2]
    fdelta = smear / freq
    C = torch.zeros((1, uvw.shape[0], 4), dtype=torch.complex64,
                    device="cuda")
    C_k, C_e = C.clone(), C.clone()
    ext().shapelet_predict(C_k, uvw_s, *dev_tables, fdelta)
    coherency._add_shapelets_torch(C_e, u, v, w, tables, fdelta)
    err = float((C_k - C_e).abs().max() / C_e.abs().max())

    kern = timed(lambda: ext().shapelet_predict(C, uvw_s, *dev_tables,
                                                fdelta),
                 args.warmup, args.repeats)
    C.zero_()
    eager = timed(lambda: coherency._add_shapelets_torch(C, u, v, w, tables,
                                                         fdelta),
                  args.warmup, args.repeats)
    print(json.dumps({
        "workload": {"stations": args.stations, "timeslots": args.timeslots,
                     "T": int(uvw.shape[0]), "sources": 3, "n0": args.n0,
                     "smear_bw": smear},
        "repeats": args.repeats,
        "kernel_ms_median_min_max": kern,
        "eager_ms_median_min_max": eager,
        "speedup_median": eager[0] / kern[0],
        "kernel_vs_eager_rel_err": err,
    }))


if __name__ == "__main__":
    main()
