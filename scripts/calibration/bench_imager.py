"""Time the exact DFT imager: the kernel of ops/csrc/dft_image.hip vs the
eager torch path (`SMARTCAL_FORCE_EAGER=1`) of the same call, and vs the
nearest-cell gridder making the same number of maps.

Workload: 62 stations, 20 timeslots (S = 37 820 samples), F = 8 sub-bands,
M = 2 maps per band (what one `CalibEnv` step images as data + residual),
npix = 128, w-term on, natural weighting, fov=None. Each timed kernel or
eager call is the whole `dft_image_cube` (weight folding and upload of the
per-frequency table included); the gridder figure is the 16 `dirty_image`
calls that make the same maps. The launch alone, on arguments already
prepared, is timed as well. Device events, after warm-up, median of
``--repeats`` runs (``--eager-repeats`` for the eager path, which takes
seconds). Prints one JSON line.
"""

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from smartcal_amd.ops import ext
from smartcal_amd.radio import array as arr
from smartcal_amd.radio import imaging


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
    ap.add_argument("--nf", default=8, type=int)
    ap.add_argument("--maps", default=2, type=int)
    ap.add_argument("--npix", default=128, type=int)
    ap.add_argument("--warmup", default=3, type=int)
    ap.add_argument("--repeats", default=20, type=int)
    ap.add_argument("--eager-warmup", default=1, type=int)
    ap.add_argument("--eager-repeats", default=3, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    rng = np.random.default_rng(0)
    ra0, dec0 = 0.3, 0.9
    layout = arr.lofar_like_layout(args.stations, rng)
    times = np.arange(args.timeslots) * 10.0
    uvw_t = arr.uvw_synthesis(layout, ra0, dec0, times)
    uvw = torch.as_tensor(uvw_t.reshape(-1, 3), dtype=torch.float32,
                          device="cuda")
    S = int(uvw.shape[0])
    freqs = np.linspace(115e6, 185e6, args.nf)
    shape = (args.nf, args.maps, S)
    vals = torch.as_tensor(
        rng.standard_normal(shape) + 1j * rng.standard_normal(shape),
        dtype=torch.complex64, device="cuda")

    def cube(**kw):
        return imaging.dft_image_cube(uvw, vals, freqs, args.npix, **kw)

    def eager():
        os.environ["SMARTCAL_FORCE_EAGER"] = "1"
        try:
            return cube()
        finally:
            del os.environ["SMARTCAL_FORCE_EAGER"]

    def gridder():
        return [imaging.dirty_image(uvw, vals[fi, j], float(f), args.npix)
                for fi, f in enumerate(freqs) for j in range(args.maps)]

    I_k, I_e = cube(), eager()
    err = float((I_k - I_e).abs().max() / I_e.abs().max())
    assert torch.equal(I_k, cube()), "kernel result changed between runs"

    kern = timed(cube, args.warmup, args.repeats)
    eag = timed(eager, args.eager_warmup, args.eager_repeats)
    grid = timed(gridder, args.warmup, args.repeats)

    # the launch alone, per sample split (0 = the automatic choice)
    uvw64 = uvw.double().contiguous()
    umax = float(uvw64[:, :2].abs().max())
    scales = freqs / imaging.C_LIGHT
    cells = np.array([(args.npix // 2 - 1) / max(umax * sc, 1.0) / args.npix
                      for sc in scales])
    fpar = torch.as_tensor(np.stack([scales, cells], axis=1),
                           dtype=torch.float64, device="cuda")
    vals_n = (vals / S).contiguous()
    launch = {
        str(n): timed(lambda n=n: ext().dft_image(uvw64, vals_n, fpar,
                                                  args.npix, 0.0, 0.0, n),
                      args.warmup, args.repeats)
        for n in (0, 1, 2, 4, 8)}
    pairs = float(args.npix) ** 2 * S * args.nf
    print(json.dumps({
        "workload": {"stations": args.stations, "timeslots": args.timeslots,
                     "S": S, "F": args.nf, "M": args.maps,
                     "npix": args.npix, "wterm": True,
                     "pixel_sample_pairs": pairs},
        "repeats": args.repeats, "eager_repeats": args.eager_repeats,
        "dft_kernel_ms_median_min_max": kern,
        "dft_eager_ms_median_min_max": eag,
        "gridder_same_maps_ms_median_min_max": grid,
        "dft_launch_ms_median_min_max_by_nsplit": launch,
        "kernel_gpairs_per_s_median": pairs / (launch["0"][0] * 1e-3) / 1e9,
        "speedup_median_kernel_vs_eager": eag[0] / kern[0],
        "dft_cost_median_vs_gridder": kern[0] / grid[0],
        "kernel_vs_eager_rel_err": err,
    }))


if __name__ == "__main__":
    main()
