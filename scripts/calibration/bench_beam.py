"""Time station-beam prediction: the kernels of ops/csrc/beam.hip vs the
eager torch composition (`SMARTCAL_FORCE_EAGER=1` path) of the same call,
and vs the beamless kernel prediction.

Workload: the `make_calibration_sky(4, …)` simulation sky (4 directions +
weak background, point sources), 62 stations of 48 elements, 20 timeslots
(T = 37 820 samples), one frequency. Each timed call is the whole
`predict_coherencies_uvw` (table building included). Device events, after
warm-up, median of ``--repeats`` runs. The launches alone, on tables
already built and uploaded, are timed as well. Prints one JSON line.
"""

import argparse
import json
import math
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from smartcal_amd.ops import ext
from smartcal_amd.radio import array as arr
from smartcal_amd.radio import coherency, sim
from smartcal_amd.radio.coherency import predict_coherencies_uvw
from smartcal_amd.radio.hessian import baseline_pq


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
    ap.add_argument("--elements", default=48, type=int)
    ap.add_argument("--K", default=4, type=int)
    ap.add_argument("--warmup", default=5, type=int)
    ap.add_argument("--repeats", default=30, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    rng = np.random.default_rng(0)
    freq, smear = 150e6, 180e3
    sky, cs_sim, _, _, _, _, ra0, dec0 = sim.make_calibration_sky(args.K, rng)
    layout = arr.lofar_like_layout(args.stations, rng)
    times = np.arange(args.timeslots) * 10.0
    uvw_t = arr.uvw_synthesis(layout, ra0, dec0, times)
    uvw = torch.as_tensor(uvw_t.reshape(-1, 3), dtype=torch.float32,
                          device="cuda")
    beam = arr.station_beam(
        layout, arr.station_elements(args.stations, args.elements, rng),
        ra0, dec0, times)

    def predict(**kw):
        return predict_coherencies_uvw(sky, cs_sim, uvw, freq, ra0, dec0,
                                       smear_bw=smear, **kw)

    def eager():
        os.environ["SMARTCAL_FORCE_EAGER"] = "1"
        try:
            return predict(beam=beam)
        finally:
            del os.environ["SMARTCAL_FORCE_EAGER"]

    C_k, C_e, C_0 = predict(beam=beam), eager(), predict()
    err = float(((C_k - C_e).abs().amax(dim=(1, 2))
                 / C_e.abs().amax(dim=(1, 2))).max())
    share = float((C_k - C_0).abs().max() / C_0.abs().max())

    kern = timed(lambda: predict(beam=beam), args.warmup, args.repeats)
    eag = timed(eager, args.warmup, args.repeats)
    plain = timed(predict, args.warmup, args.repeats)

    # the launches alone
    scale = 2.0 * math.pi / coherency.C_LIGHT * freq
    uvw_s = (uvw.double() * scale).contiguous()
    src, off = coherency._source_table(sky, cs_sim, uvw.device, freq, ra0,
                                       dec0)
    lmn = src[:, 0:3].contiguous()
    elem = torch.as_tensor(beam.elem_uvw, device="cuda")
    p_idx, q_idx = (i.to(torch.int32)
                    for i in baseline_pq(args.stations, uvw.device))
    fdelta = smear / freq
    E = ext().station_beam(elem, lmn, scale)
    k_table = timed(lambda: ext().station_beam(elem, lmn, scale),
                    args.warmup, args.repeats)
    k_beam = timed(lambda: ext().coherency_beam_predict(
        uvw_s, src, off, fdelta, E, p_idx, q_idx), args.warmup, args.repeats)
    k_plain = timed(lambda: ext().coherency_predict(uvw_s, src, off, fdelta),
                    args.warmup, args.repeats)
    print(json.dumps({
        "workload": {"stations": args.stations, "timeslots": args.timeslots,
                     "elements": args.elements, "T": int(uvw.shape[0]),
                     "clusters": len(cs_sim), "sources": len(sky),
                     "smear_bw": smear},
        "repeats": args.repeats,
        "beam_kernel_ms_median_min_max": kern,
        "beam_eager_ms_median_min_max": eag,
        "beamless_kernel_ms_median_min_max": plain,
        "station_beam_launch_ms_median_min_max": k_table,
        "coherency_beam_launch_ms_median_min_max": k_beam,
        "coherency_launch_ms_median_min_max": k_plain,
        "speedup_median_kernel_vs_eager": eag[0] / kern[0],
        "beam_cost_median_vs_beamless": kern[0] / plain[0],
        "kernel_vs_eager_rel_err_per_cluster_max": err,
        "beam_vs_beamless_rel_diff": share,
    }))


if __name__ == "__main__":
    main()
