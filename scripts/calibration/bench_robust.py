"""Time the robust update and the weighted sweep of the calibration solver.

Workload: N = 62 stations, Nf = 8 sub-bands, Ts = 2 intervals of
Tdelta = 10 timeslots (F T B = 302 560 samples), K = 4 directions, random
coherencies, data and Jones.

* one robust update (`solver._residual_weights`: residual, e², weights and
  the four sums per frequency): the kernel of ops/csrc/robust.hip plus
  `torch.sum` over its per-block partials, against the eager torch path
  (`solver._residual_weights_torch`) of the same update;
* one weighted sweep's contributions (`als_sweep_w`) against the
  unweighted ones (`als_sweep`).

Device events, after warm-up, median of ``--repeats`` runs. Prints one
JSON line and, with ``--out``, writes it to that file.
"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from smartcal_amd.ops import ext
from smartcal_amd.radio import solver
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
    ap.add_argument("--nf", default=8, type=int)
    ap.add_argument("--ts", default=2, type=int)
    ap.add_argument("--tdelta", default=10, type=int)
    ap.add_argument("--K", default=4, type=int)
    ap.add_argument("--warmup", default=3, type=int)
    ap.add_argument("--repeats", default=20, type=int)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")

    F, K, N, Ts = args.nf, args.K, args.stations, args.ts
    T, B = args.ts * args.tdelta, N * (N - 1) // 2
    g = torch.Generator(device=dev)
    g.manual_seed(0)

    def crandn(*shape):
        return torch.view_as_complex(
            torch.randn(*shape, 2, generator=g, device=dev))

    C22 = crandn(F, K, T, B, 2, 2)
    V22 = crandn(F, T, B, 2, 2)
    J = 0.4 * crandn(F, Ts, K, N, 2, 2)
    J[..., 0, 0] += 1.0
    J[..., 1, 1] += 1.0
    m = (torch.rand(F, T, B, generator=g, device=dev) > 0.05).float()
    nu = torch.full((F,), 2.0, device=dev)
    sigma2 = torch.full((F,), 3.0 * K, device=dev)
    p, q = baseline_pq(N, dev)
    t_int = torch.arange(T, device=dev) // args.tdelta
    p32, q32, t32 = (t.to(torch.int32).contiguous() for t in (p, q, t_int))

    def update_kernel():
        return solver._residual_weights(C22, V22, J, m, nu, sigma2, p, q,
                                        t_int)

    def update_eager():
        return solver._residual_weights_torch(C22, V22, J, m, nu, sigma2, p,
                                              q, t_int)

    def launch_only():
        return ext().vis_residual_weights(C22, V22, J, m, nu, sigma2, p32,
                                          q32, t32)

    def sweep_w():
        return ext().als_sweep_w(C22, V22, J, m, p32, q32, t32)

    def sweep():
        return ext().als_sweep(C22, V22, J, p32, q32, t32)

    rk, re_ = update_kernel(), update_eager()
    err_w = float((rk[2] - re_[2]).abs().max() / re_[2].abs().max())
    err_s = float(((rk[3] - re_[3]) / re_[3]).abs().max())
    assert torch.equal(rk[3], update_kernel()[3]), "sums changed between runs"

    res = {
        "workload": {"stations": N, "F": F, "Ts": Ts, "Tdelta": args.tdelta,
                     "K": K, "samples": F * T * B},
        "repeats": args.repeats,
        "robust_update_kernel_ms_median_min_max":
            timed(update_kernel, args.warmup, args.repeats),
        "robust_update_launch_only_ms_median_min_max":
            timed(launch_only, args.warmup, args.repeats),
        "robust_update_eager_ms_median_min_max":
            timed(update_eager, args.warmup, args.repeats),
        "als_sweep_w_ms_median_min_max":
            timed(sweep_w, args.warmup, args.repeats),
        "als_sweep_ms_median_min_max":
            timed(sweep, args.warmup, args.repeats),
        "kernel_vs_eager_w_rel_err": err_w,
        "kernel_vs_eager_sums_rel_err": err_s,
    }
    res["speedup_median_update_kernel_vs_eager"] = \
        res["robust_update_eager_ms_median_min_max"][0] \
        / res["robust_update_kernel_ms_median_min_max"][0]
    res["cost_median_weighted_vs_unweighted_sweep"] = \
        res["als_sweep_w_ms_median_min_max"][0] \
        / res["als_sweep_ms_median_min_max"][0]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
