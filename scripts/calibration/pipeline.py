"""End-to-end calibration pipeline CLI — the in-process equivalent of
the reference shell pipeline `doall.sh` = `dosimul.sh` → `docal.sh` →
`doinfluence.sh` → `calmean.sh` (simulate → consensus-ADMM calibrate →
influence map → mean images), with no MS files or subprocesses.
"""

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from smartcal_amd.radio import array as arr
from smartcal_amd.radio import sim, solver, influence, imaging
from smartcal_amd.radio.coherency import predict_coherencies_uvw
from smartcal_amd.radio import io as rio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", default=4, type=int, help="directions")
    ap.add_argument("--stations", default=62, type=int)
    ap.add_argument("--nf", default=8, type=int, help="sub-bands")
    ap.add_argument("--ts", default=2, type=int)
    ap.add_argument("--tdelta", default=10, type=int)
    ap.add_argument("--admm", default=10, type=int, help="-A iterations")
    ap.add_argument("--poly", default=3, type=int, help="-P order")
    ap.add_argument("--rho", default=10.0, type=float)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--save-vis", action="store_true")
    ap.add_argument("--diffuse", action="store_true",
                    help="add the shapelet diffuse sky (Stokes I, Q, U) "
                         "to the simulated data")
    ap.add_argument("--diffuse-flux", default=250.0, type=float)
    ap.add_argument("--diffuse-beta", default=None, type=float,
                    help="shapelet scale in rad (default: the model's own)")
    ap.add_argument("--beam", action="store_true",
                    help="simulate through the station array-factor beam "
                         "(calibration stays beamless)")
    ap.add_argument("--beam-elements", default=48, type=int,
                    help="elements per station")
    ap.add_argument("--imager", default="grid", choices=["grid", "dft"],
                    help="grid: nearest-cell gridder + FFT; dft: exact "
                         "direct Fourier sum with the w-term")
    ap.add_argument("--robust", action="store_true",
                    help="robust (Student's-t) noise model in calibration")
    ap.add_argument("--nulow", default=2.0, type=float,
                    help="lower bound of the robust nu (sagecal -L)")
    ap.add_argument("--nuhigh", default=30.0, type=float,
                    help="upper bound of the robust nu (sagecal -H)")
    ap.add_argument("--uvmin", default=None, type=float,
                    help="lower uv cut in wavelengths (sagecal -x)")
    ap.add_argument("--uvmax", default=None, type=float,
                    help="upper uv cut in wavelengths (sagecal -y)")
    ap.add_argument("--rfi", default=0.0, type=float,
                    help="fraction of samples given unflagged outliers of "
                         "50 x the data RMS")
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    out = Path(args.outdir)

    t0 = time.time()
    sky, cs_sim, sky_cal, cs_cal, skylmn, rho0, ra0, dec0 = \
        sim.make_calibration_sky(args.K, rng, diffuse=args.diffuse,
                                 diffuse_flux=args.diffuse_flux,
                                 diffuse_beta=args.diffuse_beta)
    layout = arr.lofar_like_layout(args.stations, rng)
    freqs = np.linspace(115e6, 185e6, args.nf)
    elements = None
    if args.beam:
        # a generator of its own: rng draws what it draws without --beam
        elements = arr.station_elements(
            args.stations, args.beam_elements,
            np.random.default_rng([args.seed, 0xBEA3]))
    vis = sim.simulate_observation(layout, sky, cs_sim, freqs, ra0, dec0,
                                   args.ts, args.tdelta, snr=5.0,
                                   device=device, rng=rng,
                                   torch_seed=args.seed,
                                   beam_elements=elements)
    if args.rfi > 0:
        # a generator of its own, as for --beam
        gen = torch.Generator(device=device)
        gen.manual_seed(int(np.random.default_rng(
            [args.seed, 0x0F1]).integers(2 ** 31)))
        vis, rfi_mask = sim.add_outliers(vis, args.rfi, 50.0, gen)
        print(f"[rfi] {int(rfi_mask.sum())} of {rfi_mask.numel()} samples "
              f"corrupted")
    print(f"[simulate] {args.stations} stations, {args.nf} sub-bands, "
          f"{vis.S} samples/band: {time.time() - t0:.2f} s")
    if args.save_vis:
        rio.save_visdata(vis, str(out / "vis.npz"))

    t0 = time.time()
    rho = np.full(args.K, args.rho, np.float32)
    wopts = {}
    if args.robust:
        wopts.update(robust=True, nulow=args.nulow, nuhigh=args.nuhigh)
    if args.uvmin is not None:
        wopts["uvmin"] = args.uvmin
    if args.uvmax is not None:
        wopts["uvmax"] = args.uvmax
    sol = solver.calibrate(vis, sky_cal, cs_cal, rho, admm_iter=args.admm,
                           poly_order=args.poly, **wopts)
    if sol.weights is not None:
        msg = f"[weights] mean {float(sol.weights.mean()):.3f}, " \
              f"{int((sol.weights == 0).sum())} samples at 0"
        if sol.nu is not None:
            msg += f", nu {[round(float(x), 2) for x in sol.nu]}"
        print(msg)
    res_pow = float(torch.linalg.vector_norm(sol.residual))
    dat_pow = float(torch.linalg.vector_norm(vis.data))
    print(f"[calibrate] -A {args.admm} -P {args.poly}: residual/data "
          f"power = {res_pow / dat_pow:.4f} ({time.time() - t0:.2f} s)")

    t0 = time.time()
    imgs_d, imgs_r, imgs_i = [], [], []
    vals_i = []
    f0 = float(np.mean(vis.freqs))
    for fi in range(args.nf):
        f = float(vis.freqs[fi])
        sI_d = 0.5 * (vis.data[fi][:, 0] + vis.data[fi][:, 3])
        sI_r = 0.5 * (sol.residual[fi][:, 0] + sol.residual[fi][:, 3])
        if args.imager == "grid":
            imgs_d.append(imaging.dirty_image(vis.uvw, sI_d, f, 128))
            imgs_r.append(imaging.dirty_image(vis.uvw, sI_r, f, 128))
        C = predict_coherencies_uvw(sky_cal, cs_cal, vis.uvw, f, ra0, dec0,
                                    smear_bw=180e3)
        Hadd = influence.hadd_for(args.K, vis.N, args.poly, vis.freqs, f0,
                                  fi, rho, None, vis.data.device)
        vals = influence.influence_values(sol.residual[fi], C,
                                          sol.J_ref_layout(fi), vis.N,
                                          vis.Tdelta, Hadd)
        sI_i = 0.5 * (vals[:, 0] + vals[:, 3])
        if args.imager == "grid":
            imgs_i.append(imaging.dirty_image(vis.uvw, sI_i, f, 128))
        else:
            vals_i.append(sI_i)
    if args.imager == "dft":
        # all bands at once: data + residual maps, then the influence maps
        sI = torch.stack([
            0.5 * (vis.data[:, :, 0] + vis.data[:, :, 3]),
            0.5 * (sol.residual[:, :, 0] + sol.residual[:, :, 3])], dim=1)
        cube = imaging.dft_image_cube(vis.uvw, sI, vis.freqs, 128)
        cube_i = imaging.dft_image_cube(
            vis.uvw, torch.stack(vals_i)[:, None], vis.freqs, 128)
        imgs_d, imgs_r = list(cube[:, 0]), list(cube[:, 1])
        imgs_i = list(cube_i[:, 0])
    data_img = imaging.weighted_mean_image(imgs_d, vis.freqs)
    res_img = imaging.weighted_mean_image(imgs_r, vis.freqs)
    inf_img = imaging.weighted_mean_image(imgs_i, vis.freqs)
    np.save(out / "data_img.npy", data_img.cpu().numpy())
    np.save(out / "res_img.npy", res_img.cpu().numpy())
    np.save(out / "influenceI.npy", inf_img.cpu().numpy())
    s0, s1, si = (float(data_img.std()), float(res_img.std()),
                  float(inf_img.std()))
    print(f"[influence+image] sigma_data={s0:.4g} sigma_res={s1:.4g} "
          f"sigma_inf={si:.4g} ({time.time() - t0:.2f} s)")
    print(f"quality: sigma_data/sigma_res = {s0 / max(s1, 1e-12):.3f}")


if __name__ == "__main__":
    main()
