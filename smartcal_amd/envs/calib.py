"""CalibEnv — ADMM-regularization tuning environment.

Re-design of the reference `calibration/calibenv.py:30-243`: identical
observation/action/reward semantics, but the whole pipeline that the
reference drives through shell scripts and external binaries
(`dosimul.sh` → `docal.sh` (mpirun sagecal-mpi_gpu) → `doinfluence.sh` →
FITS files) runs in-process on device: `radio.sim` simulates the
observation, `radio.solver.calibrate` is the consensus-ADMM solver,
`radio.influence` + `radio.imaging` produce the 128² influence map and
data/residual images. Coherencies are predicted once per episode and
cached in HBM; a step is pure GPU compute with no file or process
boundary.

Action:  (2M,) in [-1,1] → K spectral + K spatial ADMM rho in
         [LOW, HIGH] (`calibenv.py:21-22,121`).
Obs:     {'img': (1, Ninf, Ninf) influence map ×1e-3,
          'sky': (M+1, 7) metadata ×1e-3} (`calibenv.py:53-56,164-166`).
Reward:  σ_data/σ_res + 1e-4/(σ_inf+EPS) + bound-penalty
         (`calibenv.py:170`).
"""

from __future__ import annotations


import numpy as np
import torch

from .. import gymapi
from ..gymapi import Box, Dict as DictSpace
from ..radio import array as arr
from ..radio import sim as rsim
from ..radio import solver as rsolver
from ..radio import influence as rinf
from ..radio import imaging as rimg
from ..radio.coherency import predict_coherencies_uvw

LOW = 0.01
HIGH = 1000.0
INF_SCALE = 1e-3
META_SCALE = 1e-3
EPS = 0.01


class CalibEnv(gymapi.Env):
    """In-memory calibration-tuning environment (`calibenv.py:30`)."""

    metadata = {"render.modes": ["human"]}

    def __init__(self, M: int = 5, provide_hint: bool = False,
                 N_stations: int = 26, Nf: int = 8, Ts: int = 2,
                 Tdelta: int = 10, Ninf: int = 128, admm_iter: int = 6,
                 poly_order: int = 3, snr: float = 5.0, device=None,
                 inf_nfreq: int = 2, seed: int | None = None,
                 diffuse_sky: bool = False, diffuse_flux: float = 250.0,
                 diffuse_beta: float | None = None,
                 station_beam: bool = False, beam_elements: int = 48,
                 imager: str = "grid", image_fov: float | None = None,
                 image_wterm: bool = True, robust: bool = False,
                 uvmin: float | None = None, rfi_fraction: float = 0.0,
                 rfi_amplitude: float = 50.0):
        super().__init__()
        # robust (Student's-t) noise model and lower uv cut in wavelengths
        # of the calibration (`radio.solver.calibrate`; the reference's
        # `docal.sh` passes `-L 2 -x 30`), and unflagged interference in
        # the simulated data (`radio.sim.add_outliers`), drawn from a
        # generator of its own like the beam's element layouts
        self.robust = robust
        self.uvmin = uvmin
        self.rfi_fraction = rfi_fraction
        self.rfi_amplitude = rfi_amplitude
        self.rfi_rng = np.random.default_rng(
            None if seed is None else [seed, 0x0F1])
        if imager not in ("grid", "dft"):
            raise ValueError(f"imager must be 'grid' or 'dft', got "
                             f"{imager!r}")
        # "grid": nearest-cell gridder + FFT (`imaging.dirty_image`);
        # "dft": exact direct Fourier sum with the w-term
        # (`imaging.dft_image_cube`), image_fov / image_wterm apply to it
        self.imager = imager
        self.image_fov = image_fov
        self.image_wterm = image_wterm
        self.M = M
        self.K = 0
        self.provide_hint = provide_hint
        self.hint = None
        self.Ninf = Ninf
        self.Nf = Nf
        self.Ts = Ts
        self.Tdelta = Tdelta
        self.N = N_stations
        self.admm_iter = admm_iter
        self.poly_order = poly_order
        self.snr = snr
        self.inf_nfreq = min(inf_nfreq, Nf)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available()
            else torch.device("cpu"))
        self.rng = np.random.default_rng(seed)
        # shapelet diffuse component in the simulated data only
        # (`radio.sim.make_calibration_sky`)
        self.diffuse = dict(diffuse=diffuse_sky, diffuse_flux=diffuse_flux,
                            diffuse_beta=diffuse_beta)
        # station array-factor beam, likewise in the simulated data only
        # (the reference simulates with the beam and calibrates without);
        # element layouts come from a generator of their own, so that
        # self.rng draws what it draws without a beam
        self.beam_elements = beam_elements if station_beam else 0
        self.beam_rng = np.random.default_rng(
            None if seed is None else [seed, 0xBEA3])
        self.action_space = Box(low=-1.0, high=1.0, shape=(2 * M,))
        self.observation_space = DictSpace({
            "img": Box(low=-HIGH, high=HIGH, shape=(1, Ninf, Ninf)),
            "sky": Box(low=-HIGH, high=HIGH, shape=(M + 1, 7)),
        })
        self.rho_spectral = np.ones(M, np.float32)
        self.rho_spatial = np.ones(M, np.float32)
        self.sky_meta = None
        self._scenario = None

    # -- internal pipeline -------------------------------------------------

    def _simulate_episode(self):
        (sky, cs_sim, sky_cal, cs_cal, skylmn, rho0, ra0, dec0) = \
            rsim.make_calibration_sky(self.K, self.rng, **self.diffuse)
        layout = arr.lofar_like_layout(self.N, self.rng)
        freqs = np.linspace(115e6, 185e6, self.Nf)
        elements = None
        if self.beam_elements:
            elements = arr.station_elements(self.N, self.beam_elements,
                                            self.beam_rng)
        vis = rsim.simulate_observation(
            layout, sky, cs_sim, freqs, ra0, dec0, self.Ts, self.Tdelta,
            snr=self.snr, device=self.device, rng=self.rng,
            torch_seed=int(self.rng.integers(2 ** 31)),
            beam_elements=elements)
        if self.rfi_fraction > 0:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(self.rfi_rng.integers(2 ** 31)))
            vis, _ = rsim.add_outliers(vis, self.rfi_fraction,
                                       self.rfi_amplitude, gen)
        # cache calibration-model coherencies per freq (constant per episode)
        C = torch.stack([
            predict_coherencies_uvw(sky_cal, cs_cal, vis.uvw, float(f),
                                    ra0, dec0, smear_bw=180e3)
            for f in freqs])
        self._scenario = dict(sky=sky_cal, clusters=cs_cal, vis=vis,
                              C=C, skylmn=skylmn, rho0=rho0,
                              f_low=freqs[0] / 1e6, f_high=freqs[-1] / 1e6)

    def _weight_options(self) -> dict:
        """Keywords of `calibrate` for the robust model and the uv cut;
        empty by default, so that the default call is today's."""
        kw = {}
        if self.robust:
            kw["robust"] = True
        if self.uvmin is not None:
            kw["uvmin"] = self.uvmin
        return kw

    def _calibrate_and_observe(self):
        sc = self._scenario
        vis: rsim.VisData = sc["vis"]
        K = self.K
        sol = rsolver.calibrate(
            vis, sc["sky"], sc["clusters"], self.rho_spectral[:K],
            admm_iter=self.admm_iter, poly_order=self.poly_order,
            alpha=float(np.mean(self.rho_spatial[:K])),
            C_cache=sc["C"], **self._weight_options())
        # data / residual dirty images (σ over the mean image, à la
        # calmean + fits std in `calibenv.py:148-158`)
        inf_idx = np.linspace(0, self.Nf - 1, self.inf_nfreq).astype(int)
        f0 = float(np.mean(vis.freqs))
        # flagged samples are left out of every image
        def unflagged(sI, fi):
            if vis.flags is None:
                return sI
            return sI * (~vis.flags[fi]).to(torch.float32)
        sI_d = [unflagged(0.5 * (vis.data[fi][:, 0] + vis.data[fi][:, 3]),
                          fi) for fi in range(self.Nf)]
        sI_r = [unflagged(0.5 * (sol.residual[fi][:, 0]
                                 + sol.residual[fi][:, 3]), fi)
                for fi in range(self.Nf)]
        sI_i = []
        for fi in inf_idx:
            Hadd = rinf.hadd_for(K, vis.N, self.poly_order, vis.freqs, f0,
                                 int(fi), self.rho_spectral[:K],
                                 self.rho_spatial[:K], self.device)
            vals = rinf.influence_values(sol.residual[fi], sc["C"][fi],
                                         sol.J_ref_layout(int(fi)), vis.N,
                                         vis.Tdelta, Hadd)
            sI_i.append(unflagged(0.5 * (vals[:, 0] + vals[:, 3]), int(fi)))
        if self.imager == "dft":
            # two launches: data + residual maps of all bands (M = 2),
            # then the influence maps of the inf_nfreq bands
            kw = dict(npix=self.Ninf, fov=self.image_fov,
                      wterm=self.image_wterm)
            cube = rimg.dft_image_cube(
                vis.uvw, torch.stack([torch.stack(sI_d), torch.stack(sI_r)],
                                     dim=1), vis.freqs, **kw)
            cube_i = rimg.dft_image_cube(vis.uvw, torch.stack(sI_i)[:, None],
                                         vis.freqs[inf_idx], **kw)
            imgs_d, imgs_r = list(cube[:, 0]), list(cube[:, 1])
            imgs_i = list(cube_i[:, 0])
        else:
            def grid(maps, fs):
                return [rimg.dirty_image(vis.uvw, sI, float(f), self.Ninf)
                        for sI, f in zip(maps, fs)]
            imgs_d, imgs_r = grid(sI_d, vis.freqs), grid(sI_r, vis.freqs)
            imgs_i = grid(sI_i, vis.freqs[inf_idx])
        data_img = rimg.weighted_mean_image(imgs_d, vis.freqs)
        res_img = rimg.weighted_mean_image(imgs_r, vis.freqs)
        inf_img = rimg.weighted_mean_image(imgs_i, vis.freqs[inf_idx])
        return data_img, res_img, inf_img

    def _obs(self, inf_img) -> dict:
        img = inf_img.unsqueeze(0).cpu().numpy().astype(np.float32)
        return {"img": img * INF_SCALE,
                "sky": self.sky_meta * META_SCALE}

    def _update_meta_rho(self):
        self.sky_meta[:self.K, 5] = (self.rho_spectral[:self.K]
                                     - (HIGH + LOW) / 2) * (2 / (HIGH - LOW))
        self.sky_meta[:self.K, 6] = (self.rho_spatial[:self.K]
                                     - (HIGH + LOW) / 2) * (2 / (HIGH - LOW))

    # -- gym API -----------------------------------------------------------

    def reset(self):
        self.K = int(self.rng.integers(2, self.M + 1))
        self._simulate_episode()
        sc = self._scenario
        rho0 = sc["rho0"]
        self.rho_spectral[:self.K] = np.clip(rho0, LOW, HIGH)
        self.rho_spatial[:self.K] = np.clip(0.05 * rho0, LOW, HIGH)
        self.sky_meta = np.zeros((self.M + 1, 7), np.float32)
        self.sky_meta[:self.K, :5] = sc["skylmn"][:self.K]
        self.sky_meta[-1, :5] = [sc["vis"].ra0, sc["vis"].dec0, self.K,
                                 sc["f_low"] / 1000.0, sc["f_high"] / 1000.0]
        self._update_meta_rho()
        _, _, inf_img = self._calibrate_and_observe()
        if self.provide_hint:
            self.hint = np.zeros(2 * self.M, np.float32)
            self.hint[:self.K] = (self.rho_spectral[:self.K]
                                  - (HIGH + LOW) / 2) * (2 / (HIGH - LOW))
            self.hint[self.M:self.M + self.K] = \
                (0.05 * self.rho_spectral[:self.K]
                 - (HIGH + LOW) / 2) * (2 / (HIGH - LOW))
        return self._obs(inf_img)

    def step(self, action):
        action = np.asarray(action, np.float32).squeeze()
        assert action.shape[0] == 2 * self.M
        done = False
        rho = action * (HIGH - LOW) / 2 + (HIGH + LOW) / 2
        self.rho_spectral[:self.K] = rho[:self.K]
        self.rho_spatial[:self.K] = rho[self.M:self.M + self.K]
        penalty = 0.0
        for ci in range(self.K):
            for arr_ in (self.rho_spectral, self.rho_spatial):
                if arr_[ci] < LOW:
                    arr_[ci] = LOW
                    penalty += -0.1
                if arr_[ci] > HIGH:
                    arr_[ci] = HIGH
                    penalty += -0.1
        data_img, res_img, inf_img = self._calibrate_and_observe()
        sigma0 = float(data_img.std())
        sigma1 = float(res_img.std())
        sigma_inf = float(inf_img.std())
        self._update_meta_rho()
        observation = self._obs(inf_img)
        reward = sigma0 / max(sigma1, 1e-12) + 1e-4 / (sigma_inf + EPS) \
            + penalty
        info = {}
        if self.provide_hint:
            return observation, reward, done, self.hint, info
        return observation, reward, done, info

    def render(self, mode="human"):
        print(self.rho_spectral, self.rho_spatial)

    def close(self):
        pass
