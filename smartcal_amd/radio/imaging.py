"""uv gridding + FFT imaging.

Replaces the external ``excon`` imager (`calibration/doinfluence.sh:8`,
`generate_data.py:461`) for the paths the framework
needs: Stokes-I dirty images of visibility-sampled values (data maps,
residual maps, 128² influence maps) and the weighted mean over sub-bands
(`calmean.sh`). Gridding is a scatter-add into the uv plane (index_put_
accumulate → hipBLAS-free, bandwidth-bound) followed by a centered
inverse FFT; conjugate symmetry is enforced so images are real.

:func:`dft_image` / :func:`dft_image_cube` / :func:`dft_psf` are the exact
alternative for the small maps: the direct Fourier sum per pixel, with the
w-term, natural or uniform weighting and an image centre anywhere on the
sky (``excon -P``). No gridding, so nothing aliases. On the GPU the whole
(frequency, map) cube is one launch of ``ops/csrc/dft_image.hip``; on the
CPU (and with ``SMARTCAL_FORCE_EAGER=1``) a chunked float64 torch sum.
"""

from __future__ import annotations


import math

import numpy as np
import torch

C_LIGHT = 2.99792458e8

__all__ = ["dirty_image", "image_std", "weighted_mean_image",
           "dft_image", "dft_image_cube", "dft_psf"]


def dirty_image(uvw: torch.Tensor, values: torch.Tensor, freq: float,
                npix: int = 128, fov: float | None = None) -> torch.Tensor:
    """Dirty image (npix, npix) float32 of complex per-sample ``values``.

    uvw: (S, 3) meters; values: (S,) complex (e.g. Stokes I);
    fov: field of view in direction-cosine units (image spans ±fov/2);
    uv cell follows from du = 1/fov. With fov=None the cell auto-scales
    so the longest sampled baseline lands on the grid edge (what excon's
    default pixel scaling effectively does for our synthetic layouts).
    """
    dev = uvw.device
    lam = C_LIGHT / freq
    u = uvw[:, 0] / lam
    v = uvw[:, 1] / lam
    if fov is None:
        umax = float(torch.maximum(u.abs().max(), v.abs().max()).item())
        du = max(umax, 1.0) / (npix // 2 - 1)
    else:
        du = 1.0 / fov
    iu = torch.round(u / du).long() + npix // 2
    iv = torch.round(v / du).long() + npix // 2
    ok = (iu >= 0) & (iu < npix) & (iv >= 0) & (iv < npix)
    grid = torch.zeros((npix, npix), dtype=torch.complex64, device=dev)
    wsum = torch.zeros((), dtype=torch.float32, device=dev)
    vals = values[ok]
    grid.index_put_((iv[ok], iu[ok]), vals, accumulate=True)
    # conjugate symmetry: V(-u,-v) = V*(u,v)
    iu2 = npix - iu[ok]
    iv2 = npix - iv[ok]
    ok2 = (iu2 >= 0) & (iu2 < npix) & (iv2 >= 0) & (iv2 < npix)
    grid.index_put_((iv2[ok2], iu2[ok2]), vals[ok2].conj(), accumulate=True)
    nvis = float(ok.sum()) + float(ok2.sum())
    img = torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(grid)))
    return (img.real * (npix * npix / max(nvis, 1.0))).to(torch.float32)


def image_std(uvw: torch.Tensor, vis4: torch.Tensor, freq: float,
              npix: int = 256, fov: float = 2.0) -> float:
    """std of the Stokes-I dirty image of (S,4) visibilities — the
    reference's image-noise estimate (`demixingenv.py:221-231`,
    `calibenv.py:148-158`)."""
    sI = 0.5 * (vis4[:, 0] + vis4[:, 3])
    return float(dirty_image(uvw, sI, freq, npix, fov).std().item())


def weighted_mean_image(images: list[torch.Tensor],
                        freqs) -> torch.Tensor:
    """Frequency-weighted mean image à la `calmean.sh` (weights ∝ f²
    normalized)."""
    w = torch.as_tensor([float(f) ** 2 for f in freqs],
                        device=images[0].device)
    w = w / w.sum()
    out = torch.zeros_like(images[0])
    for wi, im in zip(w, images):
        out += wi * im
    return out


# -- exact direct-Fourier-sum imager ----------------------------------------

_EAGER_ELEMS = 1 << 22      # pixel × sample phases per eager chunk (f64)


def _uniform_weights(u: torch.Tensor, v: torch.Tensor, du: float,
                     g: torch.Tensor) -> torch.Tensor:
    """g / (number of live samples in the sample's uv cell). The cell
    (round(u/du), round(v/du)) has no grid limit and is folded onto one
    half-plane, so a sample and another sample's conjugate share a count;
    samples of zero weight are not counted."""
    iu = torch.round(u / du).long()
    iv = torch.round(v / du).long()
    flip = (iu < 0) | ((iu == 0) & (iv < 0))
    iu = torch.where(flip, -iu, iu)
    iv = torch.where(flip, -iv, iv)
    live = g != 0
    if not bool(live.any()):
        return g
    span = 2 * int(iv.abs().max()) + 1
    key = iu * span + (iv + span // 2)
    _, inverse, counts = torch.unique(key[live], return_inverse=True,
                                      return_counts=True)
    out = torch.zeros_like(g)
    out[live] = g[live] / counts[inverse].to(g.dtype)
    return out


def _dft_eager(uvw: torch.Tensor, vals: torch.Tensor, fpar: torch.Tensor,
               npix: int, lc: float, mc: float) -> torch.Tensor:
    """Σ_s Re[vals · e^{−2πi·phase}] in float64, pixels in chunks."""
    F, M, S = vals.shape
    dev = uvw.device
    ax = torch.arange(npix, dtype=torch.float64, device=dev) - npix // 2
    out = torch.zeros((F, M, npix * npix), dtype=torch.float32, device=dev)
    if S == 0:
        return out.view(F, M, npix, npix)
    step = max(1, _EAGER_ELEMS // S)
    for f in range(F):
        scale, cell = float(fpar[f, 0]), float(fpar[f, 1])
        l = (lc + ax * cell).repeat(npix)                 # x fastest
        m = (mc + ax * cell).repeat_interleave(npix)
        r2 = l * l + m * m
        sky = r2 <= 1.0
        nm1 = torch.sqrt(torch.clamp(1.0 - r2, min=0.0)) - 1.0
        nm1 = torch.where(sky, nm1, torch.zeros_like(nm1))
        lmn = torch.stack([l, m, nm1], dim=1)             # (P, 3)
        uvw_f = (uvw * scale).T.contiguous()              # (3, S)
        vr = vals[f].real.to(torch.float64).T.contiguous()   # (S, M)
        vi = vals[f].imag.to(torch.float64).T.contiguous()
        for p0 in range(0, npix * npix, step):
            ph = (2.0 * math.pi) * (lmn[p0:p0 + step] @ uvw_f)    # (p, S)
            img = torch.cos(ph) @ vr + torch.sin(ph) @ vi         # (p, M)
            img = img * sky[p0:p0 + step, None]
            out[f, :, p0:p0 + step] = img.T.to(torch.float32)
    return out.view(F, M, npix, npix)


def dft_image_cube(uvw: torch.Tensor, values: torch.Tensor, freqs,
                   npix: int = 128, fov: float | None = None, *,
                   center=(0.0, 0.0), wterm: bool = True,
                   weighting: str = "natural",
                   weights: torch.Tensor | None = None,
                   nsplit: int = 0) -> torch.Tensor:
    """Exact dirty-image cube (F, M, npix, npix) float32 by direct Fourier
    sum; all maps share ``uvw`` and one call is one kernel launch.

        I[y, x] = (1/Σ_s g_s) · Σ_s g_s · Re[V_s · exp(−2πi (u_s·l_x
                                        + v_s·m_y + w_s·(n_xy − 1)))]
        l_x = l_c + (x − npix//2)·cell,  m_y = m_c + (y − npix//2)·cell,
        cell = fov/npix,  n_xy = sqrt(1 − l_x² − m_y²)

    with u, v, w in wavelengths at each frequency. The sign is that of
    ``predict_coherencies_uvw``: a source predicted at (l, m) with flux F
    images at (l, m) with value F. Pixels with l² + m² > 1 are 0.

    uvw: (S, 3) meters, any float dtype (upcast to f64 as given);
    values: (F, M, S) complex; freqs: F frequencies in Hz.
    center: direction cosines (l_c, m_c) of the image centre. Take them
      from ``coords.radectolm(ra, dec, ra0, dec0)[:2]`` —
      ``coords.lmtoradec`` flips the sign of l and is not its inverse.
    wterm=False drops the w term.
    fov=None: ``dirty_image``'s rule per frequency, du = max(umax, 1) /
      (npix//2 − 1), fov = 1/du — both imagers cover the same field.
    weights: (S,) real, multiplies g_s; 0 flags a sample.
    weighting: "natural" (g_s = weights_s or 1) or "uniform" (g_s =
      weights_s / number of unflagged samples in the sample's uv cell of
      side du = 1/fov, conjugates folded onto one half-plane).
    nsplit: sample slices of the kernel (0 = choose for occupancy); any
      value gives run-to-run bit-identical results. The torch path ignores
      it.
    """
    if weighting not in ("natural", "uniform"):
        raise ValueError(f"weighting must be 'natural' or 'uniform', "
                         f"got {weighting!r}")
    freqs = np.atleast_1d(np.asarray(freqs, np.float64))
    if values.dim() != 3 or values.shape[0] != len(freqs) \
            or values.shape[2] != uvw.shape[0]:
        raise ValueError(f"values {tuple(values.shape)} is not (F, M, S) "
                         f"for F = {len(freqs)}, S = {uvw.shape[0]}")
    if not values.is_complex():
        raise ValueError("values must be complex")
    dev = uvw.device
    F, M, S = values.shape
    uvw64 = uvw.to(torch.float64)
    scales = freqs / C_LIGHT                      # wavelengths per meter
    if fov is None:
        umax_m = float(uvw64[:, :2].abs().max()) if S else 0.0
        fovs = [(npix // 2 - 1) / max(umax_m * sc, 1.0) for sc in scales]
    else:
        fovs = [float(fov)] * F
    g = torch.ones(S, dtype=torch.float64, device=dev) if weights is None \
        else weights.to(device=dev, dtype=torch.float64)
    if g.shape != (S,):
        raise ValueError(f"weights {tuple(g.shape)} is not (S,) = ({S},)")
    if weighting == "uniform":
        g = torch.stack([
            _uniform_weights(uvw64[:, 0] * sc, uvw64[:, 1] * sc, 1.0 / fv, g)
            for sc, fv in zip(scales, fovs)])                     # (F, S)
    else:
        g = g.expand(F, S)
    gsum = g.sum(dim=1, keepdim=True)
    gn = torch.where(gsum != 0, g / gsum, torch.zeros_like(g))
    vals = values.to(torch.complex128) * gn[:, None, :]
    if not wterm:
        uvw64 = uvw64.clone()
        uvw64[:, 2] = 0.0
    fpar = torch.as_tensor(
        np.stack([scales, np.asarray(fovs) / npix], axis=1),
        dtype=torch.float64)
    lc, mc = float(center[0]), float(center[1])
    from ..ops import ext, use_hip
    if use_hip(uvw):
        return ext().dft_image(
            uvw64.contiguous(), vals.to(torch.complex64).contiguous(),
            fpar.to(dev), int(npix), lc, mc, int(nsplit))
    return _dft_eager(uvw64, vals, fpar, int(npix), lc, mc)


def dft_image(uvw: torch.Tensor, values: torch.Tensor, freq: float,
              npix: int = 128, fov: float | None = None,
              **kw) -> torch.Tensor:
    """Exact dirty image of ``values`` (S,) → (npix, npix), or of M maps
    (M, S) → (M, npix, npix), at one frequency; see
    :func:`dft_image_cube` for the definition and the keyword arguments
    (center, wterm, weighting, weights)."""
    single = values.dim() == 1
    vals =values[None, None] if single else values[None]
    cube = dft_image_cube(uvw, vals, [float(freq)], npix, fov, **kw)
    return cube[0, 0] if single else cube[0]


def dft_psf(uvw: torch.Tensor, freq: float, npix: int = 128,
            fov: float | None = None, **kw) -> torch.Tensor:
    """Point-spread function (npix, npix): :func:`dft_image` of all-ones
    values, peak 1 at the image centre for center = (0, 0)."""
    ones = torch.ones(uvw.shape[0], dtype=torch.complex64, device=uvw.device)
    return dft_image(uvw, ones, freq, npix, fov, **kw)
