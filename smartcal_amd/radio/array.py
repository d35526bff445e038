"""Synthetic interferometer array: station layout, uvw synthesis, az/el.

Replaces the reference's externally-created MeasurementSets (`makems`,
template MS + casacore in `calibration/generate_data.py:118-224` and the
casacore-measures az/el/separation math in
`calibration/influence_tools.py:16-216`). Everything is computed from a
parametric station layout and standard earth-rotation synthesis; arrays
never touch disk (MI355X-native: uvw for a full observation is a few MB
resident in HBM).
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

__all__ = ["StationLayout", "lofar_like_layout", "uvw_synthesis",
           "azel_of", "separation", "StationBeam", "station_elements",
           "station_beam"]

# LOFAR core latitude (rad) — used for az/el synthesis
SITE_LAT = math.radians(52.915)
EARTH_OMEGA = 2.0 * math.pi / 86164.0905   # sidereal rate (rad/s)


def enu_to_xyz(enu: np.ndarray, lat: float) -> np.ndarray:
    """ENU (..., 3) → equatorial XYZ (..., 3) at a site of latitude ``lat``
    (standard geodetic rotation)."""
    e, n, u = enu[..., 0], enu[..., 1], enu[..., 2]
    x = -math.sin(lat) * n + math.cos(lat) * u
    y = e
    z = math.cos(lat) * n + math.sin(lat) * u
    return np.stack([x, y, z], axis=-1)


def synthesis_rotation(ra0: float, dec0: float, times_s: np.ndarray,
                       ha0: float = 0.0):
    """Rows (ru, rv, rw), each (Nt, 3), of the XYZ → uvw rotation for
    phase center (ra0, dec0): the hour angle advances at the sidereal
    rate."""
    H = ha0 + EARTH_OMEGA * np.asarray(times_s, np.float64) - ra0
    sH, cH = np.sin(H), np.cos(H)
    sd, cd = math.sin(dec0), math.cos(dec0)
    # rows of the rotation for each time
    zero = np.zeros_like(sH)
    ru = np.stack([sH, cH, zero], axis=1)                   # (Nt,3)
    rv = np.stack([-sd * cH, sd * sH, np.full_like(sH, cd)], axis=1)
    rw = np.stack([cd * cH, -cd * sH, np.full_like(sH, sd)], axis=1)
    return ru, rv, rw


@dataclass
class StationLayout:
    """Station positions in a local East-North-Up frame (meters)."""
    enu: np.ndarray          # (N, 3)
    latitude: float = SITE_LAT

    @property
    def n_stations(self) -> int:
        return self.enu.shape[0]

    def baselines_xyz(self) -> np.ndarray:
        """Per-baseline (p<q lexicographic) coordinate differences in the
        equatorial (X, Y, Z) frame used by uvw synthesis."""
        xyz = enu_to_xyz(self.enu, self.latitude)          # (N,3)
        N = xyz.shape[0]
        pi, qi = np.triu_indices(N, k=1)
        return xyz[pi] - xyz[qi]                            # (B,3)


def lofar_like_layout(N: int = 62, rng: np.random.Generator | None = None,
                      core_frac: float = 0.6, rmax: float = 40e3,
                      rcore: float = 2e3) -> StationLayout:
    """Dense core + log-spiral remote arms, loosely like LOFAR: N stations,
    ~core_frac in an rcore-radius core, the rest out to rmax."""
    rng = rng or np.random.default_rng(0)
    ncore = int(N * core_frac)
    nrem = N - ncore
    th = rng.uniform(0, 2 * math.pi, ncore)
    rr = rcore * np.sqrt(rng.uniform(0.001, 1.0, ncore))
    core = np.stack([rr * np.cos(th), rr * np.sin(th)], axis=1)
    # remote: 3 spiral arms, logarithmic radius growth
    arm = rng.integers(0, 3, nrem)
    tt = rng.uniform(0.15, 1.0, nrem)
    radius = rcore * (rmax / rcore) ** tt
    ang = arm * 2 * math.pi / 3 + 1.5 * np.log(radius / rcore) \
        + rng.normal(0, 0.08, nrem)
    rem = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)
    en = np.concatenate([core, rem], axis=0)
    up = rng.normal(0, 2.0, (N, 1))
    return StationLayout(np.concatenate([en, up], axis=1))


def uvw_synthesis(layout: StationLayout, ra0: float, dec0: float,
                  times_s: np.ndarray, ha0: float = 0.0) -> np.ndarray:
    """uvw (Ntime, B, 3) in meters for phase center (ra0, dec0).

    Standard synthesis rotation: hour angle advances at the sidereal
    rate; the baseline XYZ vector maps to uvw via the (H0, dec0)
    projection matrix.
    """
    Lxyz = layout.baselines_xyz()                           # (B,3)
    ru, rv, rw = synthesis_rotation(ra0, dec0, times_s, ha0)
    u = ru @ Lxyz.T                                          # (Nt,B)
    v = rv @ Lxyz.T
    w = rw @ Lxyz.T
    return np.stack([u, v, w], axis=2)                       # (Nt,B,3)


@dataclass
class StationBeam:
    """Element positions of every station, relative to the station
    centre, in the uvw frame of every timeslot — what the array-factor
    beam of `radio.coherency` is summed over."""
    elem_uvw: np.ndarray     # (Tt, N, Ne, 3) float64, meters

    @property
    def n_time(self) -> int:
        return self.elem_uvw.shape[0]

    @property
    def n_stations(self) -> int:
        return self.elem_uvw.shape[1]

    @property
    def n_elem(self) -> int:
        return self.elem_uvw.shape[2]


def station_elements(N: int, n_elem: int, rng: np.random.Generator,
                     radius: float = 15.0) -> np.ndarray:
    """Element ENU offsets (N, n_elem, 3) in meters from each station's
    centre: one random pattern within ``radius``, turned by a rotation of
    the station's own (as LOFAR stations are), up = 0."""
    th = rng.uniform(0, 2 * math.pi, n_elem)
    rr = radius * np.sqrt(rng.uniform(0.0, 1.0, n_elem))
    e0, n0 = rr * np.cos(th), rr * np.sin(th)
    rot = rng.uniform(0, 2 * math.pi, N)
    c, s = np.cos(rot)[:, None], np.sin(rot)[:, None]
    enu = np.zeros((N, n_elem, 3))
    enu[:, :, 0] = c * e0 - s * n0
    enu[:, :, 1] = s * e0 + c * n0
    return enu


def station_beam(layout: StationLayout, elem_enu: np.ndarray, ra0: float,
                 dec0: float, times_s: np.ndarray,
                 ha0: float = 0.0) -> StationBeam:
    """Rotate element offsets (N, Ne, 3) ENU into the uvw frame of every
    timeslot: the ENU → XYZ rotation of `StationLayout.baselines_xyz`,
    then the (H_t, dec0) matrix of `uvw_synthesis`."""
    elem_enu = np.asarray(elem_enu, np.float64)
    if elem_enu.ndim != 3 or elem_enu.shape[0] != layout.n_stations \
            or elem_enu.shape[2] != 3:
        raise ValueError(
            f"element offsets of shape {elem_enu.shape} do not match "
            f"(N = {layout.n_stations}, Ne, 3)")
    xyz = enu_to_xyz(elem_enu, layout.latitude)              # (N,Ne,3)
    ru, rv, rw = synthesis_rotation(ra0, dec0, times_s, ha0)
    rot = np.stack([ru, rv, rw], axis=1)                     # (Nt,3,3)
    return StationBeam(np.ascontiguousarray(
        np.einsum("tcx,pex->tpec", rot, xyz)))


def azel_of(ra, dec, lst: float, latitude: float = SITE_LAT):
    """Azimuth/elevation (rad) of (ra, dec) at local sidereal time lst.
    Replaces the casacore measures conversion of
    `influence_tools.py:16-74`."""
    ra = np.asarray(ra, np.float64)
    dec = np.asarray(dec, np.float64)
    H = lst - ra
    sin_el = np.sin(latitude) * np.sin(dec) \
        + np.cos(latitude) * np.cos(dec) * np.cos(H)
    el = np.arcsin(np.clip(sin_el, -1, 1))
    az = np.arctan2(-np.sin(H) * np.cos(dec),
                    np.sin(dec) * np.cos(latitude)
                    - np.cos(dec) * np.sin(latitude) * np.cos(H))
    return np.mod(az, 2 * math.pi), el


def separation(ra, dec, ra0: float, dec0: float):
    """Great-circle separation (rad) from (ra0, dec0)."""
    ra = np.asarray(ra, np.float64)
    dec = np.asarray(dec, np.float64)
    cs = np.sin(dec) * math.sin(dec0) \
        + np.cos(dec) * math.cos(dec0) * np.cos(ra - ra0)
    return np.arccos(np.clip(cs, -1, 1))
