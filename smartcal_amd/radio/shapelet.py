"""Random shapelet-mode models (diffuse-sky components).

Parity with `calibration_tools.generate_random_shapelet_model`
(`calibration_tools.py:1254-1296`): the mode-file text format (position
line, n0/beta line, n0² coefficients with 1/|order|^1.2 attenuation,
linear-transform trailer), optional 10% perturbed twin for calibration,
plus a parser and a basis evaluator so diffuse components can be
rendered into images without external tools.

Prediction (this project's definition; SAGECal's own sign convention for
theta and its mode normalisation are not checked against): a model is
``(n0, beta, c[n0²], a, b, theta)`` with ``(a, b, theta)`` the linear
transform trailer ``L a b theta`` (absent → 1, 1, 0). With (x, y) the
offsets from the source centre::

    x' = ( cosθ·x + sinθ·y) / a,   y' = (−sinθ·x + cosθ·y) / b
    I(x, y) = Σ_{i,j<n0} c[i·n0+j] · φ_i(x';β) · φ_j(y';β)
    φ_n(x;β) = β^(−1/2) ψ_n(x/β),  ψ_n(t) = (2^n n! √π)^(−1/2) H_n(t) e^(−t²/2)

and its Fourier transform with kernel e^{+i(ux+vy)} (`shapelet_uv`)::

    u' = cosθ·u + sinθ·v,   v' = −sinθ·u + cosθ·v
    F(u, v) = 2π·β·a·b · Σ_{i,j} c[i·n0+j] · i^(i+j) · ψ_i(β·a·u') · ψ_j(β·b·v')
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

__all__ = ["generate_random_shapelet_model", "parse_shapelet_model",
           "shapelet_basis", "ShapeletModel", "load_shapelet_model",
           "shapelet_image", "shapelet_uv", "hermite_functions",
           "MAX_N0"]

MAX_N0 = 32     # mode-order cap of the prediction paths (LDS-staged n0²)


@dataclass
class ShapeletModel:
    """One shapelet source shape: n0² mode coefficients at scale beta
    plus the linear transform (a, b, theta) of the mode-file trailer."""
    n0: int
    beta: float
    coeff: np.ndarray           # (n0²,), index i·n0+j
    a: float = 1.0
    b: float = 1.0
    theta: float = 0.0


def generate_random_shapelet_model(rng: np.random.Generator,
                                   ra_hms=(1, 2, 3.0), dec_dms=(4, 5, 6.0),
                                   perturbed: bool = False):
    """→ (text, n0, beta, coeff[, perturbed_text])."""
    n0 = int(rng.integers(10, 20))
    beta = float(rng.random()) + 0.1
    if beta * n0 > 2:
        beta = (2 + float(rng.random()) * 0.001) / n0
    coeff = rng.standard_normal((n0, n0))
    x = np.arange(1, n0 + 1)
    coeff = (coeff / (np.abs(np.outer(x, x)) ** 1.2)).reshape(-1)

    def fmt(b, c):
        lines = [" ".join(str(v) for v in (*ra_hms, *dec_dms)),
                 f"{n0} {b}"]
        lines += [f"{i} {c[i]}" for i in range(n0 * n0)]
        lines.append(f"L 1.0 1.0 {math.pi / 2}")
        lines.append("#model created by smartcal_amd")
        return "\n".join(lines) + "\n"

    text = fmt(beta, coeff)
    if not perturbed:
        return text, n0, beta, coeff
    beta_p = beta + 0.1 * beta * float(rng.random())
    noise = rng.standard_normal((n0, n0)).reshape(-1)
    noise = noise / np.linalg.norm(noise) * 0.1 * np.linalg.norm(coeff)
    return text, n0, beta, coeff, fmt(beta_p, coeff + noise)


def parse_shapelet_model(text: str):
    """→ (position_tuple, n0, beta, coeff (n0²,))."""
    lines = [l for l in text.splitlines() if l and not l.startswith("#")]
    pos = tuple(float(v) for v in lines[0].split())
    n0_s, beta_s = lines[1].split()
    n0, beta = int(n0_s), float(beta_s)
    coeff = np.zeros(n0 * n0)
    for ln in lines[2:2 + n0 * n0]:
        i, v = ln.split()
        coeff[int(i)] = float(v)
    return pos, n0, beta, coeff


def load_shapelet_model(text: str) -> ShapeletModel:
    """Mode-file text → ShapeletModel, including the ``L a b theta``
    trailer (a = b = 1, theta = 0 when the file has none)."""
    _, n0, beta, coeff = parse_shapelet_model(text)
    a, b, theta = 1.0, 1.0, 0.0
    for ln in text.splitlines():
        tok = ln.split()
        if tok and tok[0] == "L":
            a, b, theta = (float(v) for v in tok[1:4])
    return ShapeletModel(n0, beta, coeff, a, b, theta)


def _hermite(n: int, x: np.ndarray) -> np.ndarray:
    h0 = np.ones_like(x)
    if n == 0:
        return h0
    h1 = 2 * x
    for k in range(1, n):
        h0, h1 = h1, 2 * x * h1 - 2 * k * h0
    return h1


def shapelet_basis(n0: int, beta: float, l: np.ndarray,
                   m: np.ndarray) -> np.ndarray:
    """Gauss-Hermite shapelet basis evaluated at direction cosines
    (l, m): (n0², P) for P sample points."""
    xl = l / beta
    xm = m / beta
    gl = np.exp(-0.5 * xl ** 2)
    gm = np.exp(-0.5 * xm ** 2)
    out = np.zeros((n0 * n0, l.size))
    for a in range(n0):
        na = 1.0 / math.sqrt((2 ** a) * math.factorial(a)
                             * math.sqrt(math.pi) * beta)
        ha = _hermite(a, xl) * gl * na
        for b in range(n0):
            nb = 1.0 / math.sqrt((2 ** b) * math.factorial(b)
                                 * math.sqrt(math.pi) * beta)
            out[a * n0 + b] = ha * _hermite(b, xm) * gm * nb
    return out


def hermite_functions(n0: int, t: np.ndarray) -> np.ndarray:
    """Normalised Hermite functions ψ_0..ψ_{n0−1} at t: (n0, P), f64.

    Three-term recurrence on ψ itself (never H_n · exp separately, which
    overflows × underflows on long baselines); exact zeros once
    e^(−t²/2) underflows."""
    t = np.asarray(t, np.float64).reshape(-1)
    out = np.zeros((n0, t.size))
    out[0] = math.pi ** -0.25 * np.exp(-0.5 * t * t)
    if n0 > 1:
        out[1] = math.sqrt(2.0) * t * out[0]
    for n in range(1, n0 - 1):
        out[n + 1] = t * math.sqrt(2.0 / (n + 1)) * out[n] \
            - math.sqrt(n / (n + 1)) * out[n - 1]
    return out


def shapelet_image(model: ShapeletModel, x: np.ndarray,
                   y: np.ndarray) -> np.ndarray:
    """Image-domain brightness at offsets (x, y) from the source centre
    (module docstring), built on `shapelet_basis`."""
    x = np.asarray(x, np.float64).reshape(-1)
    y = np.asarray(y, np.float64).reshape(-1)
    ct, st = math.cos(model.theta), math.sin(model.theta)
    xp = (ct * x + st * y) / model.a
    yp = (-st * x + ct * y) / model.b
    return model.coeff @ shapelet_basis(model.n0, model.beta, xp, yp)


def shapelet_uv(model: ShapeletModel, u: np.ndarray,
                v: np.ndarray) -> np.ndarray:
    """Visibility shape factor F(u, v) (module docstring), complex128;
    u, v in rad⁻¹ (metres · 2πf/c). The CPU oracle of the prediction
    paths."""
    u = np.asarray(u, np.float64).reshape(-1)
    v = np.asarray(v, np.float64).reshape(-1)
    n0 = model.n0
    ct, st = math.cos(model.theta), math.sin(model.theta)
    pu = hermite_functions(n0, model.beta * model.a * (ct * u + st * v))
    pv = hermite_functions(n0, model.beta * model.b * (-st * u + ct * v))
    k = np.arange(n0)
    cij = model.coeff.reshape(n0, n0) * 1j ** ((k[:, None] + k[None, :]) % 4)
    return (2.0 * math.pi * model.beta * model.a * model.b) \
        * np.einsum("ij,ip,jp->p", cij, pu, pv)


def correct_shapelet_modes(text: str) -> str:
    """Rescale shapelet coefficients by i!/(i+1)! per row block — parity
    with `calibration/correct_shapelet_modes.py:4-30` (mode-file format
    conversion between SAGECal versions)."""
    lines = text.splitlines()
    out = [lines[0], lines[1]]
    n0 = int(lines[1].split()[0])
    idx = 2
    for ci in range(n0):
        scale = 1.0 / (ci + 1)          # i!/(i+1)!
        for cj in range(n0):
            num, val = lines[idx].split()
            out.append(f"{num} {float(val) * scale}")
            idx += 1
    out.extend(lines[idx:])
    return "\n".join(out) + "\n"
