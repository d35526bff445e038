"""Record tests/golden/chain_fwd_golden.npz: the outputs of the fp32
mlp_chain_fwd kernel for fixed seeded inputs.

Run on the GPU from a checkout whose kernel is trusted (the commit before a
change to the chain kernel); tests/test_gpu_learn_path.py then demands that
the current kernel reproduces every recorded y / zhat / rstd bit for bit.
The fixture holds outputs only, plus a SHA-256 of the input bytes, so a
change of the input generator cannot go unnoticed.

    python scripts/record_chain_golden.py [--root CHECKOUT] [--out FILE]
"""

import argparse
import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent.parent

CHAINS = [(70, 96, 40), (2, 128, 64), (420, 512, 256, 128)]
BATCH = 17
SEED = 20240607
ACT_ELU = 1


def make_inputs(dims):
    """x and per-layer W, b, gamma, beta from a seeded CPU generator."""
    g = torch.Generator().manual_seed(SEED + sum(dims))
    x = torch.randn(BATCH, dims[0], generator=g)
    layers = []
    for k, n in zip(dims[:-1], dims[1:]):
        W = torch.randn(n, k, generator=g) / k ** 0.5
        b = torch.randn(n, generator=g) * 0.1
        gamma = torch.rand(n, generator=g) + 0.5
        beta = torch.randn(n, generator=g) * 0.1
        layers.append((W, b, gamma, beta))
    return x, layers


def input_digest(x, layers) -> str:
    h = hashlib.sha256()
    h.update(x.numpy().tobytes())
    for tensors in layers:
        for t in tensors:
            h.update(t.numpy().tobytes())
    return h.hexdigest()


def chain_name(dims) -> str:
    return "x".join(str(d) for d in dims)


def run_chain(ext, x, layers, dev):
    cols = list(zip(*[[t.to(dev) for t in lay] for lay in layers]))
    Ws, bs, gs, bes = (list(c) for c in cols)
    return ext.mlp_chain_fwd(x.to(dev), Ws, bs, gs, bes,
                             [ACT_ELU] * len(layers), False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE),
                    help="checkout whose built extension records the golden")
    ap.add_argument("--out", default=str(HERE / "tests" / "golden"
                                         / "chain_fwd_golden.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import smartcal_amd.ops as ops
    dev = torch.device("cuda:0")
    out = {}
    for dims in CHAINS:
        x, layers = make_inputs(dims)
        name = chain_name(dims)
        out[f"{name}/sha256"] = np.array(input_digest(x, layers))
        ys, zhats, rstds = run_chain(ops.ext(), x, layers, dev)
        for l in range(len(layers)):
            out[f"{name}/y{l}"] = ys[l].cpu().numpy()
            out[f"{name}/zhat{l}"] = zhats[l].cpu().numpy()
            out[f"{name}/rstd{l}"] = rstds[l].cpu().numpy()
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, "from", Path(ops.__file__).resolve().parent)


if __name__ == "__main__":
    main()
