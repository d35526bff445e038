"""bench.py command line: --steps, ms_per_step, --dump-outputs, --full."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def test_bench_dump_outputs_cpu(tmp_path):
    """A tiny CPU run writes every output of the last timed step as a
    float32 .npy and reports the steps it really timed."""
    env = dict(os.environ, PYTHONPATH=str(ROOT), CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    out_dir = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps",
         "3", "--warmup", "1", "--full", "--dump-outputs", str(out_dir)],
        cwd=tmp_path, env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines()
                      if l.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / 1000.0 - 1.0) < 1e-6
    shapes = {"action": (2,), "reward": (), "obs_A": (400,),
              "obs_eig": (20,), "solution_x": (20,)}
    nets = ["actor", "critic_1", "critic_2", "target_critic_1",
            "target_critic_2"]
    names = sorted(p.stem for p in out_dir.glob("*.npy"))
    assert names == sorted(list(shapes) + [n + "_params" for n in nets])
    total = 0
    for name in names:
        a = np.load(out_dir / f"{name}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        if name in shapes:
            assert a.reshape(-1).shape == (int(np.prod(shapes[name])),), name
        else:
            assert a.ndim == 1 and a.size > 0, name
        total += a.nbytes
    assert total <= 64 * 2 ** 20
