"""The calibration pipeline CLI with the robust noise model, a uv cut and
simulated interference (tiny config)."""

import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _run(script, *args, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    return subprocess.run([sys.executable, str(ROOT / script), *args],
                          cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=600)


def test_bench_robust_help(tmp_path):
    r = _run("scripts/calibration/bench_robust.py", "--help", cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]


def test_calibration_pipeline_robust_tiny(tmp_path):
    r = _run("scripts/calibration/pipeline.py", "--robust", "--rfi", "0.05",
             "--stations", "8", "--nf", "2", "--K", "2", "--ts", "1",
             "--tdelta", "4", "--admm", "2", "--poly", "2", "--uvmin", "30",
             "--nulow", "2", "--nuhigh", "30", cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[rfi]" in r.stdout and "[weights]" in r.stdout
    assert "nu [" in r.stdout
    assert (tmp_path / "influenceI.npy").exists()
