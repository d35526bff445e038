"""The sky-prediction kernels (coherency_kernel, coherency_beam_kernel,
station_beam_kernel, shapelet_kernel, shapelet_beam_kernel) against
tests/golden/sky_predict_golden.npz, recorded by
scripts/record_sky_golden.py before the kernels came to share one
source-term body: same input tables, every output bit for bit. And a
launch of nothing leaves no error behind (GPU)."""

import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "sky_predict_golden.npz"


def _load_recorder():
    spec = importlib.util.spec_from_file_location(
        "record_sky_golden", ROOT / "scripts" / "record_sky_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    return _load_recorder()


@pytest.fixture(scope="module")
def scenario(rec):
    return rec.make_scenario()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_scenario_reaches_every_edge(rec, scenario):
    sky, clusters, beam, uvw = scenario
    inputs = rec.kernel_inputs(sky, clusters, uvw, torch.device("cuda:0"))
    src, off, hdr = inputs[0], inputs[1], inputs[2]
    assert off.tolist() == [0, 130, 132, 132]      # chunk of 128 crossed;
    assert src[129, 4] == 1.0                      # empty point table last
    assert int(src[:130, 4].sum()) == 44
    assert sorted(hdr[:2, 11].tolist()) == [4.0, 7.0]
    assert hdr[2, 3] == 0.0 and hdr[2, 4] != 0.0   # sI = 0, sQ ≠ 0
    assert beam.elem_uvw.shape == (2, 24, 7, 3)
    assert uvw.shape == (2 * 276, 3)


def test_kernel_inputs_match_the_recorded_digest(rec, scenario, gold):
    sky, clusters, _, uvw = scenario
    inputs = rec.kernel_inputs(sky, clusters, uvw, torch.device("cuda:0"))
    # a changed table build fails here; it never skips
    assert rec.digest(*inputs) == str(gold["inputs/sha256"])


def test_station_beam_table_matches_recorded_golden(rec, scenario, gold):
    from smartcal_amd.ops import ext
    sky, clusters, beam, uvw = scenario
    dev = torch.device("cuda:0")
    inputs = rec.kernel_inputs(sky, clusters, uvw, dev)
    E = rec.beam_table(ext(), beam, inputs, dev)
    assert E.shape == (2, 135, 24)
    assert rec.digest(E.cpu().numpy()) == str(gold["E/sha256"])


@pytest.mark.parametrize("case", ["plain", "plain_smear", "beam",
                                  "beam_smear"])
def test_prediction_matches_recorded_golden(case, rec, scenario, gold):
    name, with_beam, smear_bw = next(c for c in rec.CASES if c[0] == case)
    sky, clusters, beam, uvw = scenario
    C = rec.run_case(sky, clusters, beam, uvw, torch.device("cuda:0"),
                     with_beam, smear_bw).cpu()
    assert C.shape == (3, 552, 4) and C.dtype == torch.complex64
    if f"{name}/C" in gold.files:
        want = torch.from_numpy(gold[f"{name}/C"])
        diff = torch.view_as_real(C) != torch.view_as_real(want)
        print(f"{name}: {int(diff.sum())} of {diff.numel()} floats differ, "
              f"max |Δ| {float((C - want).abs().max()):.3e}")
        assert torch.equal(C, want), name
    assert rec.digest(C.numpy()) == str(gold[f"{name}/sha256"]), name


def test_empty_launch_leaves_no_error_behind():
    from smartcal_amd.ops import ext
    dev = torch.device("cuda:0")
    src = torch.zeros(1, 11, dtype=torch.float64, device=dev)
    src[0, 3] = 1.0
    off = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    C = ext().coherency_predict(
        torch.zeros(0, 3, dtype=torch.float64, device=dev), src, off, 0.0)
    assert C.shape == (1, 0, 4) and C.dtype == torch.complex64
    # the next binding that reads the launch status must find it clean
    E = ext().station_beam(
        torch.zeros(1, 3, 1, 3, dtype=torch.float64, device=dev),
        torch.tensor([[0.01, -0.02, -2.5e-4]], dtype=torch.float64,
                     device=dev), 3.0)
    assert E.shape == (1, 1, 3)
    assert torch.equal(E.cpu(), torch.ones(1, 1, 3, dtype=torch.complex128))
