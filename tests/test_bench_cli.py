"""bench.py's command line (no GPU): --full / --dump-outputs are there, --steps
is validated, and the dumped MSM result reads back exactly."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_is_exact(tmp_path):
    rng = np.random.default_rng(5)
    out = rng.integers(0, 1 << 63, size=12, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # high bit and low bit set
    bench.dump_outputs(str(tmp_path / "d"), 0, out)
    bench.dump_outputs(str(tmp_path / "d"), 3, out)
    w = np.load(tmp_path / "d" / "msm_out.npy")
    assert w.dtype == np.float64 and w.shape == (24,)
    back = w.astype(np.uint64)
    assert np.array_equal(back[0::2] | (back[1::2] << np.uint64(32)), out)
    assert np.array_equal(np.load(tmp_path / "d" / "msm_out_rank3.npy"), w)
