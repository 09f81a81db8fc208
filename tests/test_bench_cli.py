"""bench.py's own plumbing, without a GPU: the --dump-outputs writer and the command line."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _arrays():
    rng = np.random.RandomState(3)
    return {"losses": np.asarray([0.5, -1.25, 2.0, 3.5]), "G_params": rng.rand(1000).astype(np.float32),
            "frames": rng.rand(2, 3, 64, 64).astype(np.float32), "mask": np.arange(12, dtype=np.int32)}


def test_dump_outputs_whole_arrays_under_the_budget(tmp_path):
    a = _arrays()
    bench.dump_outputs(str(tmp_path), a)
    assert sorted(os.listdir(tmp_path)) == ["G_params.npy", "frames.npy", "losses.npy", "mask.npy"]
    for name, v in a.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == (np.float64 if v.dtype == np.float64 else np.float32)
        assert np.array_equal(got, v.astype(got.dtype))


def test_dump_outputs_samples_large_arrays_within_the_budget_and_repeatably(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 16 * 1024)
    a = _arrays()
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), a)
    total = sum(os.path.getsize(tmp_path / "one" / f) - 128 for f in os.listdir(tmp_path / "one"))     # less the .npy headers
    assert total <= 16 * 1024
    assert np.array_equal(np.load(tmp_path / "one" / "losses.npy"), a["losses"])                  # small arrays stay whole
    assert np.array_equal(np.load(tmp_path / "one" / "G_params.npy"), a["G_params"])
    frames = np.load(tmp_path / "one" / "frames.npy")
    assert 0 < frames.size < a["frames"].size and np.isin(frames, a["frames"]).all()                  # a sample of the elements
    for f in os.listdir(tmp_path / "one"):
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))          # the same sample every run


def test_command_line_has_full_and_dump_outputs_and_checks_steps():
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
