"""bench.py --dump-outputs (CPU-only checks of the writer): float32 files, the size budget, and a
sample of an output over budget that is the same on every run."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_dump_writes_every_output_as_float32(bench, tmp_path):
    logits = np.arange(12, dtype=np.float32).reshape(4, 3) / 7
    grad = np.linspace(-1, 1, 50, dtype=np.float32)
    notes = bench.dump_outputs(str(tmp_path / "d"), {"logits": logits, "loss": np.float32([0.5]),
                                                     "flat_grad": grad, "count": np.arange(3),
                                                     "wide": np.float64([1 / 3])})
    assert notes == {}
    assert sorted(os.listdir(tmp_path / "d")) == ["count.npy", "flat_grad.npy", "logits.npy",
                                                  "loss.npy", "wide.npy"]
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in ("logits", "loss", "flat_grad", "count", "wide")}
    assert got["count"].dtype == np.float32 and got["wide"].dtype == np.float64
    np.testing.assert_array_equal(got["logits"], logits)
    np.testing.assert_array_equal(got["flat_grad"], grad)
    assert got["loss"].tolist() == [0.5] and got["wide"].tolist() == [1 / 3]


def test_dump_over_budget_keeps_a_fixed_sample(bench, tmp_path):
    big = np.random.default_rng(5).standard_normal(1000).astype(np.float32)
    small = np.ones(10, dtype=np.float32)
    runs = []
    for d in ("a", "b"):
        notes = bench.dump_outputs(str(tmp_path / d), {"flat_grad": big, "loss": small},
                                   max_bytes=1024, sample=200)
        assert set(notes) == {"flat_grad"}
        runs.append(np.load(tmp_path / d / "flat_grad.npy"))
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) < 1024 + 2 * 128
        np.testing.assert_array_equal(np.load(tmp_path / d / "loss.npy"), small)
    np.testing.assert_array_equal(runs[0], runs[1])
    assert runs[0].shape == (200,)
    idx = np.sort(np.random.default_rng(0).choice(1000, 200, replace=False))
    np.testing.assert_array_equal(runs[0], big[idx])


def test_dump_refuses_more_than_the_budget(bench, tmp_path):
    with pytest.raises(ValueError, match="budget"):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(100, np.float32), "b": np.zeros(100, np.float32)},
                           max_bytes=400, sample=100)
    assert os.listdir(tmp_path) == []


def test_steps_below_one_is_an_error(bench, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--steps" in capsys.readouterr().err
