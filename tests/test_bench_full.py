"""bench.py without and with --full: a plain run measures the headline alone and leaves every
secondary figure null; --full measures them as well."""
import importlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


@pytest.fixture
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_full_is_off_by_default(bench):
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def run_bench(*args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2"] + list(args)
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert all(out[k] is not None for k in HEADLINE)
    assert out["value"] > 0 and out["steps"] == 5 and out["warmup"] == 2
    return out


@pytest.mark.gpu
def test_plain_run_measures_the_headline_alone():
    out = run_bench()
    assert out["with_optimizer"] is None and out["cpu_baseline"] is None
    roof = out["roofline"]
    assert roof["kernels"] is None and roof["dominant_kernel"] is None
    assert roof["copy_peak_GBps_measured_here"] is None
    assert roof["gpu_ms_per_step_hip_events"] > 0
    assert "optimizer" not in out["legs"] and "reported with --full" in out["legs"]


@pytest.mark.gpu
def test_full_run_adds_the_secondary_figures():
    out = run_bench("--full", "--no-cpu-baseline")
    assert out["with_optimizer"]["ms_per_step"] > 0
    assert out["cpu_baseline"] is None                # --no-cpu-baseline
    roof = out["roofline"]
    assert roof["kernels"] and roof["dominant_kernel"] in roof["kernels"]
    assert roof["copy_peak_GBps_measured_here"] > 0
    assert "optimizer" in out["legs"] and "reported with --full" not in out["legs"]
