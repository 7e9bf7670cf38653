"""bench.py end to end on one GPU at a small shape (n = 1e6, m = 10: BASELINE configs[1], whose reference rows are on
file).  A plain run prints the headline line and nothing that takes a run of its own; --full adds the rooflines and
the in-run parity check after the very same timed steps, so both runs hand the caller the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "1000000", "--steps", "5",
           "--warmup", "12"] + list(args)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs(tmp_path):
    detail = os.path.join(ROOT, "bench_detail.json")
    before = os.path.getmtime(detail) if os.path.exists(detail) else None
    plain = run_bench("--dump-outputs", str(tmp_path / "plain"))
    assert (os.path.getmtime(detail) if os.path.exists(detail) else None) == before   # the line is the whole record
    assert plain["full"] is False and plain["steps"] == 5 and plain["value"] > 0
    assert plain["value"] == pytest.approx(1e3 / plain["ms_per_step"], rel=1e-4)
    assert plain["config"]["n"] == 1_000_000 and plain["warmup_run"] >= 12
    for k in ("roofline", "roofline_wtv", "cpu_baseline", "detail"):
        assert k not in plain, k
    full = run_bench("--full", "--no-cpu-baseline", "--no-live-traffic", "--dump-outputs", str(tmp_path / "full"))
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data"):
        assert full[k] == plain[k], k
    assert full["roofline"]["frac"] > 0 and full["config"]["parity_in_run"]["ok"] is True
    # the same timed steps: the same iterate, gradient and saved state at the last one (fixed-order reductions)
    for name in ("x", "g", "f", "isave", "dsave", "sample_rows"):
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / (name + ".npy")),
                                      np.load(tmp_path / "full" / (name + ".npy")), err_msg=name)
