"""The Fortran face of the entries at index lists: examples/qn_idx_dev.f90 drives the built-in quadratic through
lbfgsb_module's setulb_dev to a NEW_X return, pins the rows that lbfgsb_kkt reports at a bound and prints the 3 x 3
marginal covariance and correlations at three free rows, from the plain model (lbfgsb_qn_block, H) and from the model
pinned at the active rows (lbfgsb_qn_shift_block), the largest gathered entry of the pairs (lbfgsb_qn_rows) and the
distance of the columns at the indices (lbfgsb_qn_cols, lbfgsb_qn_shift_cols) from the blocks.  The same run through
the Python face must give the same indices and the same matrices (1e-12 relative to the largest entry, the tolerance
of tests/test_gpu_qn_shift_fortran.py for host results); the columns' entries at the indices are the blocks' within
1e-12 of the largest entry (the two are summed in different orders)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_idx_dev")
COL = re.compile(r"^QNIDX col =\s*(\d+)\s+pinned =\s*(\d+)\s*$")
IDX = re.compile(r"^QNIDX idx\s+(\d+)\s+(\d+)\s+(\d+)\s*$")
MAT = re.compile(r"^QNIDX (H|Hcorr|S|Scorr)\s+(\d)\s+(\S+)\s+(\S+)\s+(\S+)\s*$")
ROWS = re.compile(r"^QNIDX rows\s+(\S+)\s*$")
COLS = re.compile(r"^QNIDX cols\s+(\S+)\s+(\S+)\s*$")


def python_path(n, m, iters):
    import torch
    import lbfgsb_amd as la
    sol = la.DeviceSolver(n, m)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        while True:
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif t.startswith("NEW_X") and sol.isave[29] < iters:
                continue
            else:
                break
        assert t.startswith("NEW_X"), t
        status = sol.kkt(x, l, u, nbd, g, 0.0, pg=False, mult=False).status
        pin = status >= 1
        d = torch.zeros(n, dtype=torch.float64, device="cuda")
        d[pin] = float("inf")
        sh = sol.qn_shift(d)
        # the recipe of INTEGRATION.md: the free rows as kkt_indices hands them out, three of them
        free = sol.kkt_indices(status, (-1, 0)).cpu().numpy()
        idx = np.array([free[0], free[free >= n // 2][0], free[-1]], np.int64)
        op = sol.qn_operator(inverse=True)
        mats = {"H": op.marginal(idx), "S": sh.block(idx)}
        for key in ("H", "S"):
            sd = np.sqrt(np.diag(mats[key]))
            mats[key + "corr"] = mats[key] / np.outer(sd, sd)
        rmax = np.abs(sol.qn_rows(idx)).max()
        return int(sol.isave[27]), sh.pinned, idx, mats, rmax
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_idx_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    idxs = [c for c in map(IDX.match, lines) if c]
    rows = [c for c in map(ROWS.match, lines) if c]
    dist = [c for c in map(COLS.match, lines) if c]
    assert len(cols) == 1 and len(idxs) == 1 and len(rows) == 1 and len(dist) == 1, r.stdout[-1500:]
    got = {k: np.full((3, 3), np.nan) for k in ("H", "Hcorr", "S", "Scorr")}
    for mt in filter(None, map(MAT.match, lines)):
        got[mt.group(1)][int(mt.group(2)) - 1] = [float(mt.group(j)) for j in (3, 4, 5)]
    pcol, pinned, idx, mats, rmax = python_path(n, m, iters)
    assert int(cols[0].group(1)) == pcol == m
    assert int(cols[0].group(2)) == pinned and 0 < pinned < n
    assert [int(idxs[0].group(j)) for j in (1, 2, 3)] == list(idx)
    for key in ("H", "Hcorr", "S", "Scorr"):
        err, scale = np.abs(got[key] - mats[key]).max(), np.abs(mats[key]).max()
        print("%s: Fortran and Python differ by %.2e (largest entry %.3e)" % (key, err, scale))
        assert np.isfinite(got[key]).all() and err <= 1e-12 * scale
        assert np.array_equal(got[key], got[key].T)
    assert np.all(np.diag(got["H"]) > 0.0) and np.all(np.diag(got["S"]) > 0.0)
    assert np.array_equal(np.diag(got["Hcorr"]), np.ones(3)) or np.abs(np.diag(got["Hcorr"]) - 1.0).max() <= 4e-16
    assert abs(float(rows[0].group(1)) - rmax) <= 1e-12 * rmax and rmax > 0.0
    ch, cs = float(dist[0].group(1)), float(dist[0].group(2))
    print("columns against blocks: %.2e (H), %.2e (pinned model)" % (ch, cs))
    assert ch <= 1e-12 * np.abs(mats["H"]).max() and cs <= 1e-12 * np.abs(mats["S"]).max()
