"""The Fortran face of the draws and densities of the model plus a diagonal: examples/qn_shift_draw_dev.f90 drives the
built-in quadratic through lbfgsb_module's setulb_dev to a NEW_X return, pins the rows that lbfgsb_kkt reports at a
bound, adds the prior precision mu = 0.5 (lbfgsb_qn_shift_set) and prints the log-densities of two draws by both routes
(lbfgsb_qn_shift_draw_logpdf; lbfgsb_qn_shift_logpdf at the stored draws), their quadratic forms (lbfgsb_qn_shift_quad)
and the norms of the first draw and of L v, v = 1 (lbfgsb_qn_shift_sqrt).  The same run through the Python face must
give the same numbers to 1e-12 relative, the tolerance of tests/test_gpu_qn_draw_fortran.py (the device work is the
same; only the host's final sums over the n entries are added in another order), and nothing on a pinned row."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_shift_draw_dev")
COL = re.compile(r"^QNSHIFTDRAW col =\s*(\d+)\s+pinned =\s*(\d+)\s*$")
ROW = re.compile(r"^QNSHIFTDRAW (logp|logq|quad|norms)\s+(.*)$")


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
        pin = sol.kkt(x, l, u, nbd, g, 0.0, pg=False, mult=False).status >= 1
        d = torch.zeros(n, dtype=torch.float64, device="cuda")
        d[pin] = float("inf")
        sh = sol.qn_shift(d, 0.5)
        dr, lp = sh.sample(2, 1, log_prob=True)
        lv = sh.sqrt(torch.ones(n, dtype=torch.float64, device="cuda")).cpu().numpy()
        d0 = dr[0].cpu().numpy()
        return (int(sol.isave[27]), sh.pinned, dict(logp=lp, logq=sh.log_prob(dr), quad=sh.quad(dr),
                                                    norms=[np.sqrt(np.sum(d0 * d0)), np.sqrt(np.sum(lv * lv)), 0.0]))
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_shift_draw_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    rows = {t.group(1): [float(v) for v in t.group(2).split()] for t in map(ROW.match, lines) if t}
    assert len(cols) == 1 and sorted(rows) == ["logp", "logq", "norms", "quad"], r.stdout[-1500:]
    pcol, pinned, ref = python_path(n, m, iters)
    assert int(cols[0].group(1)) == pcol == m
    assert int(cols[0].group(2)) == pinned and 0 < pinned < n
    for key, want in ref.items():
        print(key, rows[key], list(want))
        assert len(rows[key]) == len(want)
        for a, b in zip(rows[key], want):
            assert abs(a - b) <= 1e-12 * abs(b), (key, rows[key], list(want))
