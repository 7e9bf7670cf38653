"""The Fortran face of the curvature-model operator: examples/qn_dev.f90 drives the built-in quadratic through
lbfgsb_module's setulb_dev, then prints |H g| and sum diag(H) from lbfgsb_qn_apply / lbfgsb_qn_diag at its last
iterate.  The same run through the Python face must give the same numbers (the device work is the same; only the
host's final sums over the n entries are added in another order)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_dev")
QN = re.compile(r"^QN col =\s*(\d+)\s+\|Hg\| =\s*(\S+)\s+sum diag\(H\) =\s*(\S+)\s*$")


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
        hg = sol.qn_apply(g, inverse=True).cpu().numpy()
        dh = sol.qn_diag(inverse=True).cpu().numpy()
        return int(sol.isave[27]), float(np.sqrt(np.sum(hg * hg))), float(np.sum(dh))
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_dev_matches_python(n, m, iters):
    if not os.path.exists(EXE):
        pytest.skip("%s not built (needs amdflang at build time)" % EXE)
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    got = [QN.match(ln.strip()) for ln in r.stdout.splitlines()]
    got = [g for g in got if g]
    assert len(got) == 1, r.stdout[-1500:]
    col, hg, ds = int(got[0].group(1)), float(got[0].group(2)), float(got[0].group(3))
    pcol, phg, pds = python_path(n, m, iters)
    assert col == pcol == m
    assert abs(hg - phg) <= 1e-12 * abs(phg), (hg, phg)
    assert abs(ds - pds) <= 1e-12 * abs(pds), (ds, pds)
