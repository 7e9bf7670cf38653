"""The Fortran face of the square roots, log-determinants and draws of the curvature model:
examples/qn_draw_dev.f90 drives the built-in quadratic through lbfgsb_module's setulb_dev, then prints log det H,
|H^(1/2) g| and the norm of one draw from N(0, H) (lbfgsb_qn_logdet, lbfgsb_qn_apply with LBFGSB_QN_H_SQRT,
lbfgsb_qn_draw with seed 1, sample 0, no mean) at its last iterate.  The same run through the Python face must give
the same numbers (the device work is the same; only the host's final sums over the n entries are added in another
order)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_draw_dev")
QN = re.compile(r"^QNDRAW col =\s*(\d+)\s+logdetH =\s*(\S+)\s+\|H\^1/2 g\| =\s*(\S+)\s+\|draw\| =\s*(\S+)\s*$")


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
        rg = sol.qn_apply(g, sqrt=True, inverse=True).cpu().numpy()
        d = sol.qn_draw(1, 1, first=0, inverse=True)[0].cpu().numpy()
        return (int(sol.isave[27]), sol.qn_logdet(inverse=True), float(np.sqrt(np.sum(rg * rg))),
                float(np.sqrt(np.sum(d * d))))
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_draw_dev_matches_python(n, m, iters):
    if not os.path.exists(EXE):
        pytest.skip("%s not built (needs amdflang at build time)" % EXE)
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    got = [QN.match(ln.strip()) for ln in r.stdout.splitlines()]
    got = [g for g in got if g]
    assert len(got) == 1, r.stdout[-1500:]
    col = int(got[0].group(1))
    vals = [float(got[0].group(k)) for k in (2, 3, 4)]
    pcol, *pvals = python_path(n, m, iters)
    assert col == pcol == m
    for a, b in zip(vals, pvals):
        assert abs(a - b) <= 1e-12 * abs(b), (vals, pvals)
