"""The Fortran face of the eigen-decomposition of the curvature model: examples/qn_eig_dev.f90 drives the built-in
quadratic through lbfgsb_module's setulb_dev and prints, at its last iterate, the bulk eigenvalue and the
eigenvalues of H (lbfgsb_qn_eig) and, for the eigenvector of the largest one (lbfgsb_qn_eigvec), the residual
|H u - lambda u| with H u from lbfgsb_qn_apply.  The same run through the Python face must give the same eigenvalues
(1e-12 relative, the tolerance of tests/test_gpu_qn_gram_fortran.py), and the printed residual lies below the bound
of tests/test_gpu_qn_root.py::_check_root for H: 1e-10 cond(B) |lambda u|, cond(B) from the Rayleigh quotient of B
on an orthonormal basis of the exported pairs (B is theta I on the complement)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_eig_dev")
COL = re.compile(r"^QNEIG col =\s*(\d+)\s+r =\s*(\d+)\s*$")
BULK = re.compile(r"^QNEIG bulk\s+(\S+)\s*$")
LAM = re.compile(r"^QNEIG lambda\s+(\d+)\s+(\S+)\s*$")
TOP = re.compile(r"^QNEIG top\s+(\S+)\s+(\S+)\s+(\S+)\s*$")


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
        bulk, lam = sol.qn_eig(inverse=True)
        wa, _ = sol.export_state()
        head, col, theta = int(sol.isave[26]), int(sol.isave[27]), float(sol.dsave[0])
        cols = [(head - 1 + j) % m for j in range(col)]
        W = np.concatenate([wa[:m * n].reshape(m, n)[cols], wa[m * n:2 * m * n].reshape(m, n)[cols]]).T
        Q, _ = np.linalg.qr(W)
        Qt = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()
        ev = np.concatenate([[theta], np.linalg.eigvalsh((Qt @ sol.qn_apply(Qt).T).cpu().numpy())])
        return col, bulk, lam, ev.max() / ev.min()
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_eig_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    bulks = [float(b.group(1)) for b in map(BULK.match, lines) if b]
    lams = [float(v.group(2)) for v in map(LAM.match, lines) if v]
    tops = [t for t in map(TOP.match, lines) if t]
    assert len(cols) == 1 and len(bulks) == 1 and len(tops) == 1, r.stdout[-1500:]
    pcol, bulk, lam, cond = python_path(n, m, iters)
    assert int(cols[0].group(1)) == pcol == m and int(cols[0].group(2)) == len(lam) == len(lams)
    assert abs(bulks[0] - bulk) <= 1e-12 * bulk
    assert np.all(np.abs(np.array(lams) - lam) <= 1e-12 * np.abs(lam))
    top, res, unorm = (float(tops[0].group(j)) for j in (1, 2, 3))
    print("top eigenvalue %.16e, |H u - lambda u| = %.3e, |u| = %.16f, cond %.3e" % (top, res, unorm, cond))
    assert top == lams[-1] and abs(unorm - 1.0) <= 1e-10 * cond
    assert res <= 1e-10 * cond * top * unorm
