"""The Fortran face of the quadratic forms and log-densities of the curvature model: examples/qn_logpdf_dev.f90
drives the built-in quadratic through lbfgsb_module's setulb_dev, then prints the log-densities of two draws from
N(0, H) at its last iterate twice: from lbfgsb_qn_draw_logpdf (seed 1, samples 0 and 1, no mean, scale 1) and from
lbfgsb_qn_logpdf at the two stored draws.  The same run through the Python face must give the same numbers (the same
device work and host arithmetic), and the two routes must agree within qn_logpdf's tolerance of
tests/test_gpu_qn_quad.py, 1/2 1e-10 (|B|_2 |d|^2 + n) at scale 1, d the stored draw.  |B|_2 without the dense model:
B maps the span of the stored pairs into itself and is theta I on its complement, so its largest eigenvalue is the
larger of theta and that of Q'BQ, Q an orthonormal basis of the span (as _cond_and_norm of the root tests)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_logpdf_dev")
QN = re.compile(r"^QNLOGPDF col =\s*(\d+)\s+draw =\s*(\S+)\s+(\S+)\s+at =\s*(\S+)\s+(\S+)\s*$")


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
        d, lp = sol.qn_draw(2, 1, first=0, inverse=True, return_logpdf=True)
        at = sol.qn_logpdf(d, inverse=True)
        wa, _ = sol.export_state()
        Q, _ = np.linalg.qr(wa[:2 * m * n].reshape(2 * m, n).T)          # the ring is full: every column is a pair's
        BQ = sol.qn_apply(torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()).cpu().numpy()
        nb = max(float(sol.dsave[0]), float(np.linalg.eigvalsh(0.5 * (BQ @ Q + (BQ @ Q).T)).max()))
        tol = 0.5 * 1e-10 * (nb * (d * d).sum(dim=1).cpu().numpy() + n)
        return int(sol.isave[27]), [float(v) for v in lp] + [float(v) for v in at], tol
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_logpdf_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    got = [QN.match(ln.strip()) for ln in r.stdout.splitlines()]
    got = [g for g in got if g]
    assert len(got) == 1, r.stdout[-1500:]
    col = int(got[0].group(1))
    vals = [float(got[0].group(k)) for k in (2, 3, 4, 5)]
    pcol, pvals, tol = python_path(n, m, iters)
    assert col == pcol == m
    print("fortran %s\npython  %s" % (vals, pvals))
    for a, b in zip(vals, pvals):
        assert abs(a - b) <= 1e-12 * abs(b), (vals, pvals)
    for j in range(2):  # the two routes
        print("draw %d: |the two routes| = %.3e (tolerance %.3e)" % (j, abs(vals[j] - vals[2 + j]), tol[j]))
        assert abs(vals[j] - vals[2 + j]) <= tol[j], (j, vals)
