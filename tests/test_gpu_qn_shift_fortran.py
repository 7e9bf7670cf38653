"""The Fortran face of the model plus a diagonal: examples/qn_shift_dev.f90 drives the built-in quadratic through
lbfgsb_module's setulb_dev to a NEW_X return, pins the rows that lbfgsb_kkt reports at a bound
(lbfgsb_qn_shift_set) and prints log det of the model on the free rows (lbfgsb_qn_shift_logdet) and the residual
|B x - v| over the free rows of x = lbfgsb_qn_shift_solve(v), v = 1, with B x from lbfgsb_qn_apply.  The same run
through the Python face must give the same pinned count and log det (1e-12 relative, the tolerance of
tests/test_gpu_qn_eig_fortran.py) and the same residual up to its bound, 1e-10 cond(B) |v_F| -- cond(B) from the
Rayleigh quotient of B on an orthonormal basis of the exported pairs (B is theta I on the complement); the free block
of B is no worse conditioned than B."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_shift_dev")
COL = re.compile(r"^QNSHIFT col =\s*(\d+)\s+pinned =\s*(\d+)\s*$")
LOGDET = re.compile(r"^QNSHIFT logdet\s+(\S+)\s*$")
RES = re.compile(r"^QNSHIFT residual\s+(\S+)\s+(\S+)\s+(\S+)\s*$")


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
        v = torch.ones(n, dtype=torch.float64, device="cuda")
        xs = sh.solve(v)
        r = (sol.qn_apply(xs) - v)[~pin]
        wa, _ = sol.export_state()
        head, col, theta = int(sol.isave[26]), int(sol.isave[27]), float(sol.dsave[0])
        cols = [(head - 1 + j) % m for j in range(col)]
        W = np.concatenate([wa[:m * n].reshape(m, n)[cols], wa[m * n:2 * m * n].reshape(m, n)[cols]]).T
        Q, _ = np.linalg.qr(W)
        Qt = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()
        ev = np.concatenate([[theta], np.linalg.eigvalsh((Qt @ sol.qn_apply(Qt).T).cpu().numpy())])
        return col, sh.pinned, int(pin.sum().item()), sh.logdet(), torch.linalg.norm(r).item(), ev.max() / ev.min()
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_shift_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    lds = [float(v.group(1)) for v in map(LOGDET.match, lines) if v]
    ress = [t for t in map(RES.match, lines) if t]
    assert len(cols) == 1 and len(lds) == 1 and len(ress) == 1, r.stdout[-1500:]
    pcol, pinned, npin, logdet, pres, cond = python_path(n, m, iters)
    assert int(cols[0].group(1)) == pcol == m
    assert int(cols[0].group(2)) == pinned == npin and 0 < pinned < n
    assert abs(lds[0] - logdet) <= 1e-12 * abs(logdet)
    res, vnorm, xpin = (float(ress[0].group(j)) for j in (1, 2, 3))
    bound = 1e-10 * cond * vnorm
    print("log det %.16e (Python %.16e), |B x - v| on the free rows %.3e (Python %.3e, bound %.3e), cond %.3e"
          % (lds[0], logdet, res, pres, bound, cond))
    assert vnorm == np.sqrt(n - pinned) and xpin == 0.0
    assert res <= bound and pres <= bound
