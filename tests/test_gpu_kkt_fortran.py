"""The Fortran face of the active-set report: examples/kkt_dev.f90 solves the reference's first driver problem on
device buffers through lbfgsb_module's setulb_dev, then prints the summary of lbfgsb_kkt and the first indices of
lbfgsb_kkt_list at the solution.  The same run through the Python face gives the same numbers: the device work is
the same."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "kkt_dev")


def python_path(n, m, iters):
    import torch
    import lbfgsb_amd as la
    from oracle import pyoracle as po
    p = po.problem_rosenbrock(n, m)  # (driver1's problem and tolerances)
    sol = la.DeviceSolver(n, m)
    try:
        x = torch.from_numpy(p.x0.copy()).cuda()
        g = torch.zeros_like(x)
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        while True:
            t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(1, x, g)
            elif not t.startswith("NEW_X") or (iters > 0 and sol.isave[29] >= iters):
                break
        rep = sol.kkt(x, l, u, nbd, g, tol=p.pgtol, pg=False)
        idx = sol.kkt_indices(rep.status, (1, 2, 3)).cpu().numpy()
        return t, rep, idx
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(25, 5, 0), (25, 5, 11), (1000, 7, 8)])
def test_kkt_dev_matches_python(n, m, iters):
    """iters = 0: to convergence (at n = 25 driver1's solution is interior: an empty list); iters > 0: an iterate on
    the way at which the CPU oracle's run of the same problem has variables on their lower bound (3 of 25 at
    iterate 11; 496 of 1000 at iterate 8)"""
    if not os.path.exists(EXE):
        pytest.skip("%s not built (needs amdflang at build time)" % EXE)
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = {k: v for k, v in re.findall(r"^\s*(KKT \w+|task) =(.*)$", r.stdout, re.M)}
    assert set(lines) == {"KKT counts", "KKT values", "KKT active", "task"}, r.stdout[-1500:]
    counts = [int(v) for v in lines["KKT counts"].split()]
    values = [float(v) for v in lines["KKT values"].split()]
    nact, shown = lines["KKT active"].split(":")
    shown = [int(v) for v in shown.split()]
    task, rep, idx = python_path(n, m, iters)
    assert lines["task"].strip() == task and task.startswith("NEW_X" if iters else "CONVERGENCE"), (lines["task"], task)
    assert counts == rep.counts.tolist(), (counts, rep)
    assert values == rep.values.tolist(), (values, rep)     # (es24.16 round-trips a double)
    assert int(nact) == idx.size == rep.n_lower + rep.n_upper + rep.n_fixed
    if iters:
        assert idx.size > 0, rep
    assert shown == idx[:8].tolist()
    assert rep.n_outside == 0 and sum(counts[:5]) == n
