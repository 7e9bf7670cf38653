"""The Fortran face of the model over a range of shifts: examples/qn_path_dev.f90 drives the built-in quadratic
through lbfgsb_module's setulb_dev to a NEW_X return, pins the rows that lbfgsb_kkt reports at a bound
(lbfgsb_qn_path_set) and prints the curve log det (B_FF + mu I) at five shifts (lbfgsb_qn_path_logdet), the length of
the Newton step of the free variables (lbfgsb_qn_path_solve, scalars alone) and the trust-region step of the gradient
at half that length (lbfgsb_qn_path_trust) with the step's checksums.  The same run through the Python face makes
the same calls on the same data, so every printed number must come back to its 17 printed digits: the passes are
deterministic (fixed grids, fixed order of the partial sums) and the host algebra is the same code."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_path_dev")
COL = re.compile(r"^QNPATH col =\s*(\d+)\s+pinned =\s*(\d+)\s*$")
LOGDET = re.compile(r"^QNPATH logdet\s+(\S+)\s+(\S+)\s+(\d+)\s*$")
NEWTON = re.compile(r"^QNPATH newton\s+(\S+)\s+(\S+)\s*$")
TRUST = re.compile(r"^QNPATH trust\s+(\S+)\s+(\S+)\s+(\S+)\s+(\d+)\s+(\d+)\s*$")
STEP = re.compile(r"^QNPATH step\s+(\S+)\s+(\S+)\s+(\S+)\s*$")
MUS = [0.0, 0.1, 1.0, 10.0, 100.0]


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
        path = sol.qn_path(status)
        ld, info = path.logdet(MUS)
        _, n2, vx = path.solve(g, [0.0], out=False, norms=True)
        tr = path.trust(g, 0.5 * float(np.sqrt(n2[0])))
        step = tr.step.cpu().numpy()
        pin = (status >= 1).cpu().numpy()
        # the example's sums run in index order, in double
        ssum = sabs = 0.0
        for v in step.tolist():
            ssum += v
            sabs += abs(v)
        return dict(col=int(sol.isave[27]), pinned=path.pinned, npin=int(pin.sum()), ld=ld, info=info,
                    newton=(float(np.sqrt(n2[0])), float(vx[0])), tr=tr, ssum=ssum, sabs=sabs,
                    spin=float(np.abs(step[pin]).max()) if pin.any() else 0.0)
    finally:
        sol.close()


def test_qn_path_dev_matches_python():
    n, m, iters = 1000, 5, 12
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    lds = [v for v in map(LOGDET.match, lines) if v]
    nws = [v for v in map(NEWTON.match, lines) if v]
    trs = [v for v in map(TRUST.match, lines) if v]
    sts = [v for v in map(STEP.match, lines) if v]
    assert len(cols) == 1 and len(lds) == 5 and len(nws) == 1 and len(trs) == 1 and len(sts) == 1, r.stdout[-1500:]
    p = python_path(n, m, iters)
    assert int(cols[0].group(1)) == p["col"] == m
    assert int(cols[0].group(2)) == p["pinned"] == p["npin"] and 0 < p["pinned"] < n
    fmt = lambda v: float("%.16e" % v)  # noqa: E731  (what the example prints of a double)
    for j, v in enumerate(lds):
        assert float(v.group(1)) == MUS[j] and int(v.group(3)) == int(p["info"][j]) == 0
        assert float(v.group(2)) == fmt(p["ld"][j]), (j, v.group(2), p["ld"][j])
    assert np.all(np.diff(p["ld"]) > 0)
    assert (float(nws[0].group(1)), float(nws[0].group(2))) == (fmt(p["newton"][0]), fmt(p["newton"][1]))
    tr = p["tr"]
    assert [float(trs[0].group(j)) for j in (1, 2, 3)] == [fmt(tr.mu), fmt(tr.norm), fmt(tr.predicted)]
    assert int(trs[0].group(4)) == int(tr.on_boundary) == 1 and int(trs[0].group(5)) == tr.iters
    assert [float(sts[0].group(j)) for j in (1, 2, 3)] == [fmt(p["ssum"]), fmt(p["sabs"]), 0.0] and p["spin"] == 0.0
    print("log det curve %s, trust mu %.6e, ||step|| %.6e, predicted %.6e in %d evaluations"
          % (np.array2string(p["ld"], precision=6), tr.mu, tr.norm, tr.predicted, tr.iters))
