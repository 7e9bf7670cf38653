"""The Fortran face of the Gram matrices of the curvature model: examples/qn_gram_dev.f90 drives the built-in
quadratic through lbfgsb_module's setulb_dev, draws three samples from N(0, H) at its last iterate (seed 1, samples 0
to 2, no mean, scale 1) and prints their 3 x 3 Gram matrices around their mean under B and under H (lbfgsb_qn_gram).
The same run through the Python face must give the same numbers (the same device work and host arithmetic), at the
tolerance of tests/test_gpu_qn_logpdf_fortran.py: 1e-12 relative, entry by entry."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_gram_dev")
COL = re.compile(r"^QNGRAM col =\s*(\d+)\s*$")
ROW = re.compile(r"^QNGRAM ([BH])\s+(\S+)\s+(\S+)\s+(\S+)\s*$")


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
        d = sol.qn_draw(3, 1, first=0, inverse=True)
        mean = (d[0] + d[1] + d[2]) / 3.0                                  # (the example's order of operations)
        return int(sol.isave[27]), sol.qn_gram(d, center=mean), sol.qn_gram(d, center=mean, inverse=True)
    finally:
        sol.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 10, 14)])
def test_qn_gram_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [int(c.group(1)) for c in map(COL.match, lines) if c]
    rows = [rw for rw in map(ROW.match, lines) if rw]
    assert len(cols) == 1 and len(rows) == 6, r.stdout[-1500:]
    got = {key: np.array([[float(rw.group(j)) for j in (2, 3, 4)] for rw in rows if rw.group(1) == key])
           for key in "BH"}
    pcol, gb, gh = python_path(n, m, iters)
    assert cols[0] == pcol == m
    for key, ref in (("B", gb), ("H", gh)):
        assert got[key].shape == (3, 3)
        print("%s fortran\n%s\npython\n%s" % (key, got[key], ref))
        assert np.array_equal(got[key], got[key].T)
        assert np.all(np.abs(got[key] - ref) <= 1e-12 * np.abs(ref)), key
        # around their mean the three differences add up to zero: so does every row of the matrix, up to rounding
        assert np.all(np.abs(ref.sum(axis=1)) <= 1e-10 * np.abs(ref).sum(axis=1))
