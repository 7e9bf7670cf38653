"""The Fortran face of the pairs in and out: examples/qn_pairs_dev.f90 drives the built-in quadratic through
lbfgsb_module's setulb_dev to a NEW_X return, reads the stored pairs back on the device (lbfgsb_qn_pairs_get), loads
them into a second context that never runs (lbfgsb_qn_pairs_set), pushes one more pair there (lbfgsb_qn_pairs_push)
and prints the sum and the sum of squares of H g from both contexts.  The same steps through the Python face must
give the same counts and theta exactly and the same checksums within 1e-12 of the sum of |entries| (resp. of the sum
of squares; the tolerance of tests/test_gpu_qn_idx_fortran.py for host results: the two faces add n terms in different
orders), and the model context must reproduce the run's H g to the same tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "qn_pairs_dev")
COL = re.compile(r"^QNPAIRS col =\s*(\d+)\s+theta =\s*(\S+)\s*$")
SUM = re.compile(r"^QNPAIRS (run|model|pushed)\s+(\S+)\s+(\S+)\s*$")
PUSH = re.compile(r"^QNPAIRS stored =\s*(-?\d+)\s+col =\s*(\d+)\s+theta =\s*(\S+)\s*$")


def python_path(n, m, iters):
    import torch
    import lbfgsb_amd as la
    sol, model = la.DeviceSolver(n, m), la.DeviceSolver(n, m)
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
        S, Y, theta = sol.qn_pairs()
        out = dict(col=int(S.shape[0]), theta=theta, run=sol.qn_apply(g, inverse=True).cpu().numpy())
        model.qn_set_pairs(S, Y, theta=theta)
        out["model"] = model.qn_apply(g, inverse=True).cpu().numpy()
        s = torch.from_numpy(1.0 / (1.0 + (np.arange(1, n + 1) % 7))).cuda()
        out["stored"] = model.qn_push_pair(s, 2.0 * s)
        out["col2"], out["theta2"] = int(model.qn_pairs()[0].shape[0]), model.qn_pairs()[2]
        out["pushed"] = model.qn_apply(g, inverse=True).cpu().numpy()
        return out
    finally:
        sol.close(), model.close()


@pytest.mark.parametrize("n,m,iters", [(100000, 5, 12), (20011, 17, 9)])
def test_qn_pairs_dev_matches_python(n, m, iters):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("no Fortran compiler (amdflang): the Fortran face is not built")
    assert os.path.exists(EXE), "%s is missing although amdflang is here: the build of the example failed" % EXE
    r = subprocess.run([EXE, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln.strip() for ln in r.stdout.splitlines()]
    cols = [c for c in map(COL.match, lines) if c]
    push = [c for c in map(PUSH.match, lines) if c]
    sums = {c.group(1): (float(c.group(2)), float(c.group(3))) for c in map(SUM.match, lines) if c}
    assert len(cols) == 1 and len(push) == 1 and set(sums) == {"run", "model", "pushed"}, r.stdout[-1500:]
    py = python_path(n, m, iters)
    assert int(cols[0].group(1)) == py["col"] >= 2 and float(cols[0].group(2)) == py["theta"]
    assert (int(push[0].group(1)), int(push[0].group(2))) == (py["stored"], py["col2"]) == (1, min(m, py["col"] + 1))
    assert float(push[0].group(3)) == py["theta2"] == 2.0
    for key in ("run", "model", "pushed"):
        v = py[key]
        for got, ref, scale in ((sums[key][0], v.sum(), np.abs(v).sum()), (sums[key][1], (v * v).sum(), (v * v).sum())):
            print("%s: Fortran and Python differ by %.2e (scale %.3e)" % (key, abs(got - ref), scale))
            assert abs(got - ref) <= 1e-12 * scale
    err = np.abs(py["model"] - py["run"]).max()
    print("the model context against the run: %.2e (largest entry %.3e)" % (err, np.abs(py["run"]).max()))
    assert err <= 1e-12 * np.abs(py["run"]).max()
    assert np.abs(py["pushed"] - py["model"]).max() > 1e-6 * np.abs(py["model"]).max()  # (the push changed the model)
