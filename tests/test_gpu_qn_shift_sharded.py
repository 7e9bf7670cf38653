"""The model plus a diagonal on sharded contexts: 2 and 3 rank processes on one GPU (a gloo host group, or the
library's communicator path with the shared-memory RCCL stand-in of tests/fake_rccl.cpp), n = 4099 split unevenly,
m = 10, every third row pinned and a run of 40 pinned rows across every rank boundary.  log det and the pinned count
are the same bits on every rank, and the concatenated solves and diagonals are within 1e-12 (relative, in the 2-norm)
of ONE context's that imported the concatenated state."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,mode,iters", [(2, "gloo", 14), (3, "fakerccl", 13)])
def test_sharded_shift(oracle_built, tmp_path, monkeypatch, world, mode, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_shift_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m = 4099, 10
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_shift_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qnshift"))
    assert len({int(p["n_loc"]) for p in parts}) == world                # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m
    d = wk.shift(n, world)
    for r in range(1, world):                                             # pins on both sides of every boundary
        e = wk.cut(n, world, r)[0]
        assert np.isinf(d[e - 1]) and np.isinf(d[e])
    for tag in ("s0", "s1"):
        for key in ("_logdet", "_pinned"):
            assert len({p[tag + key].tobytes() for p in parts}) == 1, tag + key   # the same bits on every rank
        assert int(parts[0][tag + "_pinned"]) == int(np.isinf(d).sum())

    rng = np.random.default_rng(wk.SEED)
    V = torch.from_numpy(rng.standard_normal((wk.K, n))).cuda()
    dt = torch.from_numpy(d).cuda()

    def close(tag, sh):
        x = np.concatenate([p[tag + "_x"] for p in parts], axis=1)
        dg = np.concatenate([p[tag + "_diag"] for p in parts])
        ref_x, ref_d, ref_l = sh.solve(V).cpu().numpy(), sh.diag().cpu().numpy(), sh.logdet()
        ex = np.linalg.norm(x - ref_x) / np.linalg.norm(ref_x)
        ed = np.linalg.norm(dg - ref_d) / np.linalg.norm(ref_d)
        el = abs(float(parts[0][tag + "_logdet"]) - ref_l) / abs(ref_l)
        print("%s: sharded against one rank: solve %.2e, diag %.2e, log det %.2e (relative)" % (tag, ex, ed, el))
        assert ex <= 1e-12 and ed <= 1e-12 and el <= 1e-12
        assert np.all(x[:, np.isinf(d)] == 0.0) and np.all(dg[np.isinf(d)] == 0.0)
        assert sh.pinned == int(parts[0][tag + "_pinned"])

    with one_context(n, m) as one:
        close("s0", one.qn_shift(dt, wk.MU))
        import_glued(one, parts, n, m)
        close("s1", one.qn_shift(dt, wk.MU))
