"""Log-determinants, draws and square roots of the curvature model on sharded contexts: 2 and 3 rank processes on
one GPU (a gloo host group, or the library's communicator path with the shared-memory RCCL stand-in of
tests/fake_rccl.cpp), n = 4099 split unevenly.  log det is the same number on every rank; the concatenated draws
equal the draws of ONE context that imported the concatenated state -- a draw is a function of (seed, global row,
sample), not of the sharding -- and are bit-identical while no pair is stored."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,mode,m,iters", [(2, "gloo", 7, 10), (3, "fakerccl", 5, 9)])
def test_sharded_logdet_and_draws(oracle_built, tmp_path, monkeypatch, world, mode, m, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_root_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n = 4099
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_root_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qnroot"))
    assert len({int(p["n_loc"]) for p in parts}) > 1                       # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m and int(parts[0]["head"]) > 1          # a full ring whose head has wrapped
    for key in ("ldb", "ldh", "ld0"):
        assert len({float(p[key]) for p in parts}) == 1, key               # the same bits on every rank
    assert float(parts[0]["ld0"]) == 0.0                                    # no pair, theta = 1

    rng = np.random.default_rng(17)
    mean = torch.from_numpy(rng.standard_normal(n)).cuda()
    V = torch.from_numpy(rng.standard_normal((3, n))).cuda()
    with one_context(n, m) as one:
        d0 =one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE).cpu().numpy()
        assert np.array_equal(np.concatenate([p["d0"] for p in parts], axis=1), d0)   # bit-identical at col = 0
        import_glued(one, parts, n, m)
        ldb, ldh = one.qn_logdet(), one.qn_logdet(inverse=True)
        print("log det B: sharded %.16e, one rank %.16e" % (float(parts[0]["ldb"]), ldb))
        assert abs(float(parts[0]["ldb"]) - ldb) <= 1e-12 * abs(ldb)
        assert abs(float(parts[0]["ldh"]) - ldh) <= 1e-12 * abs(ldh)
        for key, inverse in (("db", False), ("dh", True)):
            ref = one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE, inverse=inverse).cpu().numpy()
            got = np.concatenate([p[key] for p in parts], axis=1)
            err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            print("%s: |sharded - one rank| / |one rank| = %.3e" % (key, err))
            assert err <= 1e-12
        ref = one.qn_apply(V, sqrt=True, inverse=True).cpu().numpy()
        got = np.concatenate([p["rh"] for p in parts], axis=1)
        assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
