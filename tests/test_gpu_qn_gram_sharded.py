"""Gram matrices of the curvature model on sharded contexts: 2 and 3 rank processes on one GPU (a gloo host group, or
the library's communicator path with the shared-memory RCCL stand-in of tests/fake_rccl.cpp), n = 1000 split
unevenly, m = 17 (two column tiles, pieces of at most 2 vectors), k = 5 (pieces 2 + 2 + 1: three cross launches).
Every rank gets the same bits, and every entry is within 1e-12 |d_a|_A |d_b|_A of ONE context's that imported the
concatenated state."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,mode,iters", [(2, "gloo", 21), (3, "fakerccl", 20)])
def test_sharded_gram(oracle_built, tmp_path, monkeypatch, world, mode, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_gram_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m = 1000, 17
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_gram_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qngram"))
    assert len({int(p["n_loc"]) for p in parts}) == world                # an uneven split
    assert [int(p["row0"]) for p in parts] == [wk.cut(n, world, r)[0] for r in range(world)]
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m
    for key in ("g0", "gb", "gh", "gn"):
        assert len({p[key].tobytes() for p in parts}) == 1, key            # the same bits on every rank
        assert parts[0][key].shape == (wk.K, wk.K) and np.array_equal(parts[0][key], parts[0][key].T)
    got = parts[0]

    rng = np.random.default_rng(wk.SEED)
    cen = torch.from_numpy(rng.standard_normal(n)).cuda()
    V = torch.from_numpy(rng.standard_normal((wk.K, n))).cuda()

    def close(name, a, b):
        na = np.sqrt(np.diag(b))
        tol = 1e-12 * np.outer(na, na)
        err = np.abs(a - b)
        print("%s: max |sharded - one rank| / (1e-12 |d_a|_A |d_b|_A) = %.3e" % (name, (err / tol).max()))
        assert np.all(err <= tol), name

    with one_context(n, m) as one:
        close("g0", got["g0"], one.qn_gram(V, center=cen))
        import_glued(one, parts, n, m)
        close("gb", got["gb"], one.qn_gram(V, center=cen))
        close("gh", got["gh"], one.qn_gram(V, center=cen, inverse=True))
        close("gn", got["gn"], one.qn_gram(V, inverse=True))
