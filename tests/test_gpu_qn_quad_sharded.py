"""Quadratic forms and Gaussian log-densities of the curvature model on sharded contexts: 2 and 3 rank processes on
one GPU (a gloo host group, or the library's communicator path with the shared-memory RCCL stand-in of
tests/fake_rccl.cpp), n = 4099 split unevenly, m = 10.  Every rank gets the same bits; the values are within 1e-10
relative of ONE context's that imported the concatenated state; z'z of a draw does not depend on the sharding to that
bound, and the concatenated draws equal the single context's (bit for bit while no pair is stored)."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOG2PI = float(np.log(2.0 * np.pi))


def _zz(lp, n, scale, logdet):
    return -2.0 * lp - (n * LOG2PI + 2.0 * n * np.log(abs(scale)) + logdet)


@pytest.mark.parametrize("world,mode,iters", [(2, "gloo", 14), (3, "fakerccl", 13)])
def test_sharded_quad_and_logpdf(oracle_built, tmp_path, monkeypatch, world, mode, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_quad_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m = 4099, 10
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_quad_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qnquad"))
    assert len({int(p["n_loc"]) for p in parts}) > 1                       # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m and int(parts[0]["head"]) > 1          # a full ring whose head has wrapped
    keys = ("q0", "lp0", "qb", "qh", "lpb", "lph", "lpdb", "lpdh")
    for key in keys:
        assert len({p[key].tobytes() for p in parts}) == 1, key            # the same bits on every rank
    got = parts[0]

    rng = np.random.default_rng(17)
    mean = torch.from_numpy(rng.standard_normal(n)).cuda()
    V = torch.from_numpy(rng.standard_normal((3, n))).cuda()

    def close(name, a, b):
        err = np.abs(a - b).max() / np.abs(b).max()
        print("%s: |sharded - one rank| / |one rank| = %.3e" % (name, err))
        assert np.all(np.abs(a - b) <= 1e-10 * np.abs(b)), name

    with one_context(n, m) as one:
        d0, lp0 = one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE, return_logpdf=True)
        assert np.array_equal(np.concatenate([p["d0"] for p in parts], axis=1), d0.cpu().numpy())
        close("q0", got["q0"], one.qn_quad(V, center=mean))
        close("z'z, no pair", _zz(got["lp0"], n, wk.SCALE, 0.0), _zz(lp0, n, wk.SCALE, 0.0))
        import_glued(one, parts, n, m)
        close("qb", got["qb"], one.qn_quad(V, center=mean))
        close("qh", got["qh"], one.qn_quad(V, center=mean, inverse=True))
        close("lpb", got["lpb"], one.qn_logpdf(V, mean=mean, scale=wk.SCALE, inverse=False))
        close("lph", got["lph"], one.qn_logpdf(V, mean=mean, scale=wk.SCALE, inverse=True))
        for dk, lk, ldk, inverse in (("db", "lpdb", "ldb", False), ("dh", "lpdh", "ldh", True)):
            ref, lp = one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE, inverse=inverse,
                                  return_logpdf=True)
            ref = ref.cpu().numpy()
            rows = np.concatenate([p[dk] for p in parts], axis=1)
            err = np.linalg.norm(rows - ref) / np.linalg.norm(ref)
            print("%s: |sharded - one rank| / |one rank| = %.3e" % (dk, err))
            assert err <= 1e-12
            close(lk, got[lk], lp)
            close("z'z of " + dk, _zz(got[lk], n, wk.SCALE, float(got[ldk])),
                  _zz(lp, n, wk.SCALE, one.qn_logdet(inverse=inverse)))
