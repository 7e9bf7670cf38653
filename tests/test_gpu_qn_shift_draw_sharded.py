"""Draws and densities of the model plus a diagonal on a sharded context: two rank processes on one GPU through the
host reducer (a gloo group), n = 4099 split unevenly, m = 10, every third row pinned and a run of 40 pinned rows across
the rank boundary (the shift of tests/_mr_common.py).  The log-densities, the quadratic forms and the pinned
count are the same bits on both ranks; the concatenated draws and factor products are within 1e-13 (relative, in the
2-norm) of ONE context's that imported the concatenated state -- a draw is a function of (seed, global row, sample),
not of the sharding -- and the host numbers within 1e-12 relative of that context's."""
import os
import sys

import numpy as np
import pytest

from _sharded import import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_sharded_shift_draws(oracle_built, tmp_path):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_shift_draw_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m, world, iters = 4099, 10, 2, 14
    parts = launch_workers("_qn_shift_draw_mr_worker.py", world, n, m, iters, prefix=str(tmp_path / "qnshiftdraw"))
    assert len({int(p["n_loc"]) for p in parts}) == world                # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1 and int(parts[0]["col"]) == m
    d = wk.shift(n, world)
    pin = np.isinf(d)
    for tag in ("s0", "s1"):
        for key in ("_logp", "_quad", "_logq", "_pinned"):
            assert len({p[tag + key].tobytes() for p in parts}) == 1, tag + key   # the same bits on both ranks
        assert int(parts[0][tag + "_pinned"]) == int(pin.sum())

    rng = np.random.default_rng(wk.SEED)
    V = torch.from_numpy(rng.standard_normal((wk.K, n))).cuda()
    mean = torch.from_numpy(rng.standard_normal(n)).cuda()
    dt = torch.from_numpy(d).cuda()

    def close(tag, sh):
        ref = wk.entries(sh, V, mean)
        for key in ("draws", "root"):
            got = np.concatenate([p[tag + "_" + key] for p in parts], axis=1)
            err = np.linalg.norm(got - ref[key]) / np.linalg.norm(ref[key])
            print("%s %s: sharded against one rank %.2e (relative)" % (tag, key, err))
            assert err <= 1e-13
            want = mean.cpu().numpy()[pin] if key == "draws" else np.zeros(int(pin.sum()))
            assert np.array_equal(got[:, pin], np.broadcast_to(want, (wk.K, int(pin.sum()))))
        for key in ("logp", "quad", "logq"):
            err = np.abs(parts[0][tag + "_" + key] - ref[key]) / np.abs(ref[key])
            print("%s %s: sharded against one rank %s (relative)" % (tag, key, err))
            assert np.all(err <= 1e-12)
        assert int(ref["pinned"]) == int(parts[0][tag + "_pinned"])

    with one_context(n, m) as one:
        close("s0", one.qn_shift(dt, wk.MU))
        import_glued(one, parts, n, m)
        close("s1", one.qn_shift(dt, wk.MU))
