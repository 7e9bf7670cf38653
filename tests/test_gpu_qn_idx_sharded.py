"""The entries at index lists on sharded contexts: 2 and 3 rank processes on one GPU (a gloo host group, or the
library's communicator path with the shared-memory RCCL stand-in of tests/fake_rccl.cpp), n = 4099 split unevenly,
m = 10.  Every rank passes the same global list, which holds the rows on both sides of every cut.  The host results
are the same bytes on every rank; the rows of the pairs equal exactly those of ONE context that imported the
concatenated state, the blocks are within 1e-12 (relative to the largest entry) of that context's, and the
concatenated columns within 1e-12 in the relative 2-norm."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

HOST = ("rows", "b_sq", "b_rect", "h_sq", "h_rect", "s_sq", "s_rect")


@pytest.mark.parametrize("world,mode,iters", [(2, "gloo", 14), (3, "fakerccl", 13)])
def test_sharded_idx(oracle_built, tmp_path, monkeypatch, world, mode, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_idx_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m = 4099, 10
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_idx_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qnidx"))
    assert len({int(p["n_loc"]) for p in parts}) == world                # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m
    ia, ib = wk.lists(n, world)
    for r in range(1, world):                                             # the rows on both sides of every cut
        e = wk.cut(n, world, r)[0]
        assert e - 1 in ia and e in ia and e - 1 in ib and e in ib
    for key in HOST:
        assert len({p[key].tobytes() for p in parts}) == 1, key           # the same bytes on every rank

    d = torch.from_numpy(wk.shift(n, world)).cuda()
    with one_context(n, m) as one:
        import_glued(one, parts, n, m)
        sh = one.qn_shift(d, wk.MU)
        ref = dict(rows=one.qn_rows(ia), s_sq=sh.block(ia), s_rect=sh.block(ia, ib),
                   s_cols=sh.columns(ia).cpu().numpy())
        for inv, tag in ((False, "b"), (True, "h")):
            ref[tag + "_sq"], ref[tag + "_rect"] = one.qn_block(ia, inverse=inv), one.qn_block(ia, ib, inverse=inv)
            ref[tag + "_cols"] = one.qn_cols(ia, inverse=inv).cpu().numpy()
    got = parts[0]
    assert got["rows"].shape == (len(ia), 2 * m) and np.array_equal(got["rows"], ref["rows"])   # exactly
    assert np.abs(got["rows"]).max() > 0.0
    for key in HOST[1:]:
        err, scale = np.abs(got[key] - ref[key]).max(), np.abs(ref[key]).max()
        print("%s: sharded against one rank: %.2e (largest entry %.3e)" % (key, err, scale))
        assert err <= 1e-12 * scale
    pinned = np.isinf(wk.shift(n, world))
    assert pinned[ia].any() and np.all(got["s_sq"][pinned[ia], :] == 0.0) and np.all(got["s_rect"][:, pinned[ib]] == 0.0)
    for key in ("b_cols", "h_cols", "s_cols"):
        cols = np.concatenate([p[key] for p in parts], axis=1)
        err = np.linalg.norm(cols - ref[key]) / np.linalg.norm(ref[key])
        print("%s: sharded against one rank: %.2e (relative 2-norm)" % (key, err))
        assert cols.shape == (len(ia), n) and err <= 1e-12
    assert np.all(np.concatenate([p["s_cols"] for p in parts], axis=1)[:, pinned] == 0.0)
