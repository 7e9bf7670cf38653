"""The pairs in and out on sharded contexts: 3 rank processes on one GPU (a gloo host group, or the library's
communicator path with the shared-memory RCCL stand-in of tests/fake_rccl.cpp), n = 1027 split unevenly, m = 10, the
dyadic family (every sum exact, whatever the split).  No rank ever runs: each loads its rows of m - 1 pairs, pushes
two more -- the second wraps the ring -- and reads the pairs back.  theta and log det B are the same bytes on every
rank, and the glued pairs and the glued H v equal those of ONE context over all rows that did the same, bit for bit."""
import os
import sys

import numpy as np
import pytest

from _sharded import fake_rccl, launch_workers

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("mode", ["gloo", "fakerccl"])
def test_sharded_pairs(oracle_built, tmp_path, monkeypatch, mode):
    import torch
    import lbfgsb_amd as la
    sys.path.insert(0, HERE)
    try:
        import _qn_pairs_mr_worker as wk
        from _qn_pairs_seq import sequence
    finally:
        sys.path.remove(HERE)
    n, m, world = 1027, 10, 3
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_pairs_mr_worker.py", world, mode, n, m, prefix=str(tmp_path / "qnpairs"))
    assert len({int(p["n_loc"]) for p in parts}) == world  # an uneven split
    for key in ("stored", "theta", "logdet"):
        assert len({p[key].tobytes() for p in parts}) == 1, key  # the same bytes on every rank
    assert parts[0]["stored"].tolist() == [1, 1]

    pairs, states = sequence(n, m, m + 1)
    one = la.DeviceSolver(n, m)
    try:
        ref = wk.act(one, pairs, states, m, slice(0, n), torch.device("cuda", 0))
    finally:
        one.close()
    Sr, Yr = states[m + 1].pairs()
    assert states[m + 1].head == 2 and np.array_equal(ref["S"].T, Sr) and np.array_equal(ref["Y"].T, Yr)
    assert float(ref["theta"]) == states[m + 1].theta
    for key in ("S", "Y", "hv"):
        glued = np.concatenate([p[key] for p in parts], axis=1)
        assert glued.shape == ref[key].shape and glued.tobytes() == ref[key].tobytes(), key
    assert parts[0]["theta"].tobytes() == ref["theta"].tobytes()
    assert parts[0]["logdet"].tobytes() == ref["logdet"].tobytes()
