"""The curvature-model operator on sharded contexts: 2 and 3 rank processes on one GPU, reduced through a gloo
host group (host reducer) or the library's communicator path with the shared-memory RCCL stand-in
(tests/fake_rccl.cpp).  Every rank calls collectively with its own rows; the concatenated outputs must equal the
dense numpy model built from the concatenated per-rank exports (theta I updated by the pairs in ring order)."""
import numpy as np
import pytest

from _sharded import fake_rccl, launch_workers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,mode,n,m,iters", [
    (2, "gloo", 2003, 5, 9),         # ragged split, the ring wrapped
    (3, "gloo", 3001, 20, 24),       # two column tiles (16 + 4) per W'V block, wrapped
    (2, "fakerccl", 2003, 7, 10),    # the communicator path: all-gather of the partials, sums in rank order
    (3, "fakerccl", 1501, 3, 8),
])
def test_sharded_operator_matches_dense_model(oracle_built, tmp_path, monkeypatch, world, mode, n, m, iters):
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qn"))
    assert len({(int(p["col"]), int(p["head"]), float(p["theta"])) for p in parts}) == 1
    col, head, theta = int(parts[0]["col"]), int(parts[0]["head"]), float(parts[0]["theta"])
    assert col == m and head > 1                     # a full ring whose head has wrapped
    Ws = np.concatenate([p["ws"] for p in parts], axis=1).T
    Wy = np.concatenate([p["wy"] for p in parts], axis=1).T
    B = theta * np.eye(n)
    for j in range(col):
        c = (head - 1 + j) % m
        s, y = Ws[:, c], Wy[:, c]
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
    H = np.linalg.inv(B)
    cond = np.linalg.cond(B)
    V = parts[0]["V"]
    bv = np.concatenate([p["bv"] for p in parts], axis=1)
    hv = np.concatenate([p["hv"] for p in parts], axis=1)
    h1 = np.concatenate([p["h1"] for p in parts])
    assert np.linalg.norm(bv - V @ B.T) <= 1e-10 * np.linalg.norm(B, 2) * np.linalg.norm(V)
    ref = V @ H.T
    assert np.linalg.norm(hv - ref) <= 1e-10 * cond * np.linalg.norm(ref)
    assert np.linalg.norm(h1 - hv[1]) <= 1e-13 * np.linalg.norm(hv[1])   # one vector alone or inside a block
    db = np.concatenate([p["db"] for p in parts])
    dh = np.concatenate([p["dh"] for p in parts])
    assert np.abs(db - np.diag(B)).max() <= 1e-10 * np.abs(np.diag(B)).max()
    assert np.abs(dh - np.diag(H)).max() <= 1e-10 * cond * np.abs(np.diag(H)).max()
