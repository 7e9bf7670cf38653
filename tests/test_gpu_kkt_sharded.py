"""The active-set report on sharded contexts: 2 and 3 rank processes on one GPU, reduced through a gloo host group
(host reducer) or the library's communicator path with the shared-memory RCCL stand-in (tests/fake_rccl.cpp).
Every rank calls lbfgsb_hip_kkt collectively with its own rows: the summary is identical on every rank and equals
the single-rank one bit for bit; the per-rank outputs and lists, concatenated in rank order, equal the single-rank
ones; the indices are global."""
import numpy as np
import pytest

from _sharded import fake_rccl, launch_workers

pytestmark = pytest.mark.gpu
MASKS = (0b01100, 0b00011, 0b10000, 31)
TOL = float(np.float32(1e-3))


def _case(n, seed):
    """mixed nbd, rows at and an ulp outside their bounds, l == u and u < l rows, zeros and values at the tolerance
    in g, NaN in the bounds that nbd says do not exist"""
    rng = np.random.default_rng(seed)
    nbd = rng.integers(0, 4, n).astype(np.int32)
    l = rng.uniform(-2.0, 0.0, n)
    u = l + rng.uniform(0.1, 2.0, n)
    k = rng.random(n)
    u[k < 0.06] = l[k < 0.06]
    u[(k >= 0.06) & (k < 0.10)] -= 3.0
    x = l + (u - l) * rng.random(n)
    r = rng.random(n)
    x = np.where(r < 1 / 6, l, x)
    x = np.where((r >= 1 / 6) & (r < 1 / 3), u, x)
    x = np.where((r >= 1 / 3) & (r < 0.35), np.nextafter(l, -np.inf), x)
    x = np.where((r >= 0.35) & (r < 0.37), np.nextafter(u, np.inf), x)
    g = rng.standard_normal(n)
    q = rng.random(n)
    g = np.where(q < 0.1, 0.0, g)
    g = np.where((q >= 0.1) & (q < 0.2), np.sign(g) * TOL, g)
    l[(nbd == 0) | (nbd == 3)] = np.nan
    u[(nbd == 0) | (nbd == 1)] = np.nan
    return dict(x=x, l=l, u=u, nbd=nbd, g=g)


@pytest.mark.parametrize("world,mode,n", [
    (2, "gloo", 2003),        # ragged split, an odd first row on rank 1
    (3, "gloo", 9001),        # more than one list chunk on every rank
    (2, "fakerccl", 2003),    # the communicator path: all-gather of the summaries, combined in rank order
    (3, "fakerccl", 1501),
])
def test_sharded_report_equals_single_rank(oracle_built, tmp_path, monkeypatch, world, mode, n):
    import torch
    import lbfgsb_amd as la
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    case = _case(n, 40 + n)
    np.savez(str(tmp_path / "case.npz"), **case)
    parts = launch_workers("_kkt_mr_worker.py", world, mode, tmp_path / "case.npz", repr(TOL),
                           prefix=str(tmp_path / "kkt"))
    # the single-rank report of the same arrays
    sol = la.DeviceSolver(n, 3)
    try:
        dev = [torch.from_numpy(case[k]).cuda() for k in ("x", "l", "u", "nbd", "g")]
        rep = sol.kkt(*dev, tol=TOL)
        one = {mask: sol.kkt_indices(rep.status, [c for c in range(-1, 4) if mask >> (c + 1) & 1]).cpu().numpy()
               for mask in MASKS}
        status, pg, mult = rep.status.cpu().numpy(), rep.pg.cpu().numpy(), rep.mult.cpu().numpy()
    finally:
        sol.close()
    assert rep.n_outside > 0 and rep.n_fixed > 0 and rep.n_weak > 0 and rep.n_leaving > 0, rep
    for p in parts:
        assert np.array_equal(p["cnt"], rep.counts), (p["cnt"], rep.counts)
        assert p["val"].tobytes() == rep.values.tobytes(), (p["val"], rep.values)
    assert [int(p["row0"]) for p in parts] == [la.block_partition(n, world, r)[0] for r in range(world)]
    assert np.array_equal(np.concatenate([p["status"] for p in parts]), status)
    assert np.concatenate([p["pg"] for p in parts]).tobytes() == pg.tobytes()
    assert np.concatenate([p["mult"] for p in parts]).tobytes() == mult.tobytes()
    for mask in MASKS:
        got = np.concatenate([p["idx%d" % mask] for p in parts])
        assert got.dtype == np.int64 and np.array_equal(got, one[mask]), mask
        for r, p in enumerate(parts):  # global indices: every rank's list lies in its own block of rows
            row0, n_loc = la.block_partition(n, world, r)
            idx = p["idx%d" % mask]
            assert idx.size == 0 or (idx[0] >= row0 and idx[-1] < row0 + n_loc), (mask, r)
