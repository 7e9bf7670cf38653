"""LBFGSB_F_FOLLOW_BOUNDS on sharded contexts: 2 and 3 rank processes on one GPU, reduced through a gloo host group
or the library's communicator path with the shared-memory RCCL stand-in (tests/fake_rccl.cpp), as in
test_gpu_qn_sharded.py.  Edits touch rows of one rank only, and one rank alone passes a new u pointer: every rank
must rebuild at the same entry (the changed-row count is reduced over the ranks), see the same task sequence,
and the rows must equal the single-rank run of the same edits."""
import numpy as np
import pytest

from _sharded import fake_rccl, launch_workers

pytestmark = pytest.mark.gpu
N, M, ITERS = 3001, 6, 14


def _run(tmp_path, tag, world, mode):
    return launch_workers("_follow_mr_worker.py", world, mode, N, M, ITERS, prefix=str(tmp_path / tag))


@pytest.mark.parametrize("world,mode", [(2, "gloo"), (3, "gloo"), (2, "fakerccl"), (3, "fakerccl")])
def test_sharded_edits_rebuild_on_every_rank_together(oracle_built, tmp_path, monkeypatch, world, mode):
    one = _run(tmp_path, "single", 1, "single")[0]
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = _run(tmp_path, "mr", world, mode)
    for pt in parts:
        assert list(pt["tasks"]) == list(one["tasks"])
        assert np.array_equal(pt["stats"][1:], parts[0]["stats"][1:])     # the same rebuilds on every rank
    assert int(parts[0]["stats"][2]) == 3, parts[0]["stats"]            # u edit, a pointer, l and nbd edits
    r1, rk = one["rows"], parts[0]["rows"]
    assert r1.shape == rk.shape and r1.shape[0] == ITERS
    assert np.array_equal(r1[:, :4], rk[:, :4])
    assert np.all(np.abs(r1[:, 4] - rk[:, 4]) <= 1e-10 * np.abs(r1[:, 4]))
    x = np.concatenate([pt["x"] for pt in parts])
    assert np.max(np.abs(x - one["x"])) <= 1e-10 * np.max(np.abs(one["x"]))
