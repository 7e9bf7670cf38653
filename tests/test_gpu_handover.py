"""The breakpoint hand-over of the update pass (option spec_capture = 1) on walks it SERVES.

update_scan_kernel appends every row whose breakpoint lies in [0, cand_hi] to a list; the next Cauchy walk takes that
list for every breakpoint up to cand_hi, without a window pass (solver_provider.inl: spec_queue, spec_land, the first
branch of window_fetch).  A list that misses a row fails nothing: the walk skips a breakpoint and the run quietly
leaves the reference.  So these tests run the constructed cases of tests/_handover_cases.py -- walks that cross one to
a few breakpoints in chosen rows, iteration after iteration (pinned from the oracle alone by
tests/test_handover_cases_cpu.py) -- and demand BOTH that walks were served (path_counts()[2], floors below) and that
the run is the reference's:

  a. every call replayed by the oracle from the run's own previous state (tests/test_gpu_fuzz.py: drive_with_replay,
     replay_all): natural order (MC = 5 / 10 with the new-row sums, the pair-shared MC = 20 pass refused by the host),
     the free-row layout (the export of the harness un-sorts the tiles: the layout kernels run on an all-ones mask,
     the pair-shared instantiation over the whole tiles + one workgroup for the rows behind them), and two_pass = 0
     (the instantiations without the new-row sums, MC = 5 / 10 / 20);
  b. undisturbed runs (no export between calls, so the tiles stay packed): spec_capture 0 against 1.  The hand-over
     changes who delivers the breakpoints, not which or in which (t, index) order: every return bit for bit;
  c. several ranks: the two-stage host all-gather of spec_land (counts, then `keep` records) with 2 ranks, the
     communicator's all-gather with 3, the ranks' records merged by (t, global index).

Floors for the served walks (conditions, not measurements; the observed count stands beside each): >= 2 wherever one
launch covers all rows; >= 1 on the layout where n is no multiple of the tile of 128 rows -- there the host refuses the
hand-over once col - 1 >= 6 (lbk::update_scan_hands_over), so only the first iterations are served.
"""
import hashlib

import numpy as np
import pytest

import _handover_cases as hc

pytestmark = pytest.mark.gpu

NATURAL = {"spec_capture": 1}
LAYOUT = {"spec_capture": 1, "compact_w": 2, "compact_policy": 2}
THREE_PASS = {"spec_capture": 1, "two_pass": 0}


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _floor(case, layout):
    return 1 if layout and not case.whole_tiles else 2


# Walks served in 40 iterations as OBSERVED on the MI355X (tests a and b alike, both entries; a later change that
# silences the hand-over shows as a drop) -- what the CPU model predicts (Case.served, tests/_handover_cases.py), except where
# the host refuses: natural order at m = 20 beyond 10 old pairs, the layout at n % 128 != 0 beyond 5.
#              natural  layout  two_pass = 0
#   n255_m10      9       2        9
#   n255_m7       9       2        9
#   n383_m10      8       2        8
#   n256_m10      7       7        7
#   n384_m10      7       7        7
#   n255_m3       5       5        5
#   n1000_m20     8       -       15
#   n510_w2      10 on each of 2 ranks (natural order); n700_w3: 3 on each of 3 ranks (layout)

REPLAY = ([("natural", NATURAL, False, c) for c in hc.SINGLE] +
          [("layout", LAYOUT, False, c) for c in hc.SINGLE if c.m <= 10] +
          [("two_pass0", THREE_PASS, False, c) for c in hc.SINGLE] +
          [("layout_pp", LAYOUT, True, c) for c in hc.SINGLE if c.m <= 10])


@pytest.mark.parametrize("label,opts,pp,case", REPLAY, ids=["%s-%s" % (r[0], r[3].name) for r in REPLAY])
def test_every_call_is_the_oracles_step(env, label, opts, pp, case):
    """40 iterations, every call reproduced by ONE oracle call from the run's previous state (integers exactly,
    floats to 1e-10), and walks served by the hand-over"""
    from test_gpu_fuzz import LAST, drive_with_replay
    po = env["po"]
    p, _ = case.problem(po)
    split, ncalls = drive_with_replay(po, p, hc.ITERS, pp=pp, replay_all=True, options=dict(opts))
    handed = LAST["path_counts"][2]
    print("\n%s %s: %d walks served, split %s of %d calls" % (label, case.name, handed, split, ncalls))
    assert handed >= _floor(case, "compact_w" in opts), (label, case.name, handed)     # observed: table above


def _digest(t):
    return hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()


def _undisturbed(env, p, max_iter, pp, **options):
    """driven like _run of tests/test_gpu_compact.py: nothing is exported before the run ends"""
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(p.n, p.m, options=options)
    try:
        xs = [torch.from_numpy(p.x0.copy()).cuda(), torch.full((p.n,), 7.0, dtype=torch.float64, device="cuda")]
        gs = [torch.zeros_like(xs[0]), torch.full_like(xs[0], -3.0)]
        x, g = xs[0], gs[0]
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        rows = []
        for _ in range(200000):
            if pp:
                t, cur = sol.setulb_pp(xs, l, u, nbd, gs, p.factr, p.pgtol)
                x, g = xs[cur], gs[cur]
            else:
                t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            sol.sync()
            rows.append((t, tuple(int(v) for v in sol.isave[21:44]), sol.f.tobytes(), _digest(x),
                         None if pp and t.startswith("FG") else _digest(g)))   # (pp: the buffer about to be written)
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            elif not t.startswith("NEW_X") or sol.isave[29] >= max_iter:
                break
        handed, stats = sol.path_counts()[2], sol.compact_stats()
        wa, iwa = sol.export_state()
        return dict(rows=rows, handed=handed, stats=stats, wa=wa.tobytes(), iwa=iwa.tobytes())
    finally:
        sol.close()


UNDISTURBED = ([("natural", False, c) for c in hc.SINGLE] + [("layout", True, c) for c in hc.SINGLE if c.m <= 10])


@pytest.mark.parametrize("label,layout,case", UNDISTURBED, ids=["%s-%s" % (r[0], r[2].name) for r in UNDISTURBED])
def test_handover_changes_no_return_of_an_undisturbed_run(env, label, layout, case):
    """spec_capture 0 against 1 with no export between the calls -- on the layout (compact_policy = 2,
    compact_min_rows = 0) the tiles are re-sorted in every iteration and STAY packed for the update pass.  Every
    return equal bit for bit: task, isave(22:44), f, the digests of x and g, and the exported state at the end."""
    po = env["po"]
    p, _ = case.problem(po)
    extra = dict(compact_w=2, compact_policy=2, compact_min_rows=0) if layout else {}
    a = _undisturbed(env, p, hc.ITERS, pp=layout, spec_capture=0, **extra)
    b = _undisturbed(env, p, hc.ITERS, pp=layout, spec_capture=1, **extra)
    print("\n%s %s: %d walks served, compact_stats %s, %d returns" % (label, case.name, b["handed"], b["stats"],
                                                                       len(b["rows"])))
    assert a["handed"] == 0
    if layout:
        for r in (a, b):
            assert r["stats"][3] == 1 and r["stats"][0] >= 3, r["stats"]       # it did re-sort
    for k, (ra, rb) in enumerate(zip(a["rows"], b["rows"])):
        assert ra == rb, "%s %s: return %d differs: %s | %s" % (label, case.name, k, ra[:3], rb[:3])
    assert len(a["rows"]) == len(b["rows"])
    assert a["wa"] == b["wa"] and a["iwa"] == b["iwa"], "exported state differs"
    assert b["handed"] >= _floor(case, layout), (label, case.name, b["handed"])        # observed: table above


@pytest.mark.parametrize("world,mode,name,layout,floor", [(2, "gloo", "n510_w2", False, 2),
                                                          (3, "fakerccl", "n700_w3", True, 1)])
def test_sharded_handover(oracle_built, tmp_path, monkeypatch, world, mode, name, layout, floor):
    """every rank bounds ITS last n_loc % 128 rows; the walk is replicated, so every rank must count the same served
    walks, and the rows are the single-rank oracle's (as tests/test_gpu_multirank.py demands of a sharded run)"""
    from _sharded import fake_rccl, launch_workers
    po = oracle_built
    case = hc.BY_NAME[name]
    assert case.world == world
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    if layout:
        monkeypatch.setenv("LBFGSB_TEST_COMPACT", "1")
    monkeypatch.setenv("LBFGSB_TEST_SPEC_CAPTURE", "1")
    res = launch_workers("_mr_worker.py", world, mode, case.n, case.m, hc.ITERS, "stair",
                         prefix=str(tmp_path / "out.json"))
    p, _ = case.problem(po)
    rows = []
    s = po.run(po.Engine("oracle"), p, max_iter=hc.ITERS,
               snapshot=lambda k, s: rows.append([int(s.isave[29]), int(s.isave[33]), int(s.isave[32]),
                                                  int(s.isave[37]), float(s.f[0])])
               if s.task_s.startswith("NEW_X") else None)
    print("\n%s: walks served per rank %s" % (name, res["handed"]))
    assert len(res["rows"]) == len(rows) == hc.ITERS
    for a, b in zip(res["rows"], rows):
        assert a[:4] == b[:4], (a, b)
        assert a[4] == pytest.approx(b[4], rel=1e-9)
    assert np.max(np.abs(np.array(res["x"]) - s.x)) <= 1e-8 * max(1.0, np.max(np.abs(s.x)))
    assert len(res["handed"]) == world and len(set(res["handed"])) == 1, res["handed"]
    assert res["handed"][0] >= floor, res["handed"]         # observed: 10 (2 ranks, natural order), 3 (3 ranks, layout)
