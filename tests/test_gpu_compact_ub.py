"""Option "cw_ub": with all three bound arrays uniform (uniform_bounds mask 7, no dictionary) and the memory full
(m = 10), the dense lane-pair update pass over W on the tile-local free-row layout reads l, u and nbd ONCE per
workgroup from the 64-byte buffers instead of once per row and trip (update_scan_kernel_dense_ub).  The arithmetic
on the three values is the same expression for expression, so what must hold is equality, never closeness:
  * with compact_w = 2 a run under cw_ub = 1 and the same run under cw_ub = 0 are bit for bit the same after EVERY
    call (task, x, g, f, isave, dsave) and in the exported state -- iwhere with it -- at every NEW_X return and at
    the end.  (The export puts W back into natural row order; at an FG return that would take the layout away from
    the update pass that follows, so it is made at the NEW_X returns, behind which compact_policy = 2 re-sorts anyway.
    The traces of the moving and the frozen layout export at the end only.)
  * for n around the tile, m = 5 (the form has no kernel there) and m = 10, both entries, with and without the
    deferred set-up, nt 0 / 1, and a uniform nbd of 0, 1, 2 and 3;
  * on single tiles of every fill, the 64 free rows behind an odd start included;
  * the form is launched with mask 7 and only then: not with partial masks, streamed or dictionary-coded bounds,
    never under cw_ub = 0;
  * a uniform edit of u at a NEW_X return under LBFGSB_F_FOLLOW_BOUNDS (the mask stays 7) reaches the next launch:
    the same bits as cw_ub = 0, the oracle's rows, and two calls around the edit from the oracle's state;
  * a free set that moves after the last re-sort, and the refusal of a layout older than the free set, are those of
    cw_ub = 0.
"""
import numpy as np
import pytest

from test_gpu_compact import _digest
from test_gpu_compact_dense import HALVES, _bound_forms, _pinned_problem, _tile_counts

pytestmark = pytest.mark.gpu

BASE = {"compact_w": 2, "compact_policy": 2}
ENTRIES = [(True, False, 0), (True, True, 1), (False, False, 1), (False, False, 0)]     # (ping-pong, deferred, nt)


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _trace(env, p, max_iter, pp=True, defer=False, follow=False, events=None, policy_after=None, export_each=True,
           **options):
    """the run of p with these options: one record per CALL (FG returns too), the exported state (wa, iwa: iwhere is
    iwa[n:2n]) at the NEW_X returns if export_each, else at the end.  events: {iteration: edit(l, u, nbd)} made at
    that NEW_X return on the device arrays; policy_after = (iteration, compact_policy).  A refused call ends the trace
    with its error text."""
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(p.n, p.m, defer_lnsrch=defer, same_stream_objective=defer, follow_bounds=follow,
                          options=dict(BASE, **options))
    try:
        xs = [torch.from_numpy(p.x0.copy()).cuda(), torch.full((p.n,), 7.0, dtype=torch.float64, device="cuda")]
        gs = [torch.zeros_like(xs[0]), torch.full_like(xs[0], -3.0)]
        x, g = xs[0], gs[0]
        l, u = torch.from_numpy(p.l.copy()).cuda(), torch.from_numpy(p.u.copy()).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        calls, states, cols, nfree, masks, err = [], [], set(), [], set(), None
        ub_at_edit = None
        for _ in range(20000):
            try:
                if pp:
                    t, cur = sol.setulb_pp(xs, l, u, nbd, gs, p.factr, p.pgtol)
                    x, g = xs[cur], gs[cur]
                else:
                    t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
                sol.sync()
            except la.capi.LbfgsbError as e:
                err = str(e)
                break
            calls.append((t, sol.isave[21:44].tobytes(), sol.dsave[[0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15]].tobytes(),
                          sol.f.tobytes(), _digest(x), _digest(g)))
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
                continue
            if not t.startswith("NEW_X"):
                break
            it = int(sol.isave[29])
            cols.add(int(sol.isave[27]))
            nfree.append(int(sol.isave[37]))
            masks.add(sol.uniform_bounds())
            if export_each:
                wa, iwa = sol.export_state()
                states.append((wa.tobytes(), iwa.tobytes()))
            if events and it in events:
                events[it](l, u, nbd)
                torch.cuda.synchronize()
                ub_at_edit = sol.ub_launches()
            if policy_after is not None and it == policy_after[0]:
                sol.set_option("compact_policy", policy_after[1])
            if it >= max_iter:
                break
        stats = sol.compact_stats()
        dense, ubl = sol.dense_launches(), sol.ub_launches()
        if err is None and not export_each:
            wa, iwa = sol.export_state()
            states.append((wa.tobytes(), iwa.tobytes()))
        return dict(calls=calls, states=states, cols=cols, nfree=nfree, masks=masks, err=err, stats=stats,
                    dense=dense, ubl=ubl, ub_at_edit=ub_at_edit, x=x.cpu().numpy())
    finally:
        sol.close()


def _same(a, b, what):
    assert len(a["calls"]) == len(b["calls"]), (what, len(a["calls"]), len(b["calls"]))
    for k, (ca, cb) in enumerate(zip(a["calls"], b["calls"])):
        for name, va, vb in zip(("task", "isave", "dsave", "f", "x", "g"), ca, cb):
            assert va == vb, "%s: call %d (%s): %s differs" % (what, k, ca[0][:12], name)
    assert a["err"] == b["err"], (what, a["err"], b["err"])
    assert len(a["states"]) == len(b["states"]), (what, len(a["states"]), len(b["states"]))
    for k, (sa, sb) in enumerate(zip(a["states"], b["states"])):
        assert sa[1] == sb[1], "%s: export %d: iwa (iwhere) differs" % (what, k)
        assert sa[0] == sb[0], "%s: export %d: wa differs" % (what, k)
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    assert a["dense"] == b["dense"], (what, a["dense"], b["dense"])      # (the form counts as a dense launch)
    assert a["masks"] == b["masks"], (what, a["masks"], b["masks"])


def _ab(env, p, max_iter, what, launched, **kw):
    """launched: True = the kernel of the form must have run, False = it must not"""
    a = _trace(env, p, max_iter, cw_ub=1, **kw)
    b = _trace(env, p, max_iter, cw_ub=0, **kw)
    _same(a, b, what)
    assert b["ubl"] == 0, (what, b["ubl"])
    assert (1 <= a["ubl"] <= a["dense"][1]) if launched else a["ubl"] == 0, (what, a["ubl"], a["dense"])
    return a


@pytest.mark.parametrize("n", [127, 128, 129, 1000, 128 * 37 + 5])
@pytest.mark.parametrize("m", [5, 10])
def test_bit_for_bit_around_the_tile(env, n, m):
    """2 m + 4 iterations of the uniform box (mask 7): both entries, the deferred set-up, nt 0 / 1.  The form exists
    for m = 10 alone and takes whole tiles (the rows behind them go to the plain instantiation)."""
    po = env["po"]
    p = po.problem_quadratic(n, m)
    for pp, defer, nt in ENTRIES:
        a = _ab(env, p, 2 * m + 4, "quadratic n=%d m=%d pp=%d defer=%d nt=%d" % (n, m, pp, defer, nt),
                m == 10 and n >= 128, pp=pp, defer=defer, nt=nt)
        assert a["masks"] == {7} and a["err"] is None and a["stats"][3] == 1, (a["masks"], a["err"], a["stats"])
        assert max(a["cols"]) == m


@pytest.mark.parametrize("nbd", [0, 1, 2, 3])
def test_every_uniform_nbd(env, nbd):
    """the kernels branch on nbd: unbounded, lower, both, upper -- one value for every row"""
    po = env["po"]
    p = po.problem_quadratic(128 * 37 + 5, 10)
    p.nbd[:] = nbd
    for pp, defer, nt in ENTRIES[:2]:
        a = _ab(env, p, 24, "uniform nbd=%d pp=%d defer=%d" % (nbd, pp, defer), True, pp=pp, defer=defer, nt=nt)
        assert a["masks"] == {7} and a["err"] is None


@pytest.mark.parametrize("pp,defer,nt", ENTRIES)
def test_single_tiles_of_every_fill(env, pp, defer, nt):
    """tiles with 0, 1, 2, 63, 64, 65, 127 and 128 free rows, odd and even counts in the first half, 64 free rows
    behind an odd start (the half that does not fit the 32 pieces and loads its W entries the old way)"""
    po = env["po"]
    p, free = _pinned_problem(po, 10)
    a = _ab(env, p, 26, "pinned pp=%d defer=%d nt=%d" % (pp, defer, nt), True, pp=pp, defer=defer, nt=nt)
    inside = (a["x"] > -1.0) & (a["x"] < 1.0)
    assert np.array_equal(inside, free)
    counts = _tile_counts(inside)
    assert counts == HALVES
    assert {c0 + c1 for c0, c1 in counts} >= {0, 1, 63, 64, 65, 127, 128}
    assert (1, 64) in counts and (63, 64) in counts
    assert a["masks"] == {7} and max(a["cols"]) == 10


@pytest.mark.parametrize("form", ["uniform", "uniform_off", "dictionary", "streamed", "mixed"])
def test_dispatch_by_the_form_of_the_bounds(env, form):
    """launched with mask 7 alone; with every other form of the bounds the counter stays 0 and nothing changes"""
    po = env["po"]
    name, p, opts, mask = [f for f in _bound_forms(po, 10) if f[0] == form][0]
    a = _ab(env, p, 16, "bounds " + name, form == "uniform", **opts)
    if mask is None:
        assert all(k & 8 for k in a["masks"]), a["masks"]
    else:
        assert a["masks"] == {mask}, (name, a["masks"], mask)
    assert a["dense"][0] >= 1 and a["dense"][1] >= 1, a["dense"]      # (the dense kernels ran in every form)


def _tighten(l, u, nbd): u[:] = 0.5      # noqa: E302,E704
def _loosen(l, u, nbd): u[:] = 1.5       # noqa: E302,E704


@pytest.mark.parametrize("edit", [_tighten, _loosen], ids=["tighten", "loosen"])
def test_uniform_edit_of_u_at_new_x_is_followed(env, edit):
    """u changes by a uniform amount at the NEW_X return of iteration 13 (memory full): nothing new comes from the
    host, the next launch reads the rebuilt 64-byte buffer"""
    from test_gpu_follow_bounds import oracle_rows, row_of, same_rows
    po = env["po"]
    n, m, at, last = 4099, 10, 13, 22
    p = po.problem_quadratic(n, m)
    a = _ab(env, p, last, "follow " + edit.__name__, True, follow=True, pp=False, events={at: edit})
    assert a["masks"] == {7} and a["err"] is None
    # the form ran before the edit and after it
    assert 1 <= a["ub_at_edit"] < a["ubl"], (a["ub_at_edit"], a["ubl"])
    # ... and the run is the oracle's with the same edit at the same return (the suite's rule for whole trajectories:
    # counters exactly, f, x, g to 1e-10)
    exp, _ = oracle_rows(po, po.problem_quadratic(n, m), {("NEW_X", at): edit}, max_iter=last)
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(n, m, follow_bounds=True, options=dict(BASE, cw_ub=1))
    got = []
    try:
        x, g = torch.from_numpy(p.x0.copy()).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda")
        l, u = torch.from_numpy(p.l.copy()).cuda(), torch.from_numpy(p.u.copy()).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        for _ in range(20000):
            t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            elif t.startswith("NEW_X"):
                it = int(sol.isave[29])
                got.append(row_of(it, sol.isave, sol.f[0], x.cpu().numpy(), g.cpu().numpy()))
                if it == at:
                    edit(l, u, nbd)
                    torch.cuda.synchronize()
                if it >= last:
                    break
            else:
                break
        assert sol.ub_launches() >= 1
    finally:
        sol.close()
    same_rows(got, exp)
    assert len(exp) == last


def test_two_calls_around_a_uniform_edit_from_the_oracles_state(env):
    """the oracle's state at a first trial point with the memory full: call 1 (the update pass as its evaluation)
    gives the oracle's NEW_X return with the old u, then u is edited on both sides and call 2 (walk, storing pass)
    gives the oracle's next return with the new u -- integers exactly, floats to 1e-10"""
    from test_gpu_parity import _dev, compare_states, oracle_snapshots
    po, torch, la = env["po"], env["torch"], env["la"]
    n, m = 1000, 10
    p = po.problem_quadratic(n, m)
    snaps = oracle_snapshots(po, p, 60)
    tested = 0
    for k in range(4, len(snaps) - 1):
        s0, s1 = snaps[k - 1], snaps[k]
        if not (s1.task_s.startswith("NEW_X") and s0.task_s.startswith("FG_LN") and int(s0.isave[35]) == 1
                and int(s0.isave[27]) == m):
            continue
        pe = po.problem_quadratic(n, m)
        _tighten(pe.l, pe.u, pe.nbd)
        s2 = s1.copy()
        po.call(po.Engine("oracle"), pe, s2)
        s = s0.copy()
        s.f[0] = p.fg(s.x, s.g)
        sol = la.DeviceSolver(n, m, follow_bounds=True, options=dict(BASE, cw_ub=1))
        try:
            x, g = _dev(torch, s.x), _dev(torch, s.g)
            l, u, nbd = _dev(torch, p.l), _dev(torch, p.u), _dev(torch, p.nbd.astype(np.int32))
            sol.import_state(s.wa, s.iwa, s.isave)
            for name_ in ("task", "csave", "lsave", "isave", "dsave"):
                getattr(sol, name_)[:] = getattr(s, name_)
            sol.f[0] = s.f[0]

            def snapshot():
                torch.cuda.synchronize()
                wa, iwa = sol.export_state()
                return po.State(n, m, x.cpu().numpy(), g.cpu().numpy(), sol.f.copy(), wa, iwa, sol.task.copy(),
                                sol.csave.copy(), sol.lsave.copy(), sol.isave.copy(), sol.dsave.copy())
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            compare_states(snapshot(), s1, n, m, po, skip=("xp",), check_indx2=False, check_iwhere=False)
            _tighten(l, u, nbd)
            torch.cuda.synchronize()
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            out2 = snapshot()
            compare_states(out2, s2, n, m, po, skip=("xp",), check_indx2=False,
                           check_iwhere=out2.task_s.startswith("FG_LN"))
            # (test_uniform_edit_of_u_at_new_x_is_followed counts the form's launches behind an edit)
            assert sol.uniform_bounds() == 7
        finally:
            sol.close()
        tested += 1
        if tested >= 3:
            break
    assert tested >= 1


def _rosenbrock_above_one(po, n):
    """the reference's driver problem with ONE lower bound, l = 1 (mask 7): from x0 = 3 nearly every row starts at
    its bound and about one more leaves it in every iteration, far beyond the point where the memory is full"""
    p = po.problem_rosenbrock(n, 10, 0.0, 0.0)
    p.l[:] = 1.0
    return p


def test_free_set_moves_after_the_last_resort(env):
    """the update pass runs on the layout of the iteration before: a row its own n-loop sets free fetches its entries
    in the kernel body, whichever way the bounds came"""
    po = env["po"]
    for n in (1000, 128 * 37 + 5):
        a = _ab(env, _rosenbrock_above_one(po, n), 40, "moving free set n=%d" % n, True, export_each=False)
        assert a["err"] is None and a["stats"][0] >= 10 and a["masks"] == {7}, (a["err"], a["stats"], a["masks"])
        nf = a["nfree"]
        assert sum(1 for k in range(12, len(nf)) if nf[k] > nf[k - 1]) >= 5, nf     # (col = m from iteration 11 on)


def test_stale_layout_is_still_refused(env):
    """the tiles are sorted in every iteration up to the 12th (memory full, the form running) and never again: the
    first storing pass that meets a free row without a layout bit refuses (E_STATE) -- at the same call with the
    bounds held by the kernel body"""
    po = env["po"]
    a = _ab(env, _rosenbrock_above_one(po, 1000), 40, "frozen layout", True, policy_after=(12, 0), export_each=False)
    assert a["err"] is not None and "older than the free set" in a["err"], a["err"]
    assert a["stats"][2] == 1 and a["masks"] == {7}, (a["stats"], a["masks"])
