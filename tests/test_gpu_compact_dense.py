"""Option "cw_dense": the two passes over W on the tile-local free-row layout fetch a tile's (half tile's) run of
layout-free entries of each stored column by 16-byte loads and hand the entries to the lanes that own the rows
through LDS (SubsmTripCW2, UpdScanPairTripCW) -- instead of two 8-byte loads per column in which every lane takes part.
Only loads change: not one floating-point operation or its order.  What must hold:
  * with compact_w = 2, a run under cw_dense = 1 and the same run under cw_dense = 0 are bit for bit the same after
    EVERY call: task, x, g, f, isave, dsave, and the exported state at the end;
  * that on tiles with 0, 1, 2, 63, 64, 65, 127 and 128 layout-free rows, odd and even counts in the first half
    (the last active lane of a run then reads one slot past it; a full tile must not read past the tile; 64 free rows
    behind an odd start do not fit the 32 pieces of a half and load the old way);
  * for every form of the bounds (uniform, dictionary-coded, streamed, mixed), each also within the one-step tolerance
    of the oracle;
  * with the free set changing after the last re-sort (the update pass fetches a newly free row in its body);
  * the storing pass still refuses a layout that is older than the free set.
"""
import numpy as np
import pytest

from test_gpu_compact import _digest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _trace(env, p, max_iter, pp=True, defer=False, policy_after=None, **options):
    """the run of p with these options: one record per CALL (FG returns too) + the exported state; policy_after =
    (iteration, compact_policy): switch the packing policy once that iteration is reached.  A refused call ends the
    trace with its error text."""
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(p.n, p.m, defer_lnsrch=defer, same_stream_objective=defer, options=options or None)
    try:
        xs = [torch.from_numpy(p.x0.copy()).cuda(), torch.full((p.n,), 7.0, dtype=torch.float64, device="cuda")]
        gs = [torch.zeros_like(xs[0]), torch.full_like(xs[0], -3.0)]
        x, g = xs[0], gs[0]
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        calls, cols, stps, nfree, err = [], set(), set(), [], None
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
            # (isave(22:44) and dsave without its wall-clock timers, as test_gpu_compact.py compares them: what is in
            #  front of isave(22) names the context)
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
            cols.add(int(sol.isave[27]))
            stps.add(float(sol.dsave[13]))
            nfree.append(int(sol.isave[37]))
            if policy_after is not None and sol.isave[29] == policy_after[0]:
                sol.set_option("compact_policy", policy_after[1])
            if sol.isave[29] >= max_iter:
                break
        stats = sol.compact_stats()
        dense, ub = sol.dense_launches(), sol.uniform_bounds()
        wa = iwa = None
        if err is None:
            wa, iwa = sol.export_state()
        return dict(calls=calls, cols=cols, stps=stps, nfree=nfree, err=err, stats=stats, dense=dense, ub=ub,
                    x=x.cpu().numpy(),
                    wa=None if wa is None else wa.tobytes(), iwa=None if iwa is None else iwa.tobytes())
    finally:
        sol.close()


def _same(a, b, what):
    assert len(a["calls"]) == len(b["calls"]), (what, len(a["calls"]), len(b["calls"]))
    for k, (ca, cb) in enumerate(zip(a["calls"], b["calls"])):
        for name, va, vb in zip(("task", "isave", "dsave", "f", "x", "g"), ca, cb):
            assert va == vb, "%s: call %d (%s): %s differs" % (what, k, ca[0][:12], name)
    assert a["err"] == b["err"], (what, a["err"], b["err"])
    assert a["wa"] == b["wa"] and a["iwa"] == b["iwa"], (what, "exported state differs")
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])


def _ab(env, p, max_iter, what, **kw):
    a = _trace(env, p, max_iter, cw_dense=1, **kw)
    b = _trace(env, p, max_iter, cw_dense=0, **kw)
    _same(a, b, what)
    # the two runs did take the two load paths: the dense storing kernel whenever a full tile and a stored pair
    # exist, the dense update kernel (lane pairs: m = 10) once more than 5 pairs are stored
    assert b["dense"] == (0, 0), (what, b["dense"])
    if p.n >= 128 and max(a["cols"], default=0) >= 2:
        assert a["dense"][0] >= 1, (what, a["dense"])
    if p.n >= 128 and p.m == 10 and max(a["cols"], default=0) >= 8:
        assert a["dense"][1] >= 1, (what, a["dense"])
    return a


# ---- a problem whose free set is chosen row by row ----
# f = sum c_i (x_i - t_i)^2 / 2 + eps sum (x_{i+1} - x_i)^2 / 2 on [-1, 1]^n: a row with t_i = 3 ends at its upper
# bound (its gradient there is c_i (1 - 3) + eps (...) < 0 for eps = 0.05), a row with |t_i| <= 0.4 stays inside.
HALVES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (63, 0), (30, 33), (64, 0), (33, 31), (0, 64), (1, 64), (64, 1),
          (33, 32), (63, 64), (64, 63), (64, 64), (17, 40), (40, 17)]


def _pinned_problem(po, m, tail=5, l=None, u=None, nbd=None, name="pinned"):
    rng = np.random.default_rng(77)
    n = 128 * len(HALVES) + tail
    free = np.zeros(n, bool)
    for k, (c0, c1) in enumerate(HALVES):
        free[128 * k + rng.choice(64, c0, replace=False)] = True
        free[128 * k + 64 + rng.choice(64, c1, replace=False)] = True
    free[128 * len(HALVES):] = rng.random(tail) < 0.5
    t = np.where(free, rng.uniform(-0.4, 0.4, n), 3.0)
    c = rng.uniform(0.5, 2.0, n)
    eps = 0.05

    def fg(x, g):
        d = np.diff(x)
        g[:] = c * (x - t)
        g[:-1] -= eps * d
        g[1:] += eps * d
        return float(0.5 * np.sum(c * (x - t) ** 2) + 0.5 * eps * np.sum(d * d))
    p = po.Problem(name, n, m, np.zeros(n), np.full(n, -1.0) if l is None else l, np.full(n, 1.0) if u is None else u,
                   np.full(n, 2, np.int32) if nbd is None else nbd, 0.0, 0.0, fg)
    return p, free


def _tile_counts(free):
    nt = free.size // 128
    f = free[:128 * nt].reshape(nt, 2, 64).sum(axis=2)
    return [(int(a), int(b)) for a, b in f]


@pytest.mark.parametrize("m", [5, 10])
@pytest.mark.parametrize("pp,defer,nt", [(True, False, 0), (True, True, 1), (False, False, 1), (False, False, 0)])
def test_single_tiles_of_every_count(env, m, pp, defer, nt):
    """tiles with tf in {0, 1, 2, 63, 64, 65, 127, 128}, odd and even c0, re-sorted in every iteration"""
    po = env["po"]
    p, free = _pinned_problem(po, m)
    a = _ab(env, p, 2 * m + 6, "pinned m=%d pp=%d defer=%d nt=%d" % (m, pp, defer, nt), pp=pp, defer=defer,
            compact_w=2, compact_policy=2, nt=nt)
    # the free set the layout was sorted to is the designed one: the counts were reached
    inside = (a["x"] > -1.0) & (a["x"] < 1.0)
    assert np.array_equal(inside, free)
    counts = _tile_counts(inside)
    assert counts == HALVES
    assert {c0 + c1 for c0, c1 in counts} >= {0, 1, 2, 63, 64, 65, 127, 128}
    assert {c0 % 2 for c0, c1 in counts if c1 > 0} == {0, 1}
    assert (1, 64) in counts and (63, 64) in counts      # 64 free rows behind an odd start
    assert a["stats"][0] >= 3 and a["stats"][3] == 1, a["stats"]
    assert min(a["cols"]) < m and max(a["cols"]) == m, a["cols"]     # col < m and col = m


@pytest.mark.parametrize("n", [127, 128, 129, 1000, 128 * 37 + 5])
@pytest.mark.parametrize("m", [5, 10])
def test_sizes_around_the_tile(env, n, m):
    """no full tile, exactly one, one + a partial one, several; classic and ping-pong entries"""
    po = env["po"]
    p = po.problem_quadratic(n, m, mixed_nbd=True)
    for pp in (True, False):
        a = _ab(env, p, 2 * m + 4, "quadmix n=%d m=%d pp=%d" % (n, m, pp), pp=pp, compact_w=2, compact_policy=2)
        assert a["stats"][3] == 1
    r = po.problem_rosenbrock(n, m, 0.0, 0.0)
    a = _ab(env, r, 2 * m + 4, "rosenbrock n=%d m=%d" % (n, m), compact_w=2, compact_policy=2)
    assert any(s != 1.0 for s in a["stps"])


def _bound_forms(po, m):
    """(name, problem, options, uniform-bounds mask the passes must see: bit 0 l, 1 u, 2 nbd; None = dictionary-coded, bit 3):
    the pinned problem under every form of the bounds.  The pinned rows end at u, so u stays 1 wherever a row is
    pinned; a varying u is wider on the free rows only (their targets stay inside [-0.4, 0.4])."""
    rng = np.random.default_rng(5)
    n = 128 * len(HALVES) + 5
    free = _pinned_problem(po, m)[1]
    wide_l = -1.0 - rng.uniform(0.0, 0.5, n)
    wide_u = np.where(free, 1.0 + rng.uniform(0.0, 0.5, n), 1.0)
    few_l = np.where(np.arange(n) % 3 == 0, -1.0, -2.0)
    forms = [("uniform", {}, {}, 7), ("uniform_off", {}, {"uniform_bounds": 0}, 0),
             ("dictionary", dict(l=few_l), {"dict_bounds": 1}, None),
             ("streamed", dict(l=wide_l, u=wide_u, nbd=np.where(np.arange(n) % 5 == 0, 3, 2).astype(np.int32)),
              {"dict_bounds": 0}, 0),
             ("mixed", dict(l=wide_l), {"dict_bounds": 0}, 6)]
    return [(name, _pinned_problem(po, m, name="pinned_" + name, **kw)[0], opts, mask) for name, kw, opts, mask in forms]


@pytest.mark.parametrize("form", ["uniform", "uniform_off", "dictionary", "streamed", "mixed"])
def test_every_form_of_the_bounds(env, form):
    """bit for bit against cw_dense = 0, and two-step parity with the oracle (integers exactly, floats to 1e-10)"""
    from test_gpu_parity import _dev, compare_states, oracle_snapshots
    po, torch, la = env["po"], env["torch"], env["la"]
    m = 10
    name, p, opts, mask = [f for f in _bound_forms(po, m) if f[0] == form][0]
    a = _ab(env, p, 16, "bounds " + name, compact_w=2, compact_policy=2, **opts)
    if mask is None:      # dictionary-coded: the dictionary bit (bits 0 and 1 then mean "from the table")
        assert a["ub"] & 8, a["ub"]
    else:
        assert a["ub"] == mask, (name, a["ub"], mask)
    snaps = oracle_snapshots(po, p, 60)
    tested = 0
    for k in range(len(snaps) - 2):
        s0, s1, s2 = snaps[k], snaps[k + 1], snaps[k + 2]
        if not (s0.task_s.startswith("FG_LN") and int(s0.isave[35]) == 1 and s1.task_s.startswith("NEW_X")
                and s2.task_s.startswith("FG_LN")):
            continue
        if tested >= 6 and int(s0.isave[27]) < m:
            continue
        # (the run converges in 16 iterations; in its last ones d = z - x is the difference of nearly equal numbers,
        #  |d| ~ 1e-8, and stpmx = (bound - x) / d carries d's relative error, 1e-16 / 1e-8, past the relative 1e-9
        #  compare_states allows dsave(12): steps of ordinary size only -- two of them with the memory full)
        if int(s0.isave[29]) > 12:
            continue
        s = s0.copy()
        s.f[0] = p.fg(s.x, s.g)
        sol = la.DeviceSolver(p.n, p.m, options=dict({"compact_w": 2, "compact_policy": 2, "cw_dense": 1}, **opts))
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
                return po.State(p.n, p.m, x.cpu().numpy(), g.cpu().numpy(), sol.f.copy(), wa, iwa,
                                sol.task.copy(), sol.csave.copy(), sol.lsave.copy(), sol.isave.copy(),
                                sol.dsave.copy())
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            compare_states(snapshot(), s1, p.n, p.m, po, skip=("xp",), check_indx2=False, check_iwhere=False)
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            compare_states(snapshot(), s2, p.n, p.m, po, skip=("xp",), check_indx2=False)
        finally:
            sol.close()
        tested += 1
    assert tested >= 6, tested


def test_free_set_changes_after_the_last_resort(env):
    """the update pass runs on the layout of the iteration before: a row its own n-loop sets free has no layout bit
    yet and fetches its entries in the kernel body (reload_cols), whichever way the other rows were loaded"""
    po = env["po"]
    grew = 0
    for p in (po.problem_rosenbrock(1000, 10, 0.0, 0.0), po.problem_rosenbrock(128 * 37 + 5, 10, 0.0, 0.0),
              po.problem_quadratic(4099, 10, mixed_nbd=True)):
        a = _ab(env, p, 40, "moving free set " + p.name, compact_w=2, compact_policy=2)
        assert a["err"] is None and a["stats"][0] >= 10, (a["err"], a["stats"])
        nf = a["nfree"]
        grew += sum(1 for k in range(12, len(nf)) if nf[k] > nf[k - 1])     # (col = m from iteration 11 on)
    assert grew >= 1


@pytest.mark.parametrize("case", ["quad4099_m10", "fuzz9100"])
def test_stale_layout_is_still_refused(env, case):
    """the tiles are sorted in every iteration up to one and never again: the first storing pass that meets a free row
    without a layout bit must refuse (E_STATE), under both load paths and at the same call"""
    from test_gpu_fuzz import make
    po = env["po"]
    p, freeze = (po.problem_quadratic(4099, 10), 5) if case == "quad4099_m10" else (make(po, 9100, 3000, 1, 11), 3)
    assert p.m <= 10
    a = _ab(env, p, 40, "frozen layout " + case, compact_w=2, compact_policy=2, policy_after=(freeze, 0))
    assert a["err"] is not None and "older than the free set" in a["err"], a["err"]
    assert a["stats"][0] >= freeze - 1 and a["stats"][2] == 1, a["stats"]
