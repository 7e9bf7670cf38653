"""Bounds that the caller edits during a run (LBFGSB_F_FOLLOW_BOUNDS, lbfgsb_hip_bounds_changed).

The reference re-reads l, u and nbd on every setulb call; the oracle is the reference's own reverse-communication
loop, so it follows any edit by construction.  Here the same edits are made at the same returns on both sides:
trajectories to 30 iterations or termination, two calls from an imported state around an edit (the call after
the edit must drop what the call before it computed ahead of time from the old bounds), the announcement without
the flag, the flag without edits (bit for bit the default), and the snapshot's modes and counters.
"""
import numpy as np
import pytest

from test_gpu_parity import compare_states, nrm_close, _dev

pytestmark = pytest.mark.gpu

TIME_D = [5, 6, 7, 8, 9]      # dsave(6:10): wall-clock slots
RTOL = 1e-10


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


# ---- problems: the four bound modes of test_gpu_api's edit test ----
def make(po, mode, n=4099, m=6):
    if mode == "uniform":                          # mask 7
        return po.problem_quadratic(n, m)
    if mode == "dict":                             # mask 11: l alternates 1 / -100
        return po.problem_rosenbrock(n, m, 0.0, 0.0)
    if mode == "nbd":                              # mask 3: nbd streamed
        return po.problem_quadratic(n, m, mixed_nbd=True)
    p = po.problem_quadratic(n, m)                 # mask 6: n distinct lower bounds, l streamed
    p.l[:] = -1.0 - np.arange(n) / n
    return p


MASK = {"uniform": 7, "dict": 11, "nbd": 3, "plain": 6}


# ---- edits: (l, u, nbd) -> None, the same on numpy (oracle) and torch (GPU) arrays ----
def e_u(l, u, nbd): u[7:71] = -0.25                             # noqa: E302,E704
def e_l(l, u, nbd): l[11:75] = 0.125                            # noqa: E302,E704
def e_nbd20(l, u, nbd): nbd[8:72] = 0                           # noqa: E302,E704
def e_nbd02(l, u, nbd): nbd[5] = 0; nbd[4] = 2                   # noqa: E302,E702,E704  (mixed nbd: row 4 is 0)
def e_tighten(l, u, nbd): u[:] = 0.5                             # noqa: E302,E704
def e_loosen(l, u, nbd): u[:] = 1.5                              # noqa: E302,E704
def e_infeasible(l, u, nbd): u[:200] = -1.5; l[:200] = -1.75     # noqa: E302,E702,E704  (x_i >= -1 > u_i: x outside)


def e_to_plain(l, u, nbd):
    # uniform -> plain: n distinct upper bounds
    n = u.shape[0]
    if isinstance(u, np.ndarray):
        u[:] = 0.6 + np.arange(n) / (4.0 * n)
    else:
        import torch
        u.copy_(torch.from_numpy(0.6 + np.arange(n) / (4.0 * n)).to(u.dtype))


def e_to_dict(l, u, nbd):
    # plain -> dictionary: two values each
    l[:] = -1.0
    l[::2] = -0.5
    u[:] = 1.0
    u[1::2] = 0.75


def apply(edit, p_or_arrays):
    l, u, nbd = p_or_arrays
    edit(l, u, nbd)


def oracle_rows(po, p, events, max_iter=30):
    """events: {(kind, iter): edit}; kind 'FG_ST' / 'NEW_X' / 'FG_LN' (the first such return at that iteration)"""
    rows, done = [], set()

    def snap(k, s):
        t = s.task_s
        it = int(s.isave[29])
        key = (t[:5], it)
        if key in events and key not in done:
            done.add(key)
            apply(events[key], (p.l, p.u, p.nbd))
        if t.startswith("NEW_X"):
            rows.append(row_of(it, s.isave, s.f[0], s.x, s.g))
    s = po.run(po.Engine("oracle"), p, max_iter=max_iter, snapshot=snap)
    return rows, s.task_s


def row_of(it, isave, f, x, g):
    return (it, int(isave[33]), int(isave[32]), int(isave[37]), float(f), np.array(x, np.float64),
            np.array(g, np.float64))


def gpu_rows(env, p, events, max_iter=30, announce=False, follow=True, sol_kw=None, stats=None):
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(p.n, p.m, follow_bounds=follow, **(sol_kw or {}))
    rows, done = [], set()
    try:
        x, g = _dev(torch, p.x0.copy()), torch.zeros(p.n, dtype=torch.float64 if p.real == np.float64
                                                      else torch.float32).cuda()
        l, u, nbd = _dev(torch, p.l.copy()), _dev(torch, p.u.copy()), _dev(torch, p.nbd.astype(np.int32))
        t = ""
        for _ in range(100000):
            t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            it = int(sol.isave[29])
            key = (t[:5], it)
            if key in events and key not in done:
                done.add(key)
                apply(events[key], (l, u, nbd))
                torch.cuda.synchronize()
                if announce:
                    sol.bounds_changed()
                if stats is not None:
                    stats.append(("edit", key))
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            elif t.startswith("NEW_X"):
                rows.append(row_of(it, sol.isave, sol.f[0], x.cpu().numpy(), g.cpu().numpy()))
                if stats is not None:
                    stats.append((it, sol.uniform_bounds(), sol.bounds_stats()))
                if it >= max_iter:
                    break
            else:
                break
    finally:
        sol.close()
    return rows, t


def same_rows(got, exp, rtol=RTOL):
    assert len(got) == len(exp), (len(got), len(exp))
    for a, b in zip(got, exp):
        assert a[:4] == b[:4], ("iter, nfg, nseg, nfree", a[:4], b[:4])
        assert abs(a[4] - b[4]) <= rtol * max(abs(b[4]), 1e-2), ("f", a[0], a[4], b[4])
        nrm_close(a[5], b[5], rtol, "x at iteration %d" % a[0])
        # (near the solution g is tiny: rounding of the reassociated sums is measured against a floor)
        nrm_close(a[6], b[6], rtol, "g at iteration %d" % a[0], floor=1e-2)


TRAJ = [
    ("uniform", {("NEW_X", 3): e_u}),
    ("uniform", {("FG_ST", 0): e_tighten}),
    ("uniform", {("NEW_X", 2): e_tighten, ("NEW_X", 9): e_loosen}),
    ("uniform", {("FG_LN", 4): e_l}),
    ("uniform", {("NEW_X", 3): e_to_plain}),
    ("uniform", {("NEW_X", 5): e_infeasible}),
    ("uniform", {("NEW_X", 2): e_nbd20}),
    ("dict", {("NEW_X", 3): e_l, ("FG_LN", 6): e_nbd20}),
    ("dict", {("FG_LN", 2): e_u}),
    ("nbd", {("NEW_X", 3): e_nbd02}),
    ("nbd", {("FG_LN", 3): e_tighten}),
    ("plain", {("NEW_X", 3): e_to_dict}),
    ("plain", {("NEW_X", 4): e_l, ("FG_LN", 7): e_u}),
    ("plain", {("NEW_X", 4): e_infeasible}),
]


@pytest.mark.parametrize("mode,events", TRAJ, ids=["%s-%d" % (c[0], i) for i, c in enumerate(TRAJ)])
def test_trajectory_follows_edits_like_the_oracle(env, mode, events):
    """Every NEW_X row (iteration, nfg, nseg, nfree exactly; f, x, g to 1e-10) and the final task equal the
    oracle's when both sides make the same edits at the same returns."""
    po = env["po"]
    exp, t_exp = oracle_rows(po, make(po, mode), events)
    got, t_got = gpu_rows(env, make(po, mode), events)
    assert t_got[:20] == t_exp[:20], (t_got, t_exp)
    same_rows(got, exp)
    assert len(exp) >= 5


def test_announcement_without_the_flag_gives_the_flags_rows(env):
    """lbfgsb_hip_bounds_changed after each edit: the rows of the flag's run, bit for bit."""
    po = env["po"]
    for mode, events in (TRAJ[2], TRAJ[7], TRAJ[12]):
        a, ta = gpu_rows(env, make(po, mode), events, follow=True)
        b, tb = gpu_rows(env, make(po, mode), events, follow=False, announce=True)
        assert ta == tb
        assert len(a) == len(b)
        for ra, rb in zip(a, b):
            assert ra[:5] == rb[:5]
            assert np.array_equal(ra[5], rb[5]) and np.array_equal(ra[6], rb[6])


def _run_bits(env, p, follow, kw, opts, max_iter, pp=False):
    """NEW_X returns as bytes; pp: the ping-pong entry (setulb_pp), the iterate in the pair it names"""
    torch, la = env["torch"], env["la"]
    sol = la.DeviceSolver(p.n, p.m, follow_bounds=follow, options=opts, **kw)
    out = []
    try:
        dt = torch.float32 if p.real == np.float32 else torch.float64
        xs = (_dev(torch, p.x0.copy()), torch.zeros(p.n, dtype=dt).cuda())
        gs = (torch.zeros(p.n, dtype=dt).cuda(), torch.zeros(p.n, dtype=dt).cuda())
        l, u, nbd = _dev(torch, p.l.copy()), _dev(torch, p.u.copy()), _dev(torch, p.nbd.astype(np.int32))
        for _ in range(100000):
            if pp:
                t, cur = sol.setulb_pp(xs, l, u, nbd, gs, p.factr, p.pgtol)
            else:
                t, cur = sol.setulb(xs[0], l, u, nbd, gs[0], p.factr, p.pgtol), 0
            x, g = xs[cur], gs[cur]
            if t.startswith("FG"):
                sol.sync()
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            elif t.startswith("NEW_X"):
                d = sol.dsave.copy()
                d[TIME_D] = 0
                out.append((x.cpu().numpy().tobytes(), g.cpu().numpy().tobytes(), float(sol.f[0]),
                            sol.isave.copy().tobytes(), d.tobytes()))
                if sol.isave[29] >= max_iter:
                    break
            else:
                out.append(t)
                break
        st = sol.bounds_stats()
        packs = sol.compact_stats()[0]
    finally:
        sol.close()
    return out, st, packs


@pytest.mark.parametrize("case", ["n1e6_compact_pp_defer", "real32_m20", "wide_m40"])
def test_flag_without_edits_changes_nothing(env, case):
    """With the flag and no edit every NEW_X return (x, g, f, isave, dsave without its clock slots) is the
    default's, bit for bit; one comparison pass per entry after START, no change found.  The first case packs W
    (compact_w = 1 with the size threshold lowered), uses the ping-pong entry and LBFGSB_F_DEFER_LNSRCH -- which
    the flag turns off: the set-up then runs in its own call, with the same numbers."""
    po = env["po"]
    pp = False
    if case == "n1e6_compact_pp_defer":
        p, it, pp = po.problem_quadratic(1000000, 10), 24, True
        kw = {"defer_lnsrch": True, "same_stream_objective": True}
        opts = {"compact_w": 1, "compact_min_rows": 0}
    elif case == "real32_m20":
        p, kw, opts, it = po.problem_quadratic(20011, 20, real=np.float32), {"real32": True}, {}, 26
    else:
        p, kw, opts, it = po.problem_quadratic(20011, 40, mixed_nbd=True), {}, {}, 30
    a, st_a, packs_a = _run_bits(env, p, False, kw, opts, it, pp)
    b, st_b, packs_b = _run_bits(env, p, True, kw, opts, it, pp)
    assert len(a) == len(b) and len(a) >= 10
    for ra, rb in zip(a, b):
        assert ra == rb
    assert st_a == (0, 0, 0)
    assert st_b[0] >= len(a) and st_b[1:] == (0, 0), st_b
    if pp:
        assert packs_a >= 1 and packs_b >= 1, (packs_a, packs_b)


def test_modes_and_counters_after_each_transition(env):
    """uniform -> uniform with a new value -> plain -> dictionary; uniform_bounds() and bounds_stats() after
    each edit; a new pointer for u counts as a change."""
    po, torch = env["po"], env["torch"]
    p = make(po, "uniform")
    events = {("NEW_X", 2): e_tighten, ("NEW_X", 4): e_to_plain, ("NEW_X", 6): e_to_dict}
    log = []
    rows, _ = gpu_rows(env, p, events, max_iter=8, stats=log)
    masks = {e[0]: e[1] for e in log if e[0] != "edit"}
    st = {e[0]: e[2] for e in log if e[0] != "edit"}
    assert masks[1] == 7 and masks[2] == 7
    assert masks[3] == 7        # the new uniform value (tb.u = 0.5)
    assert masks[5] == 5        # n distinct u: streamed; l, nbd stay uniform
    assert masks[7] == 11       # two values of l and of u: dictionary
    assert st[2][1:] == (0, 0) and st[3][1:] == (1, 1) and st[5][1:] == (2, 2) and st[7][1:] == (3, 3)
    # a pointer change under the flag
    la = env["la"]
    sol = la.DeviceSolver(p.n, p.m, follow_bounds=True)
    try:
        x = _dev(torch, p.x0.copy())
        g = torch.zeros_like(x)
        l, u, nbd = _dev(torch, p.l.copy()), _dev(torch, p.u.copy()), _dev(torch, p.nbd.astype(np.int32))
        u2 = u.clone()
        for _ in range(200):
            t = sol.setulb(x, l, u if sol.isave[29] < 2 else u2, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            elif not t.startswith("NEW_X") or sol.isave[29] >= 3:
                break
        assert sol.bounds_stats()[1:] == (1, 1)
        assert sol.uniform_bounds() == 7
    finally:
        sol.close()


def test_invalid_nbd_ends_the_run(env):
    po = env["po"]
    p = make(po, "uniform")

    def bad(l, u, nbd): nbd[5] = 7     # noqa: E306,E704
    rows, t = gpu_rows(env, p, {("NEW_X", 2): bad})
    assert t.startswith("ERROR: INVALID NBD"), t
    assert rows[-1][0] == 2


# ---- two calls from an imported state around an edit ----
TWO = [("uniform", "NEW_X", e_tighten), ("uniform", "NEW_X", e_infeasible), ("uniform", "FG_LN", e_u),
       ("dict", "NEW_X", e_l), ("dict", "FG_LN", e_nbd20), ("nbd", "NEW_X", e_nbd02), ("nbd", "FG_LN", e_tighten),
       ("plain", "NEW_X", e_to_dict), ("plain", "FG_LN", e_u), ("uniform", "NEW_X", e_to_plain)]


@pytest.mark.parametrize("mode,when,edit", TWO, ids=["%s-%s-%d" % (c[0], c[1], i) for i, c in enumerate(TWO)])
def test_two_calls_around_an_edit_from_identical_state(env, mode, when, edit):
    """Import the oracle's state one return BEFORE an edit into a context with the flag; call 1 reproduces the
    oracle's next return with the old bounds (and computes the next call's products ahead of time), then the
    same edit is made on both sides and call 2 must reproduce the oracle's call with the new bounds."""
    po, torch, la = env["po"], env["torch"], env["la"]
    p = make(po, mode, n=1000, m=6)
    snaps = []
    po.run(po.Engine("oracle"), p, max_calls=40, snapshot=lambda k, s: snaps.append(s.copy()))
    tested = 0
    for k in range(4, len(snaps) - 1):
        s0, s1 = snaps[k - 1], snaps[k]
        if not s1.task_s.startswith(when) or not s0.task_s.startswith("FG_LN" if when == "NEW_X" else "NEW_X"):
            continue
        if when == "NEW_X" and int(s0.isave[35]) != 1:   # (the first trial: the update pass ran as its evaluation)
            continue
        # oracle: the call after the edit
        pe = make(po, mode, n=1000, m=6)
        apply(edit, (pe.l, pe.u, pe.nbd))
        s2 = s1.copy()
        if s2.task_s.startswith("FG"):
            s2.f[0] = pe.fg(s2.x, s2.g)
        po.call(po.Engine("oracle"), pe, s2)
        s = s0.copy()
        if s.task_s.startswith("FG"):
            s.f[0] = p.fg(s.x, s.g)
        sol = la.DeviceSolver(p.n, p.m, follow_bounds=True)
        try:
            x, g = _dev(torch, s.x), _dev(torch, s.g)
            l, u, nbd = _dev(torch, p.l), _dev(torch, p.u), _dev(torch, p.nbd.astype(np.int32))
            sol.import_state(s.wa, s.iwa, s.isave)
            sol.task[:] = s.task
            sol.csave[:] = s.csave
            sol.lsave[:] = s.lsave
            sol.isave[:] = s.isave
            sol.dsave[:] = s.dsave
            sol.f[0] = s.f[0]

            def snapshot():
                torch.cuda.synchronize()
                wa, iwa = sol.export_state()
                return po.State(p.n, p.m, x.cpu().numpy(), g.cpu().numpy(), sol.f.copy(), wa, iwa,
                                sol.task.copy(), sol.csave.copy(), sol.lsave.copy(), sol.isave.copy(),
                                sol.dsave.copy())
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            out1 = snapshot()
            compare_states(out1, s1, p.n, p.m, po, skip=("xp",), check_indx2=False, check_iwhere=False)
            apply(edit, (l, u, nbd))
            torch.cuda.synchronize()
            if out1.task_s.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
            before = sol.bounds_stats()
            sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            out2 = snapshot()
            # (iwhere: checked where call 2 ends at FG_LNSRCH -- after its cauchy and freev; at a NEW_X return it
            #  already holds the next scan's pattern by design)
            compare_states(out2, s2, p.n, p.m, po, skip=("xp",), check_indx2=False,
                           check_iwhere=out2.task_s.startswith("FG_LN"))
            after = sol.bounds_stats()
            # call 2 itself found the edit (the rebuild that import_state forces belongs to call 1)
            assert after[1] == before[1] + 1 and after[2] == before[2] + 1, (before, after)
        finally:
            sol.close()
        tested += 1
        if tested >= 3:
            break
    assert tested >= 1


def test_rebuild_behind_a_deferred_builtin_objective(env):
    """The built-in objective may leave f on the device for the next call's first fetch; a rebuild in that call
    (whose analysis fetches reuse the same slots) must not lose it: the rows equal those of an objective that
    returns f at once, with the same edits."""
    po, torch, la = env["po"], env["torch"], env["la"]
    p = po.problem_quadratic(4099, 6)
    events = {("NEW_X", 3): e_u, ("FG_LN", 5): e_to_plain}

    def run(deferred):
        sol = la.DeviceSolver(p.n, p.m, follow_bounds=True)
        rows, done = [], set()
        try:
            x, g = _dev(torch, p.x0.copy()), torch.zeros(p.n, dtype=torch.float64).cuda()
            l, u, nbd = _dev(torch, p.l.copy()), _dev(torch, p.u.copy()), _dev(torch, p.nbd.astype(np.int32))
            for _ in range(10000):
                t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
                key = (t[:5], int(sol.isave[29]))
                if key in events and key not in done:
                    done.add(key)
                    apply(events[key], (l, u, nbd))
                    torch.cuda.synchronize()
                if t.startswith("FG"):
                    if deferred:
                        sol.objective(0, x, g, deferred=True)
                    else:
                        sol.f[0] = sol.objective(0, x, g)
                elif t.startswith("NEW_X"):
                    rows.append((int(sol.isave[29]), int(sol.isave[33]), float(sol.f[0]), x.cpu().numpy().tobytes()))
                    if sol.isave[29] >= 12:
                        break
                else:
                    break
            assert sol.bounds_stats()[2] == 2
        finally:
            sol.close()
        return rows
    a, b = run(False), run(True)
    assert len(a) == len(b) == 12
    assert a == b


def test_announcement_refused_while_a_line_search_set_up_is_deferred(env):
    """Without the flag, LBFGSB_F_DEFER_LNSRCH runs a line search's set-up in the call after the one the reference
    runs it in; an edit announced at such an FG_LNSRCH return would reach it with the new bounds: refused."""
    po, torch, la = env["po"], env["torch"], env["la"]
    p = po.problem_quadratic(4099, 6)
    sol = la.DeviceSolver(p.n, p.m, defer_lnsrch=True, same_stream_objective=True)
    try:
        x, g = _dev(torch, p.x0.copy()), torch.zeros(p.n, dtype=torch.float64).cuda()
        l, u, nbd = _dev(torch, p.l.copy()), _dev(torch, p.u.copy()), _dev(torch, p.nbd.astype(np.int32))
        refused = False
        for _ in range(400):
            before = sol.defer_stats()[0]
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG_LN") and sol.defer_stats()[0] > before:
                with pytest.raises(la.LbfgsbError):
                    sol.bounds_changed()
                refused = True
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif t.startswith("NEW_X"):
                sol.bounds_changed()                  # (allowed here)
                if refused:
                    break
            else:
                break
        assert refused
    finally:
        sol.close()
