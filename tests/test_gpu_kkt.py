"""The active set, the bound multipliers and the projected gradient as device data (lbfgsb_hip_kkt /
lbfgsb_hip_kkt_list, DeviceSolver.kkt / kkt_indices) against a numpy restatement of the definitions in
include/lbfgsb_hip.h: every per-row output and the summary bit for bit (zeros by value: fmin / fmax do not fix the sign
of a zero result), every subset of the optional outputs, the ordered lists with every capacity rule, runs that call
both entries at every permitted return and compute the same bits as runs that do not, and the refusals."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
GUARD = 64  # elements behind every output that must stay as they were

# Sizes: below, at and above one wave and one workgroup of either real kind (2 / 4 rows per lane, scalar tails of
# 1 .. 3 rows), several workgroups (1000, 4099), and N_BIG.  The report's grid is grid_for(n, V) = min(2048,
# ceil(n / V / 256)) workgroups of 256 lanes with V = 2 (fp64) or 4 (fp32) rows per lane: at n / V >= 2 * 2048 * 256
# all 2048 workgroups are launched and every lane takes at least two trips.  N_BIG = 2 * 4 * 2048 * 256 + 4 * 1000 + 3
# gives fp32 two trips everywhere, a third in the first 1000 lanes and a scalar tail of 3 rows; fp64 (V = 2) four
# trips, a fifth in the first 2001 lanes and a tail of 1.
# For the lists N_BIG is 1025 chunks of 4096 rows (KKT_LIST_CHUNK): more chunk totals than the scan's 256 threads, so
# every thread scans a run of 5 chunks and the last threads none.
N_BIG = 2 * 4 * 2048 * 256 + 4 * 1000 + 3
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4099, N_BIG]
CNT = ("n_unbounded", "n_free", "n_lower", "n_upper", "n_fixed", "n_binding", "n_weak", "n_leaving", "n_outside")
VAL = ("pg_max", "mult_max", "out_max", "gfree_max")


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd, lib=lbfgsb_amd.load_library())


# ---------------------------------------------------------------------------------------------- the restatement
def make_case(n, real, seed):
    """random nbd in 0..3; a third of the rows exactly at a bound, a few one ulp outside; rows with l == u and with
    u < l; g with zeros, tiny values, values at +-TOL and both signs at bounds; unused bounds are NaN"""
    rng = np.random.default_rng(seed)
    nbd = rng.integers(0, 4, n).astype(np.int32)
    l = rng.uniform(-2.0, 0.0, n)
    u = l + rng.uniform(0.1, 2.0, n)
    k = rng.random(n)
    u[k < 0.06] = l[k < 0.06]
    inv = (k >= 0.06) & (k < 0.10)
    u[inv] = l[inv] - 0.5
    l, u = l.astype(real), u.astype(real)
    x = (l + (u - l) * rng.random(n).astype(real)).astype(real)
    r = rng.random(n)
    x = np.where(r < 1 / 6, l, x)
    x = np.where((r >= 1 / 6) & (r < 1 / 3), u, x)
    x = np.where((r >= 1 / 3) & (r < 0.35), np.nextafter(l, real(-np.inf)), x)
    x = np.where((r >= 0.35) & (r < 0.37), np.nextafter(u, real(np.inf)), x).astype(real)
    g = rng.standard_normal(n)
    q = rng.random(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = np.where(q < 0.12, 0.0 * sign, g)                                    # zeros of both signs
    g = np.where((q >= 0.12) & (q < 0.24), sign * np.finfo(real).tiny * 4, g)  # tiny
    g = np.where((q >= 0.24) & (q < 0.32), sign * TOL, g)                    # exactly at the tolerance
    g = np.where((q >= 0.32) & (q < 0.40), sign * TOL * 0.5, g).astype(real)
    l[(nbd == 0) | (nbd == 3)] = np.nan
    u[(nbd == 0) | (nbd == 1)] = np.nan
    return x, l, u, nbd, g


TOL = float(np.float32(1e-3))  # (representable in both real kinds, so that |g| == tol happens)


def restate(x, l, u, nbd, g, tol):
    """the definitions of include/lbfgsb_hip.h in numpy: operands widened to double, outputs rounded to the real kind"""
    real = x.dtype.type
    X, L, U, G = (a.astype(np.float64) for a in (x, l, u, g))
    hasl, hasu = (nbd == 1) | (nbd == 2), (nbd == 2) | (nbd == 3)
    with np.errstate(invalid="ignore"):
        st = np.zeros(x.size, np.int8)
        st[hasu & (X >= U)] = 2
        st[hasl & (X <= L)] = 1
        st[(nbd == 2) & (U - L <= 0.0)] = 3
        st[nbd == 0] = -1
        pg = G.copy()
        neg = (G < 0.0) & (nbd >= 2)
        pg[neg] = np.maximum(X - U, G)[neg]
        pos = ~(G < 0.0) & (nbd != 0) & (nbd <= 2)
        pg[pos] = np.minimum(X - L, G)[pos]
        binding = ((st == 1) & (G > 0.0)) | ((st == 2) & (G < 0.0))
        mult = np.where((st == 3) | binding, G, 0.0)
        at = (st == 1) | (st == 2)
        outside = (hasl & (X < L)) | (hasu & (X > U))
        dist = np.maximum(np.where(hasl, L - X, 0.0), np.where(hasu, X - U, 0.0))
    cnt = [int(np.sum(st == c)) for c in (-1, 0, 1, 2, 3)]
    cnt += [int(binding.sum()), int((at & (np.abs(G) <= tol)).sum()),
            int((((st == 1) & (G < -tol)) | ((st == 2) & (G > tol))).sum()), int(outside.sum())]
    mx = lambda v: float(v.max()) if v.size else 0.0  # noqa: E731
    val = [mx(np.abs(pg)), mx(np.abs(mult)), mx(dist[outside]), mx(np.abs(G)[st <= 0])]
    return st, pg.astype(real), mult.astype(real), np.array(cnt, np.int64), np.array(val, np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    ui = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    ok = (a.view(ui) == b.view(ui)) | ((a == 0) & (b == 0))
    return bool(ok.all())


def _p(t):
    return None if t is None else C.c_void_p(int(t.data_ptr()))


def raw_kkt(env, sol, dev, tol, pg=None, mult=None, status=None):
    cnt, val = np.full(9, -7, np.int64), np.full(4, -7.0)
    rc = env["lib"].lbfgsb_hip_kkt(sol.h, *[_p(t) for t in dev], float(tol), _p(pg), _p(mult), _p(status),
                                   cnt.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p))
    return rc, cnt, val


# ------------------------------------------------------------------------------------- elementwise exactness
@pytest.mark.parametrize("real32", [False, True], ids=["fp64", "real32"])
@pytest.mark.parametrize("n", SIZES)
def test_report_is_exact(env, n, real32):
    torch, la = env["torch"], env["la"]
    real = np.float32 if real32 else np.float64
    tdt = torch.float32 if real32 else torch.float64
    host = make_case(n, real, seed=1000 + n)
    dev = [torch.from_numpy(a).cuda() for a in host]
    sol = la.DeviceSolver(n, 1, real32=real32)
    try:
        sbg = np.float64(sol.projgr(*[dev[k] for k in (0, 1, 2, 3, 4)]))
        summaries = {}
        for tol in (0.0, TOL):
            st, pg, mult, cnt, val = restate(*host, tol)
            # all three outputs, each with guarded memory behind it
            o_pg = torch.full((n + GUARD,), 12345.5, dtype=tdt, device="cuda")
            o_mu = torch.full((n + GUARD,), -54321.25, dtype=tdt, device="cuda")
            o_st = torch.full((n + GUARD,), 77, dtype=torch.int8, device="cuda")
            rc, c, v = raw_kkt(env, sol, dev, tol, o_pg, o_mu, o_st)
            assert rc == 0
            print("n=%d %s tol=%g counts %s values %s" % (n, real.__name__, tol, c.tolist(), v.tolist()))
            assert np.array_equal(c, cnt), (dict(zip(CNT, c)), dict(zip(CNT, cnt)))
            assert same_bits(v, val), (dict(zip(VAL, v)), dict(zip(VAL, val)))
            assert same_bits(v[:1], np.array([sbg])), (v[0], sbg)  # bit for bit lbfgsb_hip_projgr's
            assert c[:5].sum() == n
            h_pg, h_mu, h_st = o_pg.cpu().numpy(), o_mu.cpu().numpy(), o_st.cpu().numpy()
            assert np.array_equal(h_st[:n], st)
            assert same_bits(h_pg[:n], pg)
            assert same_bits(h_mu[:n], mult)
            nz = mult != 0
            assert same_bits(h_mu[:n][nz], host[4][nz])  # a nonzero multiplier is an exact copy of g
            assert np.all(h_pg[n:] == real(12345.5)) and np.all(h_mu[n:] == real(-54321.25)) and np.all(h_st[n:] == 77)
            # every subset of the outputs: the same summary, the same rows, nothing behind them
            for w_pg, w_mu, w_st in itertools.product((False, True), repeat=3):
                if w_pg and w_mu and w_st:
                    continue
                s_pg = torch.full((n + GUARD,), 12345.5, dtype=tdt, device="cuda") if w_pg else None
                s_mu = torch.full((n + GUARD,), -54321.25, dtype=tdt, device="cuda") if w_mu else None
                s_st = torch.full((n + GUARD,), 77, dtype=torch.int8, device="cuda") if w_st else None
                rc, c2, v2 = raw_kkt(env, sol, dev, tol, s_pg, s_mu, s_st)
                assert rc == 0
                assert np.array_equal(c2, c) and v2.tobytes() == v.tobytes(), (w_pg, w_mu, w_st)
                for got, full in ((s_pg, o_pg), (s_mu, o_mu), (s_st, o_st)):
                    if got is not None:
                        assert torch.equal(got, full), (w_pg, w_mu, w_st)
            summaries[tol] = c
        # the tolerance moves n_weak and n_leaving and nothing else
        a, b = summaries[0.0], summaries[TOL]
        assert np.array_equal(np.delete(a, [6, 7]), np.delete(b, [6, 7]))
        if n >= 1000:
            assert b[6] > a[6] > 0 and 0 < b[7] < a[7], (a, b)
        # the Python face: named fields, requested tensors only
        rep = sol.kkt(*dev, tol=TOL, mult=False)
        assert [getattr(rep, k) for k in CNT] == b.tolist() and rep.mult is None
        assert rep.pg_max == float(sbg) and rep.status.dtype == torch.int8 and rep.pg.shape == (n,)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------ lists
def raw_list(env, sol, status, mask, idx, cap):
    count = np.full(1, -7, np.int64)
    rc = env["lib"].lbfgsb_hip_kkt_list(sol.h, _p(status), int(mask), _p(idx), int(cap),
                                        count.ctypes.data_as(C.c_void_p))
    return rc, int(count[0])


@pytest.mark.parametrize("n", SIZES)
def test_lists_are_ordered_and_capped(env, n):
    torch, la = env["torch"], env["la"]
    rng = np.random.default_rng(77 + n)
    st = rng.integers(-1, 4, n).astype(np.int8)
    junk = rng.random(n) < 0.05
    st[junk] = rng.choice(np.array([-128, -2, 4, 5, 100, 127], np.int8), int(junk.sum()))  # select nothing
    row0 = 5_000_000_000 if n == 1000 else (17 if n % 2 else 0)  # (global indices: 64-bit, beyond 2^32 once)
    sol = la.DeviceSolver(n, 1, n_global=row0 + n, row0=row0)
    try:
        d_st = torch.from_numpy(st).cuda()
        masks = [1 << (c + 1) for c in (-1, 0, 1, 2, 3)] + [0b01100, 0b10011, 0, 31]
        for mask in masks:
            sel = np.zeros(n, bool)
            for c in range(-1, 4):
                if mask >> (c + 1) & 1:
                    sel |= st == c
            want = row0 + np.nonzero(sel)[0].astype(np.int64)
            rc, count = raw_list(env, sol, d_st, mask, None, 0)  # the counting call
            assert rc == 0 and count == want.size, (mask, count, want.size)
            for cap in sorted({want.size, want.size // 2, max(want.size - 1, 0), 1 if want.size > 1 else 0}):
                idx = torch.full((cap + GUARD,), -99, dtype=torch.int64, device="cuda")
                rc, count = raw_list(env, sol, d_st, mask, idx, cap)
                assert rc == 0 and count == want.size, (mask, cap, count)
                h = idx.cpu().numpy()
                assert np.array_equal(h[:min(cap, want.size)], want[:cap]), (mask, cap)
                assert np.all(h[min(cap, want.size):] == -99), (mask, cap)
        got = sol.kkt_indices(d_st, (1, 2))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(),
                                                           row0 + np.nonzero((st == 1) | (st == 2))[0])
        assert sol.kkt_indices(d_st, 3).numel() == int((st == 3).sum())
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------ in a run
def _drive(env, sol, p, max_iter, at_return=None, pp=False, builtin=None, deferred_f=False):
    """run p; at_return(sol, task, x, l, u, nbd, g) at every return; returns the digest of every return"""
    torch = env["torch"]
    real = torch.float32 if sol.real == np.float32 else torch.float64
    xs = [torch.from_numpy(p.x0.astype(sol.real)).cuda(), torch.zeros(p.n, dtype=real, device="cuda")]
    gs = [torch.zeros_like(xs[0]), torch.zeros_like(xs[0])]
    x, g = xs[0], gs[0]
    l, u = torch.from_numpy(p.l.astype(sol.real)).cuda(), torch.from_numpy(p.u.astype(sol.real)).cuda()
    nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
    rows = []
    t = ""
    for _ in range(100000):
        if pp:
            t, cur = sol.setulb_pp(xs, l, u, nbd, gs, p.factr, p.pgtol)
            x, g = xs[cur], gs[cur]
        else:
            t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        sol.sync()
        rows.append((t, sol.isave.tobytes(), sol.dsave[[0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15]].tobytes(),
                     sol.f.tobytes(), hashlib.sha1(x.cpu().numpy().tobytes()).hexdigest(),
                     hashlib.sha1(g.cpu().numpy().tobytes()).hexdigest()))
        if at_return is not None:
            at_return(sol, t, x, l, u, nbd, g)
        if t.startswith("FG"):
            if builtin is not None:
                r = sol.objective(builtin, x, g, deferred=deferred_f)
                if r is not None:
                    sol.f[0] = r
                elif at_return is not None:
                    at_return(sol, "PARKED", x, l, u, nbd, g)  # (f still on the device: the entries refuse)
            else:
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
        elif not t.startswith("NEW_X") or sol.isave[29] >= max_iter:
            break
    return rows, t


RUNS = {
    "classic": dict(pp=False),
    "pingpong": dict(pp=True),
    "pingpong_defer": dict(pp=True, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
    "builtin_deferred_f": dict(pp=False, builtin=1, deferred_f=True),
}


@pytest.mark.parametrize("n,m,iters", [(25, 5, 10000), (4099, 7, 30)], ids=["to_convergence", "n4099"])
@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name, n, m, iters):
    la = env["la"]
    cfg = RUNS[name]
    # (factr = 0: the run ends by the projected-gradient test alone)
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=1e-5)
    outs = []
    seen = {"ok": 0, "refused": 0, "new_x": 0, "conv": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t, x, l, u, nbd, g):
                try:
                    rep = s.kkt(x, l, u, nbd, g, tol=p.pgtol)
                    idx = s.kkt_indices(rep.status, (1, 2, 3))
                except la.LbfgsbError as e:
                    assert "-104" in str(e), e  # E_STATE: a deferred set-up or a parked f
                    assert t.startswith("FG_LN") or t == "PARKED", t
                    seen["refused"] += 1
                    return
                seen["ok"] += 1
                assert idx.numel() == rep.n_lower + rep.n_upper + rep.n_fixed
                if t.startswith("NEW_X") or t.startswith("CONV"):
                    seen["new_x"] += 1
                    assert np.float64(rep.pg_max).tobytes() == np.float64(s.dsave[12]).tobytes(), (t, rep.pg_max)
                if t.startswith("CONV"):
                    seen["conv"] += 1
                    assert rep.n_leaving == 0, rep
            rows, last = _drive(env, sol, p, iters, at_return=at if touch else None, pp=cfg["pp"],
                                builtin=cfg.get("builtin"), deferred_f=cfg.get("deferred_f", False))
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes()))
        finally:
            sol.close()
    assert outs[0] == outs[1]
    assert seen["ok"] > 10 and seen["new_x"] > 5, seen
    if n == 25:
        assert last.startswith("CONVERGENCE: NORM_OF_PROJECTED_GRADIENT"), last
        assert seen["conv"] == 1
    if name in ("pingpong_defer", "builtin_deferred_f"):
        assert seen["refused"] > 0, seen


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_arguments(env):
    la, torch, lib = env["la"], env["torch"], env["lib"]
    n, m = 300, 5
    p = env["po"].problem_rosenbrock(n, m)
    host = make_case(n, np.float64, 5)
    dev = [torch.from_numpy(a).cuda() for a in host]
    st = torch.zeros(n, dtype=torch.int8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    cnt, val, count = np.zeros(9, np.int64), np.zeros(4), np.zeros(1, np.int64)
    pc, pv, pn = (a.ctypes.data_as(C.c_void_p) for a in (cnt, val, count))
    ptr = [_p(t) for t in dev]
    sol = la.DeviceSolver(n, m)
    try:
        # no run is needed
        assert lib.lbfgsb_hip_kkt(sol.h, *ptr, 0.0, None, None, _p(st), pc, pv) == 0
        assert lib.lbfgsb_hip_kkt_list(sol.h, _p(st), 31, _p(idx), n, pn) == 0
        for k in range(5):  # a NULL input
            bad = list(ptr)
            bad[k] = None
            assert lib.lbfgsb_hip_kkt(sol.h, *bad, 0.0, None, None, None, pc, pv) == E_ARG, k
        assert lib.lbfgsb_hip_kkt(sol.h, *ptr, 0.0, None, None, None, None, pv) == E_ARG
        assert lib.lbfgsb_hip_kkt(sol.h, *ptr, 0.0, None, None, None, pc, None) == E_ARG
        assert lib.lbfgsb_hip_kkt(None, *ptr, 0.0, None, None, None, pc, pv) == E_ARG
        for tol in (-1e-300, -1.0, float("nan")):
            assert lib.lbfgsb_hip_kkt(sol.h, *ptr, tol, None, None, None, pc, pv) == E_ARG, tol
        assert lib.lbfgsb_hip_kkt(sol.h, *ptr, float("inf"), None, None, None, pc, pv) == 0
        for args in ((None, 31, _p(idx), n, pn), (_p(st), 31, _p(idx), n, None), (_p(st), 32, _p(idx), n, pn),
                     (_p(st), -1, _p(idx), n, pn), (_p(st), 31, _p(idx), -1, pn), (_p(st), 31, None, 1, pn)):
            assert lib.lbfgsb_hip_kkt_list(sol.h, *args) == E_ARG, args
    finally:
        sol.close()
    # a deferred FG_LNSRCH: E_STATE, and the run goes on as without the calls (test_run_does_not_notice compares
    # every return); here the codes themselves
    s2 = la.DeviceSolver(n, m, defer_lnsrch=True, same_stream_objective=True)
    try:
        codes = []

        def at(s, t, x, l, u, nbd, g):
            if t.startswith("FG_LN"):
                before = (cnt.copy(), val.copy(), count.copy())
                codes.append(lib.lbfgsb_hip_kkt(s.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), 0.0, None, None, _p(st),
                                                pc, pv))
                codes.append(lib.lbfgsb_hip_kkt_list(s.h, _p(st), 31, _p(idx), n, pn))
                if codes[-2] == E_STATE:  # (the summaries are untouched)
                    assert np.array_equal(before[0], cnt) and np.array_equal(before[1], val)
                if codes[-1] == E_STATE:
                    assert np.array_equal(before[2], count)
        _drive(env, s2, p, 10, at_return=at)
        assert E_STATE in codes and all(c in (0, E_STATE) for c in codes), codes
    finally:
        s2.close()
    # a built-in objective's value still on the device
    s3 = la.DeviceSolver(n, m)
    try:
        x = torch.from_numpy(p.x0.copy()).cuda()
        g = torch.zeros_like(x)
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        args = (_p(x), _p(l), _p(u), _p(nbd), _p(g), 0.0, None, None, _p(st), pc, pv)
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert t.startswith("FG")
        s3.objective(1, x, g, deferred=True)
        st.fill_(55)
        assert lib.lbfgsb_hip_kkt(s3.h, *args) == E_STATE
        assert lib.lbfgsb_hip_kkt_list(s3.h, _p(st), 31, _p(idx), n, pn) == E_STATE
        assert bool((st == 55).all())
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert lib.lbfgsb_hip_kkt(s3.h, *args) == 0
        assert lib.lbfgsb_hip_kkt_list(s3.h, _p(st), 31, _p(idx), n, pn) == 0 and count[0] == n
    finally:
        s3.close()
