"""Entries, sub-blocks and columns of the curvature model at index lists (lbfgsb_hip_qn_rows / qn_block / qn_cols /
qn_shift_block / qn_shift_cols; DeviceSolver.qn_rows / qn_block / qn_cols, QnShifted.block / columns).
  qn_rows equals the entries of export_state's Ws / Wy exactly, in fp64 and in REAL32.
  qn_block (B and H, square and rectangular) and qn_cols against the dense numpy model built from export_state
  (tests/test_gpu_qn_shift.py, _model) at np.ix_, within the project's bound for these operators, tol cond max|ref|
  with tol = 1e-10 (fp64) or 1e-5 (REAL32); the square block symmetric bit for bit.
  qn_shift_block / qn_shift_cols, d random in [0, 10] with every second row pinned and mu = 0.3, against the inverse of
  the dense free block; pinned entries exactly +0; LBFGSB_E_STATE without a shift and after the pairs change.
Shapes: n = 64 is less than one tile of rows, 4099 = 32 tiles and 3 rows; m = 17 gives two column tiles of the columns
pass, m = 40 three.  Each shape at a state with col < m and at one whose ring has wrapped (head != 1), and col = 0 at
the FG_START return.  One index list throughout: 0, 63, 64, 127, 128, n - 1 (those below n), ten random rows, one row
repeated, and the whole list reversed behind it.  Then the tile-local layout of W read as it is, runs that call the
entries at every NEW_X return bit-identical to runs that do not, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_qn import _drive, _problem
from test_gpu_qn_root import _slow_quadratic
from test_gpu_qn_shift import _cond, _model

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
MU = 0.3


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _idx_list(n, extra=()):
    rng = np.random.default_rng(n)
    base = [i for i in (0, 63, 64, 127, 128) if i < n] + [n - 1]
    lst = base + [int(i) for i in rng.choice(n, 10, replace=False)] + [int(i) for i in extra]
    lst.append(lst[7])  # (one row repeated)
    return np.array(lst + lst[::-1], np.int64)


def _second_list(n):
    rng = np.random.default_rng(3 * n + 1)
    return np.concatenate([[n - 1, 0], rng.choice(n, 7, replace=False)]).astype(np.int64)


def _shift_d(sol):
    """d random in [0, 10], every second row pinned: the inputs of tests/test_gpu_qn_shift.py, case (c)"""
    d = np.random.default_rng(5 * sol.n).uniform(0.0, 10.0, sol.n).astype(sol.real)
    d[::2] = np.inf
    return d


def _device(env, sol, idx, ib, unit=True):
    """every entry on the device, before export_state touches the layout"""
    torch = env["torch"]
    r = dict(idx=idx, ib=ib, rows=sol.qn_rows(idx))
    for inv in (False, True):
        r["sq", inv] = sol.qn_block(idx, inverse=inv)
        r["rect", inv] = sol.qn_block(idx, ib, inverse=inv)
        r["cols", inv] = sol.qn_cols(idx, inverse=inv).cpu().numpy().astype(np.float64)
        if unit:
            e = torch.zeros((len(idx), sol.n), dtype=torch.float32 if sol.real == np.float32 else torch.float64,
                            device="cuda")
            e[torch.arange(len(idx)), torch.from_numpy(idx)] = 1.0
            r["unit", inv] = sol.qn_apply(e, inverse=inv).cpu().numpy().astype(np.float64)
    d = _shift_d(sol)
    sh = sol.qn_shift(torch.from_numpy(d).cuda(), MU)
    r["d"], r["ssq"], r["srect"] = d.astype(np.float64), sh.block(idx), sh.block(idx, ib)
    r["scols"] = sh.columns(idx).cpu().numpy()
    assert r["scols"].dtype == sol.real
    r["scols"] = r["scols"].astype(np.float64)
    return r


def _compare(sol, r, wa, tol, tag):
    n, m = sol.n, sol.m
    idx, ib = r["idx"], r["ib"]
    B, col = _model(sol, wa)
    head = int(sol.isave[26])
    w64 = wa.astype(np.float64)
    Ws, Wy = w64[:m * n].reshape(m, n), w64[m * n:2 * m * n].reshape(m, n)
    order = [(head - 1 + j) % m for j in range(col)]
    ref_rows = np.concatenate([Ws[order][:, idx].T, Wy[order][:, idx].T], axis=1).reshape(len(idx), 2 * col)
    assert r["rows"].shape == ref_rows.shape and np.array_equal(r["rows"], ref_rows)  # exactly the stored values
    cond = _cond(B)
    H = np.linalg.inv(B)
    for inv, A in ((False, B), (True, H)):
        for key, jb in (("sq", idx), ("rect", ib)):
            ref = A[np.ix_(idx, jb)]
            err, bound = np.abs(r[key, inv] - ref).max(), tol * cond * np.abs(ref).max()
            print("%s n %d col %d %s %s: off by %.2e (bound %.2e, cond %.2e)"
                  % (tag, n, col, "H" if inv else "B", key, err, bound, cond))
            assert err <= bound
        assert np.array_equal(r["sq", inv], r["sq", inv].T)  # bit for bit
        ref = A[:, idx].T
        err, bound = np.abs(r["cols", inv] - ref).max(), tol * cond * np.abs(ref).max()
        far = np.abs(r["cols", inv] - r["unit", inv]).max() if ("unit", inv) in r else float("nan")
        print("%s n %d col %d %s cols: off by %.2e (bound %.2e); from qn_apply on unit vectors %.2e"
              % (tag, n, col, "H" if inv else "B", err, bound, far))
        assert err <= bound
    # the model plus a diagonal on the free rows
    free = np.isfinite(r["d"])
    A = (B + np.diag(np.where(free, MU + r["d"], 0.0)))[np.ix_(free, free)]
    sig = np.zeros((n, n))
    sig[np.ix_(free, free)] = np.linalg.inv(A)
    cond = _cond(A)
    for key, ref in (("ssq", sig[np.ix_(idx, idx)]), ("srect", sig[np.ix_(idx, ib)]), ("scols", sig[:, idx].T)):
        got = r[key]
        err, bound = np.abs(got - ref).max(), tol * cond * np.abs(ref).max()
        print("%s n %d col %d shifted %s: off by %.2e (bound %.2e, cond %.2e)" % (tag, n, col, key, err, bound, cond))
        assert err <= bound
        zero = ref == 0.0  # (the pinned rows and columns: the reference holds exact zeros there and nowhere else)
        assert zero.any() and np.all(got[zero] == 0.0) and not np.signbit(got[zero]).any()
    assert np.array_equal(r["ssq"], r["ssq"].T)
    return col


def _check_state(env, sol, tol, tag):
    idx, ib = _idx_list(sol.n), _second_list(sol.n)
    r = _device(env, sol, idx, ib)
    wa, _ = sol.export_state()
    return _compare(sol, r, wa, tol, tag)


def _wrapped(s):
    return int(s.isave[27]) == s.m and int(s.isave[30]) > s.m and int(s.isave[26]) != 1


def _check_empty(env, s):
    """no stored pair: the block is alpha [equal], the columns are alpha e_j, the rows are empty"""
    torch = env["torch"]
    n, theta = s.n, float(s.dsave[0])
    idx, ib = _idx_list(n), _second_list(n)
    assert s.qn_rows(idx).shape == (len(idx), 0)
    for inv, alpha in ((False, theta), (True, 1.0 / theta)):
        assert np.array_equal(s.qn_block(idx, inverse=inv), alpha * (idx[:, None] == idx[None, :]))
        assert np.array_equal(s.qn_block(idx, ib, inverse=inv), alpha * (idx[:, None] == ib[None, :]))
        ref = np.zeros((len(idx), n))
        ref[np.arange(len(idx)), idx] = alpha
        assert np.array_equal(s.qn_cols(idx, inverse=inv).cpu().numpy(), ref)
    d = _shift_d(s)
    sh = s.qn_shift(torch.from_numpy(d).cuda(), MU)
    w = np.where(np.isfinite(d), 1.0 / (theta + MU + d.astype(np.float64)), 0.0)
    got = sh.block(idx, ib)
    ref = w[idx][:, None] * (idx[:, None] == ib[None, :])
    assert np.abs(got - ref).max() <= 4e-16 * np.abs(ref).max()
    assert np.all(got[ref == 0.0] == 0.0) and not np.signbit(got).any()
    cols = sh.columns(idx).cpu().numpy()
    ref = np.zeros((len(idx), n))
    ref[np.arange(len(idx)), idx] = w[idx]
    assert np.abs(cols - ref).max() <= 4e-16 * np.abs(ref).max()
    assert np.all(cols[ref == 0.0] == 0.0) and not np.signbit(cols).any()


SHAPES = [(64, 5), (1000, 10), (4099, 17), (4099, 40)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_entries_fp64(env, n, m):
    """col = 0 (FG_START), a partly filled ring and a full ring whose head has wrapped (head != 1, from isave)"""
    la = env["la"]
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)  # (no early stop: the ring fills and wraps)
    sol = la.DeviceSolver(n, m)
    seen = {}
    try:
        def at(s, t):
            col = int(s.isave[27])
            if t.startswith("FG_START") and col == 0 and "empty" not in seen:
                _check_empty(env, s)
                seen["empty"] = 0
            if not t.startswith("NEW_X") or 2 * col > n:
                return
            if "part" not in seen and max(1, m // 2) <= col < m:
                seen["part"] = _check_state(env, s, 1e-10, "part")
            elif "wrapped" not in seen and _wrapped(s):
                assert int(s.isave[26]) != 1 and int(s.isave[29]) > m
                seen["wrapped"] = _check_state(env, s, 1e-10, "wrapped")
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert set(seen) == {"empty", "part", "wrapped"}, seen
    assert 0 < seen["part"] < m and seen["wrapped"] == m


@pytest.mark.parametrize("n,m", [(1000, 10), (4099, 17)])
def test_entries_real32(env, n, m):
    """W and out fp32, every sum and host result fp64; the rows still exactly the stored values"""
    la = env["la"]
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) in (2, m + 2):
                checked.append(_check_state(env, s, 1e-5, "fp32"))
        _drive(env, sol, p, max_iter=m + 2, at_return=at)
    finally:
        sol.close()
    assert len(checked) == 2 and checked[-1] == m


def test_more_than_64_pairs(env):
    """any number of stored pairs: 65 of them (five column tiles of the columns pass), where qn_diag, the roots and
    qn_shift_set refuse"""
    la = env["la"]
    lib = la.load_library()
    n, m = 1000, 70
    sol = la.DeviceSolver(n, m)
    try:
        _, t = _drive(env, sol, _slow_quadratic(env, n, m), max_iter=400, until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65, t
        idx, ib = _idx_list(n), _second_list(n)
        r = dict(idx=idx, ib=ib, rows=sol.qn_rows(idx))
        for inv in (False, True):
            r["sq", inv], r["rect", inv] = sol.qn_block(idx, inverse=inv), sol.qn_block(idx, ib, inverse=inv)
            r["cols", inv] = sol.qn_cols(idx, inverse=inv).cpu().numpy()
        out = np.zeros((len(idx), len(idx)))
        assert lib.lbfgsb_hip_qn_shift_block(sol.h, len(idx), _pi(idx), 0, None, _pd(out), len(idx)) == E_STATE
        wa, _ = sol.export_state()
        B, col = _model(sol, wa)
        cond = _cond(B)
        H = np.linalg.inv(B)
        for inv, A in ((False, B), (True, H)):
            for key, ref in (("sq", A[np.ix_(idx, idx)]), ("rect", A[np.ix_(idx, ib)]), ("cols", A[:, idx].T)):
                err, bound = np.abs(r[key, inv] - ref).max(), 1e-10 * cond * np.abs(ref).max()
                print("col 65 %s %s: off by %.2e (bound %.2e)" % ("H" if inv else "B", key, err, bound))
                assert err <= bound
    finally:
        sol.close()


@pytest.mark.parametrize("policy", [1, 2])
def test_layout_read_as_it_is(env, policy):
    """n = 4099, m = 10 on the bounded quadratic with W packed: the list holds free rows and rows at bounds of one
    tile, whose slots the two mask words of the tile decide"""
    la, torch = env["la"], env["torch"]
    n, m = 4099, 10
    p = _problem(env, "quadratic", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": policy, "compact_min_rows": 0})
    x = torch.from_numpy(p.x0.copy()).cuda()
    g = torch.zeros_like(x)
    l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
    nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
    done = False
    try:
        for _ in range(400):
            t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
            if t.startswith("FG"):
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                continue
            assert t.startswith("NEW_X"), t
            if int(sol.isave[27]) < 2 or not sol.compact_stats()[2]:
                assert sol.isave[29] < 40, "the layout never packed"
                continue
            xh = x.cpu().numpy()
            at_l = ((p.nbd == 1) | (p.nbd == 2)) & (xh <= p.l)
            at_u = ((p.nbd == 2) | (p.nbd == 3)) & (xh >= p.u)
            free = ~(at_l | at_u)
            tiles = [tl for tl in range(n // 128) if 0 < free[128 * tl:128 * tl + 128].sum() < 128]
            assert tiles, "no tile with free rows and rows at bounds"
            rows = np.arange(128 * tiles[0], 128 * tiles[0] + 128)
            extra = list(rows[free[rows]][:3]) + list(rows[~free[rows]][:3])
            idx, ib = _idx_list(n, extra), _second_list(n)
            before = sol.compact_stats()
            assert before[2]  # W is packed at the call
            r = _device(env, sol, idx, ib)
            again = _device(env, sol, idx, ib, unit=False)
            assert sol.compact_stats() == before  # (still packed: the entries read the layout as it is)
            wa, _ = sol.export_state()  # (puts W back into natural order: after the device's part)
            _compare(sol, r, wa, 1e-10, "packed policy %d" % policy)
            for key in ("rows", ("sq", True), ("rect", False), ("cols", True), "ssq", "scols"):
                assert np.array_equal(r[key], again[key])  # reproducible bit for bit
            done = True
            break
    finally:
        sol.close()
    assert done


RUNS = {
    "natural": dict(pp=False),
    "compact_w_1": dict(pp=True, n=1_000_000, m=5, kind="quadratic", builtin=0,
                        ctor=dict(options={"compact_w": 1, "compact_min_rows": 0})),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    la, torch = env["la"], env["torch"]
    cfg = RUNS[name]
    n, m = cfg.get("n", 4099), cfg.get("m", 7)
    p = _problem(env, cfg.get("kind", "rosenbrock"), n, m)
    iters = 30
    gen = torch.Generator(device="cpu").manual_seed(9)
    d = (10.0 * torch.rand(n, generator=gen, dtype=torch.float64)).cuda()
    d[::3] = float("inf")
    idx, few = _idx_list(n), _second_list(n)[:4]
    outs = []
    counts = {"ok": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                if not t.startswith("NEW_X"):
                    return
                s.qn_rows(idx)
                s.qn_block(idx, inverse=True)
                s.qn_cols(few, inverse=True)
                sh = s.qn_shift(d, MU)
                sh.block(idx, few)
                sh.columns(few)
                counts["ok"] += 1
            rows, _ = _drive(env, sol, p, iters, at_return=at if touch else None, pp=cfg["pp"],
                             builtin=cfg.get("builtin"))
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes(), sol.compact_stats()))
        finally:
            sol.close()
    new_x = sum(1 for row in outs[1][0] if row[0].startswith("NEW_X"))
    assert counts["ok"] == new_x and new_x >= 20  # (every NEW_X return of the touched run called all five)
    assert outs[0][0] == outs[1][0]  # task, isave, dsave, f, x and g of every return
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert outs[0][3] == outs[1][3]
    if name == "compact_w_1":
        assert outs[1][3][0] > 0, outs[1][3]  # the layout did pack


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_staleness_and_refusals(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    idx = _idx_list(n)
    k = len(idx)
    a = np.zeros((k, k))
    rows = np.zeros((2 * m, k))
    out = torch.zeros((k, n), dtype=torch.float64, device="cuda")
    d = torch.rand(n, dtype=torch.float64, device="cuda")
    big = np.zeros(4097, np.int64)
    abig = np.zeros(4097)

    def calls(s, ix=idx, kk=k, mode=1, ld=k, ldo=n, o=out):
        """the five entries with one argument varied"""
        op = None if o is None else o.data_ptr()
        ip = None if ix is None else _pi(ix)
        return [lib.lbfgsb_hip_qn_rows(s.h, kk, ip, _pd(rows), ld),
                lib.lbfgsb_hip_qn_block(s.h, mode, kk, ip, 0, None, _pd(a), ld),
                lib.lbfgsb_hip_qn_cols(s.h, mode, kk, ip, op, ldo),
                lib.lbfgsb_hip_qn_shift_block(s.h, kk, ip, 0, None, _pd(a), ld),
                lib.lbfgsb_hip_qn_shift_cols(s.h, kk, ip, op, ldo)]

    def snapshot(s):
        return (s.qn_rows(idx), s.qn_block(idx, inverse=True), s.qn_cols(idx[:5], inverse=True).cpu().numpy(),
                s.qn_shift(d, 0.5).block(idx), s.qn_shift(d, 0.5).columns(idx[:5]).cpu().numpy())

    sol = la.DeviceSolver(n, m)
    try:
        assert calls(sol) == [E_STATE] * 5  # no run
        state = {}

        def at(s, t):
            if not t.startswith("NEW_X"):
                return
            it = int(s.isave[29])
            if it == 3:
                assert calls(s) == [0, 0, 0, E_STATE, E_STATE]  # before any qn_shift_set
                ref = snapshot(s)
                state["iupdat"] = int(s.isave[30])
                bad = idx.copy()
                for v in (-1, n):
                    bad[4] = v
                    assert calls(s, ix=bad) == [E_ARG] * 5, v  # an index outside 0 .. n_global - 1
                bad[4] = n - 1
                assert calls(s, ix=bad) == [0] * 5
                assert calls(s, ix=None) == [E_ARG] * 5  # NULL pointers
                assert calls(s, o=None)[2::2] == [E_ARG] * 2
                assert lib.lbfgsb_hip_qn_rows(s.h, k, _pi(idx), None, k) == E_ARG
                assert lib.lbfgsb_hip_qn_block(s.h, 1, k, _pi(idx), 0, None, None, k) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_block(s.h, k, _pi(idx), 0, None, None, k) == E_ARG
                assert calls(s, kk=0) == [E_ARG] * 5  # k < 1
                assert lib.lbfgsb_hip_qn_block(s.h, 1, k, _pi(idx), 0, _pi(idx), _pd(a), k) == E_ARG  # kb < 1
                assert lib.lbfgsb_hip_qn_shift_block(s.h, k, _pi(idx), 0, _pi(idx), _pd(a), k) == E_ARG
                got = calls(s, ld=k - 1)  # an ld that is too small
                assert got[0] == got[1] == got[3] == E_ARG
                assert calls(s, ldo=n - 1)[2::2] == [E_ARG] * 2
                # k over the cap: 4097 indices for the host results, 129 for the columns
                assert lib.lbfgsb_hip_qn_rows(s.h, 4097, _pi(big), _pd(abig), 4097) == E_ARG
                assert lib.lbfgsb_hip_qn_block(s.h, 1, 4097, _pi(big), 0, None, _pd(abig), 4097) == E_ARG
                assert lib.lbfgsb_hip_qn_block(s.h, 1, 1, _pi(big), 4097, _pi(big), _pd(abig), 1) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_block(s.h, 4097, _pi(big), 0, None, _pd(abig), 4097) == E_ARG
                assert lib.lbfgsb_hip_qn_cols(s.h, 1, 129, _pi(big), out.data_ptr(), n) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_cols(s.h, 129, _pi(big), out.data_ptr(), n) == E_ARG
                for mode in (2, 4, 5, -1):  # root modes and no mode at all
                    got = calls(s, mode=mode)
                    assert got[1] == E_ARG and got[2] == E_ARG, mode
                # after every refusal: a valid call gives what it gave before
                for x, y in zip(ref, snapshot(s)):
                    assert np.array_equal(x, y)
                state["sh"] = s.qn_shift(d, 0.5)
                assert calls(s) == [0] * 5
            elif it == 4:
                assert int(s.isave[30]) > state["iupdat"]  # one more pair is stored
                assert calls(s) == [0, 0, 0, E_STATE, E_STATE]
                with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
                    state["sh"].block(idx)
                with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
                    state["sh"].columns(idx)
                op = s.qn_operator()
                assert np.array_equal(op.marginal(idx), s.qn_block(idx, inverse=True))
                assert np.array_equal(op.block(idx, idx[:3]), s.qn_block(idx, idx[:3], inverse=True))
                assert torch.equal(op.columns(idx[:3]), s.qn_cols(idx[:3], inverse=True))
                # index arguments: a device tensor is copied to the host
                dev = torch.from_numpy(idx).cuda()
                assert np.array_equal(s.qn_block(dev), s.qn_block(idx))
                assert np.array_equal(op.shifted(d, 0.5).block(dev, list(idx[:3])), s.qn_shift(d, 0.5).block(idx, idx[:3]))
                state["again"] = True

        _drive(env, sol, p, max_iter=5, at_return=at)
        assert state.get("again")
    finally:
        sol.close()
    # the deferred line-search set-up refuses as qn_apply does
    s2 = la.DeviceSolver(n, m, defer_lnsrch=True, same_stream_objective=True)
    refused = []
    try:
        def at2(s, t):
            if t.startswith("FG_LN"):
                refused.extend(calls(s)[:3])
        _drive(env, s2, p, 10, at_return=at2)
    finally:
        s2.close()
    assert E_STATE in refused and all(r in (0, E_STATE) for r in refused), refused
