"""The model along a path of shifts on the device (DeviceSolver.qn_path -> QnPath: lbfgsb_hip_qn_path_set / _logdet /
_solve / _trust).

Dense-truth cases (tests/_qn_path_truth.py, CASES: n in {1, 63, 130, 257, 400}, every qn_mc capacity and 1, 2, 3 column
tiles, k in {1, 2, 7, 64} shifts, five masks, fp64 and REAL32, out at an even or odd element offset), per shift:
the solve entry by entry within Truth.shifted(...).bound_apply, pinned rows exactly +0, v'x within bound_quad, ||x||^2
within bound_norm2, log det within bound_logdet -- |out - ref| <= bound, no further constant -- for EVERY shift; and
against the existing route on the same state, path.solve(v, [mu]) - qn_shift(d = +inf on the pinned rows, mu).solve(v)
entry by entry within the sum of the two bounds, log det within 2 bound_logdet (REAL32: the bounds of
_qn_path_truth.route_truth, the comparison that can see a wrong shift there).  The packed layout of a run at n = 1027
has its own Truth from the qn_rows pairs and the same checks.
Where no dense truth in extended precision is affordable or N is not determined (n = 3001 with "wgrid" 2, one free row
with stored pairs, 64 pairs on 257 rows, 64 shifts on the packed layout) the path and the existing route
qn_shift(d = +inf on the pinned rows, mu) are both held to a dense fp64 solve by the normwise bound of tests/test_qn_shift_cpu.py, 1e-12 cond(A) |ref|, and
to each other by twice that; log det to 1e-10 n each, 2e-10 n to each other.
Trust steps: the norm of the device's step in longdouble against delta, mu = 0 and step = -solve(g, [0]) bit for bit
inside the region, the predicted decrease against the dense reference.  Then: no hidden passes, staleness and every
refusal with nothing written, a live qn_shift next to a live path, and a run that does not notice the calls."""
import numpy as np
import pytest

import _qn_path_truth as pt
import _qn_truth as qt
from test_gpu_qn_root import _drive, _problem
from test_gpu_qn_switches import _dev, _np, _out

pytestmark = pytest.mark.gpu

LD = qt.LD
U = qt.U


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    """after the module: the worst err / bound of every entry family of its run (run with -s to read it)"""
    yield
    for tag in sorted(qt.RATIOS):
        if tag.startswith(("path", "trust")):
            print("%-44s %.3g" % (tag, qt.RATIOS[tag]))


def _status(env, pin):
    """int8 codes: 1 (at a lower bound) on the pinned rows, 0 elsewhere; None when nothing is pinned"""
    if not pin.any():
        return None
    return env["torch"].from_numpy(np.where(pin, 1, 0).astype(np.int8)).cuda()


def _solver(env, state):
    n, m, npairs, fam, real = state
    st, tr = pt.state_truth(state)
    sol = env["la"].DeviceSolver(n, m, real32=real == np.float32)
    sol.import_state(st.wa, st.iwa, st.isave)
    return st, tr, sol


def _vec(n, real, salt=0):
    return np.random.default_rng(4242 + n + salt).standard_normal(n).astype(real)


# ------------------------------------------------------------------------------------------------ dense truth
@pytest.mark.parametrize("case", pt.CASES, ids=pt.case_id)
def test_dense_truth(env, case):
    state, mask, k, off = case
    n, real = state[0], state[4]
    st, tr, sol = _solver(env, state)
    try:
        pin = pt.pin_mask(n, mask)
        path = sol.qn_path(_status(env, pin))
        assert path.pinned == int(pin.sum())
        mus = pt.shifts(case)
        v = _vec(n, real)
        out, n2, vx = path.solve(_dev(env, v, real, off), mus, out=_out(env, k, n, real, off), norms=True)
        out = _np(out)
        assert out.dtype == real and out.shape == (k, n)
        ld, info = path.logdet(mus)
        assert not info.any()
        assert qt.pos_zero(out[:, pin]).all()
        kd = "fp32" if real == np.float32 else "fp64"
        vd = _dev(env, v, real, 0)
        dd = _dev(env, np.where(pin, np.inf, 0.0), real, 0)
        rt = pt.route_truth(state)
        # every shift; with no free row every reference value is exactly 0 and N is undetermined: exact zeros instead
        for j in range(k):
            sh = sol.qn_shift(dd, float(mus[j]))   # the existing route: d = +inf on the pinned rows, this mu
            alt, ald = _np(sh.solve(vd)), sh.logdet()
            assert sh.pinned == path.pinned
            if mask == "all":
                assert qt.pos_zero(out[j]).all() and qt.pos_zero(alt).all() and ald == 0.0 and ld[j] == 0.0
                continue
            op = pt.shifted(tr, pin, mus[j])
            ref = op.apply(v[None])
            qt.check("path solve %s" % kd, out[j:j + 1], ref, op.bound_apply(v[None], real, ref))
            qt.check("path v'x %s" % kd, vx[j], op.quad(v[None])[0, 0], op.bound_quad(v[None])[0, 0])
            qt.check("path ||x||^2 %s" % kd, n2[j], pt.norm2(op, v), pt.bound_norm2(op, v))
            qt.check("path logdet %s" % kd, ld[j], op.logdet, op.bound_logdet(op.sum_abs_log, op.cond_a))
            # ... and against the route: within the sum of the two bounds (route_truth: what the two share drops out)
            rop = pt.shifted(rt, pin, mus[j])
            rref = rop.apply(v[None])
            qt.check("path against qn_shift, solve %s" % kd, out[j:j + 1], alt[None],
                     2 * rop.bound_apply(v[None], real, rref))
            qt.check("path against qn_shift, logdet %s" % kd, ld[j], ald,
                     2 * rop.bound_logdet(rop.sum_abs_log, rop.cond_a))
        if mask == "all":
            assert not n2.any() and not vx.any()
        # the scalars alone: the same numbers, nothing written
        _, n2b, vxb = path.solve(_dev(env, v, real, off), mus, out=False, norms=True)
        assert np.array_equal(n2, n2b) and np.array_equal(vx, vxb)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ the existing route
def _dense64(S, Y, theta):
    n = S.shape[0]
    B = theta * np.eye(n)
    for j in range(S.shape[1]):
        s, y = S[:, j], Y[:, j]
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
    return B


def _both_routes(env, sol, S, Y, theta, pin, mus, real, tag):
    """path.solve / logdet and qn_shift(d, mu).solve / logdet against a dense fp64 solve on the free rows and against
    each other"""
    torch = env["torch"]
    n = S.shape[0]
    free = ~pin
    v = _vec(n, real, 7)
    vd = torch.from_numpy(v).cuda()
    d = torch.from_numpy(np.where(pin, np.inf, 0.0).astype(real)).cuda()
    path = sol.qn_path(_status(env, pin))
    out = _np(path.solve(vd, mus)).astype(np.float64)
    ld, info = path.logdet(mus)
    assert not info.any() and qt.pos_zero(out[:, pin]).all()
    B = _dense64(S, Y, theta)[np.ix_(free, free)]
    f32 = 2.0 ** -24 if real == np.float32 else 0.0
    for j, mu in enumerate(mus):
        A = B + mu * np.eye(B.shape[0])
        ev = np.linalg.eigvalsh(A)
        cond = ev[-1] / ev[0]
        ref = np.zeros(n)
        ref[free] = np.linalg.solve(A, v[free].astype(np.float64))
        sh = sol.qn_shift(d, float(mu))
        alt = _np(sh.solve(vd)).astype(np.float64)
        b = (1e-12 * cond + f32) * np.linalg.norm(ref)
        e1, e2, e12 = (np.linalg.norm(a) for a in (out[j] - ref, alt - ref, out[j] - alt))
        print("%s mu %.3e: path off by %.2e, qn_shift by %.2e, apart %.2e (bound %.2e, cond %.1e)"
              % (tag, mu, e1, e2, e12, b, cond))
        assert e1 <= b and e2 <= b and e12 <= 2 * b
        ref_ld = np.linalg.slogdet(A)[1]
        l2 = sh.logdet()
        print("   log det %.12e, qn_shift %.12e, dense %.12e" % (ld[j], l2, ref_ld))
        assert abs(ld[j] - ref_ld) <= 1e-10 * n and abs(l2 - ref_ld) <= 1e-10 * n and abs(ld[j] - l2) <= 2e-10 * n
    return path


def test_one_free_row_with_pairs(env):
    for state in ((130, 10, 10, "generic", np.float64), (257, 17, 20, "dyadic", np.float64)):
        st, tr, sol = _solver(env, state)
        try:
            S, Y = st.pairs()
            pin = pt.pin_mask(state[0], "one_free")
            _both_routes(env, sol, S, Y, float(tr.theta), pin, [-0.3, 0.0, 5.0], state[4], "one free row")
        finally:
            sol.close()


def test_cap_of_pairs_and_shifts(env):
    """LBFGSB_QN_ROOT_MAXCOL = 64 stored pairs (4 column tiles) with LBFGSB_QN_PATH_MAXK = 64 shifts in one call: the
    most coefficients the expansion's buffer ever holds.  n = 257 rows determine no N for 128 columns to any accuracy,
    so every one of the 64 solves is held to the dense fp64 solve and to the qn_shift route"""
    state = (257, 64, 64, "generic", np.float64)
    st = __import__("_qn_synth").synth(*state)
    sol = env["la"].DeviceSolver(state[0], state[1])
    try:
        sol.import_state(st.wa, st.iwa, st.isave)
        S, Y = st.pairs()
        theta = float(Y[:, -1] @ Y[:, -1] / (S[:, -1] @ Y[:, -1]))
        _both_routes(env, sol, S, Y, theta, pt.pin_mask(257, "tile_edges"), pt.MUS[64], np.float64, "col 64, k 64")
    finally:
        sol.close()


@pytest.mark.parametrize("nt", [0, 1])
def test_grid_wrap(env, nt):
    """n = 3001 with "wgrid" 2: every workgroup makes several trips in the pin, Gram, read and write passes"""
    state = (3001, 10, 14, "generic", np.float64)
    st = __import__("_qn_synth").synth(*state)
    sol = env["la"].DeviceSolver(state[0], state[1], options={"wgrid": 2, "nt": nt})
    try:
        sol.import_state(st.wa, st.iwa, st.isave)
        S, Y = st.pairs()
        y = Y[:, -1]
        theta = float(y @ y / (S[:, -1] @ y))
        pin = np.zeros(3001, bool)
        pin[::3] = True
        pin[1000:1300] = True
        _both_routes(env, sol, S, Y, theta, pin, [0.0, 0.3, 40.0], np.float64, "wgrid 2 nt %d" % nt)
    finally:
        sol.close()


@pytest.mark.parametrize("m", [5, 10])
def test_packed_layout_read_as_it_is(env, m):
    """a run with compact_w on (fp64, m <= 10): W in the tile-local layout at the NEW_X return where the path is made;
    the pairs come through qn_rows, which reads the layout as it is, and the layout is still packed afterwards"""
    la, torch = env["la"], env["torch"]
    n = 1027
    p = _problem(env, "quadratic", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": 2, "compact_min_rows": 0})
    seen = []
    try:
        def at(s, t):
            if seen or not t.startswith("NEW_X") or not s.compact_stats()[2] or int(s.isave[27]) < min(m, 4):
                return
            col = int(s.isave[27])
            before = s.compact_stats()
            rows = s.qn_rows(np.arange(n, dtype=np.int64))
            S, Y = rows[:, :col].copy(), rows[:, col:].copy()
            pin = pt.pin_mask(n, "half")
            _both_routes(env, s, S, Y, float(s.dsave[0]), pin, [0.0] + pt.MUS[64][1:], np.float64, "packed m %d" % m)
            # the dense truth of this state (g = 2: a state from a run), entry by entry, and the route within 2 bounds
            tr = qt.Truth(S, Y, theta=float(s.dsave[0]), g=2)
            v = _vec(n, np.float64, 5)
            vd = _dev(env, v, np.float64, 0)
            mus = [0.3, 7.0]
            path = s.qn_path(_status(env, pin))
            out, n2, vx = path.solve(vd, mus, out=_out(env, 2, n, np.float64, 1), norms=True)
            out, (ld, info) = _np(out), path.logdet(mus)
            assert not info.any() and qt.pos_zero(out[:, pin]).all()
            dd = _dev(env, np.where(pin, np.inf, 0.0), np.float64, 0)
            for j, mu in enumerate(mus):
                op = pt.shifted(tr, pin, mu)
                ref = op.apply(v[None])
                ba, bl = op.bound_apply(v[None], np.float64, ref), op.bound_logdet(op.sum_abs_log, op.cond_a)
                qt.check("path solve packed", out[j:j + 1], ref, ba)
                qt.check("path v'x packed", vx[j], op.quad(v[None])[0, 0], op.bound_quad(v[None])[0, 0])
                qt.check("path ||x||^2 packed", n2[j], pt.norm2(op, v), pt.bound_norm2(op, v))
                qt.check("path logdet packed", ld[j], op.logdet, bl)
                sh = s.qn_shift(dd, mu)
                qt.check("path against qn_shift, solve packed", out[j:j + 1], _np(sh.solve(vd))[None], 2 * ba)
                qt.check("path against qn_shift, logdet packed", ld[j], sh.logdet(), 2 * bl)
            _both_routes(env, s, S, Y, float(s.dsave[0]), pt.pin_mask(n, "none"), [0.3], np.float64, "packed, no pins")
            assert s.compact_stats() == before and before[2]
            seen.append(col)
        _drive(env, sol, p, max_iter=6 * m + 20, at_return=at, until=lambda s: bool(seen))
    finally:
        sol.close()
    assert seen


# ------------------------------------------------------------------------------------------------ trust steps
@pytest.mark.parametrize("state,mask", [((257, 10, 10, "generic", np.float64), "half"),
                                        ((130, 17, 20, "dyadic", np.float32), "none"),
                                        ((63, 5, 0, "dyadic", np.float64), "tile_edges")],
                         ids=["n257-col10-half-fp64", "n130-col17-none-fp32", "n63-col0-fp64"])
def test_trust(env, state, mask):
    n, real = state[0], state[4]
    st, tr, sol = _solver(env, state)
    try:
        pin = pt.pin_mask(n, mask)
        path = sol.qn_path(_status(env, pin))
        g = _vec(n, real, 3)
        gd = _dev(env, g, real, 0)
        x0, n20, _ = path.solve(gd, [0.0], norms=True)
        x0n = float(np.sqrt(n20[0]))
        f32 = qt.U32 if real == np.float32 else 0.0
        for ratio in (2.0, 0.9, 1e-3):
            delta = ratio * x0n
            for rtol in (1e-6, 0.0):
                t = path.trust(gd, delta, rtol=rtol)
                step = _np(t.step)
                assert step.dtype == real and qt.pos_zero(step[pin]).all()
                sl = step.astype(LD)
                dev_norm = float(np.sqrt(sl @ sl))
                if ratio >= 1.0:
                    assert t.mu == 0.0 and not t.on_boundary and t.iters == 1
                    assert np.array_equal(step, -_np(x0)[0])  # (bit for bit: the same sums, every sign flipped)
                    assert dev_norm <= delta
                else:
                    assert t.mu > 0.0 and t.on_boundary and 1 < t.iters <= 100
                op = pt.shifted(tr, pin, t.mu)
                ref = -op.apply(g[None])[0]
                ba = op.bound_apply(g[None], real, ref[None])[0]
                qt.check("trust step", step, ref, ba)
                # ||x|| as the host knows it, and the device's step: each within its bound of the reference's norm
                rn = float(np.sqrt(pt.norm2(op, g)))
                bn = pt.bound_norm2(op, g) / (2 * rn) * (1 + 1e-3) + 4 * U * rn
                assert abs(t.norm - rn) <= bn
                bdev = float(np.sqrt(ba @ ba)) + f32 * rn
                eff = 1e-10 if rtol == 0.0 else rtol
                print("ratio %g rtol %g: mu %.6e iters %d | ||step|| - delta | = %.3e (allowed %.3e)"
                      % (ratio, rtol, t.mu, t.iters, abs(dev_norm - delta), eff * delta + bn + bdev))
                if ratio < 1.0:
                    assert abs(t.norm - delta) <= eff * delta
                    assert abs(dev_norm - delta) <= eff * delta + bn + bdev
                # the predicted decrease -(g's + s'B s / 2) of the reference step at this mu
                gl = g.astype(LD)
                Bs = op.fwd.A @ ref - LD(t.mu) * np.where(pin, 0, ref)
                pred = -(gl @ ref + (ref @ Bs) / 2)
                bp = 0.5 * op.bound_quad(g[None])[0, 0] + 0.5 * t.mu * pt.bound_norm2(op, g) \
                    + qt.gamma(6) * (abs(float(gl @ ref)) + t.mu * rn * rn)
                qt.check("trust predicted", t.predicted, pred, bp)
        # the scalars alone
        t = path.trust(gd, 0.9 * x0n, out=False)
        assert t.step is None and t.on_boundary
        # g_F = 0: the zero step
        z = path.trust(_dev(env, np.where(pin, g, 0).astype(real), real, 0), 1.0)
        assert (z.mu, z.norm, z.predicted, z.on_boundary, z.iters) == (0.0, 0.0, 0.0, False, 0)
        assert qt.pos_zero(_np(z.step)).all()
    finally:
        sol.close()


def test_every_row_pinned_trust(env):
    state = (130, 11, 11, "dyadic", np.float64)
    st, tr, sol = _solver(env, state)
    try:
        path = sol.qn_path(_status(env, pt.pin_mask(130, "all")))
        assert path.pinned == 130
        z = path.trust(_dev(env, _vec(130, np.float64), np.float64, 0), 0.5)
        assert (z.mu, z.norm, z.predicted, z.on_boundary) == (0.0, 0.0, 0.0, False) and qt.pos_zero(_np(z.step)).all()
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ no hidden passes
def test_no_hidden_passes(env):
    """What this can show: the number of host evaluations (iters) changes with rtol while nothing else of the call does,
    and 1000 shifts of logdet leave the context's counters as they were.  What it cannot: lbfgsb_hip_stats counts the
    launches and waits of the ITERATION only -- the curvature-model passes leave the Queue's counters alone, which is
    how a run does not notice them -- so the launch counts below would be equal whatever the entries launched.  For the
    same reason "no pins: no pass over W" has no test: no counter of the library sees it."""
    state = (257, 10, 10, "generic", np.float64)
    st, tr, sol = _solver(env, state)
    try:
        path = sol.qn_path(_status(env, pt.pin_mask(257, "half")))
        before = sol.stats()
        ld, info = path.logdet(np.geomspace(1e-3, 1e5, 1000))
        after = sol.stats()
        assert not info.any() and np.all(np.diff(ld) > 0)
        assert after["launches"] == before["launches"] and after["syncs"] == before["syncs"]
        g = _dev(env, _vec(257, np.float64), np.float64, 0)
        x0 = path.trust(g, 1e30).norm
        counts = []
        for rtol in (1e-2, 1e-12):
            a = sol.stats()
            t = path.trust(g, 0.1 * x0, rtol=rtol)
            b = sol.stats()
            counts.append((b["launches"] - a["launches"], b["syncs"] - a["syncs"], t.iters))
        assert counts[0][:2] == counts[1][:2] and counts[0][2] < counts[1][2], counts
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ staleness, refusals
def test_staleness_and_refusals(env):
    la, torch = env["la"], env["torch"]
    n, m = 257, 6
    st = __import__("_qn_synth").synth(n, m, 4, "generic", np.float64)
    S, Y = st.pairs()
    sol = la.DeviceSolver(n, m)
    try:
        sol.qn_set_pairs(np.ascontiguousarray(S.T), np.ascontiguousarray(Y.T))
        v = torch.from_numpy(_vec(n, np.float64)).cuda()
        pin = pt.pin_mask(n, "half")
        path = sol.qn_path(_status(env, pin))
        sh = sol.qn_shift(None, 0.3)          # a live shift next to the live path: neither disturbs the other
        a = _np(path.solve(v, [0.3]))
        b = _np(sh.solve(v))
        path2 = sol.qn_path(None)             # ... and a new path leaves the shift alone
        assert np.array_equal(_np(sh.solve(v)), b)
        sol.qn_shift(None, 9.0)
        c = _np(path2.solve(v, [0.3]))
        assert np.allclose(c[0], b, rtol=0, atol=1e-10 * np.abs(b).max())
        path = sol.qn_path(_status(env, pin))
        assert np.array_equal(_np(path.solve(v, [0.3])), a)
        # every LBFGSB_E_ARG, nothing written
        sentinel = 12345.0
        out = torch.full((3, n), sentinel, dtype=torch.float64, device="cuda")
        theta = float(Y[:, -1] @ Y[:, -1] / (S[:, -1] @ Y[:, -1]))
        for bad, code in (([0.3, -theta, 1.0], "-101"), ([0.3, float("nan"), 1.0], "-101"),
                          ([0.3, 1.0, float("inf")], "-101"), ([0.3, 1.0, -0.999 * theta], "-104")):
            with pytest.raises(la.LbfgsbError, match=code) as ei:
                path.solve(v, bad, out=out)
            assert "j = %d" % int(np.argmax([x != x or x == float("inf") or x < 0 for x in bad])) in str(ei.value)
            assert bool((out == sentinel).all())
        ld, info = path.logdet([0.3, -theta, float("nan"), -0.999 * theta])
        assert list(info) == [0, 1, 1, 2] and np.isfinite(ld[0]) and np.isnan(ld[1:]).all()
        with pytest.raises(la.LbfgsbError, match="-101"):
            path.solve(v, [0.1] * 65, out=False, norms=True)
        lib, h = sol.lib, sol.h
        import ctypes as C
        mu1 = (C.c_double * 1)(0.3)
        res, it = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), C.c_int32(-5)
        assert lib.lbfgsb_hip_qn_path_solve(h, v.data_ptr(), 1, mu1, None, n, None, None) == la.capi.E_ARG
        assert lib.lbfgsb_hip_qn_path_solve(h, None, 1, mu1, out.data_ptr(), n, None, None) == la.capi.E_ARG
        assert lib.lbfgsb_hip_qn_path_solve(h, v.data_ptr(), 0, mu1, out.data_ptr(), n, None, None) == la.capi.E_ARG
        assert lib.lbfgsb_hip_qn_path_solve(h, v.data_ptr(), 1, mu1, out.data_ptr(), n - 1, None, None) == la.capi.E_ARG
        assert lib.lbfgsb_hip_qn_path_set(h, None, 32, None) == la.capi.E_ARG
        for delta, rtol, mit, gp in ((0.0, 0.0, 0, v.data_ptr()), (-1.0, 0.0, 0, v.data_ptr()),
                                     (float("inf"), 0.0, 0, v.data_ptr()), (float("nan"), 0.0, 0, v.data_ptr()),
                                     (1.0, 1.0, 0, v.data_ptr()), (1.0, -1e-3, 0, v.data_ptr()),
                                     (1.0, 0.0, -1, v.data_ptr()), (1.0, 0.0, 0, None)):
            assert lib.lbfgsb_hip_qn_path_trust(h, gp, delta, rtol, mit, out.data_ptr(), res, C.byref(it)) \
                == la.capi.E_ARG
        assert list(res) == [7.0] * 4 and it.value == -5 and bool((out == sentinel).all())
        # a pushed pair: the three entries refuse until the next qn_path
        s_new = _vec(n, np.float64, 11)
        assert sol.qn_push_pair(torch.from_numpy(s_new).cuda(), torch.from_numpy(2.0 * s_new).cuda()) == 1
        for call in (lambda: path.solve(v, [0.3], out=out[:1]), lambda: path.logdet([0.3]),
                     lambda: path.trust(v, 1.0, out=out[0])):
            with pytest.raises(la.LbfgsbError, match="-104.*qn_path_set again"):
                call()
        assert bool((out == sentinel).all())
        path = sol.qn_path(_status(env, pin))
        assert np.isfinite(_np(path.solve(v, [0.3]))).all()
    finally:
        sol.close()


def test_stale_after_an_iteration(env):
    la, torch = env["la"], env["torch"]
    n, m = 1000, 5
    p = _problem(env, "rosenbrock", n, m)
    sol = la.DeviceSolver(n, m)
    held = {}
    try:
        def at(s, t):
            if not t.startswith("NEW_X"):
                return
            v = torch.ones(n, dtype=torch.float64, device="cuda")
            if "path" in held:
                for call in (lambda: held["path"].solve(v, [0.1]), lambda: held["path"].logdet([0.1]),
                             lambda: held["path"].trust(v, 1.0)):
                    with pytest.raises(la.LbfgsbError, match="qn_path_set again"):
                        call()
                held["stale"] = True
            held["path"] = s.qn_path()
            held["path"].solve(v, [0.1])
        _drive(env, sol, p, max_iter=4, at_return=at)
        assert held.get("stale")
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ a run does not notice
RUNS = {
    "compact_w_1": dict(pp=True, n=1_000_000, m=5, kind="quadratic", builtin=0,
                        ctor=dict(options={"compact_w": 1, "compact_min_rows": 0})),
    "pingpong_defer": dict(pp=True, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
}
# the refusals a run may answer at a return that is no place for the calls (qn_ready); any other failure is a failure
REFUSALS = ("still deferred", "still on the device", "accepted but not stored")


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    """as tests/test_gpu_qn_shift.py::test_run_does_not_notice: the four entries at EVERY return"""
    la, torch = env["la"], env["torch"]
    cfg = RUNS[name]
    n, m = cfg.get("n", 4099), cfg.get("m", 7)
    p = _problem(env, cfg.get("kind", "rosenbrock"), n, m)
    iters = 30
    gen = torch.Generator(device="cpu").manual_seed(9)
    v = torch.randn(n, generator=gen, dtype=torch.float64).cuda()
    status = torch.zeros(n, dtype=torch.int8, device="cuda")
    status[::3] = 2
    outs = []
    counts = {"ok": 0, "refused": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                try:
                    path = s.qn_path(status)
                    path.logdet([0.0, 0.5])
                    path.solve(v, [0.0, 0.5, 3.0], norms=True)
                    path.trust(v, 0.5)
                    counts["ok"] += 1
                except la.LbfgsbError as e:
                    assert "-104" in str(e) and any(r in str(e) for r in REFUSALS), e
                    counts["refused"] += 1
            rows, _ = _drive(env, sol, p, iters, at_return=at if touch else None, pp=cfg["pp"],
                             builtin=cfg.get("builtin"))
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes(), sol.compact_stats()))
        finally:
            sol.close()
    assert counts["ok"] >= iters
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert outs[0][3] == outs[1][3]
    if name == "compact_w_1":
        assert outs[1][3][0] > 0, outs[1][3]  # the layout did pack
    else:
        assert counts["refused"] > 0


def test_trust_out_of_evaluations(env):
    """max_it = 1 outside the region: LBFGSB_E_STATE, nothing written; max_it = 2 .. 4: whatever comes back is inside
    the region (the upper end of the bracket when the iteration did not get to rtol)"""
    la, torch = env["la"], env["torch"]
    state = (257, 10, 10, "generic", np.float64)
    st, tr, sol = _solver(env, state)
    try:
        pin = pt.pin_mask(257, "half")
        path = sol.qn_path(_status(env, pin))
        g = _dev(env, _vec(257, np.float64, 3), np.float64, 0)
        x0 = path.trust(g, 1e30).norm
        for ratio in (0.5, 1e-3):
            delta = ratio * x0
            step = torch.full((257,), 12345.0, dtype=torch.float64, device="cuda")
            with pytest.raises(la.LbfgsbError, match="-104.*max_it = 1"):
                path.trust(g, delta, max_it=1, out=step)
            assert bool((step == 12345.0).all())
            full = path.trust(g, delta)
            for max_it in (2, 3, 4):
                try:
                    t = path.trust(g, delta, max_it=max_it, out=step)
                except la.LbfgsbError as e:
                    assert "-104" in str(e) and "max_it = %d" % max_it in str(e), e
                    continue
                sl = _np(t.step).astype(LD)
                assert t.iters <= max_it and t.mu > 0.0 and t.on_boundary
                assert t.norm <= delta * (1 + 1e-10) and float(np.sqrt(sl @ sl)) <= delta * (1 + 1e-10) + 1e-14 * x0
                assert t.mu >= full.mu * (1 - 1e-9)  # (the upper end: never a smaller shift than the converged one)
    finally:
        sol.close()
