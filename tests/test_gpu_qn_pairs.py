"""The stored pairs of the curvature model as device data: lbfgsb_hip_qn_pairs_get / _set / _push
(DeviceSolver.qn_pairs / qn_set_pairs / qn_push_pair).  n in {1, 127, 1027} (1027 is no multiple of the 128-row layout
tile or of a 256-lane trip), m in {3, 10, 17, 40} (17: two column tiles of 16 pairs; 40: beyond the fused width).
  1 set == import, bit for bit (fp64, the dyadic family of tests/_qn_synth.py, whose Gram sums are exact in any order):
    a context that imported synth(n, m, npairs) and a context that never ran and was handed synth's pairs give the
    same bits from qn_apply (B and H, k = 5), qn_logdet and qn_block; the importer's qn_pairs() is synth's pairs.
  2 the generic family and REAL32 against the extended-precision model of tests/_qn_truth.py after qn_set_pairs, within
    its own bounds and no other tolerance; operands lds = n + 1 apart, one element off a 16-byte boundary.
  3 push == the oracle's matupd: one sequence of 2m + 1 dyadic pairs (tests/_qn_pairs_seq.py) pushed one at a time
    gives after EVERY push the oracle's pairs exactly and the H v of a context that imported the oracle's state, bit
    for bit; a pair with y = 0 or s'y < 0 is not stored and changes nothing; the generic family against the truth.
  4 get on the packed layout equals qn_rows and leaves compact_stats alone; a run that calls qn_pairs() at every return
    ends with the same x, isave, dsave as one that never does, bit for bit.
  5 the refusals of the three entries and of setulb in model mode."""
import numpy as np
import pytest

import _qn_synth as qs
import _qn_truth as qt
from _qn_pairs_seq import sequence

pytestmark = pytest.mark.gpu

LD = qt.LD
NS = (1, 127, 1027)
MS = (3, 10, 17, 40)
# every n with one m and every m with one n, and the largest of both
SHAPES = [(1, 3), (127, 10), (1027, 17), (127, 40), (1027, 3), (1027, 40)]


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd, capi=lbfgsb_amd.capi)


def _tdt(env, real):
    return env["torch"].float32 if real == np.float32 else env["torch"].float64


def _dev(env, a, real=np.float64, odd=False):
    """a (k, n) or (n,) numpy array on the device; odd: rows n + 1 apart, the first element one element past a 16-byte
    boundary"""
    torch = env["torch"]
    a = np.asarray(a, real)
    if not odd:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    k, n = (1, a.shape[0]) if a.ndim == 1 else a.shape
    buf = torch.full((k * (n + 1) + 5,), float("nan"), dtype=_tdt(env, real), device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + k * (n + 1)].view(k, n + 1)[:, :n]
    t.copy_(torch.from_numpy(np.atleast_2d(a)))
    assert t.data_ptr() % 16 == a.itemsize and (k == 1 or t.stride(0) == n + 1)
    return t[0] if a.ndim == 1 else t


def _np(t):
    return t.cpu().numpy()


def _vectors(n, k, real=np.float64, salt=0):
    return np.random.default_rng(77 * n + k + salt).standard_normal((k, n)).astype(real)


def _pairs_np(sol):
    S, Y, theta = sol.qn_pairs()
    return _np(S).T.astype(np.float64), _np(Y).T.astype(np.float64), theta


def _idx(n):
    return np.unique(np.array([0, n // 2, n - 1, min(n - 1, 127), min(n - 1, 128)], np.int64))


def _digest(env, sol, n, k=5):
    """the bits of B V, H V, log det B and a block of H"""
    V = _dev(env, _vectors(n, k))
    return (_np(sol.qn_apply(V)).tobytes(), _np(sol.qn_apply(V, inverse=True)).tobytes(),
            np.float64(sol.qn_logdet()).tobytes(), sol.qn_block(_idx(n), inverse=True).tobytes())


# --------------------------------------------------------------------------------------- 1: set == import
@pytest.mark.parametrize("n,m", SHAPES)
def test_set_is_import_bit_for_bit(env, n, m):
    la = env["la"]
    for npairs in (0, 2, m, 2 * m + 1):
        if n == 1 and npairs:
            continue  # (synth's dyadic draw of one entry may be zero; test_push covers n = 1 with pairs)
        st = qs.synth(n, m, npairs)
        S, Y = st.pairs()
        a, b = la.DeviceSolver(n, m), la.DeviceSolver(n, m)
        try:
            a.import_state(st.wa, st.iwa, st.isave)
            b.qn_set_pairs(S.T, Y.T, theta=None)  # (b has never run)
            assert _digest(env, a, n) == _digest(env, b, n), (n, m, npairs)
            Sa, Ya, ta = _pairs_np(a)
            assert Sa.shape == (n, st.col) and np.array_equal(Sa, S) and np.array_equal(Ya, Y) and ta == st.theta
            Sb, Yb, tb = _pairs_np(b)
            assert np.array_equal(Sb, S) and np.array_equal(Yb, Y) and tb == st.theta
            v = _dev(env, _vectors(n, 1, salt=3)[0])
            assert np.array_equal(_np(b.qn_operator().matvec(v)), _np(a.qn_apply(v, inverse=True)))
        finally:
            a.close(), b.close()


# --------------------------------------------------------------------------------------- 2: against the truth
def _check_truth(env, sol, tr, real, tag):
    n = tr.n
    kd = "fp32" if real == np.float32 else "fp64"
    V = _vectors(n, 3, real, 5)
    for inverse, op in ((False, tr.B), (True, tr.H)):
        nm = "H" if inverse else "B"
        out = _np(sol.qn_apply(_dev(env, V, real, odd=True), out=_dev(env, np.zeros_like(V), real, odd=True),
                               inverse=inverse))
        ref = op.apply(V)
        qt.check("%s qn_apply %s %s" % (tag, nm, kd), out, ref, op.bound_apply(V, real, ref))
        Vabs = np.abs(V).astype(np.float64)
        bq = np.diag(op.bound_quad(Vabs)) * (1 + 4 * qt.U)
        qt.check("%s qn_quad %s %s" % (tag, nm, kd), sol.qn_quad(_dev(env, V, real, odd=True), inverse=inverse),
                 np.diag(op.quad(V)), bq)
    d = np.linspace(0.0, 3.0, n).astype(real)
    d[::3] = np.inf
    sop = tr.shifted(d, 0.3)
    out = _np(sol.qn_shift(_dev(env, d, real), 0.3).solve(_dev(env, V, real, odd=True)))
    ref = sop.apply(V)
    qt.check("%s shift solve %s" % (tag, kd), out, ref, sop.bound_apply(V, real, ref))


@pytest.mark.parametrize("n,m,real", [(127, 10, np.float64), (127, 40, np.float64), (1027, 17, np.float64),
                                      (127, 10, np.float32), (1027, 17, np.float32)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_set_against_the_truth(env, n, m, real):
    """(not n = 1: the reference reads its middle matrix off [S, Y]'[S, Y], which needs n >= 2 col; n = 1 is held to
    the importing context bit for bit in tests 1 and 3)"""
    S, Y = qs.synth(n, m, m + 2, "generic", real).pairs()
    sol = env["la"].DeviceSolver(n, m, real32=real == np.float32)
    try:
        sol.qn_set_pairs(_dev(env, S.T, real, odd=True), _dev(env, Y.T, real, odd=True))
        S2, Y2, theta = _pairs_np(sol)
        assert np.array_equal(S2, S) and np.array_equal(Y2, Y)
        tr = qt.Truth(S, Y, g=1)
        assert abs(theta - float(tr.theta)) <= qt.gamma(n + 2) * float(tr.theta)
        _check_truth(env, sol, tr, real, "set")
        # a theta of the caller's own
        sol.qn_set_pairs(_dev(env, S.T, real), _dev(env, Y.T, real), theta=1.75)
        assert sol.qn_pairs()[2] == 1.75
        tr2 = qt.Truth(S, Y, theta=1.75, g=1)
        V = _vectors(n, 2, real, 9)
        ref = tr2.H.apply(V)
        qt.check("set theta given", _np(sol.qn_apply(_dev(env, V, real), inverse=True)), ref,
                 tr2.H.bound_apply(V, real, ref))
    finally:
        sol.close()


def test_empty_model(env):
    n, m = 127, 5
    sol = env["la"].DeviceSolver(n, m)
    try:
        z = np.zeros((0, n))
        sol.qn_set_pairs(z, z, theta=2.0)
        S, Y, theta = sol.qn_pairs()
        assert tuple(S.shape) == (0, n) and theta == 2.0
        V = _vectors(n, 2)
        assert np.array_equal(_np(sol.qn_apply(_dev(env, V))), 2.0 * V)
        assert np.array_equal(_np(sol.qn_apply(_dev(env, V), inverse=True)), (1.0 / 2.0) * V)
    finally:
        sol.close()


# --------------------------------------------------------------------------------------- 3: push
@pytest.mark.parametrize("n,m", SHAPES)
def test_push_is_the_oracles_matupd(env, n, m):
    la = env["la"]
    pairs, states = sequence(n, m, 2 * m + 1)
    V = _dev(env, _vectors(n, 2))
    sol, ref = la.DeviceSolver(n, m), la.DeviceSolver(n, m)
    try:
        z = np.zeros((0, n))
        sol.qn_set_pairs(z, z, theta=1.0)
        for j, (s, y) in enumerate(pairs, 1):
            assert sol.qn_push_pair(_dev(env, s, odd=bool(j & 1)), _dev(env, y, odd=bool(j & 2))) == 1
            st = states[j]
            S, Y, theta = _pairs_np(sol)
            Sr, Yr = st.pairs()
            assert np.array_equal(S, Sr) and np.array_equal(Y, Yr) and theta == st.theta, (n, m, j)
            ref.import_state(st.wa, st.iwa, st.isave)
            assert _np(sol.qn_apply(V, inverse=True)).tobytes() == _np(ref.qn_apply(V, inverse=True)).tobytes(), j
            if j in (1, m, 2 * m + 1):
                assert _digest(env, sol, n) == _digest(env, ref, n), j
        # pairs that are not stored: nothing changes
        before = (_pairs_np(sol), _np(sol.qn_apply(V, inverse=True)).tobytes())
        s, y = pairs[0]
        assert sol.qn_push_pair(_dev(env, s), _dev(env, np.zeros(n))) == 0
        assert sol.qn_push_pair(_dev(env, s), _dev(env, -y)) == 0
        S, Y, theta = _pairs_np(sol)
        assert np.array_equal(S, before[0][0]) and np.array_equal(Y, before[0][1]) and theta == before[0][2]
        assert _np(sol.qn_apply(V, inverse=True)).tobytes() == before[1]
    finally:
        sol.close(), ref.close()


@pytest.mark.parametrize("n,m,real", [(127, 10, np.float64), (1027, 17, np.float64), (127, 10, np.float32)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_push_against_the_truth(env, n, m, real):
    pairs, states = sequence(n, m, m + 3, "generic", real)
    sol = env["la"].DeviceSolver(n, m, real32=real == np.float32)
    try:
        S0, Y0 = states[2].pairs()
        sol.qn_set_pairs(_dev(env, S0.T, real), _dev(env, Y0.T, real))
        for s, y in pairs[2:]:
            assert sol.qn_push_pair(_dev(env, s, real, odd=True), _dev(env, y, real)) == 1
        S, Y = states[-1].pairs()
        S2, Y2, theta = _pairs_np(sol)
        assert np.array_equal(S2, S) and np.array_equal(Y2, Y)
        # (g = 2: the host matrices are the sums of the pushes, the H coefficients use the Gram cache on top)
        _check_truth(env, sol, qt.Truth(S, Y, g=2), real, "push")
    finally:
        sol.close()


# --------------------------------------------------------------------------------------- 4: the layout, the run
def _run(env, sol, p, max_iter, at_return=None):
    """the few lines of a device-pointer run with the built-in host objective of the problem"""
    torch = env["torch"]
    x = torch.from_numpy(p.x0.copy()).cuda()
    g = torch.zeros_like(x)
    l, u = torch.from_numpy(p.l.copy()).cuda(), torch.from_numpy(p.u.copy()).cuda()
    nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        if at_return is not None:
            at_return(sol, t)
        if t.startswith("FG"):
            xh = x.cpu().numpy()
            gh = np.empty_like(xh)
            sol.f[0] = p.fg(xh, gh)
            g.copy_(torch.from_numpy(gh))
            torch.cuda.synchronize()
        elif not t.startswith("NEW_X") or sol.isave[29] >= max_iter:
            break
    return x.cpu().numpy(), sol.isave.copy(), sol.dsave.copy(), t


def test_get_on_the_packed_layout_and_the_unnoticed_call(env):
    la, po = env["la"], env["po"]
    n, m = 1027, 10
    p = po.problem_quadratic(n, m, True, np.float64)
    opts = {"compact_w": 2, "compact_policy": 2, "compact_min_rows": 0}
    seen = []

    def at(s, t):
        if t.startswith("NEW_X") and s.compact_stats()[2] and int(s.isave[27]) >= 2:
            col = int(s.isave[27])
            before = s.compact_stats()
            rows = s.qn_rows(np.arange(n, dtype=np.int64))
            S, Y, theta = _pairs_np(s)
            assert np.array_equal(S, rows[:, :col]) and np.array_equal(Y, rows[:, col:]) and theta == s.dsave[0]
            assert s.compact_stats() == before and before[2]
            seen.append((col, int(s.isave[26])))
        else:
            s.qn_pairs()

    a, b = la.DeviceSolver(n, m, options=opts), la.DeviceSolver(n, m, options=opts)
    try:
        ra = _run(env, a, p, 3 * m + 5, at)
        rb = _run(env, b, p, 3 * m + 5)
    finally:
        a.close(), b.close()
    assert len(seen) >= 3 and any(h > 1 for _, h in seen), seen  # (packed returns, the ring wrapped among them)
    assert ra[3] == rb[3] and ra[0].tobytes() == rb[0].tobytes()
    assert ra[1].tobytes() == rb[1].tobytes()
    keep = [0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15]  # (all of dsave but the wall-clock times of the run, dsave(6:10))
    assert ra[2][keep].tobytes() == rb[2][keep].tobytes()


# --------------------------------------------------------------------------------------- 5: refusals
def test_refusals(env):
    la, capi, po = env["la"], env["capi"], env["po"]
    n, m = 127, 5
    st = qs.synth(n, m, 4)
    S, Y = st.pairs()
    p = po.problem_quadratic(n, m, True, np.float64)
    sol, fresh = la.DeviceSolver(n, m), la.DeviceSolver(n, m)

    def refused(code, fn):
        with pytest.raises(la.LbfgsbError, match="lbfgsb_hip error %d:" % code):
            fn()
    try:
        # a fresh context has nothing to get or to push to
        refused(capi.E_STATE, sol.qn_pairs)
        refused(capi.E_STATE, lambda: sol.qn_push_pair(_dev(env, S[:, 0]), _dev(env, Y[:, 0])))
        # a run: its pairs belong to it
        x, isave, dsave, t = _run(env, sol, p, 3)
        assert t.startswith("NEW_X") and sol.qn_pairs()[0].shape[0] >= 1
        refused(capi.E_STATE, lambda: sol.qn_push_pair(_dev(env, S[:, 0]), _dev(env, Y[:, 0])))
        # get: 0 < cap < col
        import ctypes as C
        col, theta = C.c_int32(-1), C.c_double(0.0)
        buf = env["torch"].zeros((m, n), dtype=env["torch"].float64, device="cuda")
        k = sol.qn_pairs()[0].shape[0]
        if k >= 2:
            assert sol.lib.lbfgsb_hip_qn_pairs_get(sol.h, 1, C.byref(col), C.byref(theta), buf.data_ptr(), n,
                                                   buf.data_ptr(), n) == capi.E_ARG
            assert col.value == k
        assert sol.lib.lbfgsb_hip_qn_pairs_get(sol.h, m, C.byref(col), C.byref(theta), buf.data_ptr(), n - 1,
                                               buf.data_ptr(), n) == capi.E_ARG
        # set: k > m, ld < n, theta < 0 or not finite, NaN in a pair, s'y <= 0
        big = env["torch"].zeros((m + 1, n), dtype=env["torch"].float64, device="cuda")
        Sd, Yd = _dev(env, S.T), _dev(env, Y.T)
        lib, h = sol.lib, sol.h
        assert lib.lbfgsb_hip_qn_pairs_set(h, m + 1, big.data_ptr(), n, big.data_ptr(), n, 1.0) == capi.E_ARG
        assert lib.lbfgsb_hip_qn_pairs_set(h, 4, Sd.data_ptr(), n - 1, Yd.data_ptr(), n, 1.0) == capi.E_ARG
        assert lib.lbfgsb_hip_qn_pairs_set(h, 4, Sd.data_ptr(), n, Yd.data_ptr(), n, -1.0) == capi.E_ARG
        assert lib.lbfgsb_hip_qn_pairs_set(h, 4, Sd.data_ptr(), n, Yd.data_ptr(), n, float("nan")) == capi.E_ARG
        assert lib.lbfgsb_hip_qn_pairs_set(h, 0, None, 0, None, 0, 0.0) == capi.E_ARG
        assert sol.qn_pairs()[0].shape[0] == k  # (argument errors change nothing: the run's model still stands)
        Yn = Y.copy()
        Yn[3, 1] = np.nan
        with pytest.raises(la.LbfgsbError, match="error %d: .*pair 1" % capi.E_ARG):
            sol.qn_set_pairs(S.T, Yn.T)
        # ... which leaves neither a model nor a run
        v = _dev(env, _vectors(n, 1)[0])
        refused(capi.E_STATE, lambda: sol.qn_apply(v))
        refused(capi.E_STATE, sol.qn_pairs)
        refused(capi.E_STATE, lambda: sol.qn_push_pair(_dev(env, S[:, 0]), _dev(env, Y[:, 0])))
        with pytest.raises(la.LbfgsbError, match="pair 2"):
            sol.qn_set_pairs(S.T, np.where(np.arange(4) == 2, -Y, Y).T)
        refused(capi.E_STATE, lambda: sol.qn_apply(v))
        # model mode: setulb with the task of the old run is refused, START runs as on a fresh context
        sol.qn_set_pairs(S.T, Y.T)
        assert sol.qn_apply(v, inverse=True).shape == (n,)
        torch = env["torch"]
        xd = torch.from_numpy(x).cuda()
        gd = torch.zeros_like(xd)
        l, u = torch.from_numpy(p.l.copy()).cuda(), torch.from_numpy(p.u.copy()).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        assert sol.task_s.startswith("NEW_X")
        refused(capi.E_STATE, lambda: sol.setulb(xd, l, u, nbd, gd, p.factr, p.pgtol))
        assert sol.qn_apply(v, inverse=True).shape == (n,)  # (the refusal changed nothing)
        sol.set_task("START")
        ra = _run(env, sol, p, 12)
        rb = _run(env, fresh, p, 12)
        assert ra[3] == rb[3] and ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()
        refused(capi.E_STATE, lambda: sol.qn_push_pair(_dev(env, S[:, 0]), _dev(env, Y[:, 0])))  # (a run again)
    finally:
        sol.close(), fresh.close()
