"""The model plus a diagonal (lbfgsb_hip_qn_shift_set / _solve / _logdet / _diag; DeviceSolver.qn_shift): solves,
log-determinants and marginal variances of B + mu I + diag(d) on the rows that are not pinned (d_i = +inf), against
numpy.linalg.solve, slogdet and inv on the free block of the dense numpy model built from export_state.  Bounds, the
project's own for qn_apply(inverse=True), qn_diag and qn_logdet:
  solve  |out - ref| <= tol cond |ref|, tol = 1e-10 (fp64) or 1e-5 (REAL32), cond the 2-norm condition of that block;
  diag   max error <= tol cond max |ref|;     log det  |ld - ref| <= 1e-10 n.
Then: d = NULL, mu = 0 against the unshifted entries; pinned rows exactly +0; the tile-local layout of W read as it
is; REAL32; staleness and refusals; runs that call the entries at every return bit-identical to runs that do not."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_qn import _drive, _problem
from test_gpu_qn_root import _slow_quadratic

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


def _model(sol, wa=None):
    """dense B from the exported state: theta I updated by the stored pairs in ring order"""
    n, m = sol.n, sol.m
    if wa is None:
        wa, _ = sol.export_state()
    wa = wa.astype(np.float64)
    Ws = wa[:m * n].reshape(m, n).T
    Wy = wa[m * n:2 * m * n].reshape(m, n).T
    head, col, theta = int(sol.isave[26]), int(sol.isave[27]), float(sol.dsave[0])
    B = theta * np.eye(n)
    for j in range(col):
        c = (head - 1 + j) % m
        s, y = Ws[:, c], Wy[:, c]
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
    return B, col


def _cond(A):
    ev = np.linalg.eigvalsh(A)  # (symmetric positive definite: the 2-norm condition without an SVD)
    assert ev[0] > 0.0
    return ev[-1] / ev[0]


def _device_case(env, sol, d, mu, ks=(1, 3, 9)):
    """one shift on the device (d: numpy array in the solver's real kind with +inf on the pinned rows, or None): the
    solves of k random vectors, the diagonal (None beyond 32 pairs, where it must refuse) and the log det"""
    torch = env["torch"]
    n, col = sol.n, int(sol.isave[27])
    dd = np.zeros(n) if d is None else d.astype(np.float64)
    free = np.isfinite(dd)
    sh = sol.qn_shift(None if d is None else torch.from_numpy(d).cuda(), mu)
    assert sh.pinned == int((~free).sum())
    rng = np.random.default_rng(n + 31 * col + int(free.sum()))
    solves = []
    for k in ks:
        V = rng.standard_normal((k, n)).astype(sol.real)
        out = sh.solve(torch.from_numpy(V).cuda()).cpu().numpy()
        assert out.dtype == sol.real
        solves.append((V.astype(np.float64), out))
    dg = None
    if col <= 32:
        dg = sh.diag().cpu().numpy()
    else:
        with pytest.raises(env["la"].LbfgsbError, match="-101"):
            sh.diag()
    return dict(n=n, col=col, dd=dd, free=free, mu=mu, solves=solves, diag=dg, logdet=sh.logdet())


def _compare_case(res, B, tol, tag):
    """the device's results against numpy.linalg.inv and slogdet of the dense free block"""
    n, col, free, dd, mu = res["n"], res["col"], res["free"], res["dd"], res["mu"]
    nf = int(free.sum())
    A = (B + np.diag(np.where(free, mu + dd, 0.0)))[np.ix_(free, free)]
    cond = _cond(A) if nf else 1.0
    Ai = np.linalg.inv(A)
    for V, out in res["solves"]:
        assert np.all(out[:, ~free] == 0.0) and not np.signbit(out[:, ~free]).any()  # exactly +0
        ref = V[:, free] @ Ai.T
        err, bound = np.linalg.norm(out[:, free] - ref), tol * cond * np.linalg.norm(ref)
        print("%s n %d col %d k %d: solve off by %.2e (bound %.2e, cond %.2e)"
              % (tag, n, col, V.shape[0], err, bound, cond))
        assert err <= bound
    dg = res["diag"]
    if dg is not None:
        assert np.all(dg[~free] == 0.0) and not np.signbit(dg[~free]).any()
        if nf:
            ref = np.diag(Ai)
            err, bound = np.abs(dg[free] - ref).max(), tol * cond * np.abs(ref).max()
            print("%s n %d col %d: diag off by %.2e (bound %.2e)" % (tag, n, col, err, bound))
            assert err <= bound
    ld = res["logdet"]
    sign, ref = np.linalg.slogdet(A) if nf else (1.0, 0.0)
    print("%s n %d col %d: log det %.15e against %.15e (bound %.1e)" % (tag, n, col, ld, ref, 1e-10 * n))
    assert sign == 1.0 and abs(ld - ref) <= 1e-10 * n
    if nf == 0:
        assert ld == 0.0


def _check_case(env, sol, B, col, d, mu, tol, tag):
    res = _device_case(env, sol, d, mu)
    assert res["col"] == col
    _compare_case(res, B, tol, tag)


def _shifts(sol, rng):
    """(a) d random in [0, 10], (c) the same with the rows i = 0 mod 2 pinned, (d) all rows pinned"""
    n = sol.n
    a = rng.uniform(0.0, 10.0, n).astype(sol.real)
    c = a.copy()
    c[::2] = np.inf
    return a, c, np.full(n, np.inf, sol.real)


def _check_state(env, sol, tol):
    torch = env["torch"]
    n = sol.n
    B, col = _model(sol)
    a, c, d = _shifts(sol, np.random.default_rng(5 * n + col))
    _check_case(env, sol, B, col, a, MU, tol, "(a)")
    _check_case(env, sol, B, col, c, MU, tol, "(c)")
    _check_case(env, sol, B, col, d, MU, tol, "(d)")
    # (b) d = NULL, mu = 0: the unshifted entries
    sh = sol.qn_shift()
    assert sh.pinned == 0
    cond = _cond(B)
    rng = np.random.default_rng(n + col)
    for k in (1, 3, 9):
        V = torch.from_numpy(rng.standard_normal((k, n)).astype(sol.real)).cuda()
        got, ref = sh.solve(V).cpu().numpy().astype(np.float64), sol.qn_apply(V, inverse=True).cpu().numpy().astype(np.float64)
        assert np.linalg.norm(got - ref) <= tol * cond * np.linalg.norm(ref), (k, col)
    if col <= 32:
        got, ref = sh.diag().cpu().numpy().astype(np.float64), sol.qn_diag(inverse=True).cpu().numpy().astype(np.float64)
        assert np.abs(got - ref).max() <= tol * cond * np.abs(ref).max()
    assert abs(sh.logdet() - sol.qn_logdet()) <= 1e-10 * n
    return col


SHAPES = [(7, 1), (7, 3), (64, 10), (1000, 17), (1000, 40), (4099, 10)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_shifted_model_fp64(env, n, m):
    """col = 0 (FG_START), a partly filled ring and a full ring whose head has wrapped"""
    la = env["la"]
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)  # (no early stop: the ring fills and wraps)
    sol = la.DeviceSolver(n, m)
    seen = set()
    try:
        def at(s, t):
            col = int(s.isave[27])
            if 2 * col > n or not (t.startswith("NEW_X") or t.startswith("FG_START")):
                return
            head = int(s.isave[26])
            tag = "empty" if col == 0 else ("wrapped" if col == m and int(s.isave[30]) > m and (head > 1 or m == 1)
                                            else "part")
            if tag in seen or (tag == "part" and (col == m or col < max(1, m // 2))):
                return
            seen.add(tag)
            _check_state(env, s, 1e-10)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert "empty" in seen and "wrapped" in seen, seen


def test_layout_read_as_it_is(env):
    """(a) and (c) at (4099, 10) on the bounded quadratic once the tile-local layout of W is packed"""
    la = env["la"]
    n, m = 4099, 10
    p = _problem(env, "quadratic", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": 1, "compact_min_rows": 0})
    got = []
    try:
        def at(s, t):
            if got or not t.startswith("NEW_X") or int(s.isave[27]) < 2 or not s.compact_stats()[2]:
                return
            before = s.compact_stats()
            a, c, _ = _shifts(s, np.random.default_rng(17))
            ra, rc = _device_case(env, s, a, MU), _device_case(env, s, c, MU)
            assert s.compact_stats() == before  # (still packed: the passes read the layout as it is)
            B, col = _model(s)  # (export_state puts W back into natural order: after the device's part)
            _compare_case(ra, B, 1e-10, "packed (a)")
            _compare_case(rc, B, 1e-10, "packed (c)")
            got.append(col)
        _drive(env, sol, p, max_iter=40, at_return=at, until=lambda s: bool(got))
    finally:
        sol.close()
    assert got, "the layout never packed"


def test_shifted_model_real32(env):
    """(a) and (c) at (1000, 10) in a REAL32 context: d, v, out fp32, the weights and every sum fp64"""
    la = env["la"]
    n, m = 1000, 10
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) in (2, m + 2):
                B, col = _model(s)
                a, c, _ = _shifts(s, np.random.default_rng(23))
                _check_case(env, s, B, col, a, MU, 1e-5, "fp32 (a)")
                _check_case(env, s, B, col, c, MU, 1e-5, "fp32 (c)")
                checked.append(col)
        _drive(env, sol, p, max_iter=m + 2, at_return=at)
    finally:
        sol.close()
    assert len(checked) == 2 and checked[-1] == m


def test_staleness_and_refusals(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    v = torch.ones(n, dtype=torch.float64, device="cuda")
    out = torch.empty_like(v)
    d = torch.rand(n, dtype=torch.float64, device="cuda")
    val, pinned = C.c_double(0.0), C.c_int64(-1)

    def solve(s):
        return lib.lbfgsb_hip_qn_shift_solve(s.h, 1, v.data_ptr(), n, out.data_ptr(), n)

    sol = la.DeviceSolver(n, m)
    try:
        assert lib.lbfgsb_hip_qn_shift_set(sol.h, None, 0.0, None) == E_STATE  # no run
        assert solve(sol) == E_STATE
        state = {}

        def at(s, t):
            if not t.startswith("NEW_X"):
                return
            it = int(s.isave[29])
            if it == 3:
                assert solve(s) == E_STATE  # before any set
                assert lib.lbfgsb_hip_qn_shift_logdet(s.h, C.byref(val)) == E_STATE
                assert lib.lbfgsb_hip_qn_shift_diag(s.h, out.data_ptr()) == E_STATE
                assert lib.lbfgsb_hip_qn_shift_set(s.h, d.data_ptr(), 0.5, C.byref(pinned)) == 0 and pinned.value == 0
                assert solve(s) == 0
                state["x"] = out.clone()
                state["iupdat"] = int(s.isave[30])
                theta = float(s.dsave[0])
                # refusals leave the shift in force
                bad = d.clone()
                bad[7] = float("nan")
                assert lib.lbfgsb_hip_qn_shift_set(s.h, bad.data_ptr(), 0.5, None) == E_ARG
                bad[7] = -float("inf")
                assert lib.lbfgsb_hip_qn_shift_set(s.h, bad.data_ptr(), 0.5, None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_set(s.h, None, -2.0 * theta, None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_set(s.h, d.data_ptr(), -2.0 * theta, None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_set(s.h, None, float("nan"), None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_set(s.h, None, float("inf"), None) == E_ARG
                assert solve(s) == 0 and torch.equal(out, state["x"])
                assert lib.lbfgsb_hip_qn_shift_solve(s.h, 1, v.data_ptr(), n, None, n) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_solve(s.h, 1, None, n, out.data_ptr(), n) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_solve(s.h, 0, v.data_ptr(), n, out.data_ptr(), n) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_solve(s.h, 1, v.data_ptr(), n - 1, out.data_ptr(), n) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_solve(s.h, 1, v.data_ptr(), n, out.data_ptr(), n - 1) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_diag(s.h, None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_logdet(s.h, None) == E_ARG
                # an indefinite shift (B has eigenvalues below theta here): E_STATE, the shift in force stays
                B, _ = _model(s)
                mu = -0.999 * theta
                if np.linalg.eigvalsh(B).min() + mu < 0.0:
                    assert lib.lbfgsb_hip_qn_shift_set(s.h, None, mu, None) == E_STATE
                    state["indefinite"] = True
                    assert solve(s) == 0 and torch.equal(out, state["x"])
            elif it == 4:
                assert int(s.isave[30]) > state["iupdat"]  # one more pair is stored
                assert solve(s) == E_STATE
                assert lib.lbfgsb_hip_qn_shift_logdet(s.h, C.byref(val)) == E_STATE
                assert lib.lbfgsb_hip_qn_shift_diag(s.h, out.data_ptr()) == E_STATE
                sh = s.qn_operator().shifted(d, 0.5)
                with pytest.raises(la.LbfgsbError, match="-101"):
                    s.qn_shift(d, -2.0 * float(s.dsave[0]))
                assert solve(s) == 0 and np.isfinite(sh.logdet())
                state["again"] = True

        _drive(env, sol, p, max_iter=5, at_return=at)
        assert state.get("again")
    finally:
        sol.close()
    # more than 64 pairs: E_ARG; more than 32: set and solve fine, diag E_ARG (checked in test_shifted_model_fp64)
    sol = la.DeviceSolver(1000, 70)
    try:
        _, t = _drive(env, sol, _slow_quadratic(env, 1000, 70), max_iter=400, until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65, t
        assert lib.lbfgsb_hip_qn_shift_set(sol.h, None, 0.0, None) == E_ARG
    finally:
        sol.close()
    # the deferred line-search set-up and a parked built-in f refuse as qn_apply does
    s2 = la.DeviceSolver(n, m, defer_lnsrch=True, same_stream_objective=True)
    refused = []
    try:
        def at2(s, t):
            if t.startswith("FG_LN"):
                refused.append(lib.lbfgsb_hip_qn_shift_set(s.h, None, 0.0, None))
        _drive(env, s2, p, 10, at_return=at2)
    finally:
        s2.close()
    assert E_STATE in refused and all(r in (0, E_STATE) for r in refused), refused
    s3 = la.DeviceSolver(n, m)
    try:
        x = torch.from_numpy(p.x0.copy()).cuda()
        g = torch.zeros_like(x)
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert t.startswith("FG")
        s3.objective(1, x, g, deferred=True)
        assert lib.lbfgsb_hip_qn_shift_set(s3.h, None, 0.0, None) == E_STATE
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert lib.lbfgsb_hip_qn_shift_set(s3.h, None, 0.0, None) == 0
        assert solve(s3) == 0
    finally:
        s3.close()


def test_stale_object_raises(env):
    la, torch = env["la"], env["torch"]
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    sol = la.DeviceSolver(n, m)
    held = {}
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) == 2:
                held["sh"] = s.qn_shift(mu=1.0)
                held["sh"].solve(torch.ones(n, dtype=torch.float64, device="cuda"))
        _drive(env, sol, p, max_iter=3, at_return=at)
        with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
            held["sh"].solve(torch.ones(n, dtype=torch.float64, device="cuda"))
        with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
            held["sh"].logdet()
        with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
            held["sh"].diag()
    finally:
        sol.close()


RUNS = {
    "compact_w_1": dict(pp=True, n=1_000_000, m=5, kind="quadratic", builtin=0,
                        ctor=dict(options={"compact_w": 1, "compact_min_rows": 0})),
    "pingpong_defer": dict(pp=True, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    la, torch = env["la"], env["torch"]
    cfg = RUNS[name]
    n, m = cfg.get("n", 4099), cfg.get("m", 7)
    p = _problem(env, cfg.get("kind", "rosenbrock"), n, m)
    iters = 30
    g = torch.Generator(device="cpu").manual_seed(9)
    d = (10.0 * torch.rand(n, generator=g, dtype=torch.float64)).cuda()
    d[::3] = float("inf")
    V = torch.randn(2, n, generator=g, dtype=torch.float64).cuda()
    outs = []
    counts = {"ok": 0, "refused": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                try:
                    sh = s.qn_shift(d, MU)
                    sh.solve(V)
                    sh.diag()
                    counts["ok"] += 1
                except la.LbfgsbError as e:
                    assert "-104" in str(e), e  # E_STATE: a deferred set-up or a parked f
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
