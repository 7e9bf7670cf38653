"""The curvature model as a device operator (lbfgsb_hip_qn_apply / lbfgsb_hip_qn_diag, DeviceSolver.qn_*):
B = theta I - W M W' (bmv's matrix) and H = B^-1 at a setulb return, against an independent dense numpy model built
from export_state by the recursive BFGS updates from theta I in ring order; the tile-local layout of W read as it
is; runs that call the operator at every permitted return are bit-identical to runs that do not; the refusals."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104


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


def _check_dense(env, sol, tol, ks=(1, 3, 9)):
    torch = env["torch"]
    n = sol.n
    B, col = _model(sol)
    cond = np.linalg.cond(B)
    Hm = np.linalg.inv(B)
    rng = np.random.default_rng(n + 31 * col)
    dt = torch.float32 if sol.real == np.float32 else torch.float64
    for k in ks:
        V = rng.standard_normal((k, n)).astype(sol.real)
        vt = torch.from_numpy(V).cuda()
        bv = sol.qn_apply(vt).cpu().numpy().astype(np.float64)
        ref = V.astype(np.float64) @ B.T
        assert np.linalg.norm(bv - ref) <= tol * np.linalg.norm(B, 2) * np.linalg.norm(V), (k, col)
        hv = sol.qn_apply(vt, inverse=True).cpu().numpy().astype(np.float64)
        ref = V.astype(np.float64) @ Hm.T
        assert np.linalg.norm(hv - ref) <= tol * cond * np.linalg.norm(ref), (k, col, cond)
        assert vt.dtype == dt
    if col <= 32:
        d = sol.qn_diag().cpu().numpy().astype(np.float64)
        assert np.abs(d - np.diag(B)).max() <= tol * np.abs(np.diag(B)).max()
        d = sol.qn_diag(inverse=True).cpu().numpy().astype(np.float64)
        assert np.abs(d - np.diag(Hm)).max() <= tol * cond * np.abs(np.diag(Hm)).max()
    return col


def _drive(env, sol, p, max_iter, at_return=None, pp=False, builtin=None, deferred_f=False, until=None):
    """run p; at_return(sol, task) at every return; returns the digests of every return"""
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
            at_return(sol, t)
        if t.startswith("FG"):
            if builtin is not None:
                r = sol.objective(builtin, x, g, deferred=deferred_f)
                if r is not None:
                    sol.f[0] = r
                elif at_return is not None:
                    at_return(sol, "PARKED")  # (f still on the device: the entries refuse)
            else:
                xh = x.cpu().numpy()
                gh = np.empty_like(xh)
                sol.f[0] = p.fg(xh, gh)
                g.copy_(torch.from_numpy(gh))
                torch.cuda.synchronize()
        elif not t.startswith("NEW_X") or sol.isave[29] >= max_iter or (until is not None and until(sol)):
            break
    return rows, t


def _problem(env, kind, n, m, real=np.float64):
    po = env["po"]
    return po.problem_rosenbrock(n, m, real=real) if kind == "rosenbrock" else po.problem_quadratic(n, m, True, real)


SHAPES = [(7, 1), (7, 3), (64, 5), (64, 10), (1000, 17), (1000, 32), (1000, 40), (4099, 10), (4099, 40)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_dense_model_fp64(env, n, m):
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
            # (wrapped: a pair has been overwritten -- iupdat > m; with m = 1 the head never moves)
            tag = "empty" if col == 0 else ("wrapped" if col == m and int(s.isave[30]) > m and (head > 1 or m == 1)
                                            else ("full" if col == m else "part"))
            if tag in seen or (tag == "part" and col < max(1, m // 2)):
                return
            seen.add(tag)
            _check_dense(env, s, 1e-10)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert "empty" in seen and "wrapped" in seen, seen
    assert "part" in seen or m == 1, seen


def test_dense_model_terminal_and_minimize(env):
    la, torch = env["la"], env["torch"]
    p = _problem(env, "rosenbrock", 25, 5)
    sol = la.DeviceSolver(25, 5)
    try:
        _, t = _drive(env, sol, p, max_iter=10000)
        assert t.startswith("CONV") or t.startswith("ABNO"), t
        _check_dense(env, sol, 1e-10)
    finally:
        sol.close()
    sol = la.DeviceSolver(25, 5)
    try:
        x = torch.from_numpy(p.x0.copy()).cuda()
        g = torch.zeros_like(x)
        sol.minimize(x, torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda(),
                     torch.from_numpy(p.nbd.astype(np.int32)).cuda(), g, builtin=1, max_iter=200)
        assert int(sol.isave[27]) > 0
        _check_dense(env, sol, 1e-10)
        op = sol.qn_operator()
        v = torch.randn(25, dtype=torch.float64, device="cuda")
        assert torch.equal(op @ v, sol.qn_apply(v, inverse=True))
        V = torch.randn(25, 3, dtype=torch.float64, device="cuda")
        assert torch.allclose(op.matmat(V)[:, 1], op.matvec(V[:, 1].contiguous()), rtol=0, atol=1e-12)
        assert op.shape == (25, 25) and torch.equal(op.diagonal(), sol.qn_diag(inverse=True))
    finally:
        sol.close()


@pytest.mark.parametrize("n,m", [(64, 5), (1000, 10), (4099, 17)])
def test_dense_model_real32(env, n, m):
    la = env["la"]
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) in (2, m + 2):
                checked.append(_check_dense(env, s, 1e-5, ks=(1, 9)))
        _drive(env, sol, p, max_iter=m + 2, at_return=at)
    finally:
        sol.close()
    assert checked


def _all_modes(sol, torch, n, k=3):
    g = torch.Generator(device="cpu").manual_seed(5)
    dt = torch.float32 if sol.real == np.float32 else torch.float64
    V = torch.randn(k, n, generator=g, dtype=torch.float64).to(dt).cuda()
    out = [sol.qn_apply(V), sol.qn_apply(V, inverse=True), sol.qn_apply(V[0]), sol.qn_apply(V[1], inverse=True)]
    if int(sol.isave[27]) <= 32:
        out += [sol.qn_diag(), sol.qn_diag(inverse=True)]
    return [o.cpu().numpy().astype(np.float64) for o in out]


@pytest.mark.parametrize("n,policy,kind", [(4099, 1, "rosenbrock"), (4099, 2, "rosenbrock"),
                                           (1_000_000, 1, "quadratic"), (1_000_000, 2, "quadratic")])
def test_layout_read_as_it_is(env, n, policy, kind):
    la, torch = env["la"], env["torch"]
    m = 5
    p = _problem(env, kind, n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": policy, "compact_min_rows": 0})
    got = {}
    try:
        def at(s, t):
            if got or not t.startswith("NEW_X") or int(s.isave[27]) < m:
                return
            if not s.compact_stats()[2]:
                return
            before = s.compact_stats()
            got["res"] = _all_modes(s, torch, n)
            got["again"] = _all_modes(s, torch, n)
            assert s.compact_stats() == before
            got["wa"], got["iwa"] = s.export_state()
            got["isave"] = s.isave.copy()
        _drive(env, sol, p, max_iter=40, at_return=at, until=lambda s: bool(got))
    finally:
        sol.close()
    assert got, "the layout never packed"
    for a, b in zip(got["res"], got["again"]):
        assert np.array_equal(a, b)  # reproducible bit for bit
    plain = la.DeviceSolver(n, m)
    try:
        plain.import_state(got["wa"], got["iwa"], got["isave"])
        plain.isave[:] = got["isave"]
        res = _all_modes(plain, torch, n)
    finally:
        plain.close()
    for a, b in zip(got["res"], res):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


RUNS = {
    "classic": dict(pp=False),
    "pingpong": dict(pp=True),
    "defer": dict(pp=False, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
    "builtin_deferred_f": dict(pp=False, builtin=1, deferred_f=True),
    "compact_1e6": dict(pp=True, n=1_000_000, m=5, kind="quadratic", builtin=0,
                        ctor=dict(options={"compact_w": 1, "compact_min_rows": 0})),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    la, torch = env["la"], env["torch"]
    cfg = RUNS[name]
    n, m = cfg.get("n", 4099), cfg.get("m", 7)
    p = _problem(env, cfg.get("kind", "rosenbrock"), n, m)
    iters = 30
    outs = []
    counts = {"ok": 0, "refused": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                try:
                    _all_modes(s, torch, n, k=2)
                    counts["ok"] += 1
                except la.LbfgsbError as e:
                    assert "-104" in str(e), e  # E_STATE: a deferred set-up or a parked f
                    counts["refused"] += 1
            rows, _ = _drive(env, sol, p, iters, at_return=at if touch else None, pp=cfg["pp"],
                             builtin=cfg.get("builtin"), deferred_f=cfg.get("deferred_f", False))
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes(), sol.compact_stats()))
        finally:
            sol.close()
    assert counts["ok"] > iters
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert outs[0][3] == outs[1][3]
    if name == "compact_1e6":
        assert outs[1][3][0] > 0, outs[1][3]  # the layout did pack
    if name in ("defer", "builtin_deferred_f"):
        assert counts["refused"] > 0


def test_refusals_and_arguments(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    v = torch.ones(n, dtype=torch.float64, device="cuda")
    out = torch.empty_like(v)
    sol = la.DeviceSolver(n, m)
    try:
        assert lib.lbfgsb_hip_qn_apply(sol.h, 0, 1, v.data_ptr(), n, out.data_ptr(), n) == E_STATE  # no run
        assert lib.lbfgsb_hip_qn_diag(sol.h, 1, out.data_ptr()) == E_STATE
        _drive(env, sol, p, max_iter=8)
        for args in ((0, 0, v.data_ptr(), n, out.data_ptr(), n), (0, 1, v.data_ptr(), n - 1, out.data_ptr(), n),
                     (1, 1, v.data_ptr(), n, out.data_ptr(), n - 1), (0, 1, None, n, out.data_ptr(), n),
                     (2, 1, v.data_ptr(), n, out.data_ptr(), n)):
            assert lib.lbfgsb_hip_qn_apply(sol.h, *args) == E_ARG, args
        assert lib.lbfgsb_hip_qn_diag(sol.h, 0, None) == E_ARG
        assert lib.lbfgsb_hip_qn_apply(sol.h, 1, 1, v.data_ptr(), n, out.data_ptr(), n) == 0
    finally:
        sol.close()
    # more than 32 pairs: diag refused, apply fine
    sol = la.DeviceSolver(1000, 40)
    try:
        p40 = env["po"].problem_rosenbrock(1000, 40, factr=0.0, pgtol=0.0)  # (no early stop)
        _drive(env, sol, p40, max_iter=400, until=lambda s: int(s.isave[27]) > 32)
        assert int(sol.isave[27]) > 32
        w = torch.ones(1000, dtype=torch.float64, device="cuda")
        assert lib.lbfgsb_hip_qn_diag(sol.h, 0, w.data_ptr()) == E_ARG
        sol.qn_apply(w, inverse=True)
    finally:
        sol.close()
    # the deferred line-search set-up and a parked built-in f: E_STATE, and the run goes on as without the calls
    for ctor, builtin, deferred_f in ((dict(defer_lnsrch=True, same_stream_objective=True), None, False),
                                      ({}, 1, True)):
        digests = []
        for touch in (False, True):
            s2 = la.DeviceSolver(n, m, **ctor)
            refused = []
            try:
                def at(s, t):
                    if t.startswith("FG_LN") and builtin is None:
                        refused.append(lib.lbfgsb_hip_qn_apply(s.h, 1, 1, v.data_ptr(), n, out.data_ptr(), n))
                rows, _ = _drive(env, s2, p, 10, at_return=at if touch else None, builtin=builtin,
                                 deferred_f=deferred_f)
                digests.append(rows)
            finally:
                s2.close()
            if touch and builtin is None:
                assert E_STATE in refused and all(r in (0, E_STATE) for r in refused), refused
        assert digests[0] == digests[1]
    s3 = la.DeviceSolver(n, m)
    try:
        x = torch.from_numpy(p.x0.copy()).cuda()
        g = torch.zeros_like(x)
        l, u = torch.from_numpy(p.l).cuda(), torch.from_numpy(p.u).cuda()
        nbd = torch.from_numpy(p.nbd.astype(np.int32)).cuda()
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert t.startswith("FG")
        s3.objective(1, x, g, deferred=True)
        assert lib.lbfgsb_hip_qn_apply(s3.h, 1, 1, v.data_ptr(), n, out.data_ptr(), n) == E_STATE
        assert lib.lbfgsb_hip_qn_diag(s3.h, 0, out.data_ptr()) == E_STATE
        t = s3.setulb(x, l, u, nbd, g, p.factr, p.pgtol)
        assert lib.lbfgsb_hip_qn_apply(s3.h, 1, 1, v.data_ptr(), n, out.data_ptr(), n) == 0
    finally:
        s3.close()


def test_at_size_1e7(env):
    """n = 1e7, m = 10, the layout packed by the automatic policy: H v against a torch fp64 evaluation of the same
    compact formula from the exported Ws / Wy"""
    la, torch = env["la"], env["torch"]
    n, m = 10_000_000, 10
    sol = la.DeviceSolver(n, m, options={"compact_w": 1})
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        for _ in range(400):
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or (sol.isave[29] >= 12 and sol.compact_stats()[2]) or sol.isave[29] >= 60:
                break
        assert t.startswith("NEW_X"), t
        assert sol.compact_stats()[2] == 1, sol.compact_stats()  # the steady-state layout: packed
        col, head, theta = int(sol.isave[27]), int(sol.isave[26]), float(sol.dsave[0])
        assert col == m
        v = torch.randn(n, dtype=torch.float64, device="cuda")
        hv = sol.qn_apply(v, inverse=True)
        bhv = sol.qn_apply(hv)
        wa, _ = sol.export_state()
        Ws = torch.from_numpy(wa[:m * n].reshape(m, n)).cuda()
        Wy = torch.from_numpy(wa[m * n:2 * m * n].reshape(m, n)).cuda()
        order = [(head - 1 + j) % m for j in range(col)]
        S, Y = Ws[order].T, Wy[order].T
        SY = S.T @ Y
        R = torch.triu(SY)
        D = torch.diag(torch.diag(SY))
        a, b = S.T @ v, Y.T @ v
        uu = torch.linalg.solve_triangular(R, a[:, None], upper=True)[:, 0]
        w = D @ uu + (Y.T @ Y) @ uu / theta - b / theta
        cs = torch.linalg.solve_triangular(R.T, w[:, None], upper=False)[:, 0]
        ref = v / theta + S @ cs - Y @ uu / theta
        assert (torch.linalg.norm(hv - ref) / torch.linalg.norm(ref)).item() <= 1e-10
        assert (torch.linalg.norm(bhv - v) / torch.linalg.norm(v)).item() <= 1e-10
        u2 = torch.randn(n, dtype=torch.float64, device="cuda")
        bv, bu = sol.qn_apply(v), sol.qn_apply(u2)
        assert abs((u2 @ bv - v @ bu).item()) <= 1e-12 * (torch.linalg.norm(u2) * torch.linalg.norm(bv)).item()
        assert (v @ hv).item() > 0
    finally:
        sol.close()


def test_headline_properties_1e8(env):
    """n = 1e8, m = 10, the bench's problem and options (ping-pong entry, deferred line search, compact_w = 1) at a
    steady-state NEW_X return: H inverts B, B is symmetric, H is positive definite, diag(B) is B's diagonal"""
    la, torch = env["la"], env["torch"]
    n, m = 100_000_000, 10
    sol = la.DeviceSolver(n, m, same_stream_objective=True, defer_lnsrch=True, options={"compact_w": 1})
    try:
        xs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2)]
        gs = [torch.zeros_like(xs[0]) for _ in range(2)]
        l, u = torch.full_like(xs[0], -1.0), torch.full_like(xs[0], 1.0)
        nbd = torch.full((n,), 2, dtype=torch.int32, device="cuda")
        for _ in range(400):
            t, cur = sol.setulb_pp(xs, l, u, nbd, gs, 0.0, 0.0)
            if t.startswith("FG"):
                sol.objective(0, xs[cur], gs[cur], deferred=True)
            elif not t.startswith("NEW_X") or sol.isave[29] >= 16:
                break
        assert t.startswith("NEW_X") and int(sol.isave[27]) == m, t
        del xs, gs, l, u, nbd
        gen = torch.Generator(device="cuda").manual_seed(3)
        v = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        w = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        bv = sol.qn_apply(v)
        hbv = sol.qn_apply(bv, inverse=True)
        assert (torch.linalg.norm(hbv - v) / torch.linalg.norm(v)).item() <= 1e-10
        del hbv
        bw = sol.qn_apply(w)
        assert abs((w @ bv - v @ bw).item()) <= 1e-12 * (torch.linalg.norm(w) * torch.linalg.norm(bv)).item()
        del bw
        hv = sol.qn_apply(v, inverse=True)
        assert (v @ hv).item() > 0
        del hv, bv
        db = sol.qn_diag()
        e = torch.zeros_like(v)
        for i in (0, 12345, 50_000_001, n - 1):
            e.zero_()
            e[i] = 1.0
            bi = sol.qn_apply(e)[i].item()
            assert abs(db[i].item() - bi) <= 1e-12 * abs(bi), (i, db[i].item(), bi)
    finally:
        sol.close()

