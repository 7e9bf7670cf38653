"""Quadratic forms and Gaussian log-densities of the curvature model (lbfgsb_hip_qn_quad, lbfgsb_hip_qn_logpdf,
lbfgsb_hip_qn_draw_logpdf; DeviceSolver.qn_quad / qn_logpdf / qn_draw(return_logpdf=True)): d'B d and d'H d against
the dense numpy model built from export_state, log-densities against slogdet and the dense quadratic form, z'z of the
draws against the numpy Philox reference with the draws themselves bit-identical to qn_draw's, REAL32, the
tile-local layout of W read as it is, runs that call the entries at every return bit-identical to runs that do not,
and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:  # the dense model, the driver and the generator's numpy reference of the root tests
    from test_gpu_qn_root import (SHAPES, _cond_and_norm, _drive, _first_return, _model, _problem, _slow_quadratic,
                                  _wrapped, z_ref)
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
LOG2PI = float(np.log(2.0 * np.pi))


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _dt(sol, torch):
    return torch.float32 if sol.real == np.float32 else torch.float64


def _quad_refs(B, D):
    """d'B d, d'H d, |d|, |H d| per row of D from the dense model (one factorisation)"""
    HD = np.linalg.solve(B, D.T).T
    return np.einsum("ij,ij->i", D @ B.T, D), np.einsum("ij,ij->i", HD, D), np.linalg.norm(D, axis=1), \
        np.linalg.norm(HD, axis=1)


def _check_quad(env, sol, eps=1e-10, ks=(1, 3, 9)):
    """qn_quad of both modes against the dense model: |q - d'B d| <= eps |B|_2 |d|^2 and |q - d'H d| <= eps cond(B) |d|
    |H d| -- the bounds of the root tests for B V and H V, carried through one inner product.  Then what does not
    need the model: no center against a zero center, alone against inside a block, unaligned operands, twice."""
    torch = env["torch"]
    n = sol.n
    dt = _dt(sol, torch)
    B, col, theta, W = _model(sol)
    cond, nb = _cond_and_norm(B, theta, W)
    rng = np.random.default_rng(n + 31 * col)
    cen = rng.standard_normal(n).astype(sol.real)
    Vs = [rng.standard_normal((k, n)).astype(sol.real) for k in ks]
    D = np.concatenate(Vs).astype(np.float64) - cen.astype(np.float64)
    if col == 0:
        dd = np.einsum("ij,ij->i", D, D)
        qb_ref, qh_ref, dn, hn = theta * dd, dd / theta, np.sqrt(dd), np.sqrt(dd) / theta
    else:
        qb_ref, qh_ref, dn, hn = _quad_refs(B, D)
    ct = torch.from_numpy(cen).cuda()
    at = 0
    for k, V in zip(ks, Vs):
        vt = torch.from_numpy(V).cuda()
        qb, qh = sol.qn_quad(vt, center=ct), sol.qn_quad(vt, center=ct, inverse=True)
        assert qb.shape == (k,) and qb.dtype == np.float64
        sl = slice(at, at + k)
        at += k
        eb, bb = np.abs(qb - qb_ref[sl]), eps * nb * dn[sl] ** 2
        eh, bh = np.abs(qh - qh_ref[sl]), eps * cond * dn[sl] * hn[sl]
        print("n %d col %d k %d: max |q - d'Bd| = %.3e (bound %.3e), max |q - d'Hd| = %.3e (bound %.3e)"
              % (n, col, k, eb.max(), bb[eb.argmax()], eh.max(), bh[eh.argmax()]))
        assert np.all(eb <= bb), (k, col)
        assert np.all(eh <= bh), (k, col, cond)
        if col == 0 and sol.real == np.float64:  # no pair: theta d'd, d'd / theta
            assert np.all(eb <= 1e-13 * qb_ref[sl]) and np.all(eh <= 1e-13 * qh_ref[sl])
    V = torch.from_numpy(Vs[-1]).cuda()
    zero = torch.zeros(n, dtype=dt, device="cuda")
    for inverse in (False, True):
        q = sol.qn_quad(V, center=ct, inverse=inverse)
        assert np.array_equal(q, sol.qn_quad(V, center=ct, inverse=inverse))            # twice: the same bits
        assert np.array_equal(sol.qn_quad(V, inverse=inverse), sol.qn_quad(V, center=zero, inverse=inverse))
        for j in (0, V.shape[0] - 1):                                                    # alone / inside a block
            q1 = sol.qn_quad(V[j], center=ct, inverse=inverse)
            assert isinstance(q1, float) and abs(q1 - q[j]) <= 1e-13 * abs(q[j]), (j, q1, q[j])
        if sol.real == np.float64:
            # operands that are not 16-byte aligned: one row per lane, another order of the sums
            buf = torch.empty(V.numel() + 1, dtype=dt, device="cuda")
            off = buf[1:].view(V.shape)
            off.copy_(V)
            cbuf = torch.empty(n + 1, dtype=dt, device="cuda")
            cbuf[1:].copy_(ct)
            assert off.data_ptr() % 16 == 8 and cbuf[1:].data_ptr() % 16 == 8
            for qq in (sol.qn_quad(off, center=ct, inverse=inverse), sol.qn_quad(V, center=cbuf[1:], inverse=inverse)):
                assert np.all(np.abs(qq - q) <= 1e-13 * np.abs(q))
    return dict(B=B, col=col, theta=theta, cond=cond, nb=nb)


def _logpdf_ref(n, logdet_b, qb_ref, qh_ref, inverse, s):
    """log N(x; mean, s^2 A), A = H (inverse) or B, from the dense quantities"""
    logdet = -logdet_b if inverse else logdet_b
    q = qb_ref if inverse else qh_ref  # the quadratic form of A^-1
    return -0.5 * (n * LOG2PI + 2.0 * n * np.log(abs(s)) + logdet + q / (s * s))


def _check_logpdf(env, sol, mdl):
    """qn_logpdf against the dense model: tolerance 1/2 (the quadratic form's bound) / s^2 + 1/2 1e-10 n, the second
    term the bound on log det of the root tests"""
    torch = env["torch"]
    n = sol.n
    B, col, theta, cond, nb = mdl["B"], mdl["col"], mdl["theta"], mdl["cond"], mdl["nb"]
    rng = np.random.default_rng(7 * n + col)
    mean = rng.standard_normal(n)
    X = rng.standard_normal((3, n))
    D = X - mean
    if col == 0:
        dd = np.einsum("ij,ij->i", D, D)
        qb_ref, qh_ref, dn, hn = theta * dd, dd / theta, np.sqrt(dd), np.sqrt(dd) / theta
        sign, logdet_b = 1.0, n * np.log(theta)
    else:
        qb_ref, qh_ref, dn, hn = _quad_refs(B, D)
        sign, logdet_b = np.linalg.slogdet(B)
    assert sign == 1.0
    xt, mt = torch.from_numpy(X).cuda(), torch.from_numpy(mean).cuda()
    for inverse in (False, True):
        qbound = 1e-10 * nb * dn ** 2 if inverse else 1e-10 * cond * dn * hn
        for s in (1.0, 0.5, -2.0):
            lp = sol.qn_logpdf(xt, mean=mt, scale=s, inverse=inverse)
            ref = _logpdf_ref(n, logdet_b, qb_ref, qh_ref, inverse, s)
            err, tol = np.abs(lp - ref), 0.5 * qbound / (s * s) + 0.5 * 1e-10 * n
            print("n %d col %d inverse %s scale %g: max |logp - ref| = %.3e (tolerance %.3e)"
                  % (n, col, inverse, s, err.max(), tol[err.argmax()]))
            assert np.all(err <= tol), (inverse, s)
        lp1 = sol.qn_logpdf(xt[1], mean=mt, scale=0.5, inverse=inverse)
        assert isinstance(lp1, float)
        op = sol.qn_operator(inverse=inverse)
        assert op.log_prob(xt[1], mean=mt, scale=0.5) == lp1
        assert op.quad(xt[1], center=mt) == sol.qn_quad(xt[1], center=mt, inverse=inverse)
        with pytest.raises(ValueError):
            op.sqrt().quad(xt[1])
        with pytest.raises(ValueError):
            op.sqrt().log_prob(xt[1])


# ---------------------------------------------------------------- the quadratic forms and qn_logpdf, fp64
@pytest.mark.parametrize("n,m", SHAPES)
def test_quad_and_logpdf_against_dense_fp64(env, n, m):
    """col = 0 (FG_START), a partly filled ring and a full ring whose head has wrapped; qn_logpdf where n <= 1000"""
    la = env["la"]
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)  # (no early stop: the ring fills and wraps)
    sol = la.DeviceSolver(n, m)
    seen = set()
    try:
        def at(s, t):
            col = int(s.isave[27])
            if 2 * col > n or not (t.startswith("NEW_X") or t.startswith("FG_START")):
                return
            tag = "empty" if col == 0 else ("wrapped" if _wrapped(s) else ("full" if col == m else "part"))
            if tag in seen or tag == "full" or (tag == "part" and col < max(1, m // 2)):
                return
            seen.add(tag)
            mdl = _check_quad(env, s)
            if n <= 1000:
                _check_logpdf(env, s, mdl)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert "empty" in seen and "wrapped" in seen, seen
    assert "part" in seen or m == 1, seen


# ---------------------------------------------------------------- the densities of the draws
def _zz_of(logp, n, scale, logdet):
    return -2.0 * logp - (n * LOG2PI + 2.0 * n * np.log(abs(scale)) + logdet)


def _check_draw_logpdf(sol, torch, seed, k, first, mean, scale, inverse):
    """out bit for bit qn_draw's; z'z recovered from the log-densities against the numpy generator: every z within
    1e-13 (1 + |z|) of it, the rest summation order -- 1e-10 sum z_ref^2"""
    n = sol.n
    d, lp = sol.qn_draw(k, seed, first=first, mean=mean, scale=scale, inverse=inverse, return_logpdf=True)
    assert torch.equal(d, sol.qn_draw(k, seed, first=first, mean=mean, scale=scale, inverse=inverse))
    assert lp.shape == (k,) and lp.dtype == np.float64
    zz = _zz_of(lp, n, scale, sol.qn_logdet(inverse=inverse))
    for j in range(k):
        ref = float(np.sum(z_ref(seed, 0, n, first + j) ** 2))
        print("inverse %s sample %d: z'z = %.15e, reference %.15e" % (inverse, first + j, zz[j], ref))
        assert abs(zz[j] - ref) <= 1e-10 * ref, j
    return d, lp


@pytest.mark.parametrize("m", [10, 17])
def test_draw_densities(env, m):
    """first = 3, k = 5: an odd first sample split off, then a block of 4"""
    la, torch = env["la"], env["torch"]
    n, seed, k, first, scale = 4099, 20260101, 5, 3, 0.5
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)
    sol = la.DeviceSolver(n, m)
    try:
        mean = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
        _first_return(env, sol)
        for inverse in (False, True):  # no pair: the pass on an empty tile
            _check_draw_logpdf(sol, torch, seed, k, first, mean, scale, inverse)
    finally:
        sol.close()
    sol = la.DeviceSolver(n, m)
    try:
        _drive(env, sol, p, max_iter=4 * m + 40, until=_wrapped)
        assert _wrapped(sol)
        B, col, theta, W = _model(sol)
        cond, nb = _cond_and_norm(B, theta, W)
        for inverse in (False, True):
            d, lp = _check_draw_logpdf(sol, torch, seed, k, first, mean, scale, inverse)
            # the other route: qn_logpdf at the stored draws, within qn_logpdf's own tolerance
            D = (d - mean).cpu().numpy()
            dn = np.linalg.norm(D, axis=1)
            qbound = 1e-10 * nb * dn ** 2 if inverse else \
                1e-10 * cond * dn * np.linalg.norm(np.linalg.solve(B, D.T), axis=0)
            tol = 0.5 * qbound / scale ** 2 + 0.5 * 1e-10 * n
            at = sol.qn_logpdf(d, mean=mean, scale=scale, inverse=inverse)
            err = np.abs(at - lp)
            print("m %d inverse %s: max |logpdf(draw) - draw's logp| = %.3e (tolerance %.3e)"
                  % (m, inverse, err.max(), tol[err.argmax()]))
            assert np.all(err <= tol)
        op = sol.qn_operator()
        d2, lp2 = op.sample(2, seed, log_prob=True)
        assert torch.equal(d2, sol.qn_draw(2, seed)) and lp2.shape == (2,)
        assert torch.equal(op.sample(2, seed), d2)
    finally:
        sol.close()


@pytest.mark.parametrize("real32", [False, True])
def test_draws_bit_identical_on_a_capped_grid(env, real32):
    """n = 1 000 003: above every cap of the passes' grid (at most 768 workgroups of 256 lanes with two rows each),
    where a workgroup's rows depend on the grid -- qn_draw_logpdf sizes the flagged W'z pass's grid as qn_draw sizes
    the plain one's, so the draws stay the same bits.  No pair (the empty tile), then a full ring of 10 pairs: blocks
    of 1 sample (two rows per lane) and of 4 (one row per lane)."""
    la, torch = env["la"], env["torch"]
    n, m, seed = 1_000_003, 10, 99
    sol = la.DeviceSolver(n, m, real32=real32)
    try:
        dt = _dt(sol, torch)
        x = torch.zeros(n, dtype=dt, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        checked = 0
        while True:
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG_START") or (t.startswith("NEW_X") and sol.isave[29] >= m + 2):
                assert int(sol.isave[27]) == (0 if t.startswith("FG_START") else m)
                for inverse in (False, True):
                    d, lp = sol.qn_draw(5, seed, first=3, scale=0.5, inverse=inverse, return_logpdf=True)
                    assert torch.equal(d, sol.qn_draw(5, seed, first=3, scale=0.5, inverse=inverse))
                    assert np.all(np.isfinite(lp))
                    checked += 1
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or sol.isave[29] >= m + 2:
                break
        assert t.startswith("NEW_X") and checked == 4, (t, checked)
    finally:
        sol.close()


# ---------------------------------------------------------------- REAL32
@pytest.mark.parametrize("n,m", [(1000, 17), (4099, 10)])
def test_quad_and_draw_densities_real32(env, n, m):
    """fp32 pairs and vectors, fp64 differences and sums: the dense fp64 model of the exported fp32 pairs, the bounds
    with 4 * 2^-24 for 1e-10 (the vectors are rounded to fp32); z'z as in fp64 (its sums are fp64)"""
    la, torch = env["la"], env["torch"]
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) == m + 2:
                checked.append(_check_quad(env, s, eps=4.0 * 2.0 ** -24, ks=(1, 9)))
                mean = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(np.float32)).cuda()
                for inverse in (False, True):
                    _check_draw_logpdf(s, torch, 77, 5, 3, mean, 0.5, inverse)
        _drive(env, sol, p, max_iter=m + 2, at_return=at)
    finally:
        sol.close()
    assert checked and checked[0]["col"] == m


# ---------------------------------------------------------------- the layout, and the run that does not notice
def _quad_entries(sol, torch, n, k=3):
    g = torch.Generator(device="cpu").manual_seed(5)
    V = torch.randn(k, n, generator=g, dtype=torch.float64).cuda()
    d, lp = sol.qn_draw(k, 11, first=1, mean=V[0], scale=2.0, return_logpdf=True)
    assert torch.equal(d, sol.qn_draw(k, 11, first=1, mean=V[0], scale=2.0))
    return [sol.qn_quad(V, center=V[1]), sol.qn_quad(V, inverse=True), np.array([sol.qn_quad(V[0], center=V[2])]),
            sol.qn_logpdf(V, mean=V[0], scale=0.5), sol.qn_logpdf(V, inverse=False), lp, d.cpu().numpy()]


@pytest.mark.parametrize("policy", [1, 2])
def test_layout_read_as_it_is(env, policy):
    """compact_w = 2: the entries on a packed W equal the same calls after set_option("compact_w", 0).  The separable
    quadratic with all four bound types: a quarter of its rows sits at a bound and the free set stands still from
    iteration 16 on, with the ring full -- what the automatic policy waits for (driver1's Rosenbrock at m = 10 flips
    half of its rows every other iteration and never packs under it)."""
    la, torch = env["la"], env["torch"]
    n, m = 4099, 10
    p = _problem(env, "quadratic", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": policy, "compact_min_rows": 0})
    got = {}
    try:
        def at(s, t):
            if got or not t.startswith("NEW_X") or int(s.isave[27]) < m:
                return
            if not s.compact_stats()[2]:
                return
            before = s.compact_stats()
            got["res"] = _quad_entries(s, torch, n)
            got["again"] = _quad_entries(s, torch, n)
            assert s.compact_stats() == before
            s.set_option("compact_w", 0)
            assert not s.compact_stats()[2]
            got["plain"] = _quad_entries(s, torch, n)
        _drive(env, sol, p, max_iter=60, at_return=at, until=lambda s: bool(got))
    finally:
        sol.close()
    assert got, "the layout never packed"
    for a, b in zip(got["res"], got["again"]):
        assert np.array_equal(a, b)  # reproducible bit for bit
    for a, b in zip(got["res"], got["plain"]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


RUNS = {
    "classic": dict(pp=False),
    "pingpong_defer": dict(pp=True, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
    "builtin_deferred_f": dict(pp=False, builtin=1, deferred_f=True),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    la, torch = env["la"], env["torch"]
    cfg = RUNS[name]
    n, m = 4099, 7
    p = _problem(env, "rosenbrock", n, m)
    iters = 30
    outs = []
    counts = {"ok": 0, "refused": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                try:
                    _quad_entries(s, torch, n, k=3)
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
    if name != "classic":
        assert counts["refused"] > 0


# ---------------------------------------------------------------- refusals
def test_refusals_and_arguments(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    v = torch.ones(2 * n, dtype=torch.float64, device="cuda")
    out = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    res = (C.c_double * 4)()
    quad = lambda s, mode=0, k=1, vp=v.data_ptr(), ld=n, r=res: lib.lbfgsb_hip_qn_quad(s.h, mode, k, vp, ld, None, r)
    logpdf = lambda s, mode=1, k=1, xp=v.data_ptr(), ld=n, scale=1.0, r=res: \
        lib.lbfgsb_hip_qn_logpdf(s.h, mode, k, xp, ld, None, scale, r)
    dlp = lambda s, mode=1, k=1, first=0, scale=1.0, o=out.data_ptr(), ldo=n, r=res: \
        lib.lbfgsb_hip_qn_draw_logpdf(s.h, mode, k, 7, first, None, scale, o, ldo, r)
    sol = la.DeviceSolver(n, m)
    try:
        assert quad(sol) == E_STATE and logpdf(sol) == E_STATE and dlp(sol) == E_STATE  # no run
        _drive(env, sol, p, max_iter=8)
        for fn in (quad, logpdf, dlp):
            for mode in (la.QN_B_SQRT, la.QN_H_SQRT, 2, 3, 7):
                assert fn(sol, mode=mode) == E_ARG, mode
            assert fn(sol, k=0) == E_ARG and fn(sol, r=None) == E_ARG
            assert fn(sol, mode=0, k=2) == 0 and fn(sol, mode=1, k=2) == 0
        assert quad(sol, ld=n - 1) == E_ARG and logpdf(sol, ld=n - 1) == E_ARG and dlp(sol, ldo=n - 1) == E_ARG
        assert quad(sol, vp=None) == E_ARG and logpdf(sol, xp=None) == E_ARG and dlp(sol, o=None) == E_ARG
        assert dlp(sol, first=-1) == E_ARG
        for fn in (logpdf, dlp):
            for s in (0.0, float("inf"), float("-inf"), float("nan")):
                assert fn(sol, scale=s) == E_ARG, s
            assert fn(sol, scale=-2.0) == 0 and np.isfinite(res[0])
    finally:
        sol.close()
    # 40 pairs: qn_quad needs neither a root nor the diagonal; 65: beyond LBFGSB_QN_ROOT_MAXCOL for the densities
    sol = la.DeviceSolver(1000, 70)
    try:
        w = torch.ones(1000, dtype=torch.float64, device="cuda")
        o = torch.empty_like(w)
        seen = []

        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[27]) == 40 and not seen:
                seen.append(_check_quad(env, s, ks=(3,))["col"])
        _, t = _drive(env, sol, _slow_quadratic(env, 1000, 70), max_iter=400, at_return=at,
                      until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65 and seen == [40], t
        assert lib.lbfgsb_hip_qn_logpdf(sol.h, 1, 1, w.data_ptr(), 1000, None, 1.0, res) == E_ARG
        assert lib.lbfgsb_hip_qn_draw_logpdf(sol.h, 1, 1, 7, 0, None, 1.0, o.data_ptr(), 1000, res) == E_ARG
        assert lib.lbfgsb_hip_qn_quad(sol.h, 1, 1, w.data_ptr(), 1000, None, res) == 0
        assert np.isfinite(sol.qn_quad(w)) and np.isfinite(sol.qn_quad(w, inverse=True))
    finally:
        sol.close()
