"""Gram matrices of the curvature model on blocks of vectors (lbfgsb_hip_qn_gram; DeviceSolver.qn_gram,
QnOperator.gram): (V - c)'B(V - c) and (V - c)'H(V - c) against the dense numpy model built from export_state at an
empty, a partly filled and a wrapped ring, for every split of a block into pieces (k = 1 .. 5, 9); what needs no
model (symmetry and reproducibility bit for bit, the diagonal against qn_quad, a pair alone against inside a block,
unaligned operands, leading dimensions); REAL32; the tile-local layout of W read as it is; a grid above its cap
against torch; runs that call the entry at every return bit-identical to runs that do not; and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:  # the dense model and the driver of the root tests, the run configurations of the quadratic forms' tests
    from test_gpu_qn_root import SHAPES, _cond_and_norm, _drive, _model, _problem, _wrapped
    from test_gpu_qn_quad import RUNS
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
KS = (1, 2, 3, 4, 5, 9)


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _dt(sol, torch):
    return torch.float32 if sol.real == np.float32 else torch.float64


def _check_gram(env, sol, eps=1e-10, ks=KS, packed=None):
    """qn_gram of both modes against the dense model, entry by entry:
        |g_ab - d_a'B d_b| <= eps |B|_2 |d_a| |d_b|,
        |g_ab - d_a'H d_b| <= eps cond(B) max(|d_a| |H d_b|, |d_b| |H d_a|)
    (the bounds of the quadratic forms, tests/test_gpu_qn_quad.py, for two vectors), and what needs no model.  Every
    call of the entry comes first and the dense model (export_state, which puts a packed W back into natural order)
    last; packed: the compact_stats that must still hold after the last call of the entry."""
    torch = env["torch"]
    n = sol.n
    dt = _dt(sol, torch)
    fp64 = sol.real == np.float64
    col = int(sol.isave[27])
    rng = np.random.default_rng(n + 31 * col)
    cen = rng.standard_normal(n).astype(sol.real)
    Vs = [rng.standard_normal((k, n)).astype(sol.real) for k in ks]
    ct = torch.from_numpy(cen).cuda()
    got = []
    for k, V in zip(ks, Vs):
        vt = torch.from_numpy(V).cuda()
        gb, gh = sol.qn_gram(vt, center=ct), sol.qn_gram(vt, center=ct, inverse=True)
        assert gb.shape == (k, k) and gb.dtype == np.float64 and gh.shape == (k, k)
        got.append((gb, gh))
    # ---- what needs no model
    V = torch.from_numpy(Vs[-1]).cuda()
    k = V.shape[0]
    zero = torch.zeros(n, dtype=dt, device="cuda")
    lib = env["la"].load_library()
    for inverse in (False, True):
        g = sol.qn_gram(V, center=ct, inverse=inverse)
        assert np.array_equal(g, g.T)                                                     # symmetric bit for bit
        assert np.array_equal(g, got[-1][1 if inverse else 0])                            # twice: the same bits
        assert np.array_equal(sol.qn_gram(V, inverse=inverse), sol.qn_gram(V, center=zero, inverse=inverse))
        q = sol.qn_quad(V, center=ct, inverse=inverse)
        assert np.all(np.abs(np.diag(g) - q) <= 1e-13 * np.abs(q)), (np.diag(g), q)
        na = np.sqrt(np.diag(g))                                                          # |d_a|_A
        tol = 1e-13 * np.outer(na, na)
        for a, b in ((0, k - 1), (1, 2), (3, 4)):                                         # a pair alone / in the block
            if b >= k or a == b:
                continue
            g2 = sol.qn_gram(torch.stack([V[a], V[b]]), center=ct, inverse=inverse)
            assert abs(g2[0, 1] - g[a, b]) <= tol[a, b], (a, b, g2[0, 1], g[a, b])
        g1 = sol.qn_gram(V[0], center=ct, inverse=inverse)
        assert g1.shape == (1, 1) and abs(g1[0, 0] - g[0, 0]) <= tol[0, 0]
        if fp64:
            # operands that are not 16-byte aligned: one row per lane, another order of the sums
            buf = torch.empty(V.numel() + 1, dtype=dt, device="cuda")
            off = buf[1:].view(V.shape)
            off.copy_(V)
            cbuf = torch.empty(n + 1, dtype=dt, device="cuda")
            cbuf[1:].copy_(ct)
            assert off.data_ptr() % 16 == 8 and cbuf[1:].data_ptr() % 16 == 8
            for gg in (sol.qn_gram(off, center=ct, inverse=inverse), sol.qn_gram(V, center=cbuf[1:], inverse=inverse)):
                assert np.all(np.abs(gg - g) <= tol)
        wide = torch.empty((k, n + 3), dtype=dt, device="cuda")                           # ldv = n + 3
        wide[:, :n].copy_(V)
        assert np.all(np.abs(sol.qn_gram(wide[:, :n], center=ct, inverse=inverse) - g) <= tol)
        pad = np.full((k, k + 2), -7.0)                                                   # ldg = k + 2, column-major
        assert lib.lbfgsb_hip_qn_gram(sol.h, 1 if inverse else 0, k, V.data_ptr(), V.stride(0), ct.data_ptr(),
                                      pad.ctypes.data_as(C.POINTER(C.c_double)), k + 2) == 0
        assert np.array_equal(pad[:, :k], g) and np.all(pad[:, k:] == -7.0)
        ev = np.linalg.eigvalsh(g)
        assert ev[0] >= -1e-10 * np.abs(ev).max(), ev
        op = sol.qn_operator(inverse=inverse)
        assert np.array_equal(op.gram(V, center=ct), g)
        with pytest.raises(ValueError):
            op.sqrt().gram(V)
    if packed is not None:
        assert sol.compact_stats() == packed  # (packed throughout: every call above read the layout as it is)
    # ---- against the dense model
    B, mcol, theta, W = _model(sol)
    assert mcol == col
    cond, nb = _cond_and_norm(B, theta, W)
    D = np.concatenate(Vs).astype(np.float64) - cen.astype(np.float64)
    if col == 0:
        BD, HD, cond, nb = theta * D, D / theta, 1.0, theta
    else:
        BD, HD = D @ B.T, np.linalg.solve(B, D.T).T  # one factorisation for every vector
    dn, hn = np.linalg.norm(D, axis=1), np.linalg.norm(HD, axis=1)
    at = 0
    for k, (gb, gh) in zip(ks, got):
        sl = slice(at, at + k)
        at += k
        eb, bb = np.abs(gb - D[sl] @ BD[sl].T), eps * nb * np.outer(dn[sl], dn[sl])
        eh = np.abs(gh - D[sl] @ HD[sl].T)
        bh = eps * cond * np.maximum(np.outer(dn[sl], hn[sl]), np.outer(hn[sl], dn[sl]))
        print("n %d col %d k %d: max |g - D'BD| / bound = %.3e, max |g - D'HD| / bound = %.3e"
              % (n, col, k, (eb / bb).max(), (eh / bh).max()))
        assert np.all(eb <= bb), (k, col)
        assert np.all(eh <= bh), (k, col, cond)
        if col == 0 and fp64:  # no pair: theta D'D, D'D / theta
            dd = np.outer(dn[sl], dn[sl])
            assert np.all(eb <= 1e-13 * theta * dd) and np.all(eh <= 1e-13 * dd / theta)
    return dict(B=B, col=col, theta=theta, cond=cond, nb=nb)


# ---------------------------------------------------------------- against the dense model, fp64
@pytest.mark.parametrize("n,m", SHAPES)
def test_gram_against_dense_fp64(env, n, m):
    """col = 0 (FG_START), a partly filled ring and a full ring whose head has wrapped.  k = 1 .. 5 and 9: pieces of
    4, 2, 1 and 3 -> 2 + 1, at more than 10 pairs pieces of at most 2 on 16-wide tiles, several column tiles at m =
    17 and 40, cross launches of unequal pieces (4 x 1, 2 x 1, 4 x 4 ...)."""
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
            _check_gram(env, s)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert "empty" in seen and "wrapped" in seen, seen
    assert "part" in seen or m == 1, seen


# ---------------------------------------------------------------- REAL32
@pytest.mark.parametrize("n,m", [(1000, 17), (4099, 10)])
def test_gram_real32(env, n, m):
    """fp32 pairs and vectors, fp64 differences and sums: the dense fp64 model of the exported fp32 pairs, the bounds
    with 4 * 2^-24 for 1e-10 (the vectors are rounded to fp32), as the quadratic forms' REAL32 test"""
    la = env["la"]
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) == m + 2:
                checked.append(_check_gram(env, s, eps=4.0 * 2.0 ** -24))
        _drive(env, sol, p, max_iter=m + 2, at_return=at)
    finally:
        sol.close()
    assert checked and checked[0]["col"] == m


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("policy", [1, 2])
def test_gram_on_the_packed_layout(env, policy):
    """compact_w = 2 on the separable quadratic (the set-up of test_layout_read_as_it_is of the quadratic forms): W is
    read in the tile-local layout -- still packed after the last call -- and the matrices meet the fp64 bounds against
    the dense model of the exported pairs all the same"""
    la = env["la"]
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
            assert before[0] >= 1
            got["mdl"] = _check_gram(env, s, packed=before)
            got["packs"] = before[0]
        _drive(env, sol, p, max_iter=60, at_return=at, until=lambda s: bool(got))
    finally:
        sol.close()
    assert got, "the layout never packed"
    assert got["packs"] >= 1 and got["mdl"]["col"] == m


# ---------------------------------------------------------------- a capped grid
@pytest.mark.parametrize("real32", [False, True])
def test_gram_on_a_capped_grid(env, real32):
    """n = 1 000 003 (the n of test_draws_bit_identical_on_a_capped_grid): every workgroup takes more than one trip.
    k = 5 with a center, no pair and a full ring of 10.  Reference: D @ qn_apply(D).T, formed by torch in fp64 on
    the device; |g_ab - ref_ab| <= 1e-10 (|d_a| |A d_b| + |d_b| |A d_a|).  The vectors and the center are multiples
    of 1/4 of small size: their differences are exact in fp32, so D is the same matrix for both real kinds."""
    la, torch = env["la"], env["torch"]
    n, m, k = 1_000_003, 10, 5
    sol = la.DeviceSolver(n, m, real32=real32)
    try:
        dt = _dt(sol, torch)
        x = torch.zeros(n, dtype=dt, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        gen = torch.Generator(device="cpu").manual_seed(9)
        V = (torch.randint(-8, 9, (k, n), generator=gen).to(dt) / 4).cuda()
        cen = (torch.randint(-8, 9, (n,), generator=gen).to(dt) / 4).cuda()
        D = V - cen
        D64 = D.double()
        assert torch.equal(D64, V.double() - cen.double())
        dn = torch.linalg.norm(D64, dim=1)
        checked = 0
        while True:
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG_START") or (t.startswith("NEW_X") and sol.isave[29] >= m + 2):
                assert int(sol.isave[27]) == (0 if t.startswith("FG_START") else m)
                for inverse in (False, True):
                    got = sol.qn_gram(V, center=cen, inverse=inverse)
                    AD = sol.qn_apply(D, inverse=inverse).double()
                    ref = (D64 @ AD.T).cpu().numpy()
                    an = torch.linalg.norm(AD, dim=1)
                    bound = 1e-10 * (torch.outer(dn, an) + torch.outer(an, dn)).cpu().numpy()
                    err = np.abs(got - ref)
                    print("real32 %s col %d inverse %s: max |g - ref| / bound = %.3e"
                          % (real32, int(sol.isave[27]), inverse, (err / bound).max()))
                    assert np.all(err <= bound)
                    assert np.array_equal(got, got.T)
                    checked += 1
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or sol.isave[29] >= m + 2:
                break
        assert t.startswith("NEW_X") and checked == 4, (t, checked)
    finally:
        sol.close()


# ---------------------------------------------------------------- the run that does not notice
def _gram_entries(sol, torch, n, k=5):
    g = torch.Generator(device="cpu").manual_seed(5)
    V = torch.randn(k + 1, n, generator=g, dtype=torch.float64).cuda()
    return [sol.qn_gram(V[:k], center=V[k]), sol.qn_gram(V[:k], center=V[k], inverse=True), sol.qn_gram(V[0])]


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
                    _gram_entries(s, torch, n)
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
    v = torch.ones(4 * n, dtype=torch.float64, device="cuda")
    res = np.full(16, -7.0)
    rp = res.ctypes.data_as(C.POINTER(C.c_double))

    def gram(s, mode=0, k=2, vp=v.data_ptr(), ld=n, r=rp, ldg=None):
        rc = lib.lbfgsb_hip_qn_gram(s.h, mode, k, vp, ld, None, r, k if ldg is None else ldg)
        if rc != 0:
            assert np.all(res == -7.0), rc       # a refusal changes nothing
        return rc
    sol = la.DeviceSolver(n, m)
    try:
        assert gram(sol) == E_STATE                                          # no run
        _drive(env, sol, p, max_iter=8)
        for mode in (la.QN_B_SQRT, la.QN_H_SQRT, 2, 3, 7):
            assert gram(sol, mode=mode) == E_ARG, mode
        assert gram(sol, vp=None) == E_ARG and gram(sol, r=None) == E_ARG
        assert gram(sol, k=0) == E_ARG and gram(sol, k=-1) == E_ARG and gram(sol, k=65) == E_ARG
        assert gram(sol, ld=n - 1) == E_ARG and gram(sol, k=3, ldg=2) == E_ARG
        assert np.all(res == -7.0)
        assert gram(sol, mode=0, k=4) == 0 and np.all(np.isfinite(res))
        g4 = res.reshape(4, 4).copy()
        assert gram(sol, mode=1, k=4) == 0
        assert np.array_equal(g4, sol.qn_gram(v.view(4, n))) and np.array_equal(g4, g4.T)
        big = torch.ones((64, n), dtype=torch.float64, device="cuda")       # k = LBFGSB_QN_GRAM_MAXK: accepted
        g64 = sol.qn_gram(big)
        assert g64.shape == (64, 64) and np.all(g64 == g64[0, 0])
    finally:
        sol.close()
    # a deferred line-search set-up that is still live: E_STATE, nothing changed
    res[:] = -7.0
    cfg = RUNS["pingpong_defer"]
    sol = la.DeviceSolver(n, m, **cfg["ctor"])
    rcs = {}
    try:
        def at(s, t):
            rc = gram(s)
            rcs.setdefault(t[:9], set()).add(rc)
            res[:] = -7.0
        _drive(env, sol, p, max_iter=8, at_return=at, pp=cfg["pp"])
    finally:
        sol.close()
    assert E_STATE in rcs.get("FG_LNSRCH", set()), rcs
    assert 0 in rcs.get("NEW_X", set()), rcs
    assert all(rc in (0, E_STATE) for s in rcs.values() for rc in s), rcs
