"""Square roots, draws and log-densities of the model plus a diagonal (lbfgsb_hip_qn_shift_sqrt / _draw /
_draw_logpdf / _quad / _logpdf; QnShifted.sqrt / sample / quad / log_prob) against dense numpy on the free block of the
model built from export_state.  With P = B + mu I + D on the free rows, Sigma = P^-1 and cond its 2-norm condition:
  factor   n <= 64: L = sqrt(identity), |L L' - Sigma| <= tol cond |Sigma| (Frobenius); every n: sqrt of 9 random
           vectors against numpy's L = diag(sqrt w) (I + What N What')^(1/2) -- the symmetric root is unique, so this
           is the device's L -- within tol cond |L|_2 |V|_F, tol = 1e-10 (fp64) or 1e-5 (REAL32);
  draws    mean + 0.5 sqrt(z_ref) with z_ref the numpy replay of the generator (test_gpu_qn_root.z_ref), on the bound of
           test_gpu_qn_root.test_draws_against_root_of_reference_z; one sample alone against the same sample in a block
           1e-13 relative; a repeated call, and out / mean at 8 mod 16 bytes, bit for bit; pinned rows = the mean;
           with rows pinned the free rows equal numpy's L of that pin pattern applied to the SAME z_ref;
  density  draw_logpdf (from z) = log_prob of the drawn points (the quadratic form) = dense numpy, and quad = dense
           q'P q, within tol cond (1 + |value|); log det by the root's route (read off log_prob at the mean) within
           1e-10 n of logdet(); every row pinned: the log-density is exactly 0.
Then the tile-local layout of W read as it is, REAL32, refusals, and runs that do not notice the calls."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_qn import _drive, _problem
from test_gpu_qn_root import _slow_quadratic, _wrapped, z_ref
from test_gpu_qn_shift import MU, _model, _shifts

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
SEED, K, FIRST, SCALE = 20260101, 5, 3, 0.5  # (an odd first sample: a single sample, then a block of 4)


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    assert hasattr(lbfgsb_amd.QnShifted, "sample")
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


class _Dense:
    """numpy's side of one shift: P on the free rows, its condition and log det, and L through its action"""

    def __init__(self, sol, wa, B, col, dd, mu):
        n, m = sol.n, sol.m
        theta, head = float(sol.dsave[0]), int(sol.isave[26])
        self.n, self.free = n, np.isfinite(dd)
        free = self.free
        self.nf = int(free.sum())
        self.P = (B + np.diag(np.where(free, mu + dd, 0.0)))[np.ix_(free, free)]
        self.rw = 1.0 / np.sqrt(theta + mu + dd[free])  # sqrt(w) on the free rows
        self.cond, self.lnorm, self.logdet = 1.0, 0.0, 0.0
        self.Q = np.zeros((self.nf, 0))
        self.T = np.zeros((0, 0))
        if not self.nf:
            return
        ev = np.linalg.eigvalsh(self.P)
        assert ev[0] > 0.0
        self.cond, self.lnorm = ev[-1] / ev[0], ev[0] ** -0.5  # |L|_2 = |Sigma|_2^(1/2)
        sign, self.logdet = np.linalg.slogdet(self.P)
        assert sign == 1.0
        if col:
            # A = Delta^-1/2 P Delta^-1/2 = I + E with E in the range of Delta^-1/2 [S, Y]: A^-1/2 = I + Q T Q'
            wa = wa.astype(np.float64)
            cols = [(head - 1 + j) % m for j in range(col)]
            W = np.hstack([wa[:m * n].reshape(m, n).T[:, cols], wa[m * n:2 * m * n].reshape(m, n).T[:, cols]])
            self.Q, _ = np.linalg.qr(W[free] * self.rw[:, None])
            E = self.rw[:, None] * self.P * self.rw[None, :] - np.eye(self.nf)
            G = self.Q.T @ E @ self.Q
            lam, U = np.linalg.eigh(np.eye(G.shape[0]) + 0.5 * (G + G.T))
            assert lam[0] > 0.0
            self.T = (U * (lam ** -0.5 - 1.0)) @ U.T

    def L(self, V):
        """L v_j for the rows of V (k, n): sqrt(w) o (A^-1/2 v) on the free rows, 0 on the pinned ones"""
        out = np.zeros(V.shape)
        x = V[:, self.free]
        out[:, self.free] = (x + ((x @ self.Q) @ self.T) @ self.Q.T) * self.rw[None, :]
        return out

    def quad(self, V, center):
        q = (V - (0.0 if center is None else center[None, :]))[:, self.free]
        return np.einsum("ki,ki->k", q @ self.P, q)

    def logpdf(self, X, mean, scale):
        return (-0.5 * self.quad(X, mean) / scale ** 2 - 0.5 * self.nf * np.log(2.0 * np.pi)
                - self.nf * np.log(abs(scale)) + 0.5 * self.logdet)


def _odd(torch, t):
    """a copy of t that starts 8 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    o = buf[1:].view(t.shape)
    assert t.element_size() != 8 or o.data_ptr() % 16 == 8
    o.copy_(t)
    return o


def _check_shift(env, sol, wa, B, col, d, mu, tol, tag, zr):
    """every check of one shift on one state; d: numpy in the solver's kind (+inf pins) or None"""
    torch, n = env["torch"], sol.n
    f64 = sol.real == np.float64
    dd = np.zeros(n) if d is None else d.astype(np.float64)
    ref = _Dense(sol, wa, B, col, dd, mu)
    free, nf, cond = ref.free, ref.nf, ref.cond
    sh = sol.qn_shift(None if d is None else torch.from_numpy(d).cuda(), mu)
    assert sh.pinned == n - nf
    rng = np.random.default_rng(n + 37 * col + nf)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(sol.real)).cuda()
    host = lambda t: t.cpu().numpy().astype(np.float64)
    V = rng.standard_normal((9, n)).astype(sol.real)
    x_before, ld_before = sh.solve(dev(V)), sh.logdet()

    # ---- the factor
    if n <= 64 and nf:
        Ld = host(sh.sqrt(dev(np.eye(n)))).T  # (row j of the output is L e_j)
        sigma = np.zeros((n, n))
        sigma[np.ix_(free, free)] = np.linalg.inv(ref.P)
        err, bound = np.linalg.norm(Ld @ Ld.T - sigma), tol * cond * np.linalg.norm(sigma)
        print("%s n %d col %d: |L L' - Sigma| = %.2e (bound %.2e, cond %.2e)" % (tag, n, col, err, bound, cond))
        assert err <= bound
    Vn = V.copy()
    Vn[:, ~free] = np.nan  # (whatever v holds on a pinned row)
    out = host(sh.sqrt(dev(Vn)))
    assert np.all(out[:, ~free] == 0.0) and not np.signbit(out[:, ~free]).any()  # exactly +0
    err = np.linalg.norm(out - ref.L(V.astype(np.float64)))
    bound = tol * cond * ref.lnorm * np.linalg.norm(V[:, free])
    print("%s n %d col %d: |sqrt(V) - L V| = %.2e (bound %.2e)" % (tag, n, col, err, bound))
    assert err <= bound
    assert torch.equal(sh.sqrt(dev(V[0])), sh.sqrt(dev(V[:1]))[0])

    # ---- the draws
    mean_h = rng.standard_normal(n).astype(sol.real)
    mean = dev(mean_h)
    zt = dev(zr)
    rz = sh.sqrt(zt)
    want = host(mean) + SCALE * host(rz) if f64 else None
    dr, lp = sh.sample(K, SEED, first=FIRST, mean=mean, scale=SCALE, log_prob=True)
    assert torch.equal(dr, sh.sample(K, SEED, first=FIRST, mean=mean, scale=SCALE))  # the same draws without log_prob
    assert torch.equal(dr, sh.sample(K, SEED, first=FIRST, mean=mean, scale=SCALE))  # and twice
    drh = host(dr)
    assert np.array_equal(dr.cpu().numpy()[:, ~free], np.broadcast_to(mean_h[~free], (K, n - nf)))  # the mean's bits
    none = sh.sample(2, SEED)
    assert np.all(host(none)[:, ~free] == 0.0) and not np.signbit(host(none)[:, ~free]).any()
    # the pin pattern's own L on the SAME z_ref: z does not move with the pins (REAL32: and the rounding of the store)
    wantl = mean_h[None, :] + SCALE * ref.L(zr)
    err = np.linalg.norm(drh - wantl)
    bound = tol * cond * ref.lnorm * SCALE * np.linalg.norm(zr[:, free]) + (0.0 if f64 else 2.0 ** -24 *
                                                                           np.linalg.norm(wantl))
    print("%s n %d col %d: |draw - (mean + scale L z_ref)| = %.2e (bound %.2e)" % (tag, n, col, err, bound))
    assert err <= bound
    if f64:
        rn = max((torch.linalg.norm(rz[j]) / torch.linalg.norm(zt[j])).item() for j in range(K))
        err, bound = np.linalg.norm(drh - want), 1e-10 * rn * np.linalg.norm(zr)
        print("%s n %d col %d: |draw - (mean + scale sqrt(z_ref))| = %.2e (bound %.2e)" % (tag, n, col, err, bound))
        assert err <= bound
        for j in range(K):  # one sample alone or inside a block
            d1 = sh.sample(1, SEED, first=FIRST + j, mean=mean, scale=SCALE)[0]
            assert (torch.linalg.norm(d1 - dr[j]) / torch.linalg.norm(dr[j])).item() <= 1e-13, j
        off = _odd(torch, dr)
        off.zero_()
        sh.sample(K, SEED, first=FIRST, mean=_odd(torch, mean), scale=SCALE, out=off)
        assert torch.equal(off, dr)

    # ---- densities
    lq = sh.log_prob(dr, mean=mean, scale=SCALE)
    lref = ref.logpdf(drh, mean_h.astype(np.float64), SCALE) if nf else np.zeros(K)
    for j in range(K):
        b = tol * cond * (1.0 + abs(lref[j]))
        print("%s n %d col %d sample %d: log density %.12e (z), %.12e (quad), %.12e (numpy), bound %.2e"
              % (tag, n, col, FIRST + j, lp[j], lq[j], lref[j], b))
        assert abs(lp[j] - lq[j]) <= b and abs(lp[j] - lref[j]) <= b and abs(lq[j] - lref[j]) <= b
    if nf == 0:
        assert np.all(lp == 0.0) and np.all(lq == 0.0) and sh.log_prob(mean) == 0.0
    c_h = rng.standard_normal(n).astype(sol.real)
    qd, qref = sh.quad(dev(V), center=dev(c_h)), ref.quad(V.astype(np.float64), c_h.astype(np.float64))
    q0, q0ref = sh.quad(dev(Vn[0])), ref.quad(V[:1].astype(np.float64), None)[0]  # (NaN on the pinned rows: not read)
    for got, r in list(zip(qd, qref)) + [(q0, q0ref)]:
        assert abs(got - r) <= tol * cond * (1.0 + abs(r)), (tag, got, r)
    ld_root = 2.0 * (sh.log_prob(mean, mean=mean) + 0.5 * nf * np.log(2.0 * np.pi))
    print("%s n %d col %d: log det %.15e, by the root %.15e, slogdet %.15e" % (tag, n, col, ld_before, ld_root,
                                                                                ref.logdet))
    assert abs(ld_root - ld_before) <= 1e-10 * n
    # the earlier entries give the same bits after the new ones
    assert torch.equal(sh.solve(dev(V)), x_before) and sh.logdet() == ld_before


def _check_state(env, sol, tol, which="abcd"):
    n = sol.n
    wa, _ = sol.export_state()
    B, col = _model(sol, wa)
    a, c, d = _shifts(sol, np.random.default_rng(5 * n + col))
    zr = np.array([z_ref(SEED, 0, n, FIRST + j) for j in range(K)])
    for key, (dv, mu) in dict(a=(a, MU), c=(c, MU), d=(d, MU), b=(None, 0.0)).items():
        if key in which:
            _check_shift(env, sol, wa, B, col, dv, mu, tol, "(%s)" % key, zr)
    return col


SHAPES = [(7, 3), (64, 10), (1000, 17), (4099, 10)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_shifted_draws_fp64(env, n, m):
    """col = 0 (FG_START) and a full ring whose head has wrapped"""
    la = env["la"]
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)  # (no early stop: the ring fills and wraps)
    sol = la.DeviceSolver(n, m)
    seen = set()
    try:
        def at(s, t):
            col = int(s.isave[27])
            tag = "empty" if col == 0 and t.startswith("FG_START") else (
                "wrapped" if t.startswith("NEW_X") and _wrapped(s) else None)
            if tag is None or tag in seen:
                return
            seen.add(tag)
            _check_state(env, s, 1e-10)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert seen == {"empty", "wrapped"}, seen


def _entries(sol, torch, d, k=3):
    """every new entry once, as numpy arrays"""
    n = sol.n
    g = torch.Generator(device="cpu").manual_seed(5)
    V = torch.randn(k, n, generator=g, dtype=torch.float64).cuda()
    sh = sol.qn_shift(d, MU)
    dr, lp = sh.sample(k, 11, first=1, mean=V[0], scale=2.0, log_prob=True)
    return [sh.sqrt(V).cpu().numpy(), dr.cpu().numpy(), lp, sh.sample(2, 11).cpu().numpy(),
            sh.quad(V, center=V[1]), sh.log_prob(V, mean=V[1], scale=0.7)]


def test_layout_read_as_it_is(env):
    """n = 4099 with the tile-local layout of W in force (policy 1) against a plain context with the same state"""
    la, torch = env["la"], env["torch"]
    n, m = 4099, 5
    p = _problem(env, "rosenbrock", n, m)
    g = torch.Generator(device="cpu").manual_seed(13)
    d = (10.0 * torch.rand(n, generator=g, dtype=torch.float64)).cuda()
    d[::3] = float("inf")
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": 1, "compact_min_rows": 0})
    got = {}
    try:
        def at(s, t):
            if got or not t.startswith("NEW_X") or int(s.isave[27]) < m or not s.compact_stats()[2]:
                return
            before = s.compact_stats()
            got["res"] = _entries(s, torch, d)
            got["again"] = _entries(s, torch, d)
            assert s.compact_stats() == before  # (still packed: the passes read the layout as it is)
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
        res = _entries(plain, torch, d)
    finally:
        plain.close()
    for a, b in zip(got["res"], res):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


def test_shifted_draws_real32(env):
    """(a) and (c) at (1000, 10) in a REAL32 context: d, v, mean, out fp32; the weights, z and every sum fp64"""
    la = env["la"]
    n, m = 1000, 10
    p = _problem(env, "quadratic", n, m, np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    checked = []
    try:
        def at(s, t):
            if t.startswith("NEW_X") and int(s.isave[29]) in (2, m + 2):
                checked.append(_check_state(env, s, 1e-5, which="ac"))
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
    res = (C.c_double * 1)()
    nan, inf = float("nan"), float("inf")

    def calls(s, k=1, first=0, scale=1.0, vp=v.data_ptr(), op=out.data_ptr(), rp=res, ld=n):
        return [lib.lbfgsb_hip_qn_shift_sqrt(s.h, k, vp, ld, op, ld),
                lib.lbfgsb_hip_qn_shift_draw(s.h, k, 7, first, None, scale, op, ld),
                lib.lbfgsb_hip_qn_shift_draw_logpdf(s.h, k, 7, first, None, scale, op, ld, rp),
                lib.lbfgsb_hip_qn_shift_quad(s.h, k, vp, ld, None, rp),
                lib.lbfgsb_hip_qn_shift_logpdf(s.h, k, vp, ld, None, scale, rp)]

    sol = la.DeviceSolver(n, m)
    state = {}
    try:
        assert calls(sol) == [E_STATE] * 5  # no run

        def at(s, t):
            if not t.startswith("NEW_X"):
                return
            it = int(s.isave[29])
            if it == 3:
                assert calls(s) == [E_STATE] * 5  # before any set
                assert lib.lbfgsb_hip_qn_shift_set(s.h, d.data_ptr(), 0.5, None) == 0
                assert calls(s) == [0] * 5
                assert lib.lbfgsb_hip_qn_shift_draw(s.h, 1, 7, 0, None, 1.0, out.data_ptr(), n) == 0
                state["x"], state["iupdat"] = out.clone(), int(s.isave[30])
                # LBFGSB_E_ARG, nothing changed
                assert calls(s, k=0) == [E_ARG] * 5
                assert calls(s, ld=n - 1) == [E_ARG] * 5
                r = calls(s, vp=None)
                assert (r[0], r[3], r[4]) == (E_ARG,) * 3
                r = calls(s, op=None)
                assert (r[0], r[1], r[2]) == (E_ARG,) * 3
                r = calls(s, rp=None)
                assert (r[2], r[3], r[4]) == (E_ARG,) * 3
                r = calls(s, first=-1)
                assert (r[1], r[2]) == (E_ARG,) * 2
                for bad in (0.0, nan, inf, -inf):
                    r = calls(s, scale=bad)
                    assert (r[1], r[2], r[4]) == (E_ARG,) * 3, bad
                assert lib.lbfgsb_hip_qn_shift_sqrt(None, 1, v.data_ptr(), n, out.data_ptr(), n) == E_ARG
                # the shift is still in force, and a refused set leaves it there too
                assert lib.lbfgsb_hip_qn_shift_set(s.h, None, -2.0 * float(s.dsave[0]), None) == E_ARG
                assert lib.lbfgsb_hip_qn_shift_draw(s.h, 1, 7, 0, None, 1.0, out.data_ptr(), n) == 0
                assert torch.equal(out, state["x"])
            elif it == 4:
                assert int(s.isave[30]) > state["iupdat"]  # one more pair is stored
                assert calls(s) == [E_STATE] * 5
                sh = s.qn_shift(d, 0.5)
                with pytest.raises(la.LbfgsbError, match="-101"):
                    sh.sample(1, 7, scale=0.0)
                assert sh.sample(1, 7).shape == (1, n)
                state["sh"] = sh
        _drive(env, sol, p, max_iter=5, at_return=at)
        assert "sh" in state
        for call in (lambda: state["sh"].sqrt(v), lambda: state["sh"].sample(1, 7), lambda: state["sh"].quad(v),
                     lambda: state["sh"].log_prob(v)):
            with pytest.raises(la.LbfgsbError, match="qn_shift_set again"):
                call()
    finally:
        sol.close()
    # more than 64 pairs: E_ARG from qn_shift_set and from every entry that takes the root; quad has no shift to use
    nn, mm = 1000, 80
    sol = la.DeviceSolver(nn, mm)
    try:
        _, t = _drive(env, sol, _slow_quadratic(env, nn, mm), max_iter=400, until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65, t
        vv = torch.ones(nn, dtype=torch.float64, device="cuda")
        oo = torch.empty_like(vv)
        assert lib.lbfgsb_hip_qn_shift_set(sol.h, None, 0.0, None) == E_ARG
        assert lib.lbfgsb_hip_qn_shift_sqrt(sol.h, 1, vv.data_ptr(), nn, oo.data_ptr(), nn) == E_ARG
        assert lib.lbfgsb_hip_qn_shift_draw(sol.h, 1, 7, 0, None, 1.0, oo.data_ptr(), nn) == E_ARG
        assert lib.lbfgsb_hip_qn_shift_draw_logpdf(sol.h, 1, 7, 0, None, 1.0, oo.data_ptr(), nn, res) == E_ARG
        assert lib.lbfgsb_hip_qn_shift_logpdf(sol.h, 1, vv.data_ptr(), nn, None, 1.0, res) == E_ARG
        assert lib.lbfgsb_hip_qn_shift_quad(sol.h, 1, vv.data_ptr(), nn, None, res) == E_STATE
    finally:
        sol.close()


@pytest.mark.parametrize("name,ctor", [("classic", {}),
                                       ("pingpong_defer", dict(defer_lnsrch=True, same_stream_objective=True))])
def test_run_does_not_notice(env, name, ctor):
    la, torch = env["la"], env["torch"]
    n, m, iters = 4099, 7, 30
    p = _problem(env, "rosenbrock", n, m)
    g = torch.Generator(device="cpu").manual_seed(9)
    d = (10.0 * torch.rand(n, generator=g, dtype=torch.float64)).cuda()
    d[::3] = float("inf")
    outs = []
    counts = {"ok": 0, "refused": 0}
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **ctor)
        try:
            def at(s, t):
                try:
                    _entries(s, torch, d, k=2)
                    counts["ok"] += 1
                except la.LbfgsbError as e:
                    assert "-104" in str(e), e  # E_STATE: a deferred set-up or a parked f
                    counts["refused"] += 1
            rows, _ = _drive(env, sol, p, iters, at_return=at if touch else None, pp=name != "classic")
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes(), sol.compact_stats()))
        finally:
            sol.close()
    assert counts["ok"] >= iters
    assert outs[0] == outs[1]
    if name != "classic":
        assert counts["refused"] > 0
