"""Square roots, log-determinants and draws of the curvature model (lbfgsb_hip_qn_apply's root modes,
lbfgsb_hip_qn_logdet, lbfgsb_hip_qn_draw; DeviceSolver.qn_apply(sqrt=True) / qn_logdet / qn_draw): the root applied
twice against the dense numpy model built from export_state, log det against slogdet, the generator against a numpy
implementation of Philox4x32-10 + Box-Muller and its moments, draws against mean + scale A^(1/2) z of the reference
z, the tile-local layout of W read as it is, runs that call the entries at every return bit-identical to runs that
do not, and the refusals."""
import ctypes as C
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


# ---------------------------------------------------------------- the generator, in numpy
def _philox(c, k):
    """Philox4x32-10 on arrays: c = four uint64 arrays holding 32-bit words, k = two; returns the four output words"""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    lo, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + W0) & lo, (k1 + W1) & lo
    return c0, c1, c2, c3


def z_ref(seed, row0, n, sample):
    """the N(0, 1) deviates of (seed, rows row0 .. row0 + n - 1, sample) as include/lbfgsb_hip.h defines them"""
    lo, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    pair = np.uint64(sample >> 1)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    w = _philox((rows & lo, rows >> sh, full(pair & lo), full(pair >> sh)),
                (full(np.uint64(seed) & lo), full(np.uint64(seed) >> sh)))
    a, b = (w[0] << sh) | w[1], (w[2] << sh) | w[3]
    u = ((a >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    v = (b >> np.uint64(12)).astype(np.float64) * 2.0 ** -52
    r = np.sqrt(-2.0 * np.log(u))
    return r * (np.sin(2.0 * np.pi * v) if sample & 1 else np.cos(2.0 * np.pi * v))


def test_reference_generator_known_answers():
    """the numpy reference itself, on the known answers of Philox4x32-10 (needs no GPU work)"""
    one = lambda *v: tuple(np.array([x], dtype=np.uint64) for x in v)
    hexes = lambda w: tuple(int(x[0]) for x in w)
    assert hexes(_philox(one(0, 0, 0, 0), one(0, 0))) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    f = 0xffffffff
    assert hexes(_philox(one(f, f, f, f), one(f, f))) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert hexes(_philox(one(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), one(0xa4093822, 0x299f31d0))) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


N_GEN = 1_000_000
SEEDS = (1, 2 ** 40 + 12345)
SAMPLES = (0, 1, 2, 7)


@pytest.fixture(scope="module")
def zrefs():
    return {(seed, s): z_ref(seed, 0, N_GEN, s) for seed in SEEDS for s in SAMPLES}


# ---------------------------------------------------------------- helpers (as tests/test_gpu_qn.py)
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
    W = []
    for j in range(col):
        c = (head - 1 + j) % m
        s, y = Ws[:, c], Wy[:, c]
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
        W += [s, y]
    return B, col, theta, (np.array(W).T if W else np.zeros((n, 0)))


def _cond_and_norm(B, theta, W):
    """cond(B) and |B|_2 of the dense model: B maps span(W) into itself and is theta I on its complement, so its
    spectrum is theta and the eigenvalues of Q'BQ, Q an orthonormal basis of span(W)"""
    n = B.shape[0]
    if n <= 1000:
        return np.linalg.cond(B), np.linalg.norm(B, 2)
    ev = [theta]
    if W.shape[1]:
        Q, _ = np.linalg.qr(W)
        ev += list(np.linalg.eigvalsh(Q.T @ B @ Q))
    return max(ev) / min(ev), max(ev)


def _check_root(env, sol, ks=(1, 3, 9)):
    torch = env["torch"]
    n = sol.n
    B, col, theta, W = _model(sol)
    cond, nb = _cond_and_norm(B, theta, W)
    rng = np.random.default_rng(n + 31 * col)
    Vs = [rng.standard_normal((k, n)) for k in ks]
    href = np.linalg.solve(B, np.concatenate(Vs).T).T  # H V for every vector, one factorisation
    at = 0
    for k, V in zip(ks, Vs):
        vt = torch.from_numpy(V).cuda()
        rv = sol.qn_apply(vt, sqrt=True)
        bv = sol.qn_apply(rv, sqrt=True).cpu().numpy()
        err = np.linalg.norm(bv - V @ B.T)
        bound = 1e-10 * nb * np.linalg.norm(V)
        print("n %d col %d k %d: |B^1/2 B^1/2 V - B V| = %.3e, bound %.3e" % (n, col, k, err, bound))
        assert err <= bound, (k, col)
        hv = sol.qn_apply(sol.qn_apply(vt, sqrt=True, inverse=True), sqrt=True, inverse=True).cpu().numpy()
        ref = href[at:at + k]
        at += k
        err = np.linalg.norm(hv - ref)
        bound = 1e-10 * cond * np.linalg.norm(ref)
        print("n %d col %d k %d: |H^1/2 H^1/2 V - H V| = %.3e, bound %.3e" % (n, col, k, err, bound))
        assert err <= bound, (k, col, cond)
    # symmetry: u'(A^1/2 v) = v'(A^1/2 u)
    u, v = torch.from_numpy(Vs[-1][0].copy()).cuda(), torch.from_numpy(Vs[-1][-1].copy()).cuda()
    for inverse in (False, True):
        ru, rv = sol.qn_apply(u, sqrt=True, inverse=inverse), sol.qn_apply(v, sqrt=True, inverse=inverse)
        assert abs((u @ rv - v @ ru).item()) <= 1e-12 * (torch.linalg.norm(u) * torch.linalg.norm(rv)).item()
    ld_b, ld_h = sol.qn_logdet(), sol.qn_logdet(inverse=True)
    if col == 0:
        assert ld_b == n * np.log(theta) and ld_h == n * np.log(1.0 / theta)
    if n <= 1000:
        sign, ref = np.linalg.slogdet(B)
        print("n %d col %d: log det B = %.15e (slogdet %.15e), log det H = %.15e" % (n, col, ld_b, ref, ld_h))
        assert sign == 1.0 and abs(ld_b - ref) <= 1e-10 * n and abs(ld_h + ref) <= 1e-10 * n
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


def _slow_quadratic(env, n, m):
    """an unbounded quadratic with n distinct curvatures from 1 to 1e4: hundreds of iterations, a pair from each"""
    d, c = np.logspace(0.0, 4.0, n), np.cos(np.arange(n))

    def fg(x, g):
        g[:] = d * (x - c)
        return float(0.5 * np.sum(d * (x - c) ** 2))
    return env["po"].Problem("slow_quadratic", n, m, np.zeros(n), np.full(n, -1.0), np.full(n, 1.0),
                             np.zeros(n, np.int32), 0.0, 0.0, fg)


def _wrapped(s):
    m, col, head = s.m, int(s.isave[27]), int(s.isave[26])
    return col == m and int(s.isave[30]) > m and (head > 1 or m == 1)


def _first_return(env, sol):
    """one setulb call on a trivial problem: the FG_START return (no pair, theta = 1)"""
    torch = env["torch"]
    dt = torch.float32 if sol.real == np.float32 else torch.float64
    x = torch.zeros(sol.n, dtype=dt, device="cuda")
    g = torch.zeros_like(x)
    l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
    nbd = torch.zeros(sol.n, dtype=torch.int32, device="cuda")
    t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
    assert t.startswith("FG_START") and int(sol.isave[27]) == 0 and float(sol.dsave[0]) == 1.0, t


# ---------------------------------------------------------------- the square root and the log-determinant
SHAPES = [(7, 1), (64, 5), (64, 10), (1000, 17), (1000, 40), (4099, 10)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_square_root_and_logdet_fp64(env, n, m):
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
            tag = "empty" if col == 0 else ("wrapped" if _wrapped(s) else ("full" if col == m else "part"))
            if tag in seen or tag == "full" or (tag == "part" and col < max(1, m // 2)):
                return
            seen.add(tag)
            _check_root(env, s)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert "empty" in seen and "wrapped" in seen, seen
    assert "part" in seen or m == 1, seen


def test_root_refusals_and_arguments(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    v = torch.ones(n, dtype=torch.float64, device="cuda")
    out = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    val = C.c_double(0.0)
    draw = lambda s, mode=1, k=1, first=0, mean=None, scale=1.0, o=out.data_ptr(), ldo=n: \
        lib.lbfgsb_hip_qn_draw(s.h, mode, k, 7, first, mean, scale, o, ldo)
    sol = la.DeviceSolver(n, m)
    try:
        assert lib.lbfgsb_hip_qn_apply(sol.h, 4, 1, v.data_ptr(), n, out.data_ptr(), n) == E_STATE  # no run
        assert lib.lbfgsb_hip_qn_logdet(sol.h, 0, C.byref(val)) == E_STATE
        assert draw(sol) == E_STATE
        _drive(env, sol, p, max_iter=8)
        for mode in (la.QN_B_SQRT, la.QN_H_SQRT):
            assert lib.lbfgsb_hip_qn_diag(sol.h, mode, out.data_ptr()) == E_ARG
            assert lib.lbfgsb_hip_qn_apply(sol.h, mode, 1, v.data_ptr(), n, out.data_ptr(), n) == 0
            assert lib.lbfgsb_hip_qn_logdet(sol.h, mode, C.byref(val)) == E_ARG
            assert draw(sol, mode=mode) == E_ARG
        for mode in (2, 3, 6, -1):  # (no mode: 2 and 3 stay refused as before the roots existed)
            assert lib.lbfgsb_hip_qn_apply(sol.h, mode, 1, v.data_ptr(), n, out.data_ptr(), n) == E_ARG
        assert lib.lbfgsb_hip_qn_logdet(sol.h, 0, None) == E_ARG
        assert draw(sol, k=0) == E_ARG and draw(sol, first=-1) == E_ARG and draw(sol, ldo=n - 1) == E_ARG
        assert draw(sol, o=None) == E_ARG
        assert draw(sol, scale=float("inf")) == E_ARG and draw(sol, scale=float("nan")) == E_ARG
        assert draw(sol, k=2) == 0 and draw(sol, mode=0, mean=v.data_ptr(), scale=0.0) == 0
        assert torch.equal(out[:n], v)  # scale = 0: the mean
        assert lib.lbfgsb_hip_qn_logdet(sol.h, 1, C.byref(val)) == 0 and np.isfinite(val.value)
    finally:
        sol.close()
    # 65 stored pairs: beyond LBFGSB_QN_ROOT_MAXCOL
    sol = la.DeviceSolver(1000, 70)
    try:
        _, t = _drive(env, sol, _slow_quadratic(env, 1000, 70), max_iter=400, until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65, t
        w = torch.ones(1000, dtype=torch.float64, device="cuda")
        o = torch.empty_like(w)
        for mode in (la.QN_B_SQRT, la.QN_H_SQRT):
            assert lib.lbfgsb_hip_qn_apply(sol.h, mode, 1, w.data_ptr(), 1000, o.data_ptr(), 1000) == E_ARG
        assert lib.lbfgsb_hip_qn_logdet(sol.h, 0, C.byref(val)) == E_ARG
        assert lib.lbfgsb_hip_qn_draw(sol.h, 1, 1, 7, 0, None, 1.0, o.data_ptr(), 1000) == E_ARG
        sol.qn_apply(w, inverse=True)  # (the model itself: any number of pairs)
    finally:
        sol.close()


# ---------------------------------------------------------------- draws: the generator
def _moments(z):
    return np.array([z.mean(), (z * z).mean(), (z ** 3).mean(), (z ** 4).mean()])


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_against_reference_and_moments(env, zrefs, seed):
    """no pair, theta = 1, B, scale 1, no mean: out = z.  |out - z_ref| <= 1e-13 (1 + |z_ref|): log to 3 ulp and
    sinpi / cospi to 4 ulp on the device, numpy's own rounding of 2 pi v, at r <= 8.6 give <= 2e-14.  The first four
    moments, the cross-correlations of samples (0, 1) and (0, 2) and the lag-1 row correlation within 4 sigma (the
    reference alone lies within 2 sigma on these inputs)."""
    la = env["la"]
    n = N_GEN
    sol = la.DeviceSolver(n, 5)
    z = {}
    try:
        _first_return(env, sol)
        for s in SAMPLES:
            z[s] = sol.qn_draw(1, seed, first=s, inverse=False)[0].cpu().numpy()
    finally:
        sol.close()
    sig = np.array([1.0, np.sqrt(2.0), np.sqrt(15.0), np.sqrt(96.0)]) / np.sqrt(n)  # of z, z^2, z^3, z^4 means
    want = np.array([0.0, 1.0, 0.0, 3.0])
    for s in SAMPLES:
        ref = zrefs[(seed, s)]
        err = (np.abs(z[s] - ref) / (1.0 + np.abs(ref))).max()
        print("seed %d sample %d: max |out - z_ref| / (1 + |z_ref|) = %.3e, max |z| = %.3f"
              % (seed, s, err, np.abs(z[s]).max()))
        assert err <= 1e-13
        assert np.abs(z[s]).max() <= 8.6
        dev = (_moments(z[s]) - want) / sig
        print("   moments in sigma: %s (reference %s)" % (dev, (_moments(ref) - want) / sig))
        assert np.all(np.abs(dev) <= 4.0), dev
        assert np.all(np.abs((_moments(ref) - want) / sig) <= 2.0)
        lag = (z[s][1:] * z[s][:-1]).mean() * np.sqrt(n - 1)
        assert abs(lag) <= 4.0 and abs((ref[1:] * ref[:-1]).mean() * np.sqrt(n - 1)) <= 2.0, lag
    for a, b in ((0, 1), (0, 2)):
        cc = (z[a] * z[b]).mean() * np.sqrt(n)
        assert abs(cc) <= 4.0 and abs((zrefs[(seed, a)] * zrefs[(seed, b)]).mean() * np.sqrt(n)) <= 2.0, cc


def test_generator_real32(env, zrefs):
    """a REAL32 context: the fp64 deviates rounded on store -- the fp64 reference rounded to fp32, up to 1 ulp"""
    la = env["la"]
    seed = SEEDS[0]
    sol = la.DeviceSolver(N_GEN, 5, real32=True)
    try:
        _first_return(env, sol)
        for s in (0, 1, 7):
            z = sol.qn_draw(1, seed, first=s, inverse=False)[0].cpu().numpy()
            assert z.dtype == np.float32
            ref = zrefs[(seed, s)].astype(np.float32)
            assert np.all(np.abs(z - ref) <= np.spacing(np.abs(ref)))
    finally:
        sol.close()


# ---------------------------------------------------------------- draws: the operator
@pytest.mark.parametrize("m", [10, 17])
def test_draws_against_root_of_reference_z(env, m):
    la, torch = env["la"], env["torch"]
    n, seed, k, first = 4099, 20260101, 5, 3
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)
    sol = la.DeviceSolver(n, m)
    try:
        _drive(env, sol, p, max_iter=4 * m + 40, until=_wrapped)
        assert _wrapped(sol)
        zr = np.array([z_ref(seed, 0, n, first + j) for j in range(k)])
        zt = torch.from_numpy(zr).cuda()
        mean = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
        for inverse in (False, True):
            rz = sol.qn_apply(zt, sqrt=True, inverse=inverse)
            ref = (mean + 0.5 * rz).cpu().numpy()
            d = sol.qn_draw(k, seed, first=first, mean=mean, scale=0.5, inverse=inverse)
            # |A^1/2| >= |A^1/2 z| / |z| for every z: the bound below is at most 1e-10 |A^1/2| |z|
            rn = max((torch.linalg.norm(rz[j]) / torch.linalg.norm(zt[j])).item() for j in range(k))
            err = np.linalg.norm(d.cpu().numpy() - ref)
            bound = 1e-10 * rn * np.linalg.norm(zr)
            print("m %d inverse %s: |draw - ref| = %.3e, bound %.3e" % (m, inverse, err, bound))
            assert err <= bound
            for j in range(k):  # one sample alone or inside a block (another row-to-lane map of the sums)
                d1 = sol.qn_draw(1, seed, first=first + j, mean=mean, scale=0.5, inverse=inverse)[0]
                assert (torch.linalg.norm(d1 - d[j]) / torch.linalg.norm(d[j])).item() <= 1e-13, j
            assert torch.equal(d, sol.qn_draw(k, seed, first=first, mean=mean, scale=0.5, inverse=inverse))
            # an out that is not 16-byte aligned: one row per lane, the same values
            buf = torch.empty(k * n + 1, dtype=torch.float64, device="cuda")
            off = buf[1:].view(k, n)
            assert off.data_ptr() % 16 == 8
            sol.qn_draw(k, seed, first=first, mean=mean, scale=0.5, inverse=inverse, out=off)
            assert torch.equal(off, d)
            mbuf = torch.empty(n + 1, dtype=torch.float64, device="cuda")
            mbuf[1:].copy_(mean)
            assert torch.equal(sol.qn_draw(k, seed, first=first, mean=mbuf[1:], scale=0.5, inverse=inverse), d)
        op = sol.qn_operator()
        assert torch.equal(op.sample(2, seed), sol.qn_draw(2, seed))
        assert torch.equal(op.sqrt() @ mean, sol.qn_apply(mean, sqrt=True, inverse=True))
        assert op.logdet() == sol.qn_logdet(inverse=True) and op.sqrt().logdet() == 0.5 * op.logdet()
        V = torch.randn(n, 3, dtype=torch.float64, device="cuda")
        assert torch.allclose(op.sqrt().matmat(V)[:, 1], op.sqrt().matvec(V[:, 1].contiguous()), rtol=0, atol=1e-12)
    finally:
        sol.close()


# ---------------------------------------------------------------- the layout, and the run that does not notice
def _new_entries(sol, torch, n, k=3):
    g = torch.Generator(device="cpu").manual_seed(5)
    V = torch.randn(k, n, generator=g, dtype=torch.float64).cuda()
    out = [sol.qn_apply(V, sqrt=True), sol.qn_apply(V, sqrt=True, inverse=True), sol.qn_apply(V[0], sqrt=True),
           sol.qn_draw(k, 11, first=1, mean=V[0], scale=2.0), sol.qn_draw(2, 11, inverse=False)]
    res = [o.cpu().numpy() for o in out]
    res.append(np.array([sol.qn_logdet(), sol.qn_logdet(inverse=True)]))
    return res


@pytest.mark.parametrize("n,policy,kind", [(4099, 1, "rosenbrock"), (4099, 2, "rosenbrock"),
                                           (1_000_000, 1, "quadratic")])
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
            got["res"] = _new_entries(s, torch, n)
            got["again"] = _new_entries(s, torch, n)
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
        res = _new_entries(plain, torch, n)
    finally:
        plain.close()
    for a, b in zip(got["res"], res):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


RUNS = {
    "classic": dict(pp=False),
    "pingpong": dict(pp=True),
    "defer": dict(pp=False, ctor=dict(defer_lnsrch=True, same_stream_objective=True)),
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
                    _new_entries(s, torch, n, k=2)
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
    if name in ("defer", "builtin_deferred_f"):
        assert counts["refused"] > 0
