"""The states on which the parallel Cauchy-point search is compared with tests/_gcp_truth.py, one call each:
TEST HELPER shared by tests/test_gcp_truth_cpu.py (is every case what its name says, and well posed?) and
tests/test_gpu_pgcp_door.py (the door of the library on it).  Fixed seeds; nothing here calls the library.

A state is synthetic: S random, Y = A S with a positive diagonal A (so s'y > 0 and the model is positive definite),
Sy = S'Y and Ss = S'S from them, Wt by the oracle's formt, theta = y'y / s'y of the newest pair.  How long the walk
is follows from where the breakpoints are put: the model is close to theta I (few pairs, many rows), so the walk stops
near t* = 1 / theta whatever the gradient's size, and a breakpoint with t < t* is crossed -- breakpoints spread over
(0, 2 t*) make it stop in the middle, breakpoints below t* / 2 are all crossed.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from _gcp_truth import truth

EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}


@dataclass
class Case:
    name: str
    n: int
    m: int
    col: int
    head: int
    real: type
    x: np.ndarray
    l: np.ndarray
    u: np.ndarray
    nbd: np.ndarray
    g: np.ndarray
    iwhere: np.ndarray
    ws: np.ndarray
    wy: np.ndarray
    sy: np.ndarray
    ss: np.ndarray
    wt: np.ndarray
    theta: float
    path: str = "search"      # "search": sort + scans; "closed": the col = 0 closed form; "fallback": its guard -> the walk
    expect: dict = field(default_factory=dict)
    backend: str = None       # of the truth; "mpmath" where numbers 2^-66 apart meet in one sum (longdouble has 64 bits)

    @property
    def epsmch(self):
        return EPS[self.real]

    def truth(self, backend=None):
        return truth(self.x, self.l, self.u, self.nbd, self.g, self.iwhere, self.ws, self.wy, self.head, self.col,
                     self.sy, self.wt, self.theta, self.epsmch, backend=backend or self.backend)


def _formt(m, sy, ss, col, theta):
    from oracle import pyoracle as po
    wt, info = np.zeros(m * m), np.zeros(1, np.int32)
    if col:
        po.Routines().formt(m, wt, sy, ss, col, float(theta), info)
        assert info[0] == 0
    return wt


def _pairs(rng, n, m, col, head, real):
    """ws, wy (m x n, ring slot (head - 1 + j) % m = pair j, oldest first), sy, ss, wt (m*m, column-major), theta"""
    ws, wy = np.zeros((m, n), real), np.zeros((m, n), real)
    sy, ss = np.zeros((m, m)), np.zeros((m, m))
    theta = 1.0
    if col:
        a = 0.5 + 1.5 * rng.random(n)
        S = rng.normal(0, 1, (col, n)).astype(real)
        Y = (a * S).astype(real)
        for j in range(col):
            ws[(head - 1 + j) % m], wy[(head - 1 + j) % m] = S[j], Y[j]
        # (longdouble products: numpy's own loops, the same bits on every machine -- a BLAS picks its kernel by CPU)
        SX, YX = S.astype(np.longdouble), Y.astype(np.longdouble)
        sy[:col, :col], ss[:col, :col] = (SX @ YX.T).astype(np.float64), (SX @ SX.T).astype(np.float64)
        theta = float(real((YX[-1] @ YX[-1]) / (SX[-1] @ YX[-1])))
    sy, ss = sy.astype(real).flatten(order="F"), ss.astype(real).flatten(order="F")
    wt = _formt(m, sy.astype(np.float64), ss.astype(np.float64), col, theta).astype(real)
    return ws, wy, sy, ss, wt, theta


def _active_iwhere(l, u, nbd):
    """iwhere as active leaves it (:1024-1037)"""
    iw = np.zeros(nbd.size, np.int32)
    iw[nbd == 0] = -1
    iw[(nbd == 2) & (u - l <= 0)] = 3
    return iw


def _box(rng, real, g, t_want, is_bp):
    """bounds and x for a gradient g: rows with is_bp reach a bound after about t_want (in the direction -g), of
    every kind of nbd that has that bound; the others never reach one, of every kind that allows it"""
    n = g.size
    x = rng.normal(0, 1, n)
    l, u = x - 1.0 - rng.random(n), x + 1.0 + rng.random(n)
    nbd = np.zeros(n, np.int32)
    down = g > 0                                  # moves towards l
    pick = rng.random(n) < 0.5
    dist = np.where(is_bp, t_want * np.abs(g), 0.0)
    l = np.where(is_bp & down, x - dist, l)
    u = np.where(is_bp & ~down, x + dist, u)
    nbd[is_bp & down] = np.where(pick, 1, 2)[is_bp & down]
    nbd[is_bp & ~down] = np.where(pick, 3, 2)[is_bp & ~down]
    nbd[~is_bp & down] = np.where(pick, 3, 0)[~is_bp & down]
    nbd[~is_bp & ~down] = np.where(pick, 1, 0)[~is_bp & ~down]
    return x.astype(real), l.astype(real), u.astype(real), nbd


def _make(name, seed, n, nb, m, col, head=1, real=np.float64, t_hi=2.0, path="search", expect=None, edit=None):
    """nb breakpoints at times uniform in (0, t_hi / theta), the other n - nb rows moving freely"""
    rng = np.random.default_rng(seed)
    ws, wy, sy, ss, wt, theta = _pairs(rng, n, m, col, head, real)
    g = (0.5 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    is_bp = np.zeros(n, bool)
    is_bp[rng.permutation(n)[:nb]] = True
    t_want = t_hi / theta * (0.02 + 0.98 * rng.random(n))
    x, l, u, nbd = _box(rng, real, g, t_want, is_bp)
    g = g.astype(real)
    expect = dict(expect or {})
    if edit:
        edit(rng, theta, x, l, u, nbd, g, is_bp)
    if nb < n and edit is not _zero_rest:
        expect["probe"] = _probe(np.flatnonzero(~is_bp)[-1], x, l, u, nbd, g, 1.0)
    return Case(name, n, m, col, head, real, x, l, u, nbd, g, _active_iwhere(l, u, nbd), ws, wy, sy, ss, wt, theta,
                path=path, expect=expect)


def _probe(i, x, l, u, nbd, g, scale):
    """row i becomes an unbounded row at x = 0 with g = scale (a power of two): its xcp is -tsum * scale without a
    rounding, so tsum itself can be read off the oracle's and the library's Cauchy point; -> (i, scale)"""
    x[i], l[i], u[i], nbd[i], g[i] = 0.0, -1.0, 1.0, 0, scale
    return int(i), float(scale)


# ---- edits of a generated state ----
def _tie_group(rng, theta, x, l, u, nbd, g, is_bp):
    """four breakpoints at exactly t = 1/8 (well before the stop), rows far apart, both directions, every operand
    a small dyadic number so that the division (:1305, :1314) returns the same t for all of them"""
    rows = np.flatnonzero(is_bp)[[3, 40, 41, 200]]
    for k, i in enumerate(rows):
        gi = (1.0, -2.0, 0.5, -1.0)[k]
        g[i], nbd[i] = gi, 2
        if gi > 0:
            l[i], x[i], u[i] = -1.0, -1.0 + 0.125 * gi, 3.0
        else:
            u[i], x[i], l[i] = 1.0, 1.0 - 0.125 * -gi, -3.0


def _all_kinds(rng, theta, x, l, u, nbd, g, is_bp):
    """rows with l == u, rows on a bound pushed outwards (both bounds, every nbd that has the bound), a row an ulp
    beyond its bound, rows with g = 0 (bounded ones become iwhere = -3, unbounded ones stay -1)"""
    free = np.flatnonzero(~is_bp)
    k = iter(free[:24])
    for _ in range(3):
        i = next(k)
        nbd[i], l[i], u[i] = 2, x[i], x[i]                              # l == u: iwhere = 3, never looked at
    for kind in (1, 2):
        i = next(k)
        nbd[i], l[i], u[i], g[i] = kind, x[i], x[i] + 1.0, 0.7         # on l, -g points below it: iwhere = 1
        i = next(k)
        nbd[i], l[i], u[i], g[i] = kind, x[i], x[i] + 1.0, -0.7        # on l, -g points inwards: moves (kind 2: breakpoint)
    for kind in (2, 3):
        i = next(k)
        nbd[i], u[i], l[i], g[i] = kind, x[i], x[i] - 1.0, -0.7        # on u pushed outwards: iwhere = 2
        i = next(k)
        nbd[i], u[i], l[i], g[i] = kind, x[i], x[i] - 1.0, 0.7
    i = next(k)
    nbd[i], l[i], u[i], g[i] = 2, np.nextafter(x[i], np.inf), x[i] + 1.0, 0.3   # an ulp below l: xcp keeps x (:1284)
    for kind in (0, 1, 2, 3, 0, 2):
        i = next(k)
        nbd[i], g[i] = kind, 0.0
        l[i], u[i] = x[i] - 1.0, x[i] + 1.0


def _zero_rest(rng, theta, x, l, u, nbd, g, is_bp):
    """the rows that are no breakpoints do not move: g = 0 (bounded: iwhere = -3; unbounded: iwhere stays -1)"""
    g[~is_bp] = 0.0


def _clamp_case(name, seed, real):
    """The clamp f2 = max(epsmch f2_org, f2) (:1483) acting BEFORE the stop: nbig rows carry the gradient and are fixed
    early; the other breakpoints have gradients `small` times theirs, so that their share of d'd is below epsmch and f2
    sits on the clamp while they are crossed.  What then drives f1 is the coupling of those rows with the displacement
    of the big ones through W M W' (linear in `small`), and the walk ends after about dtm = -f1 / (epsmch f2_org): a
    first walk with the small rows unbounded measures that dtm, then their breakpoints are spread over twice that.
    Every number is a float32 with few significant bits (g, t and the bound 0 such that x = t |g| and the quotient
    (x - l) / g are exact), so that the same state serves a REAL32 context and the breakpoint times do not depend on
    the precision they are computed in."""
    small = 2.0 ** -33 if real == np.float64 else 2.0 ** -17
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        n, nbig, m, col = 200, 12, 4, 3
        ws, wy, sy, ss, wt, theta = _pairs(rng, n, m, col, 1, np.float32)
        kg = rng.integers(32, 64, n) / 64.0 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        big = np.zeros(n, bool)
        big[rng.permutation(n)[:nbig]] = True
        g = np.where(big, kg, kg * small)
        t_big = rng.integers(64, 512, n) / 1024.0 / 2.0         # (0.03, 0.25): all crossed
        probe = int(np.flatnonzero(~big)[-1])
        case = None
        for stage in (0, 1):
            if stage == 0:
                t = np.where(big, t_big, 0.0)
                is_bp = big
            else:
                # multiples of a power of two (at most 12 bits of them) between 1/4, which is behind the last big
                # breakpoint, and 1/4 + 2 dtm
                span = 2.0 * dtm_pre
                q = 2.0 ** (np.floor(np.log2(span)) - 8)
                t = np.where(big, t_big, (np.ceil(0.25 / q) + np.ceil(rng.random(n) * span / q)) * q)
                is_bp = np.ones(n, bool)
            is_bp[probe] = False
            down = g > 0
            x = np.where(is_bp, np.where(down, t * np.abs(g), -t * np.abs(g)), rng.integers(-8, 8, n) / 4.0)
            l = np.where(is_bp & down, 0.0, -np.inf)
            u = np.where(is_bp & ~down, 0.0, np.inf)
            nbd = np.where(is_bp, np.where(down, 1, 3), 0).astype(np.int32)
            l, u = np.where(np.isinf(l), -8.0, l), np.where(np.isinf(u), 8.0, u)
            gq = g.copy()
            pr = _probe(probe, x, l, u, nbd, gq, small)
            arrs = [a.astype(np.float32) for a in (x, l, u)] + [nbd, gq.astype(np.float32)]
            assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(arrs, (x, l, u, nbd, gq)))
            if real == np.float64:
                arrs = [a.astype(np.float64) if a.dtype == np.float32 else a for a in arrs]
            W = [a.astype(real) for a in (ws, wy, sy, ss, wt)]
            case = Case(name, n, m, col, 1, real, *arrs, _active_iwhere(l, u, nbd), *W, theta,
                        expect=dict(clamp=True, mid=True, probe=pr), backend="mpmath")
            if stage == 0:
                tr = case.truth()
                dtm_pre = float(tr.dtm)
                if not (tr.ks == nbig and tr.clamped[-1] and dtm_pre > 2.0 ** -6):
                    case = None
                    break
        if case is not None:
            tr = case.truth()
            # (margin: f1 is what is left of sums 1 / small times larger -- the double-precision walk knows it to
            #  about 1e-6 only, so a decision closer than that would turn on its rounding)
            if tr.clamped[nbig:tr.ks].any() and nbig + 5 < tr.ks < tr.nb - 5 and tr.min_margin >= 1e-4 \
                    and tr.dtm > 0:
                return case
    raise AssertionError("no seed gives a walk that crosses breakpoints on the clamp")


def _dyadic_mid(name, seed, real):
    """a walk that stops in the middle on float32 numbers with few bits (see _clamp_case): for REAL32 contexts"""
    rng = np.random.default_rng(seed)
    n, nb, m, col = 1200, 1000, 5, 5
    ws, wy, sy, ss, wt, theta = _pairs(rng, n, m, col, 1, np.float32)
    g = rng.integers(32, 64, n) / 64.0 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    is_bp = np.zeros(n, bool)
    is_bp[rng.permutation(n)[:nb]] = True
    t = rng.integers(16, 2048, n) / 1024.0 / theta
    t = np.float32(t).astype(np.float64)
    t = np.ldexp(np.round(np.ldexp(np.frexp(t)[0], 11)), np.frexp(t)[1] - 11)      # 11 significant bits
    down = g > 0
    x = np.where(is_bp, np.where(down, t * np.abs(g), -t * np.abs(g)), rng.integers(-8, 8, n) / 4.0)
    l, u = np.where(is_bp & down, 0.0, -8.0), np.where(is_bp & ~down, 0.0, 8.0)
    nbd = np.where(is_bp, np.where(down, 1, 3), np.where(rng.random(n) < 0.5, 0, np.where(down, 3, 1))).astype(np.int32)
    pr = _probe(np.flatnonzero(~is_bp)[-1], x, l, u, nbd, g, 1.0)
    arrs = [a.astype(np.float32) for a in (x, l, u)] + [nbd, g.astype(np.float32)]
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(arrs, (x, l, u, nbd, g)))
    if real == np.float64:
        arrs = [a.astype(np.float64) if a.dtype == np.float32 else a for a in arrs]
    W = [a.astype(real) for a in (ws, wy, sy, ss, wt)]
    return Case(name, n, m, col, 1, real, *arrs, _active_iwhere(l, u, nbd), *W, theta, expect=dict(mid=True, probe=pr))


def _col0_case(name, seed, kind):
    """No pair stored: the closed form t* = 1 / theta and its guard.
      closed        -- breakpoints on both sides of t*, free rows: the closed form.  Random numbers, theta = 0.7: the
                       walk's own tsum would be 1 / theta only up to its rounding, the closed form's is fl(1 / theta)
      closed_all_bp -- every row a breakpoint (nb == n), still breakpoints beyond t*: the closed form
    and, with theta = 1/2 (t* = 2) and every number a small dyadic one, so that the reference's recurrence is exact in
    double up to what it cannot hold at all, and what its walk returns is not a matter of rounding:
      all_fixed     -- every row a breakpoint below t*: nothing moves beyond t*, the guard sends the call to the walk,
                       which fixes all n (nseg = n)
      guard         -- a few rows carry the gradient and are fixed early; the others (2^-33 of it, 2^-66 of d'd) have
                       breakpoints just behind them and beyond t*: the guard triggers, the clamp ends the walk after
                       a step of about 1e-5 where the closed form would have gone on to t* = 2"""
    rng = np.random.default_rng(seed)
    n, m, theta = 160, 3, 0.5
    g = rng.choice([0.5, 1.0, 0.75, 1.25], n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    t = rng.integers(8, 256, n) / 64.0                     # (0.125, 4)
    if kind.startswith("closed"):
        theta = 0.7
        g = (0.5 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        t = (0.05 + 1.95 * rng.random(n)) / theta
    is_bp = np.ones(n, bool)
    path = "closed"
    if kind == "closed":
        is_bp[rng.permutation(n)[:40]] = False
    elif kind == "all_fixed":
        t = rng.integers(8, 120, n) / 64.0
        path = "fallback"
    elif kind == "guard":
        big = np.zeros(n, bool)
        big[rng.permutation(n)[:100]] = True
        t = np.where(big, rng.integers(8, 64, n) / 64.0, 0.0)                                     # (0.125, 1)
        near = ~big & (rng.random(n) < 0.5)
        t = np.where(near, 1.0 + rng.integers(1, 40, n) * 2.0 ** -20, t)
        t = np.where(~big & ~near, 2.0 + rng.integers(1, 64, n) / 64.0, t)
        g = np.where(big, g, g * 2.0 ** -33)
        path = "fallback"
    down = g > 0
    x = np.where(is_bp, np.where(down, t * np.abs(g), -t * np.abs(g)), rng.integers(-8, 8, n) / 4.0)
    l, u = np.where(is_bp & down, 0.0, -8.0), np.where(is_bp & ~down, 0.0, 8.0)
    nbd = np.where(is_bp, np.where(down, 1, 3), np.where(rng.random(n) < 0.5, 0, np.where(down, 3, 1))).astype(np.int32)
    expect = dict(all_fixed=kind == "all_fixed", clamp_state=kind == "guard", nb_eq_n=kind != "closed")
    if kind == "closed":
        expect["probe"] = _probe(np.flatnonzero(~is_bp)[-1], x, l, u, nbd, g, 1.0)
    z = np.zeros((m, n))
    zz = np.zeros(m * m)
    return Case(name, n, m, 0, 1, np.float64, x, l, u, nbd, g, _active_iwhere(l, u, nbd), z, z.copy(), zz, zz.copy(),
                zz.copy(), theta, path=path, expect=expect, backend="mpmath" if kind == "guard" else None)


def _spec():
    s = {}
    for nb in (1, 31, 32, 33, 1000):
        # nb = 1: a single breakpoint cannot be "in the middle"; the search runs only if it is within reach, so it is
        # crossed (ks = nb = 1, the k = 0 branches of every kernel) and the free rows end the walk
        s["mid_nb%d" % nb] = functools.partial(_make, seed=100 + nb, n=nb + 37, nb=nb, m=5, col=3,
                                               t_hi=0.5 if nb == 1 else 2.0,
                                               expect=dict(mid=nb > 1, ks_eq_nb=nb == 1, nb=nb))
    s["long_nb70001"] = functools.partial(_make, seed=7, n=70_050, nb=70_001, m=5, col=5, expect=dict(mid=True, nb=70_001))
    for col in (1, 5, 6, 10, 11, 20, 21, 32):
        s["col%d" % col] = functools.partial(_make, seed=200 + col, n=2100, nb=2000 + col, m=col, col=col,
                                             expect=dict(mid=True))
    s["ring_head4"] = functools.partial(_make, seed=31, n=700, nb=600, m=7, col=7, head=4, expect=dict(mid=True))
    s["all_crossed_free"] = functools.partial(_make, seed=41, n=330, nb=200, m=5, col=4, t_hi=0.4,
                                              expect=dict(ks_eq_nb=True, bnded=False))
    s["all_crossed_bnded"] = functools.partial(_make, seed=42, n=260, nb=200, m=5, col=4, t_hi=0.4, edit=_zero_rest,
                                               expect=dict(ks_eq_nb=True, bnded=True))
    s["all_fixed"] = functools.partial(_make, seed=43, n=200, nb=200, m=5, col=4, t_hi=0.4,
                                       expect=dict(ks_eq_nb=True, all_fixed=True))
    s["clamp"] = functools.partial(_clamp_case, seed=51, real=np.float64)
    s["tie_group"] = functools.partial(_make, seed=61, n=400, nb=300, m=5, col=3, edit=_tie_group,
                                       expect=dict(mid=True, tie=4))
    s["all_kinds"] = functools.partial(_make, seed=71, n=500, nb=400, m=6, col=4, edit=_all_kinds,
                                       expect=dict(mid=True, kinds=True))
    s["clamp_r32"] = functools.partial(_clamp_case, seed=52, real=np.float32)
    s["mid_r32"] = functools.partial(_dyadic_mid, seed=81, real=np.float32)
    s["col0_closed"] = functools.partial(_col0_case, seed=91, kind="closed")
    s["col0_closed_all_bp"] = functools.partial(_col0_case, seed=92, kind="closed_all_bp")
    s["col0_all_fixed"] = functools.partial(_col0_case, seed=93, kind="all_fixed")
    s["col0_guard"] = functools.partial(_col0_case, seed=94, kind="guard")
    return s


_SPEC = _spec()
NAMES = tuple(_SPEC)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and its truth, built once per process and shared (read only) by the tests that need them"""
    c = _SPEC[name](name)
    return c, c.truth()


def oracle_cauchy(c, perm=None):
    """the oracle's double-precision cauchy (oracle/lbfgsb_oracle.c, the twin of src/lbfgsb.f90:1157-1532) on the
    case's numbers -> dict(nseg, info, iwhere, xcp, c, tsum, sbgnrm, p, wbp, v).  REAL32 cases: their float32 numbers widened,
    epsmch of float32 -- the times of their breakpoints are exact quotients and do not change.  perm: the same
    problem with its rows in another order (iwhere and xcp come back in the case's order).  tsum is read off the
    probe row where the case has one (exact), else off a moving row ((xcp - x) / d: two more roundings)."""
    from oracle import pyoracle as po
    R = po.Routines()
    n, m = c.n, c.m
    perm = np.arange(n) if perm is None else perm
    f = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    x, l, u, g = (f(a[perm]) for a in (c.x, c.l, c.u, c.g))
    nbd, iw = np.ascontiguousarray(c.nbd[perm]), np.ascontiguousarray(c.iwhere[perm])
    xcp = np.zeros(n)
    iorder, t, d = np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
    pc = [np.zeros(2 * m) for _ in range(4)]
    nseg, info = np.zeros(1, np.int32), np.zeros(1, np.int32)
    sbg = float(R.projgr(n, l, u, nbd, x, g))
    R.cauchy(n, x, l, u, nbd, g, iorder, iw, t, d, xcp, m, f(c.wy[:, perm]).reshape(-1), f(c.ws[:, perm]).reshape(-1),
             f(c.sy), f(c.wt), float(c.theta), c.col, c.head, pc[0], pc[1], pc[2], pc[3], nseg, sbg, info, c.epsmch)
    back = np.empty(n, np.int64)
    back[perm] = np.arange(n)
    tsum = None
    if "probe" in c.expect:
        i, scale = c.expect["probe"]
        tsum = float(-xcp[back[i]] / scale)
    elif np.any(d != 0):
        i = int(np.flatnonzero(d != 0)[0])
        tsum = float((xcp[i] - x[i]) / d[i])
    return dict(nseg=int(nseg[0]), info=int(info[0]), iwhere=iw[back], xcp=xcp[back], c=pc[1][:2 * c.col].copy(),
                tsum=tsum, sbgnrm=sbg, p=pc[0][:2 * c.col].copy(), wbp=pc[2][:2 * c.col].copy(),
                v=pc[3][:2 * c.col].copy())


EPS64 = EPS[np.float64]


def rho_c(c_got, tr):
    """the error of a vector c in units of eps M_a (eps of double), largest over its components"""
    if not tr.M.size:
        return 0.0
    return float(np.max(np.abs(np.asarray(c_got, np.longdouble) - tr.c) / (EPS64 * tr.M.astype(np.longdouble))))


def rho_t(tsum_got, tr):
    """the error of tsum in units of eps tsum"""
    return float(abs(np.longdouble(tsum_got) - tr.tsum) / (EPS64 * tr.tsum))


@functools.lru_cache(maxsize=None)
def reference(name):
    """What the reference's own double-precision arithmetic makes of the case: the oracle's result on it, and its
    errors rho_c, rho_t against the truth.  One run is one realisation of the roundings and may be luckily small, so
    the errors are the largest over the case as given and over three fixed permutations of its rows (the same walk
    in exact arithmetic -- no case ends inside a group of equal breakpoints -- with its sums in other orders).
    K_c = max(4 rho_c, 2 (log2 nb + 4)) and K_t likewise are the bounds for the code under test: 4, because scans
    associate differently from the sequential sums; the floor is the depth of a scan over nb terms plus the four
    operations of the host formula."""
    c, tr = case(name)
    o = oracle_cauchy(c)
    rc, rt = [], []
    for k in range(4):
        ok = o if k == 0 else oracle_cauchy(c, np.random.default_rng(9000 + k).permutation(c.n))
        rc.append(rho_c(ok["c"], tr))
        if ok["tsum"] is not None and tr.tsum > 0:
            rt.append(rho_t(ok["tsum"], tr))
    floor = 2.0 * (np.log2(max(tr.nb, 1)) + 4.0)
    o.update(rho_c=max(rc), rho_t=max(rt) if rt else 0.0, floor=floor)
    o.update(K_c=max(4.0 * o["rho_c"], floor), K_t=max(4.0 * o["rho_t"], floor))
    return o
