"""The generalized-Cauchy-point walk of the reference (cauchy, src/lbfgsb.f90:1245-1530) restated in extended
precision: TEST HELPER, not a test and not a conftest.

The walk is taken as the reference takes it -- ONE breakpoint at a time, the running state (p, c, f1, f2, dtm, tsum)
updated by the reference's own recurrences (:1416-1497) -- in numpy.longdouble (64-bit mantissa on x86), and once
more in mpmath (200 bits) whenever a stopping decision of the longdouble walk is closer than 1e-9: nothing here
is a cumulative sum over the breakpoints, so a mistake in the scanned formulation of the code under test
(lbfgsb_amd/csrc/k_pgcp.hip) is not shared.  Two things are NOT extended, because they define the walk instead of
approximating it:

  * the breakpoint times t_i = (x_i - l_i) / g_i resp. (u_i - x_i) / -g_i are rounded to the working precision of
    the inputs, operation for operation as :1305 / :1314 do -- their order, and which of them are EQUAL, is what
    the walk is about;
  * breakpoints are taken in (t, index) order.  The reference pops equal t in the order of its heap (hpsolb
    :2079); the sums over a whole group of equal breakpoints do not depend on the order (dt = 0 inside it), the
    members fixed do when the walk ends inside one -- `Truth.ends_in_tie` says so, and no case of the tests does.

M is applied as the reference's bmv (:1057-1123) from sy and wt, vectorised over the breakpoints (the product
M wbp_k of a breakpoint does not depend on the walk's state).

Not covered: the early returns for sbgnrm <= 0 (:1245) -- the caller decides that.
"""
from dataclasses import dataclass

import numpy as np

MP_PREC = 200          # bits of the mpmath replay
UNCLEAR = 1e-9         # longdouble decisions closer than this are replayed in mpmath


class _LongDouble:
    name = "longdouble"

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.longdouble)

    @staticmethod
    def num(v):
        return np.longdouble(v)

    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def dot(a, b):
        return np.dot(a, b) if len(a) else np.longdouble(0)


class _MP:
    name = "mpmath"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.prec = MP_PREC

    def num(self, v):
        return self.mp.mpf(float(v))

    def arr(self, a):
        a = np.asarray(a)
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for k, v in enumerate(np.asarray(a, dtype=np.float64).reshape(-1)):
            flat[k] = self.mp.mpf(float(v))
        return out

    def sqrt(self, v):
        return self.mp.sqrt(v)

    def dot(self, a, b):
        s = self.mp.mpf(0)
        for u, v in zip(a, b):
            s = s + u * v
        return s


@dataclass
class Truth:
    nseg: int
    tsum: object              # extended
    iwhere: np.ndarray        # int32, as cauchy leaves it
    xcp: np.ndarray           # longdouble
    c: np.ndarray             # longdouble, 2 col
    M: np.ndarray             # float64, 2 col: sum_k dt_k (|p0_a| + sum_{j<k} |d_j wbp_ja|), the last segment's dtm included
    margins: np.ndarray       # |dtm - dt| / max(dt, dtm) of every decision :1416 the walk took (the stopping one included)
    clamped: np.ndarray       # per crossed breakpoint: f2 was set by the clamp :1483
    nb: int                   # breakpoints
    ks: int                   # breakpoints crossed
    order: np.ndarray         # 0-based rows of the breakpoints in (t, index) order
    t: np.ndarray             # their times, float64 (exact: rounded to the working precision)
    all_fixed: bool           # the exit :1436-1442 was taken
    bnded: bool
    dtm: object               # the last segment's step (after :1509)
    fixed: np.ndarray         # bool, rows fixed by THIS walk
    d: np.ndarray             # float64, the direction after the walk (0 on fixed rows)
    backend: str

    @property
    def min_margin(self):
        return float(self.margins.min()) if self.margins.size else float("inf")

    @property
    def ends_in_tie(self):
        """the walk stopped between two breakpoints of equal t: the tie order decides which rows are fixed"""
        return 0 < self.ks < self.nb and self.t[self.ks] == self.t[self.ks - 1]

    def tie_groups_crossed_whole(self, least=3):
        """sizes of the groups of >= `least` equal t that the walk crossed entirely"""
        out, k = [], 0
        while k < self.ks:
            j = k
            while j + 1 < self.nb and self.t[j + 1] == self.t[k]:
                j += 1
            if j - k + 1 >= least and j < self.ks:
                out.append(j - k + 1)
            k = j + 1
        return out


def _bmv(B, m, sy, wt, col, V):
    """bmv :1057-1123 on every row of V (k x 2 col): the product of the 2 col x 2 col middle matrix with it"""
    SY, WT = sy.reshape(m, m).T, wt.reshape(m, m).T
    v1, v2 = V[:, :col], V[:, col:]
    p2 = []
    for i in range(col):                                   # :1085-1093
        s = v2[:, i]
        for k in range(i):
            s = s + SY[i, k] * v1[:, k] / SY[k, k]
        p2.append(s)
    for j in range(col):                                   # dtrsl job 11: J x = b, J' the upper factor in wt
        s = p2[j]
        for i in range(j):
            s = s - WT[i, j] * p2[i]
        p2[j] = s / WT[j, j]
    rs = [B.sqrt(SY[i, i]) for i in range(col)]
    p1 = [v1[:, i] / rs[i] for i in range(col)]            # :1101-1103
    for j in reversed(range(col)):                         # dtrsl job 01: J' x = b
        s = p2[j]
        for i in range(j + 1, col):
            s = s - WT[j, i] * p2[i]
        p2[j] = s / WT[j, j]
    for i in range(col):                                   # :1111-1121
        s = -p1[i] / rs[i]
        for k in range(i + 1, col):
            s = s + SY[k, i] * p2[k] / SY[i, i]
        p1[i] = s
    out = np.empty(V.shape, dtype=V.dtype)
    for i in range(col):
        out[:, i], out[:, col + i] = p1[i], p2[i]
    return out


def _walk(B, x, l, u, nbd, g, iwhere, ws, wy, head, col, sy, wt, theta, epsmch):
    real = x.dtype.type
    n, m = x.size, ws.shape[0]
    col2 = 2 * col
    iw = np.array(iwhere, dtype=np.int32)
    # ---- :1270-1330, every row on its own; tl, tu, t in the working precision as the reference computes them
    neggi = -g
    live = (iw != 3) & (iw != -1)
    lo, up = nbd <= 2, nbd >= 2
    with np.errstate(invalid="ignore", over="ignore"):
        tl, tu = (x - l).astype(real), (u - x).astype(real)
    assert not np.any(live & (nbd == 0)), "an unbounded row carries iwhere = -1 (active :1024-1037)"
    xlower, xupper = lo & (tl <= 0), up & (tu <= 0)
    new = np.zeros(n, np.int32)
    new[xlower & (neggi <= 0)] = 1
    new[~xlower & xupper & (neggi >= 0)] = 2
    new[~xlower & ~xupper & (neggi == 0)] = -3
    iw[live] = new[live]
    moving = (iw == 0) | (iw == -1)
    d = np.where(moving, neggi, real(0)).astype(real)
    to_l = moving & lo & (nbd != 0) & (neggi < 0)
    to_u = moving & ~to_l & up & (neggi > 0)
    rest = moving & ~to_l & ~to_u
    bnded = not bool(np.any(rest & (neggi != 0)))
    tb = np.full(n, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        tb[to_l] = (tl[to_l] / (-neggi[to_l])).astype(real)
        tb[to_u] = (tu[to_u] / neggi[to_u]).astype(real)
    rows = np.flatnonzero(to_l | to_u)
    rows = rows[np.lexsort((rows, tb[rows]))]
    nb = rows.size
    t = tb[rows].astype(np.float64)
    ring = [(head - 1 + j) % m for j in range(col)]
    dX = B.arr(d)
    f1 = -B.dot(dX, dX)
    # p = W'd (:1293-1297), theta on the S half (:1337)
    mv = np.flatnonzero(moving)
    p = B.arr(np.zeros(col2))
    th = B.num(theta)
    for j, slot in enumerate(ring):
        p[j] = B.dot(B.arr(wy[slot, mv]), dX[mv])
        p[col + j] = th * B.dot(B.arr(ws[slot, mv]), dX[mv])
    xX, lX, uX = B.arr(x), B.arr(l), B.arr(u)
    xcp = xX.copy()
    zero = B.num(0)
    c = B.arr(np.zeros(col2))
    Mmag = B.arr(np.zeros(col2))
    fixed = np.zeros(n, bool)
    base = dict(iwhere=iw, nb=nb, order=rows, t=t, bnded=bnded, backend=B.name)
    if nb == 0 and not rest.any():                          # :1343-1347
        return Truth(nseg=0, tsum=zero, xcp=xcp, c=c, M=np.zeros(col2), margins=np.zeros(0), clamped=np.zeros(0, bool),
                     ks=0, all_fixed=False, dtm=zero, fixed=fixed, d=d.astype(np.float64), **base)
    f2 = -th * f1                                           # :1357-1363
    f2_org = f2
    syX, wtX = B.arr(sy), B.arr(wt)
    if col:
        v = _bmv(B, m, syX, wtX, col, p.reshape(1, col2))[0]
        f2 = f2 - B.dot(v, p)
    dtm = -f1 / f2
    tsum = zero
    nseg = 1
    # what a breakpoint brings with it, none of it depending on the walk's state
    WB = B.arr(np.zeros((nb, col2)))
    for j, slot in enumerate(ring):
        WB[:, j] = B.arr(wy[slot, rows])
        WB[:, col + j] = th * B.arr(ws[slot, rows])
    if col and nb:
        V = _bmv(B, m, syX, wtX, col, WB)
        WMW = (WB * V).sum(axis=1)
    tX, dB = B.arr(t), dX[rows]
    to_upper = d[rows] > 0
    zB = np.where(to_upper, uX[rows] - xX[rows], lX[rows] - xX[rows])
    pabs = np.abs(p)
    clampv = B.num(epsmch) * f2_org
    margins, clamped = [], []
    ks, all_fixed = 0, False
    tj = zero

    def margin(dtm_, dt_):
        big = max(abs(dt_), abs(dtm_))
        return float(abs(dtm_ - dt_) / big) if big != 0 else 0.0
    nleft = nb
    for k in range(nb):                                     # :1378-1497
        dt = tX[k] - tj
        margins.append(margin(dtm, dt))
        if dtm < dt:                                        # :1416
            break
        tj = tX[k]
        tsum = tsum + dt
        nleft -= 1
        ks += 1
        i = rows[k]
        dibp, zibp = dB[k], zB[k]
        d[i] = 0
        fixed[i] = True
        if to_upper[k]:
            xcp[i], iw[i] = uX[i], 2
        else:
            xcp[i], iw[i] = lX[i], 1
        if nleft == 0 and nb == n:                          # :1436-1442
            dtm = dt
            c = c + dtm * p
            Mmag = Mmag + dtm * pabs
            all_fixed = True
            clamped.append(False)
            break
        nseg += 1
        dibp2 = dibp * dibp
        f1 = f1 + dt * f2 + dibp2 - th * dibp * zibp        # :1452-1453
        f2 = f2 - th * dibp2
        if col:
            c = c + dt * p
            Mmag = Mmag + dt * pabs
            wbp, v = WB[k], V[k]
            wmc, wmp = B.dot(c, v), B.dot(p, v)
            step = dibp * wbp
            p = p - step
            pabs = pabs + np.abs(step)
            f1 = f1 + dibp * wmc
            f2 = f2 + 2 * dibp * wmp - dibp2 * WMW[k]
        clamped.append(bool(f2 < clampv))                   # :1483
        if f2 < clampv:
            f2 = clampv
        if nleft > 0:
            dtm = -f1 / f2
        elif bnded:
            f1, f2, dtm = zero, zero, zero
        else:
            dtm = -f1 / f2
    if not all_fixed:
        if dtm <= 0:                                        # :1509
            dtm = zero
        tsum = tsum + dtm
        for i in np.flatnonzero(d != 0):                    # :1515
            xcp[i] = xcp[i] + tsum * dX[i]
        if col:                                             # :1526
            c = c + dtm * p
            Mmag = Mmag + dtm * pabs
    return Truth(nseg=nseg, tsum=tsum, xcp=xcp, c=c, M=np.array([float(v) for v in Mmag]), margins=np.array(margins),
                 clamped=np.array(clamped, bool), ks=ks, all_fixed=all_fixed, dtm=dtm, fixed=fixed,
                 d=d.astype(np.float64), **base)


def truth(x, l, u, nbd, g, iwhere, ws, wy, head, col, sy, wt, theta, epsmch, backend=None):
    """x, l, u, g: float64 or float32 vectors (their dtype is the working precision of the breakpoint times);
    ws, wy: (m, n), row j the reference's column j + 1; head 1-based; sy, wt: m*m, column-major.
    backend: None (longdouble, replayed in mpmath if a decision is unclear), "longdouble" or "mpmath"."""
    x = np.ascontiguousarray(x)
    args = (x, np.asarray(l, x.dtype), np.asarray(u, x.dtype), np.asarray(nbd, np.int32), np.asarray(g, x.dtype),
            iwhere, np.asarray(ws), np.asarray(wy), int(head), int(col), np.asarray(sy), np.asarray(wt), float(theta),
            float(epsmch))
    if backend != "mpmath":
        tr = _walk(_LongDouble(), *args)
        if backend == "longdouble" or tr.min_margin >= UNCLEAR:
            return tr
    B = _MP()
    return _to_longdouble(B, _walk(B, *args))


def _to_longdouble(B, tr):
    def ld(v):   # two-piece conversion: the leading double and what is left of it
        hi = float(v)
        return np.longdouble(hi) + np.longdouble(float(v - B.num(hi)))
    tr.tsum, tr.dtm = ld(tr.tsum), ld(tr.dtm)
    tr.c = np.array([ld(v) for v in tr.c], dtype=np.longdouble)
    tr.xcp = np.array([ld(v) for v in tr.xcp], dtype=np.longdouble)
    return tr
