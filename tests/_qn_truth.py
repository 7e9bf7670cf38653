"""The limited-memory curvature model in extended precision (np.longdouble, eps < 2e-19), and the error a correct
fp64 evaluation of it is allowed.

THE REFERENCE reads the pairs as stored (the imported arrays or export_state()), oldest first, and nothing else of
the device.  It does not use the compact formula:
  B        the recursive BFGS update from theta I:   B <- B - (B s)(B s)' / s'B s + y y' / y's;
  H        the recursive inverse update:             H <- H - rho (H y s' + s y'H) + (rho^2 y'H y + rho) s s';
  log det  n log theta + sum_k (log y_k's_k - log s_k'B_k s_k);       theta = y'y / s'y of the newest pair;
  Sigma    (B + mu I + diag d)^-1 on the free rows by fp64 solves refined in longdouble (residual in longdouble,
           correction in fp64, three rounds), pinned rows and columns exactly +0.
Every operator of the library has the shape  A = diag(a) + diag(l) W N W' diag(r),  W = [S, Y]  (plain model: a =
alpha, l = r = 1; Sigma: a = l = r = w, w_i = 1 / (theta + mu + d_i); its factor L: a = r = sqrt w, l = w).  The
reference's N is read off its own dense A by least squares in longdouble (`middle`), so the bound below can be
evaluated; A itself never comes from N.

THE BOUND.  u = 2^-53, gamma_k = k u / (1 - k u).  The device forms, for a vector v,
  p = W'(r v)             2 col sums of n products each, in an order that depends on grid and vector width;
  c = N p                 on the host, through a factorisation of the 2col x 2col matrix whose inverse N is;
  out_i = a_i v_i + l_i sum_c W_ic c_c        a sum of 2 col + 1 terms.
Standard a-priori analysis (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5), Thm 10.4 with
the perturbation bound (7.4)), with absolute values throughout and q = |W|'(|r| |v|) >= |p|:
  * any order of summation:  |p^ - p| <= gamma_n q.                                           -> t_sum
  * the expansion:  gamma_(2col+2+e) (|a_i v_i| + |l_i| |W_i| |N| q); e = 0, or 8 for the shifted family, whose
    weights a, l, r are each computed on the device by at most four roundings.                 -> t_exp
  * a_i carries theta = y'y / s'y, a ratio of n-term sums:  gamma_(n+2) |a_i v_i|.            -> t_theta
  * the host step: a Cholesky / triangular solve of a d x d system (d = 2 col) has normwise backward error
    4 d (3 d + 1) u, the entries of the small matrices are themselves n-term sums (g times gamma_n, g = 1; g = 2 for
    a state taken from a run, whose sy, ss, wt are the iteration's own sums on top of the entries' Gram), so
    |c^ - c|_2 <= eta |N|_2 |q|_2,  eta = kappa (g gamma_n + 4 d (3 d + 1) u),  kappa = cond_2(N): N is the inverse
    of the matrix factorised, evaluated here inside the reference.                            -> t_host
  bound_i = t_exp + t_theta + |l_i| (|W_i| |N| gamma_n q) + |l_i| |W_i|_2 eta |N|_2 |q|_2.
A scalar v'Av (quad, gram, logpdf) is a_ dd + p'N p with dd = sum a_i v_i^2 carried along:
  gamma_(n+2) sum |a_i| v_i^2 + (2 gamma_n + gamma_(2d+2)) q'|N| q + eta |N|_2 |q|_2^2      (two vectors: q_a, q_b).
An entry A[i, j] at indices (block, diag: r_i N r_j', two nested sums of d terms) has no n-term sum of its own:
gamma_(2d+2+e) (|a_i| [i == j] +
|l_i| |W_i| |N| |W_j|' |r_j|) + gamma_(n+2) |a_i| [i == j] + |l_i| |W_i|_2 eta |N|_2 |W_j|_2 |r_j|.
log det A = sum_i log a_i + sum_i log(lambda_i / alpha):  n gamma_(n+2) + 2 u sum |log a_i| + d eta cond_2(A) -- the
relative error of alpha n times, the rounding of the product and sum, and d eigenvalues each known to eta relative
to the largest.
REAL32 outputs add 2^-24 |ref_i| for the store; an expansion over more than 16 pairs goes tile by tile of 16 and each
later tile reads the stored partial output back, so every tile but the last adds 2^-24 (|a_i v_i| + |l_i| |W_i| |N| q),
the most a partial output can be.  A REAL32 context's middle matrix of B comes from the imported fp32
wt: B-type entries are compared with the compact form (the bmv algebra) on the imported matrices widened to
longdouble -- independent of the device, not of the formula -- and held to the recursion with eta + kappa 2 d 2^-24
(each entry of the factor J rounded by 2^-24, so J J' by 2 * 2^-24 |J| |J'| <= 2 d 2^-24 |J J'|_2).
The assertion is |out - ref| <= bound entry by entry, with no further constant."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble has no extended precision on this host"
U = 2.0 ** -53
U32 = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------- dense helpers
def ld_solve(A, B, rounds=3, matvec=None):
    """A^-1 B for a longdouble A: fp64 solves refined by longdouble residuals (matvec: X -> A X, when A has a cheaper
    product than the dense one)"""
    A = np.asarray(A, LD)
    B = np.asarray(B, LD)
    A64 = A.astype(np.float64)
    X = np.linalg.solve(A64, B.astype(np.float64)).astype(LD)
    for _ in range(rounds):
        R = B - (A @ X if matvec is None else matvec(X))
        X = X + np.linalg.solve(A64, R.astype(np.float64)).astype(LD)
    return X


def theta_of(S, Y):
    if S.shape[1] == 0:
        return LD(1.0)
    s, y = S[:, -1].astype(LD), Y[:, -1].astype(LD)
    return (y @ y) / (s @ y)


def bfgs_dense(S, Y, theta):
    """(B, H, log det B, terms) by the two recursions from theta I, in longdouble; terms = (U, s'B s, y's) with
    U[:, k] = B_k s_k: the update terms of B as they were added, B = theta I + sum_k y y' / y's - u u' / s'B s"""
    n, col = S.shape
    S, Y = S.astype(LD), Y.astype(LD)
    theta = LD(theta)
    B = theta * np.eye(n, dtype=LD)
    H = np.eye(n, dtype=LD) / theta
    ld = n * np.log(theta)
    Um, sbs, yss = np.zeros((n, col), LD), np.zeros(col, LD), np.zeros(col, LD)
    for k in range(col):
        s, y = S[:, k], Y[:, k]
        Bs = B @ s
        sBs, ys = s @ Bs, y @ s
        Um[:, k], sbs[k], yss[k] = Bs, sBs, ys
        B = B - np.outer(Bs, Bs) / sBs + np.outer(y, y) / ys
        ld = ld + np.log(ys) - np.log(sBs)
        rho = 1 / ys
        Hy = H @ y
        H = H - rho * (np.outer(Hy, s) + np.outer(s, Hy)) + (rho * rho * (y @ Hy) + rho) * np.outer(s, s)
    return B, H, ld, (Um, sbs, yss)


def middle(A, a, l, r, W, rows=None):
    """N (2col x 2col) of A = diag(a) + diag(l) W N W' diag(r) on `rows`, by least squares in longdouble"""
    W = np.asarray(W, LD)
    d = W.shape[1]
    if d == 0:
        return np.zeros((0, 0), LD)
    n = W.shape[0]
    a, l, r = (np.broadcast_to(np.asarray(x, LD), (n,)) for x in (a, l, r))
    if rows is not None:
        A, a, l, r, W = A[np.ix_(rows, rows)], a[rows], l[rows], r[rows], W[rows]
    Wl, Wr = W * l[:, None], W * r[:, None]
    E = A - np.diag(a)
    return ld_solve(Wl.T @ Wl, ld_solve(Wr.T @ Wr, (Wl.T @ E @ Wr).T).T)


# ---------------------------------------------------------------------------------------------- the bmv algebra
def _trsolve(Uf, b, trans):
    """T x = b (trans False) or T'x = b for an upper triangular T, in the dtype of the operands"""
    d = Uf.shape[0]
    x = np.array(b, dtype=np.result_type(Uf, b), copy=True)
    if trans:
        for i in range(d):
            x[i] = (x[i] - Uf[:i, i] @ x[:i]) / Uf[i, i]
    else:
        for i in range(d - 1, -1, -1):
            x[i] = (x[i] - Uf[i, i + 1:] @ x[i + 1:]) / Uf[i, i]
    return x


def bmv(sy, wt, col, v):
    """the product of the 2col x 2col middle matrix of the compact form with v = (Y part; theta S part): the
    reference's bmv from sy and the Cholesky factor in wt, in the dtype of the operands"""
    D = np.diag(sy)[:col]
    L = np.tril(sy[:col, :col], -1)
    Uf = np.triu(wt[:col, :col])
    v1, v2 = v[:col], v[col:]
    p2 = _trsolve(Uf, v2 + L @ (v1 / D), True)
    p2 = _trsolve(Uf, p2, False)
    p1 = -v1 / D + (L.T @ p2) / D
    return np.concatenate([p1, p2])


def compact_n_b(sy, wt, col, theta, dtype=LD):
    """N of B = theta I + [S, Y] N [S, Y]' by the compact form: B = theta I - [Y, theta S] M^-1 [Y, theta S]'"""
    sy, wt = np.asarray(sy, dtype), np.asarray(wt, dtype)
    theta = dtype(theta)
    d = 2 * col
    Minv = np.zeros((d, d), dtype)
    for j in range(d):
        e = np.zeros(d, dtype)
        e[j] = 1
        Minv[:, j] = bmv(sy, wt, col, e)
    P = np.zeros((d, d), dtype)  # [Y, theta S] = [S, Y] P
    for i in range(col):
        P[col + i, i] = 1
        P[i, col + i] = theta
    return -(P @ Minv @ P.T)


# ---------------------------------------------------------------------------------------------- operators and bounds
class Op:
    """A = diag(a) + diag(l) W N W' diag(r) with what its bound needs.  A: the dense reference (None: built from N).
    free: boolean mask of the rows that are not pinned (None: all); pinned rows and columns of A are +0."""

    def __init__(self, W, N, a, l=1.0, r=1.0, A=None, n_terms=None, g=1, extra=0, eta_add=0.0, free=None):
        n, d = W.shape
        self.n, self.d = n, d
        self.W = np.asarray(W, LD)
        self.N = np.asarray(N, LD)
        self.a, self.l, self.r = (np.broadcast_to(np.asarray(x, LD), (n,)).copy() for x in (a, l, r))
        self.free = np.ones(n, bool) if free is None else np.asarray(free, bool)
        for x in (self.a, self.l, self.r):
            x[~self.free] = 0
        self.extra = extra
        self._cache = {}
        self.tiles = max(1, -(-(d // 2) // 16))  # column tiles of 16 pairs (qn_plan.hpp)
        self.nt = n if n_terms is None else n_terms
        self.A = A if A is not None else np.diag(self.a) + (self.W * self.l[:, None]) @ self.N @ (self.W * self.r[:, None]).T
        if d:
            sv = np.linalg.svd(self.N.astype(np.float64), compute_uv=False)
            self.n2, self.kappa = float(sv[0]), float(sv[0] / sv[-1])
        else:
            self.n2, self.kappa = 0.0, 1.0
        self.eta_add = eta_add
        self.eta = self.kappa * (g * gamma(self.nt) + 4.0 * d * (3 * d + 1) * U) + eta_add
        self.absW = np.abs(self.W).astype(np.float64)
        self.absN = np.abs(self.N).astype(np.float64)
        self.rowW = np.sqrt((self.absW ** 2).sum(axis=1))
        self.fa, self.fl, self.fr = (np.abs(x).astype(np.float64) for x in (self.a, self.l, self.r))

    def _memo(self, name, arrs, fn):
        """fn() once per (name, operands): the switch settings of a state share their references and bounds"""
        key = (name,) + tuple((a.shape, a.dtype.str, hash(a.tobytes())) if isinstance(a, np.ndarray) else a
                              for a in arrs)
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def apply(self, V):
        """A V' for V of shape (k, n), as (k, n) longdouble"""
        V = np.asarray(V)
        return self._memo("apply", (V,), lambda: (self.A @ V.astype(LD).T).T)

    def bound_apply(self, V, real=np.float64, ref=None):
        V = np.asarray(V)
        return self._memo("bound_apply", (V, real is np.float32), lambda: self._bound_apply(V, real, ref))

    def _bound_apply(self, V, real, ref):
        V = np.abs(np.asarray(V, np.float64))
        q = (V * self.fr) @ self.absW            # (k, d)
        Nq = q @ self.absN.T                     # (k, d): |N| q
        wnq = Nq @ self.absW.T                   # (k, n): |W_i| |N| q
        qn = np.sqrt((q ** 2).sum(axis=1))[:, None]
        av = self.fa * V
        b = gamma(self.d + 2 + self.extra) * (av + self.fl * wnq) + gamma(self.nt + 2) * av \
            + self.fl * wnq * gamma(self.nt) + self.fl * self.rowW * self.eta * self.n2 * qn
        if real == np.float32:
            # the store of the output, and of the partial output after every column tile but the last (the next
            # tile reads it back and adds its columns): each at most |a_i v_i| + |l_i| |W_i| |N| q in size
            b = b + U32 * np.abs(np.asarray(self.apply(V) if ref is None else ref, np.float64)) \
                + (self.tiles - 1) * U32 * (av + self.fl * wnq)
        return b

    def quad(self, Va, Vb=None):
        """Va A Vb' (ka, kb) longdouble"""
        Va = np.asarray(Va)
        Vb = Va if Vb is None else np.asarray(Vb)
        return self._memo("quad", (Va, Vb), lambda: Va.astype(LD) @ self.A @ Vb.astype(LD).T)

    def bound_quad(self, Va, Vb=None):
        Va = np.asarray(Va)
        Vb = Va if Vb is None else np.asarray(Vb)
        return self._memo("bound_quad", (Va, Vb), lambda: self._bound_quad(Va, Vb))

    def _bound_quad(self, Va, Vb):
        Va, Vb = np.abs(np.asarray(Va, np.float64)), np.abs(np.asarray(Vb, np.float64))
        qa, qb = (Va * self.fl) @ self.absW, (Vb * self.fr) @ self.absW
        na, nb = np.sqrt((qa ** 2).sum(axis=1)), np.sqrt((qb ** 2).sum(axis=1))
        return gamma(self.nt + 2) * ((Va * self.fa) @ Vb.T) \
            + (2 * gamma(self.nt) + gamma(2 * self.d + 2 + self.extra)) * (qa @ self.absN @ qb.T) \
            + self.eta * self.n2 * np.outer(na, nb)

    def bound_block(self, ia, ib):
        ia, ib = np.asarray(ia), np.asarray(ib)
        eq = (ia[:, None] == ib[None, :]) * self.fa[ia][:, None]
        wl, wr = self.absW[ia] * self.fl[ia][:, None], self.absW[ib] * self.fr[ib][:, None]
        return gamma(2 * self.d + 2 + self.extra) * (eq + wl @ self.absN @ wr.T) + gamma(self.nt + 2) * eq \
            + self.eta * self.n2 * np.outer(np.sqrt((wl ** 2).sum(axis=1)), np.sqrt((wr ** 2).sum(axis=1)))

    def bound_diag(self):
        """bound_block(i, i) for every row"""
        wl, wr = self.absW * self.fl[:, None], self.absW * self.fr[:, None]
        quad = ((wl @ self.absN) * wr).sum(axis=1)
        return gamma(2 * self.d + 2 + self.extra) * (self.fa + quad) + gamma(self.nt + 2) * self.fa \
            + self.eta * self.n2 * np.sqrt((wl ** 2).sum(axis=1)) * np.sqrt((wr ** 2).sum(axis=1))

    def bound_logdet(self, sum_abs_log, cond_a):
        n = int(self.free.sum())
        return n * gamma(self.nt + 2) + 2 * U * sum_abs_log + self.d * self.eta * cond_a


def ld_logdet(A):
    """log det of a symmetric positive definite longdouble matrix by a Cholesky factorisation in longdouble"""
    A = np.array(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    ld = LD(0)
    for j in range(n):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        assert piv > 0
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        ld = ld + 2 * np.log(L[j, j])
    return ld


class Truth:
    """everything the tests ask of one state: S, Y as stored (n x col, oldest first), theta None: of the newest pair.
    g = 2 for a state taken from a run.  real32 = (sy, wt) as imported: B-type operators then come twice, `B` from the
    compact form on those matrices and `B_rec` from the recursion with the fp32 allowance."""

    def __init__(self, S, Y, theta=None, g=1, real32=None, sy_exact=True):
        self.S, self.Y = np.asarray(S, LD), np.asarray(Y, LD)
        self.n, self.col = self.S.shape
        self.g = g
        self.theta = theta_of(self.S, self.Y) if theta is None else LD(theta)
        self.W = np.concatenate([self.S, self.Y], axis=1)
        self.Bd, self.Hd, self.logdet_b, self.terms = bfgs_dense(self.S, self.Y, self.theta)
        ev = np.linalg.eigvalsh(self.Bd.astype(np.float64))
        self.cond = float(ev[-1] / ev[0])
        NB = middle(self.Bd, self.theta, 1, 1, self.W)
        NH = middle(self.Hd, 1 / self.theta, 1, 1, self.W)
        self.real32 = real32
        # (H's middle matrix takes s'y from the imported sy: fp32 numbers in a REAL32 context, exact in the dyadic family)
        h_add = 0.0 if (real32 is None or sy_exact) else 2 * (2 * self.col) * U32
        self.H = Op(self.W, NH, 1 / self.theta, A=self.Hd, g=g)
        if h_add:
            self.H = Op(self.W, NH, 1 / self.theta, A=self.Hd, g=g, eta_add=self.H.kappa * h_add)
        if real32 is None:
            self.B = Op(self.W, NB, self.theta, A=self.Bd, g=g)
            self.B_rec = self.B
        else:
            sy, wt = real32
            N32 = compact_n_b(sy, wt, self.col, self.theta) if self.col else NB
            self.B = Op(self.W, N32, self.theta, g=g)
            kap = self.B.kappa
            self.B_rec = Op(self.W, NB, self.theta, A=self.Bd, g=g, eta_add=kap * 2 * (2 * self.col) * U32)

    def _shift_matvec(self, base, A, fr, mu, dd):
        """X -> A X for A = (B + mu I + diag d) on the free rows through the update terms of the recursion, B = theta I
        + sum_k y y' / y's - u u' / s'B s: the residual of the refinement at large n, where the dense product in
        longdouble takes seconds.  Only where B is the recursion's, and checked against the dense product."""
        if fr.size <= 400 or not self.col or base.A is not self.Bd:
            return None
        Um, sbs, yss = self.terms
        Uf, Yf = Um[fr], self.Y[fr]
        diag = self.theta + LD(mu) + dd[fr].astype(LD)
        mv = lambda X: diag[:, None] * X + Yf @ ((Yf.T @ X) / yss[:, None]) - Uf @ ((Uf.T @ X) / sbs[:, None])  # noqa: E731
        probe = np.random.default_rng(1).standard_normal((fr.size, 3)).astype(LD)
        ref = A @ probe
        assert float(np.abs(mv(probe) - ref).max()) <= 1e-16 * float(np.abs(ref).max())
        return mv

    def shifted(self, d, mu, rec=False):
        """(Sigma, L-shape): Op of (B + mu I + diag d)^-1 on the free rows (d = +inf pins), its N read off solves
        against the dense reference; and the weights for the factor L.  rec: from B_rec instead of B."""
        base = self.B_rec if rec else self.B
        n = self.n
        dd = np.zeros(n) if d is None else np.asarray(d, np.float64)
        free = np.isfinite(dd)
        fr = np.flatnonzero(free)
        w = np.zeros(n, LD)
        w[free] = 1 / (self.theta + LD(mu) + dd[free].astype(LD))
        A = base.A[np.ix_(fr, fr)] + np.diag(LD(mu) + dd[fr].astype(LD))
        Sig = np.zeros((n, n), LD)
        if fr.size:
            Sig[np.ix_(fr, fr)] = ld_solve(A, np.eye(fr.size, dtype=LD), matvec=self._shift_matvec(base, A, fr, mu, dd))
        N = middle(Sig, w, w, w, self.W, rows=fr) if (self.col and fr.size) else np.zeros((2 * self.col,) * 2, LD)
        op = Op(self.W, N, w, w, w, A=Sig, g=self.g, extra=8, free=free, eta_add=base.eta_add)
        evs = np.linalg.eigvalsh(A.astype(np.float64)) if fr.size else np.ones(1)
        op.cond_a = float(evs[-1] / evs[0])
        sign, ld = np.linalg.slogdet(A.astype(np.float64)) if fr.size else (1.0, 0.0)
        op.logdet64 = float(ld)
        op.Afree, op.rows, op.w = A, fr, w
        # the forward matrix B + mu I + diag d on the free rows (quad, log_prob), and its log det in longdouble
        full = np.zeros((n, n), LD)
        full[np.ix_(fr, fr)] = A
        am = np.zeros(n, LD)
        am[fr] = 1 / w[fr]
        fm = free.astype(np.float64)
        op.fwd = Op(self.W, base.N, am, fm, fm, A=full, g=self.g, extra=8, free=free, eta_add=base.eta_add)
        op.logdet = ld_logdet(A) if fr.size else LD(0)
        op.sum_abs_log = float(np.abs(np.log(w[fr])).sum()) if fr.size else 0.0
        return op


def pos_zero(x):
    """True where x is exactly +0 (the sign bit clear)"""
    x = np.asarray(x)
    return (x == 0) & ~np.signbit(x)


RATIOS = {}


def check(tag, out, ref, bound):
    """|out - ref| <= bound entry by entry; records the worst err / bound under `tag`"""
    out = np.asarray(out, LD)
    ref = np.broadcast_to(np.asarray(ref, LD), out.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), out.shape)
    err = np.abs(out - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), worst)
    assert np.all(err <= bound), "%s: worst err / bound = %.3g (err %.3e) at %s" % (
        tag, worst, float(err.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return worst
