"""The model along a path of shifts in extended precision, on top of tests/_qn_truth.py (unchanged): for a Truth, a pin
mask and a shift mu, `shifted(tr, pin, mu)` is Truth.shifted(d, mu) with d = +inf on the pinned rows and 0 elsewhere --
Sigma = (B_FF + mu I)^-1 dense by refined solves, its N read off it, and the bounds of _qn_truth.py for the solve
(bound_apply), v'x (bound_quad) and log det (bound_logdet).  What the path adds is ||x||^2, x = Sigma v.

||x||^2 = v'Sigma^2 v, and with w = 1 / (theta + mu) on the free rows, R = [S, Y]_F and G_F = R'R
  Sigma^2 = diag(w^2) + diag(w) R (2 w N + w^2 N G_F N) R' diag(w)
(the reference value is x'x of the reference's own x = Sigma v).  The library does not apply Sigma twice, so the bound
is not bound_quad of an Op of that shape but follows the sums the library does form:
  ||x||^2 = w^2 (vv + 2 c'p + c'G_F c),   vv = sum_F v^2,  p = R'v,  c = N (w p)
on the host from sums that the device reduced.  THE BOUND (`bound_norm2`), a priori and from absolute values as in
_qn_truth.py, with q = |R|'|v_F| >= |p|, |G| = |R|'|R| >= |G_F| entry by entry and cb = w |N| q >= |c|:
  * p, vv and the entries of G_F are n-term sums in any order: gamma_n q, gamma_n vv, gamma_n |G|;
  * c^ - c = N w (p^ - p) + (N^ - N) w p =: dc, at most dc1 = gamma_n cb entry by entry plus dc2 = eta |N|_2 w |q|_2 in
    the 2-norm, eta the host step's of _qn_truth.py for the factorisation whose inverse N is;
  * the factor enters twice, through c'p and through c'G_F c: to first order 2 dc'p + 2 dc'G_F c = 2 dc'(p + G_F c), and
    p + G_F c = T'p with T = I + w N G_F, a matrix of the reference (Sigma R = w R T: the part of R that the solve
    leaves) -- so |2 dc'(p + G_F c)| <= 2 (dc1'|T'| q + dc2 |T|_2 |q|_2): eta doubled, not squared;
  * p^ - p directly in c'p: 2 gamma_n cb'q; the rounding of G_F in c'G_F c: gamma_n cb'|G| cb;
  * w is 1 / (theta + mu) with theta a ratio of n-term sums: w^2 carries 2 gamma_(n+4);
  * the host's dot products of 2col terms and the final products: gamma_(2d+10) of the absolute value of every term.
  bound = w^2 [ gamma_(n+2) vv + 2 (dc1'|T'| q + dc2 |T|_2 |q|_2) + 2 gamma_n cb'q + gamma_n cb'|G| cb ]
          + (2 gamma_(n+4) + gamma_(2d+10)) w^2 (vv + 2 cb'q + cb'|G| cb).
No constant is fitted; if a correct result breaks the bound, the derivation is what is wrong.

CASES lists the (state, mask, shifts) of the dense-truth cases of tests/test_gpu_qn_path.py; tests/
test_qn_path_truth_cpu.py shows on the CPU that these bounds can tell a wrong shift apart on each of them."""
import numpy as np

import _qn_truth as qt

LD = qt.LD
gamma = qt.gamma


def pin_mask(n, kind):
    """the pinned rows of a mask by name"""
    pin = np.zeros(n, bool)
    if kind == "half":
        pin[::2] = True
    elif kind == "all":
        pin[:] = True
    elif kind == "one_free":
        pin[:] = True
        pin[n // 2] = False
    elif kind == "tile_edges":  # the first and last rows of every 128-row tile
        pin[0::128] = True
        pin[127::128] = True
        pin[n - 1] = True
    else:
        assert kind == "none"
    return pin


def shifted(tr, pin, mu):
    """Truth.shifted for the diagonal d in {0, +inf}, against the recursion (REAL32: with the fp32 allowance); memoised
    on the Truth"""
    memo = tr.__dict__.setdefault("_path_ops", {})
    key = (pin.tobytes(), float(mu))
    if key not in memo:
        memo[key] = tr.shifted(np.where(pin, np.inf, 0.0), mu, rec=True)
    return memo[key]


def norm2(op, v):
    """||Sigma v||^2 in longdouble"""
    x = op.apply(np.asarray(v)[None])[0]
    return x @ x


def bound_norm2(op, v):
    fr = op.rows
    if not fr.size:
        return 0.0
    n, d = op.nt, op.d
    w = float(op.w[fr[0]])
    va = np.abs(np.asarray(v, np.float64))[fr]
    vv = float(va @ va)
    R = op.absW[fr]
    q = R.T @ va
    G = R.T @ R
    cb = w * (op.absN @ q)
    qn = float(np.sqrt(q @ q))
    dc1 = gamma(n) * cb
    dc2 = op.eta * op.n2 * w * qn
    Gc = G @ cb
    size = vv + 2 * float(cb @ q) + float(cb @ Gc)
    Rf = op.W[fr]
    T = (np.eye(d, dtype=LD) + op.w[fr[0]] * (op.N @ (Rf.T @ Rf))).astype(np.float64)
    t2 = float(np.linalg.norm(T, 2)) if d else 0.0
    err = gamma(n + 2) * vv + 2 * (float(dc1 @ (np.abs(T).T @ q)) + dc2 * t2 * qn) + 2 * gamma(n) * float(cb @ q) \
        + gamma(n) * float(cb @ Gc)
    return w * w * (err + (2 * gamma(n + 4) + gamma(2 * d + 10)) * size)


# (n, m, npairs, family, real) as tests/test_gpu_qn_switches.py's _import takes it, the mask, the shifts, the offset of
# out in elements.  Every n in {1, 63, 130, 257, 400}, every col in {0, 1, 5, 6, 10, 11, 16, 17, 33} (every qn_mc
# capacity; 1, 2 and 3 tiles), every k in {1, 2, 7, 64} and each of the five masks appear; the pairs that decide a
# code path are all there -- (k, tiles) with k = 64 on 1, 2 and 3 tiles, (k, kind), (mask, kind), (offset, tiles),
# (tiles, kind) -- while (n, col) is NOT covered pairwise (45 pairs; n enters the kernels only through the trip count
# and the tail, which every col class meets at two sizes at least).  No shift is 0: a shift and
# its neighbour mu (1 + 1e-6) must differ.  mu = -0.3 is negative and inside the positive definite range of every state
# (the families' curvatures lie in [0.5, 4]).
MUS = {1: [2.0], 2: [-0.3, 5.0], 7: [-0.3, 0.1, 0.3, 1.0, 5.0, 70.0, 4e4],
       64: list(np.geomspace(1.0, 1e4, 64))}
F64, F32 = np.float64, np.float32
# REAL32 states: the bounds of their Truth carry the 2^-24 rounding of the imported middle matrix, which enters the solve
# through the pairs' part of Sigma alone; that part falls off like theta / mu against the diagonal part, so from
# mu = MU32_SEES on a shift 1e-6 off is outside the bounds of the solve and of ||x||^2 (tests/
# test_qn_path_truth_cpu.py asserts it for every such shift).  Every REAL32 list has such shifts, next to small ones
# that keep the pairs' part large in the entry-by-entry check.
MU32_SEES = 1e4
MUS32 = {2: [-0.3, 2e4], 7: [-0.3, 0.3, 5.0, 1e4, 2e4, 4e4, 1e5], 64: list(np.geomspace(1.0, 1e5, 64))}


def shifts(case):
    """the shift list of a case"""
    state, _, k, _ = case
    return (MUS32 if state[4] == F32 else MUS)[k]


def sees(case, mu):
    """whether the Truth bounds of the case's state can tell mu (1 + 1e-6) from mu in the solve and in ||x||^2 (log det:
    every shift, REAL32 through the route comparison)"""
    return case[0][4] == F64 or mu >= MU32_SEES


CASES = [
    ((1, 1, 0, "dyadic", F64), "none", 2, 0),
    ((1, 1, 0, "dyadic", F64), "all", 1, 1),
    ((63, 1, 1, "generic", F64), "half", 64, 1),
    ((63, 5, 0, "dyadic", F32), "one_free", 7, 0),   # (one free row determines no N: the dense truth has no pair here;
    ((130, 5, 0, "generic", F64), "one_free", 1, 1),  #  one free row WITH pairs is held to the qn_shift route instead)
    ((63, 16, 16, "generic", F64), "none", 2, 1),   # (2 col <= the free rows everywhere: [S, Y]_F has full rank)
    ((130, 6, 6, "generic", F64), "tile_edges", 7, 1),
    ((130, 10, 17, "dyadic", F32), "half", 2, 0),
    ((130, 11, 11, "dyadic", F64), "all", 2, 0),
    ((130, 17, 17, "generic", F64), "half", 1, 1),
    ((257, 5, 8, "generic", F64), "tile_edges", 2, 0),
    ((257, 16, 16, "generic", F64), "half", 7, 1),
    ((257, 17, 20, "generic", F32), "none", 7, 1),
    ((257, 33, 40, "dyadic", F64), "tile_edges", 1, 0),
    ((400, 10, 10, "generic", F64), "none", 1, 0),
    ((400, 33, 33, "generic", F64), "half", 2, 1),
    # the corners of the cap: k = 64 on 2 and 3 tiles (the later tiles read 64 partial outputs back), at an odd
    # offset, in REAL32
    ((130, 17, 17, "generic", F64), "none", 64, 1),
    ((130, 33, 33, "generic", F64), "tile_edges", 64, 0),
    ((130, 17, 20, "dyadic", F32), "half", 64, 1),
]


_STATES = {}


def state_truth(state):
    """(the synthetic state, its Truth) as tests/test_gpu_qn_switches.py's _import makes them, once per state"""
    import _qn_synth as qs
    if state not in _STATES:
        n, m, npairs, fam, real = state
        st = qs.synth(n, m, npairs, fam, real)
        S, Y = st.pairs()
        r32 = (st.mats("sy"), st.mats("wt")) if real == np.float32 else None
        theta = None
        if r32 is not None and st.col:  # (the context's theta: y'y over the imported fp32 s'y)
            y = Y[:, -1].astype(LD)
            theta = (y @ y) / LD(r32[0][st.col - 1, st.col - 1])
        _STATES[state] = (st, qt.Truth(S, Y, theta=theta, real32=r32, sy_exact=fam == "dyadic"))
    return _STATES[state]


def route_truth(state):
    """The Truth whose bounds hold the path against the qn_shift route.  Both routes run the same fp64 algebra on the
    same stored pairs and the same host matrices (in a REAL32 context: M^-1 from the Gram of the stored fp32 pairs)
    and differ in the order of their fp64 sums and in w G_F against a weighted Gram, so each is within the fp64 bound
    of the value they share -- the fp32 allowance of the imported middle matrix, which the reference of a REAL32 state
    carries in eta, is common to both and drops out of their difference.  fp64 states: the state's own Truth; REAL32:
    a Truth of the same pairs and theta without that allowance (its outputs still carry the 2^-24 of the store)."""
    st, tr = state_truth(state)
    if tr.real32 is None:
        return tr
    key = state + ("route",)
    if key not in _STATES:
        _STATES[key] = qt.Truth(tr.S, tr.Y, theta=tr.theta)
    return _STATES[key]


def case_id(c):
    (n, m, npairs, fam, real), mask, k, off = c
    return "n%d-m%d-pairs%d-%s-%s-%s-k%d-off%d" % (n, m, npairs, fam, "fp32" if real == F32 else "fp64", mask, k, off)
