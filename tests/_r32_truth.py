"""REAL32 routine doors, one routine deep, against double-precision truth: TEST HELPER shared by
tests/test_r32_truth_cpu.py (are the inputs well posed, do the bars bite?) and tests/test_gpu_routines_real32.py (the
doors of a REAL32 context on them).  Nothing here calls the library.

Problems: tests/test_gpu_routines.py::_fuzz_problem with x0, l, u cast to float32; the objective is evaluated in fp64 on
the widened x and f, g are rounded to float32; factr = pgtol = 0.  States: the NEW_X returns of the REAL32 oracle's run.
From a state, the reference's sequence of calls for the next iteration (matupd + formt, cauchy, freev, formk, cmprlb,
subsm, lnsrlb set-up and one more call), as _chain_at of tests/test_gpu_routines.py builds it.  Every routine is run
twice on the SAME inputs -- the float32 outputs of the REAL32 oracle's previous routine:
  ref   through po.Routines(np.float32): the reference's own all-fp32 arithmetic (the unit of class (c), and the second
        witness for decisions);
  tru   through po.Routines(np.float64) on the inputs widened with astype(np.float64) (exact), epsmch of float32: the
        truth of the same operation.
Errors are measured in units of eps32 M, M the sum of the absolute values of the terms that form the number (longdouble,
from the same inputs), never relative to the result: rho(v) = max_i |v_i - truth_i| / (eps32 M_i).  The magnitudes:
  xcp (moving rows)      |x_i| + |xcp_i - x_i|                                   (x_i + tsum d_i)
  c of cauchy            tsum M(p_a): c_a = sum_k dt_k p_a over the segments, sum_k dt_k = tsum, and p_a is itself a sum
                         over the rows that cancels -- its terms are the products |W_ij d_i|
  p of cauchy            sum over the rows that move at the start of |W_ij d_i|  (the walk only takes terms away)
  r of cmprlb            theta |xcp_i - x_i| + |g_i| + sum_j |Wy_ij a1_j| + |Ws_ij a2_j|,  a = M c of the truth
  subspace minimiser     |xcp_i| + (|r_i| + sum_j |Wy_ij wv_j| / theta + |Ws_ij wv_col+j|) / theta, wv of the truth (the
                         step before the projection or the backtracking factor alpha <= 1 shortens it)
  trial point            |stp d_i| + |t_i|
  n-length sums          sum_i |a_i b_i|
and, where a number comes out of a triangular solve or a factorisation, whose terms are not a fixed list, the largest
entry of the truth's vector or matrix: v of cauchy, WN, the step lengths of dcsrch (largest of stx, sty, stmin, stmax,
the two widths and stp), its function values (largest |f| of the search) and its slopes (sum |g_i d_i| of the search's
calls).
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import pyoracle as po
from test_gpu_routines import Locals, _fuzz_problem, _parts

F32, F64, LD = np.float32, np.float64, np.longdouble
EPS32 = float(np.finfo(F32).eps)
SUM_BAR = 1e-12       # re-ordered fp64 sums of exact products: the project's bar (test_level1_doors, the fp64 doors)

ROUTINES = ("matupd", "cauchy", "freev", "formk", "cmprlb", "subsm", "lnsrlb", "lnsrlb2")

# seed, n, m, iterations, element offset of the caller's x / g / l / u inside a larger tensor
CASES = [
    (201, 3, 2, 8, 0),          # tiny
    (202, 63, 3, 12, 0),        # less than one wave
    (203, 257, 5, 14, 0),       # one fp32 wave trip of 4 rows per lane plus one row
    (204, 1021, 10, 16, 0),     # n mod 4 = 1
    (205, 2500, 17, 24, 0),     # MC = 20 with unused slots
    (206, 1500, 20, 26, 0),     # config 5's m
    (207, 1203, 25, 30, 0),     # update pass in two parts, n mod 4 = 3
    (208, 1100, 36, 40, 0),     # m > 32
    (209, 150001, 20, 8, 0),    # many workgroups per reduction, thousands of breakpoints
    (210, 1, 1, 6, 0),          # single row
    (211, 5, 4, 10, 0),         # tiny, converged state with r near 0
    (212, 255, 7, 14, 0),       # one row short of a wave trip
    (215, 2049, 20, 12, 1),     # x / g / l / u are views at a 4-byte offset: not 16-byte aligned (seed 213: its
                                # last row sits on a bound throughout, and a lost tail would change no sum)
]


def case_id(case):
    return "n%d_m%d" % (case[1], case[2])


def problem(seed, n, m):
    p64 = _fuzz_problem(seed, n, m)

    def fg(x, g):
        g64 = np.zeros(n)
        f = p64.fg(x.astype(F64), g64)
        g[:] = g64.astype(F32)
        return float(F32(f))
    return po.Problem("r32doors%d" % seed, n, m, p64.x0.astype(F32), p64.l.astype(F32), p64.u.astype(F32), p64.nbd,
                      0.0, 0.0, fg, F32)


@functools.lru_cache(maxsize=None)
def states(case):
    """the problem and the examined NEW_X states of its REAL32 oracle run: 0, 1, 2, 3, the middle, the last two"""
    seed, n, m, iters, _ = case
    p = problem(seed, n, m)
    st = []
    po.run(po.Engine("oracle_r32"), p, max_iter=iters,
           snapshot=lambda k, s: st.append(s.copy()) if s.task_s.startswith("NEW_X") else None)
    pick = sorted(set([0, 1, 2, 3, len(st) // 2, len(st) - 2, len(st) - 1]) & set(range(len(st))))
    return p, [st[k] for k in pick]


@functools.lru_cache(maxsize=None)
def _R(real):
    return po.Routines(real)


def rho(v, truth, M):
    """largest error of v against truth in units of eps32 M (elementwise M; M_i = 0 admits no error)"""
    v, t, M = (np.asarray(a, LD).ravel() for a in (v, truth, M))
    if v.size == 0:
        return 0.0
    err = np.abs(v - t)
    pos = M > 0
    out = np.where(pos, err / (EPS32 * np.where(pos, M, 1)), np.where(err > 0, np.inf, 0.0))
    return float(np.max(out))


def xdot(a, b):
    """sum_i a_i b_i over the last axis for float32 (or widened float32) operands -> (exact, M) in longdouble: the
    products are exact in fp64"""
    pr = np.asarray(a, F64) * np.asarray(b, F64)
    return pr.sum(axis=-1, dtype=LD), np.abs(pr).sum(axis=-1, dtype=LD)


def cols(flat, n, m, head, col):
    """the col logical columns (oldest first) of a W matrix stored as the reference stores it -> (col, n)"""
    W = np.asarray(flat).reshape(m, n)
    return W[[(head - 1 + j) % m for j in range(col)]]


def mat(a, k):
    """column-major k x k"""
    return np.asarray(a).reshape(k, k).T


# ------------------------------------------------------------------------------------------------ the routines
def _matupd(real, n, m, w, y, d_eff, ip, theta, dr, stp, dtd):
    R = _R(real)
    o = {k: np.array(w[k], dtype=real) for k in ("ws", "wy", "sy", "ss", "wt")}       # (copies: updated in place)
    y, d_eff = np.ascontiguousarray(y, real), np.ascontiguousarray(d_eff, real)
    rr = float(R.lib.lbo_ddot(n, po._ptr(y), po._ptr(y)))
    iupdat, col, head, itail = ip
    it, ic, ih = (np.array([v], np.int32) for v in (itail, col, head))
    th = np.array([theta], real)
    R.matupd(n, m, o["ws"], o["wy"], o["sy"], o["ss"], d_eff, y, it, iupdat, ic, ih, th, rr, dr, stp, dtd)
    info = np.zeros(1, np.int32)
    R.formt(m, o["wt"], o["sy"], o["ss"], int(ic[0]), float(th[0]), info)
    o.update(col=int(ic[0]), head=int(ih[0]), itail=int(it[0]), theta=float(th[0]), rr=rr, info=int(info[0]))
    return o


def _cauchy(real, p, x, g, o, iwhere, theta, col, head, sbgnrm):
    R, n, m = _R(real), p.n, p.m
    c = lambda a: np.ascontiguousarray(a, real)  # noqa: E731
    iw, xcp = iwhere.copy(), np.zeros(n, real)
    wk = [np.zeros(n, np.int32), np.zeros(n, real), np.zeros(n, real)]
    pc = [np.array(o["wa8m"][2 * m * k:2 * m * (k + 1)], dtype=real) for k in range(4)]   # (copies; stale content)
    nseg, info = np.zeros(1, np.int32), np.zeros(1, np.int32)
    R.cauchy(n, c(x), c(p.l), c(p.u), p.nbd, c(g), wk[0], iw, wk[1], wk[2], xcp, m, c(o["wy"]), c(o["ws"]), c(o["sy"]),
             c(o["wt"]), theta, col, head, pc[0], pc[1], pc[2], pc[3], nseg, sbgnrm, info, EPS32)
    return NS(nseg=int(nseg[0]), info=int(info[0]), iwhere=iw, xcp=xcp, d=wk[2], p=pc[0], c=pc[1], wbp=pc[2], v=pc[3],
              ints=(int(nseg[0]), int(info[0])) + tuple(iw))


def _formk(real, p, nfree, index, nenter, ileave, indx2, iupdat, updatd, wn, snd, o, theta, col, head):
    R, c = _R(real), (lambda a: np.ascontiguousarray(a, real))
    wn, snd = c(wn).copy(), c(snd).copy()
    info = np.zeros(1, np.int32)
    R.formk(p.n, nfree, index, nenter, ileave, indx2, iupdat, int(updatd), wn, snd, p.m, c(o["ws"]), c(o["wy"]),
            c(o["sy"]), theta, col, head, info)
    return NS(wn=wn, snd=snd, info=int(info[0]))


def _cmprlb(real, p, x, g, o, xcp, wa8, index, theta, col, head, nfree, cnstnd):
    R, c = _R(real), (lambda a: np.ascontiguousarray(a, real))
    r, wa8 = np.zeros(p.n, real), c(wa8).copy()
    info = np.zeros(1, np.int32)
    R.cmprlb(p.n, p.m, c(x), c(g), c(o["ws"]), c(o["wy"]), c(o["sy"]), c(o["wt"]), c(xcp), r, wa8, index, theta, col,
             head, nfree, int(cnstnd), info)
    return NS(r=r, wa8=wa8, info=int(info[0]))


def _subsm(real, p, x, g, o, xcp, r, wv, wn, index, theta, col, head, nfree):
    R, c = _R(real), (lambda a: np.ascontiguousarray(a, real))
    xs, ds, xps, wv = c(xcp).copy(), c(r).copy(), np.zeros(p.n, real), c(wv).copy()
    iword, info = np.zeros(1, np.int32), np.zeros(1, np.int32)
    R.subsm(p.n, p.m, nfree, index, c(p.l), c(p.u), p.nbd, xs, ds, xps, c(o["ws"]), c(o["wy"]), theta, c(x), c(g), col,
            head, iword, wv, c(wn), info)
    return NS(x=xs, d=ds, xp=xps, wv=wv, iword=int(iword[0]), info=int(info[0]), ints=(int(iword[0]), int(info[0])))


LS_NAMES = ("fold", "gd", "gdold", "stp", "dnorm", "dtd", "xstep", "stpmx")


def ls_fresh(x, nfgv):
    """the line search's variables before its set-up call"""
    n = x.size
    return NS(x=x.copy(), t=np.zeros(n, x.dtype), r=np.zeros(n, x.dtype), sc=np.zeros(8), ic=[0, 0, nfgv, 0],
              task=po.pad60("NEW_X"), csave=po.pad60(""), is2=np.zeros(2, np.int32), ds13=np.zeros(13))


def _lnsrlb(real, p, st, f, g, d, z, it, boxed, cnstnd):
    """one call of lnsrlb from the variables st (of ls_fresh, or a former call's result) -> the variables after it;
    sc = fold, gd, gdold, stp, dnorm, dtd, xstep, stpmx; ic = ifun, iback, nfgv, info"""
    R, c = _R(real), (lambda a: np.ascontiguousarray(a, real))
    x, t, r = c(st.x).copy(), c(st.t).copy(), c(st.r).copy()
    so = [np.array([v], real) for v in st.sc]
    io = [np.array([v], np.int32) for v in st.ic]
    task, csave, is2, ds13 = st.task.copy(), st.csave.copy(), st.is2.copy(), c(st.ds13).copy()
    R.lnsrlb(p.n, c(p.l), c(p.u), p.nbd, x, float(real(f)), so[0], so[1], so[2], c(g), c(d), r, t, c(z), so[3], so[4],
             so[5], so[6], so[7], it, io[0], io[1], io[2], io[3], task, int(boxed), int(cnstnd), csave, is2, ds13)
    out = NS(x=x, t=t, r=r, sc=np.array([float(v[0]) for v in so]), ic=[int(v[0]) for v in io], task=task, csave=csave,
             is2=is2, ds13=ds13)
    out.ints = tuple(out.ic) + (po.task_str(task), po.task_str(csave)) + tuple(int(v) for v in is2)
    return out


def _on_bound(p, x):
    """rows whose x sits exactly on a bound that they have"""
    l, u = p.l.astype(x.dtype), p.u.astype(x.dtype)
    return (((p.nbd == 1) | (p.nbd == 2)) & (x == l)) | (((p.nbd == 2) | (p.nbd == 3)) & (x == u))


def _ls_units(ref, tru, f_seen, Mgd):
    """truth and magnitudes of what a line-search call leaves through dcsrch: stp, and dsave13 = ginit, gtest, gx, gy,
    finit, fx, fy, stx, sty, stmin, stmax, width, width1"""
    ds = np.asarray(tru.ds13, F64)
    steps = max(float(np.max(np.abs(ds[7:13]))), abs(float(tru.sc[3])))
    M = np.concatenate([[Mgd, 1e-3 * Mgd, Mgd, Mgd], [f_seen] * 3, [steps] * 6])
    return dict(ds13=(ref.ds13, ds, M), stp=(ref.sc[3:4], tru.sc[3:4], np.array([steps])))


# ------------------------------------------------------------------------------------------------ one iteration
def wn1_exact(n, m, o, iwhere, col, head):
    """formk's inner products from the stored columns (:1756-1851): -> (exact, M), 2m x 2m, the three blocks of WN1
    that formk keeps (Y'ZZ'Y and S'AA'S lower triangles; R_z on and above, L_a below the diagonal of the third)"""
    Y, S = cols(o["wy"], n, m, head, col).astype(F64), cols(o["ws"], n, m, head, col).astype(F64)
    free = iwhere <= 0
    Yf, Sf, Sa = Y * free, S * free, S * ~free
    E, M = np.zeros((2 * m, 2 * m), LD), np.zeros((2 * m, 2 * m), LD)
    for a in range(col):
        for (A, B, r0, c0, keep) in ((Yf, Y, 0, 0, lambda b: b <= a), (Sa, S, m, m, lambda b: b <= a),
                                     (Sf, Y, m, 0, lambda b: b >= a), (Sa, Y, m, 0, lambda b: b < a)):
            e, mm = xdot(B, A[a])
            for b in range(col):
                if keep(b):
                    E[r0 + a, c0 + b], M[r0 + a, c0 + b] = e[b], mm[b]
    return E, M


def chain(p, s):
    """one iteration's routines from the REAL32 oracle's state s (a NEW_X return) -> dict routine -> record with inp
    (what the door is fed), ref, tru and, per compared class (c) number, units[key] = (the reference's values, the
    truth's, M)"""
    n, m = p.n, p.m
    L = Locals(s)
    w = _parts(s)
    out = {}
    # ------------------------------------------------------------------ mainlb :812-834 + matupd + formt
    stp, gd, gdold, dtd = F32(L.stp), F32(L.gd), F32(L.gdold), F32(L.dtd)
    y = s.g - w["r"]
    if stp == 1.0:
        dr, ddum, d_eff = gd - gdold, -gdold, w["d"].copy()
    else:
        dr, ddum, d_eff = (gd - gdold) * stp, -gdold * stp, w["d"] * stp
    assert y.dtype == F32 and d_eff.dtype == F32 and type(dr) is F32
    col, head, itail, iupdat, theta, updatd = L.col, L.head, L.itail, L.iupdat, L.theta, False
    o = dict(w)
    if dr > F32(L.epsmch) * ddum:
        updatd = True
        iupdat += 1
        args = (n, m, w, y, d_eff, (iupdat, col, head, itail), theta, float(dr), float(stp), float(dtd))
        ref, tru = _matupd(F32, *args), _matupd(F64, *args)
        del tru["ws"], tru["wy"]                     # (the columns are class (a): numpy's float32 arithmetic)
        out["matupd"] = NS(w=w, y=y, d_eff=d_eff, stp=float(stp), dr=float(dr), dtd=float(dtd),
                           ip=(iupdat, col, head, itail), ref=ref, tru=tru)
        if ref["info"] or tru["info"]:       # formt fails (near convergence): mainlb drops the pairs and starts again
            return out
        for k in ("ws", "wy", "sy", "ss", "wt"):
            o[k] = ref[k]
        col, head, itail, theta = ref["col"], ref["head"], ref["itail"], ref["theta"]
    if col == 0:
        return out
    # ------------------------------------------------------------------ cauchy
    args = (p, s.x, s.g, o, w["iwhere"], theta, col, head, L.sbgnrm)
    ref, tru = _cauchy(F32, *args), _cauchy(F64, *args)
    x64 = s.x.astype(F64)
    moving = tru.d != 0
    started = tru.xcp != x64                      # rows that move at the start: they end elsewhere (or on a bound)
    Wy, Ws = cols(o["wy"], n, m, head, col), cols(o["ws"], n, m, head, col)
    dvec = -s.g.astype(F64)
    pe = np.concatenate([xdot(Wy, dvec * moving)[0], F64(theta) * xdot(Ws, dvec * moving)[0]])
    pM = np.concatenate([xdot(Wy, dvec * started)[1], F64(theta) * xdot(Ws, dvec * started)[1]])
    c2 = slice(0, 2 * col)
    with np.errstate(divide="ignore", invalid="ignore"):     # no row moves for longer than the walk lasts
        tsum = float(np.max(np.where(started, np.abs(tru.xcp - x64) / np.abs(dvec), 0.0), initial=0.0))
    units = dict(xcp=(ref.xcp[moving], tru.xcp[moving], np.abs(x64[moving]) + np.abs(tru.xcp[moving] - x64[moving])),
                 c=(ref.c[c2], tru.c[c2], np.maximum(tsum * pM, np.abs(tru.c[c2]))))
    if tru.nseg > 1:                                         # (else v = M p of the start, a work value of f2's)
        units["v"] = (ref.v[c2], tru.v[c2], np.full(2 * col, np.max(np.abs(tru.v[c2]))))
    out["cauchy"] = NS(o=o, theta=theta, col=col, head=head, sbgnrm=L.sbgnrm, ref=ref, tru=tru, moving=moving,
                       units=units, p_exact=pe, p_M=pM, crossed=tru.nseg - 1)
    oc = dict(o)
    oc["iwhere"], oc["z"] = ref.iwhere, ref.xcp
    oc["wa8m"] = np.concatenate([ref.p, ref.c, ref.wbp, ref.v])
    # ------------------------------------------------------------------ freev
    of = dict(oc)
    of["index"], of["indx2"] = w["index"].copy(), w["indx2"].copy()
    nf, ne, il, wrk = (np.array([v], np.int32) for v in (L.nfree, 0, 0, 0))
    _R(F32).freev(n, nf, of["index"], ne, il, of["indx2"], oc["iwhere"], wrk, int(updatd), int(L.cnstnd), L.iter)
    nfree, nenter, ileave = int(nf[0]), int(ne[0]), int(il[0])
    out["freev"] = NS(oc=oc, nfree_in=L.nfree, iter=L.iter, cnstnd=L.cnstnd, updatd=updatd, index=of["index"],
                      indx2=of["indx2"], got=(nfree, nenter, ileave, bool(wrk[0])))
    if nfree == 0:
        return out
    # ------------------------------------------------------------------ formk
    ok = dict(of)
    if wrk[0]:
        args = (p, nfree, of["index"], nenter, ileave, of["indx2"], iupdat, updatd, of["wn"], of["snd"], o, theta, col,
                head)
        ref = _formk(F32, *args)                    # (the reference keeps WN1 incrementally: its WN goes on to subsm)
        assert ref.info == 0
        ok["wn"], ok["snd"] = ref.wn, ref.snd
        # the door forms WN1 from scratch: the sums themselves are its truth, and the assembly + factorisations of
        # formk on THOSE sums (nothing to update: updatd = 0, nobody enters or leaves) the truth of WN
        E, M = wn1_exact(n, m, o, oc["iwhere"], col, head)
        a0 = (p, nfree, of["index"], 0, n + 1, of["indx2"], iupdat, False, np.zeros(4 * m * m))
        fac_ref = _formk(F32, *a0, E.T.astype(F32).reshape(-1), o, theta, col, head)
        fac_tru = _formk(F64, *a0, E.T.astype(F64).reshape(-1), o, theta, col, head)
        assert fac_ref.info == 0 and fac_tru.info == 0
        up = lambda a: np.triu(mat(a, 2 * m)[:2 * col, :2 * col])  # noqa: E731
        wt_ = up(fac_tru.wn)
        out["formk"] = NS(of=of, nfree=nfree, theta=theta, col=col, head=head, wn1_exact=E, wn1_M=M,
                          units=dict(wn=(up(fac_ref.wn), wt_, np.full(wt_.shape, np.max(np.abs(wt_))))))
    # ------------------------------------------------------------------ cmprlb
    ref_xcp = oc["z"]
    args = (p, s.x, s.g, o, ref_xcp, ok["wa8m"], of["index"], theta, col, head, nfree, L.cnstnd)
    ref, tru = _cmprlb(F32, *args), _cmprlb(F64, *args)
    assert ref.info == 0 and tru.info == 0
    rows = of["index"][:nfree] - 1
    plain = (not L.cnstnd) and col > 0
    g64, xcp64 = s.g.astype(F64), ref_xcp.astype(F64)
    if plain:
        Mr = np.abs(g64[rows]).astype(LD)
    else:
        a = tru.wa8[:2 * col].astype(F64)
        Mr = (F64(theta) * np.abs(xcp64 - x64) + np.abs(g64))[rows].astype(LD)
        Mr = Mr + (np.abs(Wy[:, rows].astype(F64) * a[:col, None]).sum(axis=0, dtype=LD)
                   + np.abs(Ws[:, rows].astype(F64) * (F64(theta) * a[col:, None])).sum(axis=0, dtype=LD))
    out["cmprlb"] = NS(ok=ok, nfree=nfree, theta=theta, col=col, head=head, cnstnd=L.cnstnd, rows=rows, plain=plain,
                       ref=ref, tru=tru, units=dict(r=(ref.r[:nfree], tru.r[:nfree], Mr)))
    # ------------------------------------------------------------------ subsm
    args = (p, s.x, s.g, o, ref_xcp, ref.r, ref.wa8[:2 * m], ok["wn"], of["index"], theta, col, head, nfree)
    r_in = ref.r
    ref, tru = _subsm(F32, *args), _subsm(F64, *args)
    assert ref.info == 0 and tru.info == 0
    wv = tru.wv[:2 * col].astype(F64)
    Md = (np.abs(r_in[:nfree].astype(F64)).astype(LD)
          + np.abs(Wy[:, rows].astype(F64) * wv[:col, None]).sum(axis=0, dtype=LD) / F64(theta)
          + np.abs(Ws[:, rows].astype(F64) * wv[col:, None]).sum(axis=0, dtype=LD)) / F64(theta)
    lo, up_ = p.l.astype(F64), p.u.astype(F64)
    free = np.zeros(n, bool)
    free[rows] = True
    on_bound = free & _on_bound(p, ref.x) & _on_bound(p, tru.x)         # rows both witnesses put on a bound
    inner = free & ~_on_bound(p, tru.x)
    Mx = np.zeros(n, LD)
    Mx[rows] = np.abs(xcp64[rows]) + Md
    r_full = np.zeros(n, F32)
    r_full[rows] = r_in[:nfree]
    out["subsm"] = NS(ok=ok, nfree=nfree, theta=theta, col=col, head=head, r_full=r_full, xcp=ref_xcp, ref=ref, tru=tru,
                      free=free, on_bound=on_bound, inner=inner, bounded=bool(tru.iword),
                      units=dict(x=(ref.x[inner], tru.x[inner], Mx[inner])))
    # ------------------------------------------------------------------ lnsrlb: set-up call, then one more
    z = ref.x
    d_ls = z - s.x                                # mainlb :720-722, one float32 operation
    f_now = float(s.f[0])
    # The set-up call forms d = z - x itself (the door takes mainlb :720-722 in): the same operation in each kind, the
    # float32 difference for the reference, the (exact) double one for the truth -- as the door's kernel sums the
    # unrounded difference (lnsrlb_begin_kernel), so that a row that goes to its bound has (l - x) / d = 1 exactly
    dx = z.astype(F64) - x64
    a0 = (p, ls_fresh(s.x, L.nfgv), f_now, s.g)
    a1 = (z, L.iter, L.boxed, L.cnstnd)
    ref, tru = _lnsrlb(F32, *a0, d_ls, *a1), _lnsrlb(F64, *a0, dx, *a1)
    dtd_e, dtd_M = xdot(dx, dx)
    gd_e, gd_M = xdot(g64, dx)
    stpmx_e = None
    if L.cnstnd and L.iter != 0:
        lo_, up2 = (lo - x64).astype(LD), (up_ - x64).astype(LD)
        dl = dx.astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where((dl < 0) & (p.nbd != 0) & (p.nbd <= 2), np.where(lo_ >= 0, 0.0, lo_ / dl),
                         np.where((dl > 0) & (p.nbd >= 2), np.where(up2 <= 0, 0.0, up2 / dl), np.inf))
        stpmx_e = min(LD(1.0e10), np.min(q))
    units = _ls_units(ref, tru, abs(f_now), float(gd_M))
    out["lnsrlb"] = NS(ol=dict(ok, z=z), nfree=nfree, z=z, d=d_ls, f=f_now, iter=L.iter, nfgv=L.nfgv, boxed=L.boxed,
                       cnstnd=L.cnstnd, ref=ref, tru=tru, units=units, dtd=(dtd_e, dtd_M), gd=(gd_e, gd_M),
                       stpmx=stpmx_e)
    if po.task_str(ref.task).startswith("FG_LN") and ref.ic[3] == 0:
        g2 = np.zeros(n, F32)
        f2 = p.fg(ref.x.copy(), g2)
        first = ref
        a1 = (p, first, f2, g2, d_ls, z, L.iter, L.boxed, L.cnstnd)
        ref, tru = _lnsrlb(F32, *a1), _lnsrlb(F64, *a1)
        gd2_e, gd2_M = xdot(g2, d_ls)
        units = _ls_units(ref, tru, max(abs(f_now), abs(f2)), float(max(gd_M, gd2_M)))
        if tru.sc[3] != 1.0:
            units["x"] = (ref.x, tru.x, np.abs(tru.sc[3] * d_ls.astype(F64)) + np.abs(first.t.astype(F64)))
        out["lnsrlb2"] = NS(first=first, f=f2, g=g2, ref=ref, tru=tru, units=units, gd=(gd2_e, gd2_M))
    return out


def rho_ref(rec):
    """the REAL32 oracle's rho on a record, per compared number"""
    return {k: rho(r, t, M) for k, (r, t, M) in rec.units.items()}


class Tally:
    """per case: routine -> states examined, worst rho_ref, worst rho_gpu, bar, states decided by the REAL32 oracle
    only"""

    def __init__(self, name):
        self.name = name
        self.rows = {k: dict(states=0, rho_ref=0.0, rho_gpu=0.0, bar=0.0, r32_only=0, ints_equal=0) for k in ROUTINES}
        self.bounded = 0

    def add(self, routine, rho_ref_=0.0, rho_gpu=0.0, bar=0.0, r32_only=False, ints_equal=True):
        r = self.rows[routine]
        r["states"] += 1
        r["r32_only"] += int(r32_only)
        r["ints_equal"] += int(ints_equal)
        for k, v in (("rho_ref", rho_ref_), ("rho_gpu", rho_gpu), ("bar", bar)):
            r[k] = max(r[k], v)

    def table(self, gpu=True):
        lines = ["%s: routine    states  ints=truth   rho_ref%s"
                 % (self.name, "   rho_gpu       bar  by REAL32 only" if gpu else "")]
        for k in ROUTINES:
            r = self.rows[k]
            lines.append("   %-10s %6d %11d %9.3g" % (k, r["states"], r["ints_equal"], r["rho_ref"])
                         + ("%10.3g %9.3g %15d" % (r["rho_gpu"], r["bar"], r["r32_only"]) if gpu else ""))
        lines.append("   bounded subsm in %d states" % self.bounded)
        return "\n".join(lines)
