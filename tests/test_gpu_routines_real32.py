"""The routine doors of a REAL32 context (fp32 storage and kernels, fp64 partial sums and host algebra:
include/lbfgsb_hip.h) ONE ROUTINE deep against double-precision truth, at the shapes where the float instantiations have
their tails: tests/_r32_truth.py builds the states, the inputs of every routine (the REAL32 oracle's outputs of the
previous one), the truth (the fp64 oracle routine on the widened inputs), the REAL32 oracle's own result and the
magnitudes M; tests/test_r32_truth_cpu.py shows on the CPU that the inputs are well posed and that the bars reject a
lost tail and an fp32 accumulator.

Decisions (nseg, info, iwhere; iword; ifun, iback, nfgv, info, task, csave, isave of dcsrch) equal the truth's or the
REAL32 oracle's; where they equal only the latter, the floats of that routine are left out in that state (at most 1 in
4 per case, 1 in 10 overall -- asserted).  freev's and matupd's integers follow from integers: equal, always.

Class (a), bit for bit: integers, Index, Indx2, iwhere, strings, ip of matupd; t = x, r = g, xp = xcp; rows of xcp and
of the subspace minimiser that do not move or sit on a bound; r = 0 off the free rows, r = -g where cmprlb has nothing
to add; the columns of W and the entries of Sy, Ss that matupd only moves; wbp (a row of W, its S half times theta: the
product of two float32 is exact in double, its one rounding is numpy's); the new columns wy = g - r, ws = stp d and
d = z - x equal numpy's float32 arithmetic -- the kernels form them in fp64 and round once (pend_y / pend_s,
kernels_common.hpp:205-211; lnsrlb_begin_kernel, k_misc.hip:812-826), which for one +, - or * of two float32 is the
float32 operation itself (53 >= 2 * 24 + 2 bits).  Ss's new diagonal entry, stp^2 dtd for stp != 1, is formed in double
and rounded once (matupd_small, solver.hip:1552): half an fp32 ulp of the truth, not the reference's two roundings.

Class (b), the contract -- n-length sums of products of stored float32 numbers, exact in fp64, so that only the fp64
summation error remains: |got - exact| <= 1e-12 M for the sums that come back as doubles (theta dr = y'y; dtd, gd, stpmx
of the line search; projgr), + eps32 |exact| for those seen through the float32 export (the new row of Sy and column of
Ss, the WN1 blocks of formk, p of cauchy).  The operands are the door's own: the columns it stored (export), and for
dtd / gd / stpmx of the set-up call the z and x it read -- lnsrlb_begin_kernel sums the UNROUNDED d = z - x
(k_misc.hip:812-814), so that a row that goes to its bound has (l - x) / d = 1 exactly.  projgr comes back as the
double it was formed in: equal to numpy's fp64 arithmetic on the widened operands, and its float32 rounding to the
REAL32 oracle's.

Class (c), through a solve or per-row arithmetic: rho_gpu <= max(4 rho_ref, floor), rho in units of eps32 M
(_r32_truth.py), rho_ref the REAL32 oracle's on the same state, floor = the fp32 roundings of the door's expression + 2:
  xcp, moving rows     1 + 2   x + tsum d in double, rounded by xcp_free (kernels_common.hpp:483)
  c, v of cauchy       1 + 2   host doubles (solver_walk.inl:489-510), rounded by the export (solver_state.inl:23-36)
  WN                   1 + 2   host doubles (formk_factor, solver_subspace.inl), rounded by the export
  r of cmprlb          1 + T + 2   cmprlb_init_kernel's store (k_wide.hip:409) and one store per tile of 32 columns
                       (tile_axpy_kernel, k_wide.hip:61-67), T = ceil(col / 32)
  subspace minimiser   T + 2 + 2   the tiles' stores of the direction, its store scaled by 1 / theta (k_wide.hip:436,
                       read again by the backtracking branch, k_misc.hip:766) and the store of z (k_wide.hip:454 /
                       k_misc.hip:779): the longer of the two branches
  stp, dsave13         0 + 2   host doubles from fp64 sums
  trial point          1 + 2   stp d + t in double, one store (lnsrlb_step_kernel, k_misc.hip:858)
Wt is not compared: no door runs formt (r_matupd leaves it to the caller, as mainlb does).  p of cauchy is class (b):
the host keeps it in double from the fp64 sums and takes the crossed rows' terms away again.
"""
import numpy as np
import pytest

import _r32_truth as rt
from _r32_truth import EPS32, F32, F64, LD, SUM_BAR, mat
from oracle import pyoracle as po
from test_gpu_routines import _pack, _parts

pytestmark = pytest.mark.gpu

TOTAL = dict(decided=0, r32_only=0, cases=0)


class _Ctx:
    """a REAL32 context that mirrors the reference's lists, the problem's vectors on the device"""

    def __init__(self, p, offset):
        import torch
        import lbfgsb_amd
        self.torch, self.p, self.offset = torch, p, offset
        self.dev = torch.device("cuda", 0)
        self.sol = lbfgsb_amd.DeviceSolver(p.n, p.m, device=0, real32=True, mirror_index=True)
        self.l, self.u = self.vec(p.l), self.vec(p.u)
        self.nbd = torch.from_numpy(np.ascontiguousarray(p.nbd, np.int32)).to(self.dev)

    def vec(self, a):
        """a float32 vector on the device; offset != 0: a view that many elements into a larger tensor"""
        a = np.ascontiguousarray(a, F32)
        if not self.offset:
            return self.torch.from_numpy(a).to(self.dev)
        big = self.torch.zeros(a.size + 8, dtype=self.torch.float32, device=self.dev)
        v = big[self.offset:self.offset + a.size]
        v.copy_(self.torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * self.offset
        return v

    def imp(self, s, parts, nfree=None):
        wa, iwa = _pack(s, parts)
        isv = s.isave.astype(np.int32)
        if nfree is not None:
            isv[37] = nfree
        self.sol.import_state(wa, iwa, isv)

    def exp(self, s):
        wa, iwa = self.sol.export_state()
        assert wa.dtype == F32
        st = s.copy()
        st.wa, st.iwa = wa, iwa
        return _parts(st)


def _class_c(T, routine, rec, got, floor, tag):
    """rho_gpu <= max(4 rho_ref, floor) for every compared number of the record; -> (rho_ref, rho_gpu, bar), the
    worst"""
    worst = (0.0, 0.0, 0.0)
    for k, (r, t, M) in rec.units.items():
        rr, rg = rt.rho(r, t, M), rt.rho(got[k], t, M)
        fl = floor[k] if isinstance(floor, dict) else floor
        bar = max(4.0 * rr, fl)
        assert rg <= bar, "%s %s %s: rho_gpu %.3g > max(4 rho_ref = %.3g, floor %g)" % (tag, routine, k, rg, 4 * rr, fl)
        if rg >= worst[1]:
            worst = (rr, rg, bar)
    return worst


def _sum_bar(got, exact, M, exported, what):
    got, exact, M = (np.asarray(a, LD) for a in (got, exact, M))
    bound = SUM_BAR * M + (EPS32 * np.abs(exact) if exported else 0)
    err = np.atleast_1d(np.abs(got - exact))
    bad = err > bound
    assert not np.any(bad), "%s: |got - exact| %.3e > %.3e" % (what, float(err[bad][0]),
                                                               float(np.atleast_1d(bound)[bad][0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(M > 0, err / (EPS32 * M), 0.0), initial=0.0))


def _decided(T, routine, got, rec, tag):
    """the door's decisions equal the truth's or the REAL32 oracle's; -> they equal the truth's"""
    eq_t, eq_r = got == rec.tru.ints, got == rec.ref.ints
    assert eq_t or eq_r, "%s %s: decisions match neither the truth nor the REAL32 oracle" % (tag, routine)
    TOTAL["decided"] += 1
    TOTAL["r32_only"] += int(not eq_t)
    if not eq_t:
        T.add(routine, r32_only=True, ints_equal=False)
    return eq_t


def _chain_doors(C, T, s, ch, tag):
    """the doors on the records of one state"""
    p, sol = C.p, C.sol
    n, m = p.n, p.m
    xd, gd_ = C.vec(s.x), C.vec(s.g)
    out32 = lambda: C.vec(np.full(n, 9.0, F32))  # noqa: E731
    host = lambda t: t.cpu().numpy()  # noqa: E731
    # ------------------------------------------------------------------ matupd
    if "matupd" in ch:
        rec = ch["matupd"]
        ref, tru = rec.ref, rec.tru
        C.imp(s, rec.w)
        ip = np.array(rec.ip, np.int32)
        th_g = sol.r_matupd(gd_, rec.stp, rec.dr, rec.dtd, ip)
        e = C.exp(s)
        col, head = ref["col"], ref["head"]
        assert list(ip) == [rec.ip[0], col, head, ref["itail"]]
        slot = slice((ref["itail"] - 1) * n, ref["itail"] * n)
        y_g, s_g = e["wy"][slot], e["ws"][slot]
        assert np.array_equal(y_g, rec.y), tag + " wy = g - r is not numpy's float32 difference"
        assert np.array_equal(s_g, rec.d_eff), tag + " ws = stp d is not numpy's float32 product"
        assert np.array_equal(e["ws"], ref["ws"]) and np.array_equal(e["wy"], ref["wy"]), tag + " other W columns"
        SYg, SSg, SYr, SSr = (mat(a, m) for a in (e["sy"], e["ss"], ref["sy"], ref["ss"]))
        k = col - 1
        assert np.array_equal(np.tril(SYg[:k, :k]), np.tril(SYr[:k, :k])), tag + " Sy's old entries"
        assert np.array_equal(np.triu(SSg[:k, :k]), np.triu(SSr[:k, :k])), tag + " Ss's old entries"
        assert SYg[k, k] == F32(rec.dr) and SSg[k, k] == F32(mat(tru["ss"], m)[k, k]), tag + " diagonal entries"
        Wy, Ws = rt.cols(e["wy"], n, m, head, col), rt.cols(e["ws"], n, m, head, col)
        yy, yyM = rt.xdot(y_g, y_g)
        _sum_bar(th_g * rec.dr, yy, yyM, False, tag + " theta dr = y'y")
        rg = max(_sum_bar(SYg[k, :k], *(a[:k] for a in rt.xdot(Wy, s_g)), True, tag + " new row of Sy"),
                 _sum_bar(SSg[:k, k], *(a[:k] for a in rt.xdot(Ws, s_g)), True, tag + " new column of Ss"))
        e_, M_ = rt.xdot(Wy, s_g)
        T.add("matupd", rt.rho(SYr[k, :k], e_[:k], M_[:k]), rg, 0.0)
    # ------------------------------------------------------------------ cauchy
    if "cauchy" in ch:
        rec = ch["cauchy"]
        ref, tru, col, c2 = rec.ref, rec.tru, rec.col, slice(0, 2 * rec.col)
        C.imp(s, rec.o)
        xcp_d = out32()
        ns, inf = sol.r_cauchy(xd, C.l, C.u, C.nbd, gd_, rec.theta, col, rec.head, rec.sbgnrm, xcp_d)
        e = C.exp(s)
        got = host(xcp_d)
        assert np.array_equal(e["z"], got), tag + " z = xcp"
        if _decided(T, "cauchy", (ns, inf) + tuple(e["iwhere"]), rec, tag):
            still = ~rec.moving
            assert np.array_equal(got[still], tru.xcp[still].astype(F32)), \
                tag + " a row of xcp that does not move, or sits on a bound, is not bit-equal to x / the bound"
            w8 = e["wa8m"]
            if rec.crossed > 0:
                assert np.array_equal(w8[4 * m:4 * m + 2 * col], tru.wbp[c2].astype(F32)), tag + " wbp"
            _sum_bar(w8[c2], rec.p_exact, rec.p_M, True, tag + " p of cauchy")
            T.add("cauchy", *_class_c(T, "cauchy", rec, dict(xcp=got[rec.moving], c=w8[2 * m:2 * m + 2 * col],
                                                             v=w8[6 * m:6 * m + 2 * col]), 3, tag))
    # ------------------------------------------------------------------ freev
    if "freev" in ch:
        rec = ch["freev"]
        nfree, nenter, ileave, wrk = rec.got
        C.imp(s, rec.oc, nfree=rec.nfree_in)
        got = sol.r_freev(rec.iter, rec.cnstnd, rec.updatd)
        e = C.exp(s)
        if rec.iter > 0 and rec.cnstnd:
            assert got == rec.got, (tag, got, rec.got)
            assert np.array_equal(e["indx2"][:nenter], rec.indx2[:nenter]), tag + " entering variables"
            assert np.array_equal(e["indx2"][ileave - 1:], rec.indx2[ileave - 1:]), tag + " leaving variables"
        else:
            assert got[0] == nfree and got[3] == wrk
        assert np.array_equal(e["index"], rec.index), tag + " Index"
        T.add("freev")
    # ------------------------------------------------------------------ formk
    if "formk" in ch:
        rec = ch["formk"]
        col = rec.col
        C.imp(s, rec.of, nfree=rec.nfree)
        assert sol.r_formk(col, rec.head, rec.theta) == 0
        e = C.exp(s)
        G = mat(e["snd"], 2 * m)
        low = np.tril(np.ones((col, col), bool))
        rg = 0.0
        for (r0, c0, sel) in ((0, 0, low), (m, m, low), (m, 0, np.ones((col, col), bool))):
            blk = (slice(r0, r0 + col), slice(c0, c0 + col))
            rg = max(rg, _sum_bar(G[blk][sel], rec.wn1_exact[blk][sel], rec.wn1_M[blk][sel], True,
                                  tag + " WN1 block (%d, %d)" % (r0, c0)))
        worst = _class_c(T, "formk", rec, dict(wn=np.triu(mat(e["wn"], 2 * m)[:2 * col, :2 * col])), 3, tag)
        T.add("formk", worst[0], max(worst[1], rg), worst[2])
    # ------------------------------------------------------------------ cmprlb
    if "cmprlb" in ch:
        rec = ch["cmprlb"]
        rows = rec.rows
        C.imp(s, rec.ok, nfree=rec.nfree)
        r_d = out32()
        assert sol.r_cmprlb(xd, gd_, rec.theta, rec.col, rec.head, rec.cnstnd, r_d) == 0
        got = host(r_d)
        mask = np.zeros(n, bool)
        mask[rows] = True
        assert not got[~mask].any(), tag + " r off the free rows"
        if rec.plain:
            assert np.array_equal(got[rows], -s.g[rows]), tag + " r = -g"
        T.add("cmprlb", *_class_c(T, "cmprlb", rec, dict(r=got[rows]), 1 + -(-rec.col // 32) + 2, tag))
    # ------------------------------------------------------------------ subsm
    if "subsm" in ch:
        rec = ch["subsm"]
        C.imp(s, rec.ok, nfree=rec.nfree)
        xh_d = out32()
        iw_g, inf_g = sol.r_subsm(xd, C.l, C.u, C.nbd, gd_, C.vec(rec.r_full), rec.theta, rec.col, rec.head, xh_d)
        e = C.exp(s)
        got = host(xh_d)
        assert np.array_equal(e["xp"], rec.xcp), tag + " xp = xcp"
        assert np.array_equal(e["z"], got), tag + " z = the subspace minimiser"
        assert np.array_equal(got[~rec.free], rec.xcp[~rec.free]), tag + " rows outside the subspace moved"
        T.bounded += int(rec.bounded)
        if _decided(T, "subsm", (iw_g, inf_g), rec, tag):
            assert np.array_equal(got[rec.on_bound], rec.tru.x[rec.on_bound].astype(F32)), \
                tag + " a row that subsm puts on a bound is not bit-equal to it"
            T.add("subsm", *_class_c(T, "subsm", rec, dict(x=got[rec.inner]), -(-rec.col // 32) + 2 + 2, tag))
    # ------------------------------------------------------------------ lnsrlb: set-up call, then one more
    if "lnsrlb" in ch:
        rec = ch["lnsrlb"]
        C.imp(s, rec.ol, nfree=rec.nfree)
        x_g = C.vec(s.x)
        sc = np.zeros(8)
        ic = np.array([rec.iter, 0, 0, rec.nfgv, 0, int(rec.boxed), int(rec.cnstnd)], np.int32)
        task_g, csave_g = po.pad60("NEW_X"), po.pad60("")
        is2_g, ds13_g = np.zeros(2, np.int32), np.zeros(13)

        def ints():
            return tuple(int(v) for v in ic[1:5]) + (po.task_str(task_g), po.task_str(csave_g)) \
                + tuple(int(v) for v in is2_g)

        def trial(r):
            xg = host(x_g)
            if po.task_str(task_g).startswith("FG_LN") and sc[3] == 1.0:
                assert np.array_equal(xg, rec.z), tag + " a unit step's trial point is not bit-equal to z"
            return xg
        sol.r_lnsrlb(x_g, C.l, C.u, C.nbd, gd_, rec.f, sc, ic, task_g, csave_g, is2_g, ds13_g)
        e = C.exp(s)
        assert np.array_equal(e["t"], s.x) and np.array_equal(e["r"], s.g), tag + " t = x, r = g"
        assert np.array_equal(e["d"], rec.d), tag + " d = z - x is not numpy's float32 difference"
        _sum_bar(sc[5], *rec.dtd, False, tag + " dtd")
        _sum_bar(sc[1], *rec.gd, False, tag + " gd")
        if rec.stpmx is not None:
            _sum_bar(sc[7], rec.stpmx, abs(rec.stpmx), False, tag + " stpmx")
        else:
            assert sc[7] == (1.0 if rec.cnstnd else 1.0e10)
        dn = float(np.sqrt(rec.dtd[0]))
        assert sc[0] == rec.f and sc[2] == sc[1] and abs(sc[4] - dn) <= SUM_BAR * dn
        assert ic[4] != 0 or abs(sc[6] - sc[3] * sc[4]) <= SUM_BAR * abs(sc[6]), tag + " xstep"
        if _decided(T, "lnsrlb", ints(), rec, tag):
            trial(rec)
            T.add("lnsrlb", *_class_c(T, "lnsrlb", rec, dict(ds13=ds13_g, stp=sc[3:4]), 2, tag))
        if "lnsrlb2" in ch:
            # one more call, from the REAL32 oracle's variables after the set-up call (d, t, z: the context's own,
            # bit-equal to them as just asserted)
            rec2, first = ch["lnsrlb2"], ch["lnsrlb2"].first
            x_g = C.vec(first.x)
            sc[:] = first.sc
            ic[1:5] = first.ic
            task_g[:], csave_g[:], is2_g[:], ds13_g[:] = first.task, first.csave, first.is2, first.ds13
            sol.r_lnsrlb(x_g, C.l, C.u, C.nbd, C.vec(rec2.g), rec2.f, sc, ic, task_g, csave_g, is2_g, ds13_g)
            _sum_bar(sc[1], *rec2.gd, False, tag + " gd of the second call")
            if _decided(T, "lnsrlb2", ints(), rec2, tag):
                xg = trial(rec2)
                T.add("lnsrlb2", *_class_c(T, "lnsrlb2", rec2, dict(ds13=ds13_g, stp=sc[3:4], x=xg),
                                           dict(ds13=2, stp=2, x=3), tag))


@pytest.mark.parametrize("case", rt.CASES, ids=[rt.case_id(c) for c in rt.CASES])
def test_real32_routine_doors(oracle_built, case):
    p, sts = rt.states(case)
    T = rt.Tally(rt.case_id(case))
    before = dict(TOTAL)
    C = _Ctx(p, case[4])
    try:
        for k, s in enumerate(sts):
            _chain_doors(C, T, s, rt.chain(p, s), "%s state %d (iteration %d):" % (T.name, k, int(s.isave[29])))
    finally:
        C.sol.close()
    print("\n" + T.table())
    TOTAL["cases"] += 1
    decided, r32_only = TOTAL["decided"] - before["decided"], TOTAL["r32_only"] - before["r32_only"]
    assert 4 * r32_only <= decided, "%d of %d decisions follow the REAL32 oracle only" % (r32_only, decided)
    need = 3 if p.n >= 63 else 1
    for r in ("matupd", "cauchy", "freev", "formk", "cmprlb", "subsm", "lnsrlb"):
        assert T.rows[r]["states"] >= need, (r, T.rows[r])


def test_states_left_out_overall():
    """over all cases of test_real32_routine_doors that ran in this session: at most 1 decision in 10 is the REAL32
    oracle's alone"""
    assert TOTAL["cases"] > 0, "runs behind test_real32_routine_doors"
    print("\ndecisions %d, by the REAL32 oracle only %d (%d cases)"
          % (TOTAL["decided"], TOTAL["r32_only"], TOTAL["cases"]))
    assert 10 * TOTAL["r32_only"] <= TOTAL["decided"], TOTAL


@pytest.mark.parametrize("case", rt.CASES, ids=[rt.case_id(c) for c in rt.CASES])
def test_active_errclb_projgr_real32(oracle_built, case):
    """active and errclb against the REAL32 oracle, bit for bit -- the five inputs of test_active_and_errclb_doors
    with the offenders in the last n mod 4 rows (the scalar tail of a float32 row trip) -- and projgr: the door returns
    the double it formed, max |proj g_i| of numpy's fp64 arithmetic on the widened operands, whose float32 rounding is
    the REAL32 oracle's sbgnrm"""
    p, sts = rt.states(case)
    n = p.n
    R = po.Routines(F32)
    C = _Ctx(p, case[4])
    try:
        sol = C.sol
        x_o, iw_o = p.x0.copy(), np.zeros(n, np.int32)
        fl = [np.zeros(1, np.int32) for _ in range(4)]
        R.active(n, p.l, p.u, p.nbd, x_o, iw_o, *fl)
        x_g = C.vec(p.x0)
        assert sol.r_active(x_g, C.l, C.u, C.nbd) == tuple(bool(v[0]) for v in fl[:3])
        assert np.array_equal(x_g.cpu().numpy(), x_o)
        assert np.array_equal(sol.export_state()[1][n:2 * n], iw_o)
        a, b = max(n - max(n % 4, 2), 0), n - 1
        for bad_nbd, bad_box in ((None, None), (a, None), (None, b), (a, b), (b, a)):
            l, u, nbd = p.l.copy(), p.u.copy(), p.nbd.copy()
            if bad_nbd is not None:
                nbd[bad_nbd] = 5
            if bad_box is not None:
                nbd[bad_box], l[bad_box], u[bad_box] = 2, 1.0, 0.0
            task_o = po.pad60("START")
            info, k = np.zeros(1, np.int32), np.zeros(1, np.int32)
            R.errclb(n, p.m, 1e7, l, u, nbd, task_o, info, k)
            t_g, info_g, k_g = sol.r_errclb(C.vec(l), C.vec(u), C.torch.from_numpy(nbd).to(C.dev), 1e7)
            assert t_g == po.task_str(task_o)
            assert (info_g, k_g) == (int(info[0]), int(k[0]) if info[0] else 0)
        for s in sts[-2:]:
            x, g, l, u = (v.astype(F64) for v in (s.x, s.g, p.l, p.u))
            lo, up = (p.nbd != 0) & (p.nbd <= 2), p.nbd >= 2
            pg = np.where(g < 0, np.where(up, np.maximum(x - u, g), g), np.where(lo, np.minimum(x - l, g), g))
            got = sol.projgr(C.vec(s.x), C.l, C.u, C.nbd, C.vec(s.g))
            assert got == float(np.max(np.abs(pg))), (got, float(np.max(np.abs(pg))))
            assert F32(got) == F32(R.projgr(n, p.l, p.u, p.nbd, s.x, s.g))
    finally:
        C.sol.close()
