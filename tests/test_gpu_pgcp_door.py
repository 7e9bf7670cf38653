"""The opt-in parallel search for the generalized Cauchy point (LBFGSB_F_PARALLEL_GCP: k_pgcp.hip, solver_pgcp.inl,
the closed form and its guard at the top of cauchy() in solver_walk.inl) ONE CALL deep, through the Cauchy door of a
context created with parallel_gcp=True and option pg_min = 0: every case of tests/_gcp_cases.py is imported as a
state, r_cauchy is called once, and what comes back is compared with the extended-precision walk of
tests/_gcp_truth.py (tests/test_gcp_truth_cpu.py shows that every case is well posed and takes the branch it is
named after).

Per case:
  * the path ran -- stats()["cauchy_fullsorts"] rises by exactly 1 for the search (col > 0), not at all for the
    closed form (col = 0) and for the calls its guard sends to the walk; those give, bit for bit, what a context
    WITHOUT the flag gives (no public counter tells closed form and fallback apart), and the closed form's tsum is
    fl(1 / theta) itself, which a walk reaches only up to its rounding;
  * nseg, info and the whole iwhere equal the truth's -- equal, not close: no decision of these walks is nearer than
    1e-6, and none ends inside a group of equal breakpoints;
  * c (work vector 2, first 2 col entries): |c_gpu,a - c_truth,a| <= K eps M_a, K = max(4 rho_ref, 2 (log2 nb + 4)),
    M_a the magnitude sum of c_a, rho_ref the ORACLE's error on the case in the same unit (_gcp_cases.reference);
    eps is that of double in REAL32 contexts too (the gathered inputs widen exactly, the scans run in double) --
    there c is EXPORTED as float32, one rounding of c_a itself, which the bound allows for;
  * xcp, in xcp_out and in the exported z: rows fixed by the walk are bit-equal to their bound, rows that do not
    move bit-equal to x, the others within 2 eps_T (|x| + tsum |g|) + E_t |g| of the truth, E_t = K_t eps tsum the
    share of tsum's own error (K_t like K, from the oracle's tsum); where the case has a probe row (x = 0, g a power
    of two, unbounded: xcp = -tsum g without a rounding) tsum itself is held to E_t.

The work vectors p, wbp and v are NOT compared: the search leaves p = W'd of the start and does not touch wbp and v,
where the reference's walk leaves the last breakpoint's.  Nothing reads them after cauchy(): wbp and v are local to
it, p (wa(1:2m)) is overwritten by cmprlb's M c before anything reads it, and closed_ok -- which would hand p to
the subspace step -- stays false on this path.

The DEFAULT walk -- a context without the flag, what every iteration runs -- goes through the same cases and the same
assertions in test_default_walk_against_the_extended_precision_walk, minus those about the search itself, plus p, wbp
and v against the oracle's: the sequential walk does leave them.
"""
import numpy as np
import pytest

import _gcp_cases as gc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

EPS = gc.EPS64


def _door(c, sbgnrm, flag=True):
    """one r_cauchy call on the case's state -> what it left"""
    import torch
    import lbfgsb_amd
    n, m = c.n, c.m
    r32 = c.real == np.float32
    dev = torch.device("cuda", 0)
    sol = lbfgsb_amd.DeviceSolver(n, m, device=0, real32=r32, parallel_gcp=flag,
                                  options={"pg_min": 0} if flag else None)
    try:
        off = po.wa_offsets(n, m)
        wa = np.zeros(po.wa_len(n, m), c.real)
        for k, a in (("ws", c.ws), ("wy", c.wy), ("sy", c.sy), ("ss", c.ss), ("wt", c.wt)):
            wa[off[k][0]:off[k][0] + off[k][1]] = np.asarray(a, c.real).reshape(-1)
        wa[off["wa8m"][0]:off["wa8m"][0] + 8 * m] = 7.0           # (stale work vectors: c must be WRITTEN)
        iwa = np.concatenate([np.zeros(n, np.int32), c.iwhere, np.zeros(n, np.int32)])
        isave = np.zeros(44, np.int32)
        isave[26], isave[27] = c.head, c.col
        sol.import_state(wa, iwa, isave)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        xcp_d = torch.full((n,), 9.0, dtype=torch.float32 if r32 else torch.float64, device=dev)
        before = sol.stats()["cauchy_fullsorts"]
        nseg, info = sol.r_cauchy(T(c.x), T(c.l), T(c.u), T(c.nbd), T(c.g), c.theta, c.col, c.head, sbgnrm, xcp_d)
        sorts = sol.stats()["cauchy_fullsorts"] - before
        wa2, iwa2 = sol.export_state()
    finally:
        sol.close()
    w8 = wa2[off["wa8m"][0]:off["wa8m"][0] + 8 * m]
    return dict(nseg=nseg, info=info, sorts=sorts, iwhere=iwa2[n:2 * n].copy(), xcp=xcp_d.cpu().numpy(),
                z=wa2[off["z"][0]:off["z"][0] + n].copy(), c=w8[2 * m:2 * m + 2 * c.col].astype(np.float64),
                p=w8[:2 * c.col].astype(np.float64), wbp=w8[4 * m:4 * m + 2 * c.col].astype(np.float64),
                v=w8[6 * m:6 * m + 2 * c.col].astype(np.float64))


def _compare(name, got, search):
    """what one r_cauchy call left (got, of _door) against the extended-precision walk of the case; search: the call
    went through a context with the flag, and the assertions about the search itself apply"""
    c, tr = gc.case(name)
    ref = gc.reference(name)
    eps_T = gc.EPS[c.real]
    r32 = c.real == np.float32

    # ---- the path ran
    if search:
        assert got["sorts"] == (1 if c.path == "search" else 0), "full sorts of the parallel search: %d" % got["sorts"]
    else:
        assert got["sorts"] == 0, "a context without the flag sorted: %d" % got["sorts"]

    # ---- integers and sets
    assert (got["nseg"], got["info"]) == (tr.nseg, 0), (got["nseg"], tr.nseg)
    diff = np.flatnonzero(got["iwhere"] != tr.iwhere)
    assert diff.size == 0, "iwhere differs in %d rows, first %s" % (diff.size, diff[:8])

    # ---- tsum, where a probe row shows it without a rounding
    tsum = float(tr.tsum)
    E_t = ref["K_t"] * EPS * tsum
    rho_t = None
    if "probe" in c.expect:
        i, scale = c.expect["probe"]
        for key in ("xcp", "z"):
            t_gpu = -float(got[key][i]) / scale
            rho_t = gc.rho_t(t_gpu, tr)
            assert abs(np.longdouble(t_gpu) - tr.tsum) <= E_t + (eps_T * tsum if r32 else 0.0), \
                "tsum (%s): rho_gpu %.3g, bound K_t %.3g (rho_ref %.3g)" % (key, rho_t, ref["K_t"], ref["rho_t"])
        if search and c.path == "closed":
            assert -got["z"][i] / scale == 1.0 / c.theta, "the closed form's tsum is fl(1 / theta)"

    # ---- c
    rho_gpu = None
    if c.col:
        err = np.abs(got["c"].astype(np.longdouble) - tr.c)
        bound = ref["K_c"] * EPS * tr.M + (eps_T * np.abs(tr.c).astype(np.float64) if r32 else 0.0)
        rho_gpu = gc.rho_c(got["c"], tr)
        worst = int(np.argmax(err / bound))
        assert np.all(err <= bound), \
            "c: rho_gpu %.3g, bound K %.3g (rho_ref %.3g, floor %.3g); component %d: |diff| %.3e > %.3e" \
            % (rho_gpu, ref["K_c"], ref["rho_c"], ref["floor"], worst, float(err[worst]), float(bound[worst]))
    print("\n%-19s nb %6d ks %6d | c: rho_ref %9.3g K %9.3g rho_gpu %9s | tsum: rho_ref %9.3g K_t %9.3g rho_gpu %9s"
          % (name, tr.nb, tr.ks, ref["rho_c"], ref["K_c"], "-" if rho_gpu is None else "%.3g" % rho_gpu,
             ref["rho_t"], ref["K_t"], "-" if rho_t is None else "%.3g" % rho_t))

    # ---- xcp
    x64, g64 = c.x.astype(np.float64), c.g.astype(np.float64)
    moving = tr.d != 0
    still = ~tr.fixed & ~moving
    bound_val = np.where(tr.iwhere == 2, c.u, c.l)
    for key in ("xcp", "z"):
        v = got[key]
        assert v.dtype == c.real
        assert np.array_equal(v[tr.fixed], bound_val[tr.fixed]), key + ": a fixed row is not bit-equal to its bound"
        assert np.array_equal(v[still], c.x[still]), key + ": a row that does not move is not bit-equal to x"
        err = np.abs(v[moving].astype(np.longdouble) - tr.xcp[moving]).astype(np.float64)
        tol = 2.0 * eps_T * (np.abs(x64[moving]) + tsum * np.abs(g64[moving])) + E_t * np.abs(g64[moving])
        k = int(np.argmax(err - tol)) if err.size else 0
        assert np.all(err <= tol), "%s: moving row %d off by %.3e > %.3e" % (key, np.flatnonzero(moving)[k], err[k], tol[k])

    # ---- the guard's fallback is the exact walk: bit for bit what a context without the flag returns
    if search and c.path == "fallback":
        plain = _door(c, ref["sbgnrm"], flag=False)
        assert (plain["nseg"], plain["info"], plain["sorts"]) == (got["nseg"], 0, 0)
        assert np.array_equal(plain["iwhere"], got["iwhere"])
        assert np.array_equal(plain["z"], got["z"]) and np.array_equal(plain["xcp"], got["xcp"])


@pytest.mark.parametrize("name", gc.NAMES)
def test_one_call_against_the_extended_precision_walk(oracle_built, name):
    c, _ = gc.case(name)
    _compare(name, _door(c, gc.reference(name)["sbgnrm"]), search=True)


@pytest.mark.parametrize("name", gc.NAMES)
def test_default_walk_against_the_extended_precision_walk(oracle_built, name):
    """The walk EVERY iteration runs (a context without the flag: the provider and the host replay of cauchy() in
    solver_walk.inl), one call deep on the same cases and held to the same truth with the same bounds: nseg, info, the
    whole iwhere, c, tsum at the probe row, xcp.  What is about the search itself is left out (the sort counter stays
    0 here, and a walk reaches fl(1 / theta) only up to its rounding).  The sequential walk does leave p, wbp and v
    the way the reference's does -- p = W'd over the rows that still move, wbp and v = M wbp of the last breakpoint
    it crossed (untouched where it crossed none) -- so these are compared with the oracle's, 1e-9 of their largest
    entry; a REAL32 context exports them as float32, one rounding of each entry, which the bound allows for as the
    bound on c does.  p's largest entry is taken over the call: the walk starts from W'd over all moving rows and takes
    the crossed rows' terms away again, so that what is left can be a remainder of cancellation alone -- all_crossed_bnded
    ends with p = 0 in exact arithmetic (the oracle leaves 2e-14, the library 0 or as little), clamp with 1e-9 of its
    starting value, known to 2e-15 in either code: errors of the size of an ulp of the START value, which is therefore
    part of the scale."""
    c, tr = gc.case(name)
    got = _door(c, gc.reference(name)["sbgnrm"], flag=False)
    _compare(name, got, search=False)
    if not c.col:
        return
    o = gc.oracle_cauchy(c)
    assert (o["nseg"], o["info"]) == (got["nseg"], 0)
    crossed = tr.ks - (1 if tr.all_fixed else 0)       # (the all-fixed exit :1436 leaves before wbp is written)
    eps_x = gc.EPS[c.real] if c.real == np.float32 else 0.0
    ring = [(c.head - 1 + j) % c.m for j in range(c.col)]
    d0 = np.where((tr.d != 0) | tr.fixed, -c.g, 0).astype(np.float64)      # the direction the walk starts with
    p0 = np.concatenate([c.wy[ring].astype(np.float64) @ d0, c.theta * (c.ws[ring].astype(np.float64) @ d0)])
    for key in ("p",) + (("wbp", "v") if crossed > 0 else ()):
        a, b = got[key], o[key]
        top = max(float(np.max(np.abs(b))), float(np.max(np.abs(p0))) if key == "p" else 0.0)
        tol = 1e-9 * top + eps_x * np.abs(b)
        k = int(np.argmax(np.abs(a - b) - tol))
        assert np.all(np.abs(a - b) <= tol), "%s[%d]: %r vs the oracle's %r" % (key, k, a[k], b[k])
