"""The extended-precision walk of tests/_gcp_truth.py and the cases of tests/_gcp_cases.py, without a GPU: is the
helper right, is every case what its name says, and is it well posed -- so that tests/test_gpu_pgcp_door.py may
demand EQUAL nseg and iwhere of the parallel Cauchy-point search, not "within 2"?

Per case (fixed seeds):
  * the oracle's double-precision cauchy gives the truth's nseg and iwhere;
  * validity: the smallest decision margin |dtm - dt| / max(dt, dtm) over the walk is >= 1e-6, so no stopping
    decision can turn on double rounding, and the walk does not end inside a group of equal breakpoints;
  * the branch the case is named after was taken in the truth;
  * rho_ref -- the oracle's own error in c, in units of eps M_a, and in tsum, in units of eps tsum -- is printed
    (run with -s for the table): the GPU test's bounds are made of it.
"""
import numpy as np
import pytest

import _gcp_cases as gc
from _gcp_truth import _LongDouble, _bmv


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    return oracle_built


@pytest.mark.parametrize("name", gc.NAMES)
def test_case_is_well_posed_and_takes_its_branch(name):
    c, tr = gc.case(name)
    ref = gc.reference(name)
    e = c.expect
    crossed_on_clamp = int(tr.clamped[:tr.ks].sum())
    print("\n%-19s n %6d nb %6d ks %6d nseg %6d margin %.2e clamped %3d ks==nb %d all_fixed %d bnded %d ties %s "
          "rho_ref(c) %9.3g rho_ref(tsum) %9.3g K_c %9.3g K_t %9.3g [%s]"
          % (name, c.n, tr.nb, tr.ks, tr.nseg, tr.min_margin, crossed_on_clamp, tr.ks == tr.nb, tr.all_fixed, tr.bnded,
             tr.tie_groups_crossed_whole(), ref["rho_c"], ref["rho_t"], ref["K_c"], ref["K_t"], tr.backend))
    # the reference's own arithmetic agrees with the truth on everything discrete
    assert ref["info"] == 0
    assert ref["nseg"] == tr.nseg
    assert np.array_equal(ref["iwhere"], tr.iwhere)
    # validity
    assert tr.min_margin >= 1e-6, "ill-posed case: a stopping decision within %.1e" % tr.min_margin
    assert not tr.ends_in_tie, "ill-posed case: the walk ends inside a group of equal breakpoints"
    assert ref["sbgnrm"] > 0.0
    # the case is what its name says
    assert tr.nb >= 1 and (c.col > 0) == (c.path == "search")
    if "nb" in e:
        assert tr.nb == e["nb"]
    if e.get("mid"):
        assert 0.2 * tr.nb < tr.ks < 0.8 * tr.nb and tr.dtm > 0
    if e.get("ks_eq_nb"):
        assert tr.ks == tr.nb
    if "bnded" in e:
        assert tr.bnded == e["bnded"] and tr.nb < c.n and not tr.all_fixed
        assert (tr.dtm == 0) == e["bnded"]                 # :1486-1491 against :1492-1494
    assert tr.all_fixed == bool(e.get("all_fixed"))
    if tr.all_fixed:
        assert tr.nb == c.n and tr.nseg == tr.ks and np.all(tr.fixed)
    else:
        assert tr.nseg == 1 + tr.ks
    if e.get("clamp"):
        # crossed while f2 sat on the clamp, AFTER the rows that carry the gradient, and the walk went on
        assert crossed_on_clamp >= 5 and tr.clamped[tr.ks - 1] and tr.ks < tr.nb
    elif c.path == "search" and not e.get("bnded"):
        assert crossed_on_clamp == 0
    if e.get("tie"):
        assert e["tie"] in tr.tie_groups_crossed_whole(3)
    if e.get("kinds"):
        assert set(np.unique(c.nbd)) == {0, 1, 2, 3}
        assert {-3, -1, 0, 1, 2, 3} <= set(np.unique(tr.iwhere))
        on_bound = (tr.iwhere > 0) & ~tr.fixed & (tr.iwhere != 3)
        assert on_bound.sum() >= 4 and np.any(c.x[on_bound] < c.l[on_bound])    # (one of them an ulp below l)
    if c.path == "closed":
        tstar = 1.0 / np.longdouble(c.theta)                                    # the walk of :1378-1497 ends at t*
        assert abs(tr.tsum - tstar) <= 1e-16 * tstar and 0 < tr.ks < tr.nb
        assert (tr.nb == c.n) == e["nb_eq_n"]
    if e.get("clamp_state"):
        # the guard's case: the clamp set f2 at the last crossing and the step behind it is the clamp's, far from t*
        assert tr.clamped[tr.ks - 1] and 0 < tr.dtm < 1e-3 and tr.tsum < 0.6 / c.theta
    if "probe" in e:
        i, scale = e["probe"]
        assert tr.iwhere[i] == -1 and tr.xcp[i] == -tr.tsum * np.longdouble(scale)


def test_truth_agrees_with_itself_in_200_bits():
    """the longdouble walk against the mpmath walk where longdouble is ample (every number of one size): what is
    left of longdouble's own rounding must be small against the unit the tests measure in, one eps of double times
    the magnitude sum (longdouble rounds 2^-11 of that per operation; tsum comes from a difference, f1)"""
    for name in ("mid_nb33", "all_crossed_free", "tie_group"):
        c, tr = gc.case(name)
        assert tr.backend == "longdouble"
        mp = c.truth(backend="mpmath")
        assert (mp.nseg, mp.ks, mp.nb) == (tr.nseg, tr.ks, tr.nb) and np.array_equal(mp.iwhere, tr.iwhere)
        assert gc.rho_c(mp.c.astype(np.longdouble), tr) < 0.1, "c differs by more than a tenth of an eps M_a"
        assert gc.rho_t(mp.tsum, tr) < 0.1
        assert np.max(np.abs(mp.xcp - tr.xcp)) < 1e-17


def test_truth_replays_an_unclear_decision_in_mpmath():
    """theta = 1/2, no pair: the first segment's dtm is exactly 2; a breakpoint 2^-42 on either side of it is a
    decision within 1e-12, which the helper must not leave to longdouble"""
    from _gcp_truth import truth
    z = np.zeros((1, 3))
    for t0, crossed in ((2.0 - 2.0 ** -42, True), (2.0 + 2.0 ** -42, False)):
        x = np.array([t0, 0.0, 3.0])
        tr = truth(x, np.zeros(3), np.full(3, 8.0), np.array([1, 0, 1], np.int32), np.ones(3),
                   np.array([0, -1, 0], np.int32), z, z, 1, 0, np.zeros(1), np.zeros(1), 0.5, 2.0 ** -52)
        assert tr.backend == "mpmath" and tr.min_margin < 1e-12
        assert tr.ks == int(crossed) and tr.nseg == 1 + int(crossed)
        assert tr.iwhere.tolist() == [1 if crossed else 0, -1, 0]
        assert tr.tsum == 2.0 and tr.xcp[1] == -2.0


def test_bmv_of_the_truth_is_the_oracles(oracle_built):
    """the helper's product with the middle matrix against the oracle's bmv (:1057-1123), one routine deep"""
    import ctypes as C
    po = oracle_built
    c, _ = gc.case("col11")
    lib = po.Routines().lib
    lib.lbo_bmv.restype = None
    lib.lbo_bmv.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(3)
    V = rng.normal(0, 1, (7, 2 * c.col))
    B = _LongDouble()
    got = _bmv(B, c.m, B.arr(c.sy), B.arr(c.wt), c.col, B.arr(V))
    for k in range(V.shape[0]):
        out, info = np.zeros(2 * c.col), np.zeros(1, np.int32)
        lib.lbo_bmv(c.m, po._ptr(c.sy), po._ptr(c.wt), c.col, po._ptr(np.ascontiguousarray(V[k])), po._ptr(out),
                    po._ptr(info))
        assert info[0] == 0
        assert np.max(np.abs(got[k].astype(np.float64) - out)) <= 1e-11 * np.max(np.abs(out))
