"""The two helpers of tests/test_gpu_qn_switches.py, checked without a GPU: the synthesiser of curvature-model states
(tests/_qn_synth.py), the extended-precision reference (tests/_qn_truth.py), and that the derived bound tells a right
evaluation from a wrong one -- the passes emulated in numpy (fp64 sums, the compact form through the oracle's sy and
wt) pass it, and each of five ways of getting them slightly wrong fails it; a -0 where a pinned row must hold +0 is
caught by the sign check the GPU module uses (pos_zero), which the bound has no part in."""
import numpy as np
import pytest

import _qn_synth as qs
import _qn_truth as qt

LD = qt.LD


@pytest.fixture(scope="module")
def po(oracle_built):
    return oracle_built


CASES = [((130, 5, 3), (3, 1)), ((130, 10, 17), (10, 8)), ((259, 17, 17), (17, 1)), ((259, 33, 40), (33, 8))]


@pytest.fixture(scope="module")
def states(po):
    out = {}
    for (n, m, npairs), _ in CASES:
        for fam in ("dyadic", "generic"):
            st = qs.synth(n, m, npairs, fam)
            S, Y = st.pairs()
            out[(n, m, npairs, fam)] = (st, qt.Truth(S, Y))
    return out


@pytest.mark.parametrize("fam", ["dyadic", "generic"])
@pytest.mark.parametrize("case,want", CASES)
def test_synthesiser(states, case, want, fam):
    st, tr = states[case + (fam,)]
    assert st.info == 0 and (st.col, st.head) == want and st.iupdat == case[2]
    assert np.all(st.sty_diag > 0.0)
    assert abs(st.theta - float(tr.theta)) <= 4 * qt.gamma(st.n) * st.theta  # (the oracle's y'y / s'y)
    assert tr.cond <= 10.0  # (a well-conditioned model: the bound's condition factors stay small)
    # the packed state: the oracle's small matrices where import_state reads them, nothing else
    off = qs.po.wa_offsets(st.n, st.m)
    used = sum(off[k][1] for k in ("ws", "wy", "sy", "ss", "wt"))
    assert not st.wa[used:].any() and not st.iwa.any()
    assert [int(st.isave[i]) for i in (26, 27, 30)] == [st.head, st.col, st.iupdat]


@pytest.mark.parametrize("real", [np.float64, np.float32])
def test_dyadic_grams_are_exact_in_fp32(po, real):
    st = qs.synth(259, 33, 40, "dyadic", real)
    S, Y = st.pairs()
    Sl, Yl = S.astype(LD), Y.astype(LD)
    for A, Bm in ((S, S), (S, Y), (Y, Y)):
        exact = A.astype(LD).T @ Bm.astype(LD)
        f32 = (A.astype(np.float32).T @ Bm.astype(np.float32))
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(LD), exact)
        assert np.array_equal((A.T @ Bm).astype(LD), exact)
    # the imported sy, ss (rounded to `real`) are the exact Grams in ring order
    c = st.col
    assert np.array_equal(np.tril(st.mats("sy")[:c, :c]).astype(LD), np.tril(Sl.T @ Yl))
    assert np.array_equal(np.triu(st.mats("ss")[:c, :c]).astype(LD), np.triu(Sl.T @ Sl))


@pytest.mark.parametrize("fam", ["dyadic", "generic"])
@pytest.mark.parametrize("case,want", CASES)
def test_reference(states, case, want, fam):
    st, tr = states[case + (fam,)]
    n = st.n
    assert float(np.abs(tr.Bd @ tr.Hd - np.eye(n, dtype=LD)).max()) <= 1e-17
    assert float(np.abs(tr.Bd - tr.Bd.T).max()) <= 1e-18 * float(np.abs(tr.Bd).max())
    sign, ld = np.linalg.slogdet(tr.Bd.astype(np.float64))
    assert sign == 1.0 and abs(ld - float(tr.logdet_b)) <= 1e-11
    # N read off the dense matrices reproduces them: every operator is alpha I + W N W'
    for op, alpha in ((tr.B, tr.theta), (tr.H, 1 / tr.theta)):
        back = alpha * np.eye(n, dtype=LD) + tr.W @ op.N @ tr.W.T
        assert float(np.abs(back - op.A).max()) <= 1e-16 * float(np.abs(op.A).max())
    # the shifted inverse: A Sigma = I on the free rows, pinned rows and columns exactly +0
    d = np.linspace(0.0, 3.0, n)
    d[::3] = np.inf
    d[110:150] = np.inf
    sh = tr.shifted(d, 0.3)
    assert float(np.abs(sh.Afree @ sh.A[np.ix_(sh.rows, sh.rows)] - np.eye(sh.rows.size, dtype=LD)).max()) <= 1e-17
    pinned = ~sh.free
    assert qt.pos_zero(sh.A[pinned]).all() and qt.pos_zero(sh.A[:, pinned]).all()
    back = np.diag(sh.a) + (tr.W * sh.l[:, None]) @ sh.N @ (tr.W * sh.r[:, None]).T
    assert float(np.abs(back - sh.A).max()) <= 1e-15 * float(np.abs(sh.A).max())
    # the longdouble Cholesky that the shifted log det is held to, against fp64 slogdet of the same block
    assert abs(float(sh.logdet) - sh.logdet64) <= 1e-11


# ------------------------------------------------------------------------------ the passes of qn_apply(B), emulated
def _emulate(st, V, mutate=None):
    """B V' as the library forms it, in fp64: p = [S, Y]'v, the middle matrix through sy and wt (bmv), the expansion"""
    head = st.head % st.m + 1 if mutate == "head" else st.head
    S, Y = qs.ring_pairs(st.wa, st.n, st.m, st.col, head)
    col, theta = st.col, st.theta
    sy, wt = st.mats("sy"), st.mats("wt")
    out = np.zeros_like(V)
    for j, v in enumerate(V):
        rows = slice(0, st.n - 1) if mutate == "last_row" else slice(0, st.n)
        if mutate == "fp32_sums":
            sv = (S[rows] * v[rows, None]).astype(np.float32).sum(axis=0, dtype=np.float32).astype(np.float64)
            yv = (Y[rows] * v[rows, None]).astype(np.float32).sum(axis=0, dtype=np.float32).astype(np.float64)
        else:
            sv, yv = S[rows].T @ v[rows], Y[rows].T @ v[rows]
        if mutate == "tail_twice":
            sv, yv = sv + S[-1] * v[-1], yv + Y[-1] * v[-1]
        if mutate == "column":
            yv[col // 2] = 0.0
        p = qt.bmv(sy, wt, col, np.concatenate([yv, theta * sv]))
        out[j] = theta * v - Y @ p[:col] - theta * (S @ p[col:])
    return out


MUTATIONS = ["column", "last_row", "tail_twice", "fp32_sums", "head"]


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(5)
    return {n: rng.standard_normal((3, n)) for n in (130, 259)}


@pytest.mark.parametrize("fam", ["dyadic", "generic"])
@pytest.mark.parametrize("case,want", CASES)
def test_honest_emulation_passes(states, vectors, case, want, fam):
    """also: B of the recursion agrees with the compact form through the oracle's sy and wt (unit vectors)"""
    st, tr = states[case + (fam,)]
    for V in (vectors[st.n], np.eye(st.n)[[0, 63, 64, st.n - 1]]):
        out = _emulate(st, V)
        w = qt.check("cpu emulation", out, tr.B.apply(V), tr.B.bound_apply(V))
        print("n %d col %d %s: worst err / bound %.3g" % (st.n, st.col, fam, w))


@pytest.mark.parametrize("mutate", MUTATIONS)
@pytest.mark.parametrize("fam", ["dyadic", "generic"])
@pytest.mark.parametrize("case,want", CASES[1:])
def test_wrong_emulations_fail(states, vectors, case, want, fam, mutate):
    st, tr = states[case + (fam,)]
    V = vectors[st.n]
    out = _emulate(st, V, mutate)
    with pytest.raises(AssertionError):
        qt.check("cpu mutation", out, tr.B.apply(V), tr.B.bound_apply(V))


def test_minus_zero_on_a_pinned_row_fails():
    x = np.array([0.0, 1.0, -0.0]) * 3.0
    assert list(qt.pos_zero(x)) == [True, False, False]
    assert not qt.pos_zero(np.float32(-0.0) * np.ones(2, np.float32)).any()


def test_real32_compact_reference(po):
    """a REAL32 state: the compact form on the imported fp32 matrices is within the fp32 allowance of the recursion,
    and not within the fp64 bound (so the two references are told apart where wt is rounded)"""
    st = qs.synth(259, 17, 17, "dyadic", np.float32)
    S, Y = st.pairs()
    tr = qt.Truth(S, Y, real32=(st.mats("sy"), st.mats("wt")))
    V = np.random.default_rng(2).standard_normal((2, st.n)).astype(np.float32)
    qt.check("cpu real32", tr.B.apply(V), tr.B_rec.apply(V), tr.B_rec.bound_apply(V))
    assert tr.B_rec.eta > tr.B.eta
