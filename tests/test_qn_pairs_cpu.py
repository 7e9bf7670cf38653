"""CPU tests of the host side of lbfgsb_hip_qn_pairs_set / _push: qn_pairs_factor, qn_pairs_append and qn_gram_append
of host_dense.hpp through a g++-built doorway (tests/qn_pairs_shim.cpp), against the oracle's Routines.matupd and
Routines.formt on the dyadic family (tests/_qn_synth.py: every Gram sum is exact, so every comparison is bit for bit).
  qn_pairs_append applied npairs in {1, m - 1, m, 2m + 1} times to the exact Gram sums of one sequence of pairs
  (tests/_qn_pairs_seq.py) gives the oracle's sy, ss, wt, col, head, itail and theta after every pair.
  qn_gram_append keeps S'Y of the ring, both triangles, through the same steps.
  qn_pairs_factor on the Gram of synth(...).pairs() gives synth's sy, ss, wt and theta, also after the ring wrapped.
  qn_pairs_factor refuses a pair with s'y = 0 (naming it) and a Gram that makes formt fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _qn_pairs_seq import sequence
from _qn_synth import synth

HERE = os.path.dirname(os.path.abspath(__file__))
N = 127
MS = [3, 10, 17, 40]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_pairs_shim")
    so = str(out / "libqn_pairs_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_pairs_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    V, D, I = C.c_void_p, C.c_double, C.c_int
    lib.qp_factor.argtypes = [I, I, V, V, V, D, V, V, V, V]
    lib.qp_append.argtypes = [I, V, V, V, V, V, V, V, V, V, D, D, D, D]
    lib.qp_gram_append.argtypes = [I, I, V, V, V, D]
    return lib


def _F(a):
    """an [i, j] matrix as column-major storage"""
    return np.asfortranarray(a).reshape(-1, order="F").copy()


@pytest.mark.parametrize("m", MS)
def test_append_is_the_oracles_matupd_and_formt(shim, m):
    npairs = 2 * m + 1
    pairs, states = sequence(N, m, npairs)
    sy, ss, wt = np.zeros(m * m), np.zeros(m * m), np.zeros(m * m)
    col, head, itail = (np.array([v], np.int32) for v in (0, 1, 0))
    theta = np.array([1.0])
    ring, sty = [], np.zeros(m * m)
    for j, (s, y) in enumerate(pairs, 1):
        c = len(ring)
        s_old = np.array([p[0] @ s for p in ring] + [0.0])
        y_old = np.array([p[1] @ s for p in ring] + [0.0])
        info = shim.qp_append(m, _p(col), _p(head), _p(itail), _p(sy), _p(ss), _p(wt), _p(theta), _p(s_old),
                              _p(y_old), float(s @ s), float(s @ y), float(y @ y), 0.0)
        assert info == 0
        cnew = np.array([p[0] @ y for p in ring] + [0.0])
        assert shim.qp_gram_append(m, c, _p(sty), _p(cnew), _p(y_old), float(s @ y)) == min(c + 1, m)
        ring = (ring + [(s, y)])[-m:]
        S, Y = np.array([p[0] for p in ring]), np.array([p[1] for p in ring])
        assert np.array_equal(sty[:len(ring) ** 2].reshape(len(ring), len(ring)).T, S @ Y.T)
        if j in (1, m - 1, m, npairs):
            st = states[j]
            assert (int(col[0]), int(head[0]), int(itail[0])) == (st.col, st.head, st.itail)
            assert theta[0] == st.theta
            for got, ref in ((sy, st.sy), (ss, st.ss), (wt, st.wt)):
                assert np.array_equal(got.reshape(m, m).T, ref)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("wrap", [False, True])
def test_factor_is_the_oracles_state(shim, m, wrap):
    st = synth(N, m, 2 * m + 1 if wrap else m - 1)
    S, Y = st.pairs()
    k = st.col
    sy, ss, wt, theta = np.zeros(m * m), np.zeros(m * m), np.zeros(m * m), np.zeros(1)
    assert shim.qp_factor(m, k, _p(_F(S.T @ S)), _p(_F(S.T @ Y)), _p(_F(Y.T @ Y)), 0.0, _p(sy), _p(ss), _p(wt),
                          _p(theta)) == 0
    assert theta[0] == st.theta
    for got, ref in ((sy, st.sy), (ss, st.ss), (wt, st.wt)):
        assert np.array_equal(got.reshape(m, m).T, ref)
    # a theta of the caller's own: formt with it
    assert shim.qp_factor(m, k, _p(_F(S.T @ S)), _p(_F(S.T @ Y)), _p(_F(Y.T @ Y)), 2.5, _p(sy), _p(ss), _p(wt),
                          _p(theta)) == 0
    assert theta[0] == 2.5


def test_factor_refuses(shim):
    m = 5
    S, Y = synth(N, m, 4).pairs()
    sy, ss, wt, theta = np.zeros(m * m), np.zeros(m * m), np.zeros(m * m), np.zeros(1)
    args = lambda sts, sty, yty, th: (m, 4, _p(_F(sts)), _p(_F(sty)), _p(_F(yty)), th, _p(sy), _p(ss), _p(wt),  # noqa
                                      _p(theta))
    Y0 = Y.copy()
    Y0[:, 2] = 0.0  # s'y = 0 in pair 2
    assert shim.qp_factor(*args(S.T @ S, S.T @ Y0, Y0.T @ Y0, 0.0)) == 3
    Yn = Y.copy()
    Yn[0, 1] = np.nan
    assert shim.qp_factor(*args(S.T @ S, S.T @ Yn, Yn.T @ Yn, 1.0)) == 2
    bad = S.T @ S
    bad[0, 0] = -1.0  # no S gives this S'S: T = theta S'S + L D^-1 L' is not positive definite
    assert shim.qp_factor(*args(bad, S.T @ Y, Y.T @ Y, 0.0)) == -3
    assert shim.qp_factor(m, 0, None, None, None, 0.0, _p(sy), _p(ss), _p(wt), _p(theta)) == -1
    assert shim.qp_factor(m, 0, None, None, None, 1.5, _p(sy), _p(ss), _p(wt), _p(theta)) == 0 and theta[0] == 1.5
