"""CPU tests of the host algebra behind the factor of the model plus a diagonal (lbfgsb_hip_qn_shift_sqrt / _draw /
_logpdf; host_dense.hpp, qn_shift_root) through a g++-built doorway (tests/qn_shift_root_shim.cpp).  The pairs are BFGS
pairs of a random SPD quadratic (tests/test_qn_root_cpu.py, _pairs), n = 300, col in {0, 1, 3, 10, 17, 40}; the
weights w = 1 / (theta + mu + d) are made in numpy, with and without half the rows at w = 0 (pinned).  With
P = B + mu I + D on the free rows, Sigma = P^-1 embedded in n x n (zero on pinned rows and columns) and the dense
L = diag(sqrt w) + diag(w) [S, Y] C [S, Y]' diag(sqrt w) from the C that qn_shift_root returns:
  |L L' - Sigma| <= 1e-12 cond(P) |Sigma| (Frobenius norms);
  sum log Delta - logsum within 1e-10 n of slogdet(P);
  d = 0, mu = 0, no pin: L L' = H, the dense inverse model from qn_coef_h, on the same bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_qn_root_cpu import _dense_b, _p, _pairs

HERE = os.path.dirname(os.path.abspath(__file__))
N = 300
COLS = [0, 1, 3, 10, 17, 40]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_shift_root_shim")
    so = str(out / "libqn_shift_root_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_shift_root_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    assert hasattr(lib, "qsr_root")
    return lib


def _set(rng, col):
    if col == 0:
        z = np.zeros((N, 0))
        return z, z.copy(), 0, 1.7, np.zeros((1, 1), order="F"), 1
    S, Y, c, theta, sy, ss = _pairs(rng, N, col, col)
    assert c == col
    return S, Y, col, theta, sy, col


def _root(shim, S, Y, col, theta, sy, m, w):
    """(the dense L, logsum) from qn_shift_factor's factor and qn_shift_root's C"""
    d = 2 * col
    W = np.hstack([S, Y])
    gw = np.asfortranarray(W.T @ (w[:, None] * W))
    gw = np.asfortranarray(0.5 * (gw + gw.T))
    sts = np.asfortranarray(S.T @ S)
    kf, cm = np.zeros((max(d, 1), max(d, 1)), order="F"), np.zeros((max(d, 1), max(d, 1)), order="F")
    ld, logsum = C.c_double(0.0), C.c_double(0.0)
    assert shim.qsr_factor(col, C.c_double(theta), _p(sy), m, _p(sts), _p(gw), _p(kf), C.byref(ld)) == 0
    assert shim.qsr_root(col, C.c_double(theta), _p(kf), _p(gw), _p(cm), C.byref(logsum)) == 0
    cm = cm[:d, :d]
    if d:
        assert np.array_equal(cm, cm.T)
    rw = np.sqrt(w)
    L = np.diag(rw) + (w[:, None] * W) @ cm @ (W.T * rw[None, :])
    return L, logsum.value


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_factor_and_logdet_against_dense(shim, col, pin):
    rng = np.random.default_rng(200 * col + pin)
    S, Y, col, theta, sy, m = _set(rng, col)
    mu = 0.3
    dd = rng.uniform(0.0, 1e4, N) * (rng.uniform(size=N) < 0.5)  # (d from 0 to 1e4, half of it zero)
    free = np.ones(N, bool)
    if pin:
        free[::2] = False
    delta = theta + mu + dd
    w = np.where(free, 1.0 / delta, 0.0)
    L, logsum = _root(shim, S, Y, col, theta, sy, m, w)
    P = (_dense_b(S, Y, theta) + np.diag(mu + dd))[np.ix_(free, free)]
    cond = np.linalg.cond(P)
    sigma = np.zeros((N, N))
    sigma[np.ix_(free, free)] = np.linalg.inv(P)
    assert np.all(L[~free, :] == 0.0) and np.all(L[:, ~free] == 0.0)
    err, bound = np.linalg.norm(L @ L.T - sigma), 1e-12 * cond * np.linalg.norm(sigma)
    print("col %d pin %d: L L' off by %.2e (bound %.2e, cond %.2e)" % (col, pin, err, bound, cond))
    assert err <= bound
    ld = np.log(delta[free]).sum() - logsum
    sign, ref_ld = np.linalg.slogdet(P)
    print("col %d pin %d: log det %.12e against %.12e (bound %.1e)" % (col, pin, ld, ref_ld, 1e-10 * N))
    assert sign > 0 and abs(ld - ref_ld) <= 1e-10 * N


@pytest.mark.parametrize("col", COLS)
def test_unshifted_is_h(shim, col):
    rng = np.random.default_rng(77 + col)
    S, Y, col, theta, sy, m = _set(rng, col)
    L, logsum = _root(shim, S, Y, col, theta, sy, m, np.full(N, 1.0 / theta))
    B = _dense_b(S, Y, theta)
    cond = np.linalg.cond(B)
    H = np.eye(N) / theta
    if col:
        sty, yty = np.asfortranarray(S.T @ Y), np.asfortranarray(Y.T @ Y)
        dg = np.ascontiguousarray(np.diag(sty))
        nh = np.zeros((2 * col, 2 * col))
        for k in range(2 * col):
            e = np.zeros(2 * col)
            e[k] = 1.0
            cs, cy = np.zeros(col), np.zeros(col)
            assert shim.qsr_coef_h(col, C.c_double(theta), _p(sty), _p(yty), _p(dg), _p(np.ascontiguousarray(e[:col])),
                                   _p(np.ascontiguousarray(e[col:])), _p(cs), _p(cy)) == 0
            nh[:, k] = np.concatenate([cs, cy])
        W = np.hstack([S, Y])
        H = H + W @ nh @ W.T
    err, bound = np.linalg.norm(L @ L.T - H), 1e-12 * cond * np.linalg.norm(H)
    print("col %d: L L' off H by %.2e (bound %.2e, cond %.2e)" % (col, err, bound, cond))
    assert err <= bound
    ld = N * np.log(theta) - logsum
    assert abs(ld - np.linalg.slogdet(B)[1]) <= 1e-10 * N


@pytest.mark.parametrize("col", COLS)
def test_all_rows_pinned(shim, col):
    rng = np.random.default_rng(9 + col)
    S, Y, col, theta, sy, m = _set(rng, col)
    L, logsum = _root(shim, S, Y, col, theta, sy, m, np.zeros(N))
    assert np.all(L == 0.0) and logsum == 0.0
