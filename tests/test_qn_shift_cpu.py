"""CPU tests of the host algebra behind the model plus a diagonal (lbfgsb_hip_qn_shift_*; host_dense.hpp,
qn_shift_factor and qn_shift_coef) through a g++-built doorway (tests/qn_shift_shim.cpp).  The pairs are BFGS pairs of
a random SPD quadratic (tests/test_qn_root_cpu.py, _pairs), n = 300, col in {0, 1, 3, 10, 17, 40}; the weights
w = 1 / (theta + mu + d) are made in numpy, with and without half the rows at w = 0 (pinned).  With
A = (B + mu I + D) on the free rows, dense:
  the solve through the coefficients, w o (v + S cs + Y cy), within 1e-12 cond(A) of numpy.linalg.solve;
  the coefficients themselves within 1e-12 cond(K) of a dense solve with K;
  log det = sum log Delta + log|det K| - log|det M^-1| within 1e-10 n of slogdet;
  d = 0, mu = 0, no pin: the coefficients are qn_coef_h's (cs / theta, cy / theta) to 1e-12 cond(B);
  an indefinite B + mu I is refused as the inertia failure (2)."""
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
    out = tmp_path_factory.mktemp("qn_shift_shim")
    so = str(out / "libqn_shift_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_shift_shim.cpp"), "-o", so])
    return C.CDLL(so)


def _set(rng, col):
    if col == 0:
        z = np.zeros((N, 0))
        return z, z.copy(), 0, 1.7, np.zeros((1, 1), order="F"), np.zeros((1, 1), order="F"), 1
    S, Y, c, theta, sy, ss = _pairs(rng, N, col, col)
    assert c == col
    return S, Y, col, theta, sy, ss, col


def _factor(shim, S, Y, col, theta, sy, m, w):
    """(rc, kf, log|det K|, rc of M^-1, log|det M^-1|)"""
    d = 2 * col
    W = np.hstack([S, Y])
    gw = np.asfortranarray(W.T @ (w[:, None] * W))
    sts = np.asfortranarray(S.T @ S)
    kf, km = np.zeros((max(d, 1), max(d, 1)), order="F"), np.zeros((max(d, 1), max(d, 1)), order="F")
    ld, lm = C.c_double(0.0), C.c_double(0.0)
    rm = shim.qs_factor(col, C.c_double(theta), _p(sy), m, _p(sts), None, _p(km), C.byref(lm))
    rc = shim.qs_factor(col, C.c_double(theta), _p(sy), m, _p(sts), _p(gw), _p(kf), C.byref(ld))
    return rc, kf, ld.value, rm, lm.value


def _dense_k(S, Y, theta, w):
    """K = M^-1 - W' diag(w) W in the [Y, theta S] order"""
    col = S.shape[1]
    sty = S.T @ Y
    minv = np.block([[-np.diag(np.diag(sty)), np.tril(sty, -1).T], [np.tril(sty, -1), theta * (S.T @ S)]])
    Ww = np.hstack([Y, theta * S])
    return minv - Ww.T @ (w[:, None] * Ww) if col else np.zeros((0, 0))


def _coef(shim, col, theta, kf, stv, ytv):
    cs, cy = np.zeros(max(col, 1)), np.zeros(max(col, 1))
    assert shim.qs_coef(col, C.c_double(theta), _p(kf), _p(stv), _p(ytv), _p(cs), _p(cy)) == 0
    return cs[:col], cy[:col]


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_solve_and_logdet_against_dense(shim, col, pin):
    rng = np.random.default_rng(100 * col + pin)
    S, Y, col, theta, sy, ss, m = _set(rng, col)
    mu = 0.3
    dd = rng.uniform(0.0, 1e4, N) * (rng.uniform(size=N) < 0.5)  # (d from 0 to 1e4, half of it zero)
    free = np.ones(N, bool)
    if pin:
        free[::2] = False
    delta = theta + mu + dd
    w = np.where(free, 1.0 / delta, 0.0)
    rc, kf, ldk, rm, ldm = _factor(shim, S, Y, col, theta, sy, m, w)
    assert rc == 0 and rm == 0
    B = _dense_b(S, Y, theta)
    A = (B + np.diag(mu + dd))[np.ix_(free, free)]
    cond = np.linalg.cond(A)
    # log det
    ld = np.log(delta[free]).sum() + ldk - ldm
    sign, ref_ld = np.linalg.slogdet(A)
    print("col %d pin %d: log det %.12e against %.12e (bound %.1e)" % (col, pin, ld, ref_ld, 1e-10 * N))
    assert sign > 0 and abs(ld - ref_ld) <= 1e-10 * N
    # the inertia numpy sees, and the coefficients against a dense solve with K
    K = _dense_k(S, Y, theta, w)
    if col:
        ev = np.linalg.eigvalsh(K)
        assert (ev < 0).sum() == col and (ev > 0).sum() == col
    for trial in range(3):
        v = rng.standard_normal(N)
        stv, ytv = S.T @ (w * v), Y.T @ (w * v)
        cs, cy = _coef(shim, col, theta, kf, np.ascontiguousarray(stv), np.ascontiguousarray(ytv))
        if col:
            z = np.linalg.solve(K, np.concatenate([ytv, theta * stv]))
            ref_c = np.concatenate([theta * z[col:], z[:col]])
            e_c = np.linalg.norm(np.concatenate([cs, cy]) - ref_c)
            b_c = 1e-12 * np.linalg.cond(K) * np.linalg.norm(ref_c)
            print("  coefficients off by %.2e (bound %.2e)" % (e_c, b_c))
            assert e_c <= b_c
        out = w * (v + S @ cs + Y @ cy)
        ref = np.zeros(N)
        ref[free] = np.linalg.solve(A, v[free])
        err = np.linalg.norm(out - ref)
        print("  solve off by %.2e (bound %.2e, cond %.2e)" % (err, 1e-12 * cond * np.linalg.norm(ref), cond))
        assert err <= 1e-12 * cond * np.linalg.norm(ref)
        assert np.all(out[~free] == 0.0)


@pytest.mark.parametrize("col", COLS)
def test_all_rows_pinned(shim, col):
    rng = np.random.default_rng(7 + col)
    S, Y, col, theta, sy, ss, m = _set(rng, col)
    rc, kf, ldk, rm, ldm = _factor(shim, S, Y, col, theta, sy, m, np.zeros(N))
    assert rc == 0 and rm == 0 and ldk == ldm  # (K = M^-1 by the same arithmetic: log det 0 exactly)


@pytest.mark.parametrize("col", COLS[1:])
def test_unshifted_is_qn_coef_h(shim, col):
    rng = np.random.default_rng(31 + col)
    S, Y, col, theta, sy, ss, m = _set(rng, col)
    w = np.full(N, 1.0 / theta)
    rc, kf, ldk, rm, ldm = _factor(shim, S, Y, col, theta, sy, m, w)
    assert rc == 0
    cond = np.linalg.cond(_dense_b(S, Y, theta))
    sty, yty = np.asfortranarray(S.T @ Y), np.asfortranarray(Y.T @ Y)
    dg = np.ascontiguousarray(np.diag(sty))
    v = rng.standard_normal(N)
    stv, ytv = np.ascontiguousarray(S.T @ v), np.ascontiguousarray(Y.T @ v)
    hs, hy = np.zeros(col), np.zeros(col)
    assert shim.qs_coef_h(col, C.c_double(theta), _p(sty), _p(yty), _p(dg), _p(stv), _p(ytv), _p(hs), _p(hy)) == 0
    cs, cy = _coef(shim, col, theta, kf, stv / theta, ytv / theta)
    got, ref = np.concatenate([cs, cy]) / theta, np.concatenate([hs, hy])
    err = np.linalg.norm(got - ref)
    print("col %d: coefficients of H off by %.2e (bound %.2e)" % (col, err, 1e-12 * cond * np.linalg.norm(ref)))
    assert err <= 1e-12 * cond * np.linalg.norm(ref)


@pytest.mark.parametrize("col", [1, 3, 10])
def test_indefinite_shift_refused(shim, col):
    """mu = -0.999 theta keeps every Delta_i positive, but B has an eigenvalue below 0.999 theta along a pair whose
    curvature is below theta: B + mu I is indefinite, K loses the inertia (col, col), the Schur factor fails (2)"""
    rng = np.random.default_rng(55 + col)
    S, Y, col, theta, sy, ss, m = _set(rng, col)
    mu = -0.999 * theta
    assert np.linalg.eigvalsh(_dense_b(S, Y, theta) + mu * np.eye(N)).min() < 0.0
    w = np.full(N, 1.0 / (theta + mu))
    rc, kf, ldk, rm, ldm = _factor(shim, S, Y, col, theta, sy, m, w)
    assert rc == 2 and rm == 0
    ev = np.linalg.eigvalsh(_dense_k(S, Y, theta, w))
    assert (ev > 0).sum() != col
