"""CPU tests of the host algebra behind the curvature-model operator (lbfgsb_hip_qn_apply / qn_diag): the
coefficients of B v (through bmv's middle matrix) and of H v = B^-1 v (the compact inverse of Byrd, Nocedal and
Schnabel), and the 2col x 2col matrices N of the diagonals, against a dense numpy model built by the recursive
BFGS updates from theta I -- on random pair sets with s'y > 0, including a full memory whose ring has wrapped."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_shim")
    so = str(out / "libqn_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_shim.cpp"), "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pairs(rng, n, m, npairs):
    """npairs BFGS pairs (s'y > 0) stored in a ring of m slots as the reference stores them: the matrices sy, ss
    in logical order (oldest first) and the columns of Ws / Wy in ring order from head"""
    A = rng.standard_normal((n, n))
    A = A @ A.T / n + np.eye(n)  # a positive definite Hessian: y = A s
    S, Y = [], []
    for _ in range(npairs):
        s = rng.standard_normal(n)
        S.append(s)
        Y.append(A @ s + 1e-3 * rng.standard_normal(n))
    col = min(npairs, m)
    S, Y = np.array(S[-col:]).T, np.array(Y[-col:]).T  # n x col, oldest first
    assert np.all(np.einsum("ij,ij->j", S, Y) > 0)
    theta = float(Y[:, -1] @ Y[:, -1] / (S[:, -1] @ Y[:, -1]))
    sy = np.zeros((m, m), order="F")
    ss = np.zeros((m, m), order="F")
    sy[:col, :col] = np.tril(S.T @ Y)
    ss[:col, :col] = np.triu(S.T @ S)
    return S, Y, col, theta, sy, ss


def _dense_b(S, Y, theta):
    n = S.shape[0]
    B = theta * np.eye(n)
    for j in range(S.shape[1]):
        s, y = S[:, j], Y[:, j]
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
    return B


CASES = [(12, 1, 1), (12, 3, 2), (20, 5, 5), (40, 10, 17), (70, 17, 30), (80, 32, 32), (90, 32, 45)]


@pytest.mark.parametrize("n,m,npairs", CASES)
def test_coefficients_against_dense_model(shim, n, m, npairs):
    rng = np.random.default_rng(1000 * n + npairs)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs)
    wt = np.zeros((m, m), order="F")
    assert shim.qs_formt(m, _p(wt), _p(sy), _p(ss), col, C.c_double(theta)) == 0
    B = _dense_b(S, Y, theta)
    H = np.linalg.inv(B)
    sty = np.asfortranarray(S.T @ Y)
    yty = np.asfortranarray(Y.T @ Y)
    dg = np.ascontiguousarray(np.diag(sty))
    for trial in range(3):
        v = rng.standard_normal(n)
        stv, ytv = np.ascontiguousarray(S.T @ v), np.ascontiguousarray(Y.T @ v)
        cs, cy = np.zeros(col), np.zeros(col)
        assert shim.qs_coef_b(m, _p(sy), _p(wt), col, C.c_double(theta), _p(stv), _p(ytv), _p(cs), _p(cy)) == 0
        bv = theta * v + S @ cs + Y @ cy
        assert np.linalg.norm(bv - B @ v) <= 1e-11 * np.linalg.norm(B, 2) * np.linalg.norm(v)
        assert shim.qs_coef_h(col, C.c_double(theta), _p(sty), _p(yty), _p(dg), _p(stv), _p(ytv), _p(cs),
                              _p(cy)) == 0
        hv = v / theta + S @ cs + Y @ cy
        ref = H @ v
        assert np.linalg.norm(hv - ref) <= 1e-11 * np.linalg.cond(B) * np.linalg.norm(ref)


@pytest.mark.parametrize("n,m,npairs", [c for c in CASES if min(c[1], c[2]) <= 32])
def test_diagonal_matrices(shim, n, m, npairs):
    rng = np.random.default_rng(7 + n + npairs)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs)
    wt = np.zeros((m, m), order="F")
    assert shim.qs_formt(m, _p(wt), _p(sy), _p(ss), col, C.c_double(theta)) == 0
    B = _dense_b(S, Y, theta)
    H = np.linalg.inv(B)
    sty = np.asfortranarray(S.T @ Y)
    yty = np.asfortranarray(Y.T @ Y)
    dg = np.ascontiguousarray(np.diag(sty))
    R = np.hstack([S, Y])  # rows r_i of [S, Y]
    for mode, alpha, ref, scale in ((0, theta, B, 1.0), (1, 1.0 / theta, H, np.linalg.cond(B))):
        nm = np.zeros((2 * col, 2 * col), order="F")
        assert shim.qs_nmat(mode, m, _p(sy), _p(wt), col, C.c_double(theta), _p(sty), _p(yty), _p(dg),
                            _p(nm)) == 0
        assert np.array_equal(nm, nm.T)  # symmetrised
        # the whole matrix, then its diagonal as the kernel forms it from the packed triangle
        full = alpha * np.eye(n) + R @ nm @ R.T
        assert np.abs(full - ref).max() <= 1e-11 * scale * np.abs(ref).max()
        mc = 5 if col <= 5 else 10 if col <= 10 else 20 if col <= 20 else 32
        packed = np.zeros((2 * mc) * (2 * mc + 1) // 2)
        shim.qs_pack_n(col, mc, _p(nm), _p(packed))
        rp = np.zeros((n, 2 * mc))
        rp[:, :col], rp[:, mc:mc + col] = S, Y
        iu = np.triu_indices(2 * mc)
        d = alpha + np.einsum("ik,k->i", rp[:, iu[0]] * rp[:, iu[1]], packed)
        assert np.abs(d - np.diag(ref)).max() <= 1e-11 * scale * np.abs(np.diag(ref)).max()


def test_no_pairs(shim):
    """col = 0: no coefficients (B = theta I, H = I / theta)"""
    z = np.zeros(1)
    assert shim.qs_coef_h(0, C.c_double(2.0), _p(z), _p(z), _p(z), _p(z), _p(z), _p(z), _p(z)) == 0
    assert shim.qs_coef_b(4, _p(z), _p(z), 0, C.c_double(2.0), _p(z), _p(z), _p(z), _p(z)) == 0


def test_nonpositive_curvature_refused(shim):
    col = 2
    sty = np.asfortranarray(np.array([[1.0, 0.5], [0.2, -1.0]]))
    dg = np.ascontiguousarray(np.diag(sty))
    yty = np.asfortranarray(np.eye(2))
    v = np.ones(2)
    cs, cy = np.zeros(2), np.zeros(2)
    assert shim.qs_coef_h(col, C.c_double(1.0), _p(sty), _p(yty), _p(dg), _p(v), _p(v), _p(cs), _p(cy)) == 2
