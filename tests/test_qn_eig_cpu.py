"""CPU tests of the host algebra behind the eigenvalues and eigenvectors of the curvature model (lbfgsb_hip_qn_eig /
lbfgsb_hip_qn_eigvec; host_dense.hpp, qn_eig over qn_spectrum) through a g++-built doorway (tests/qn_eig_shim.cpp),
against dense numpy models built by the recursive BFGS updates: the pair sets of tests/test_qn_root_cpu.py (its CASES,
shrinking steps, nearly parallel pairs, the indefinite model) plus sets with fewer rows than columns.  With
A = alpha I + W N W', the r returned eigenvalues and U = W C formed in numpy:
  rank r <= min(2col, n) (< 2col for parallel pairs), {lambda} u {alpha x (n - r)} against eigvalsh(A), U'U = I,
  A U = U Lambda, alpha I + U diag(lambda - alpha) U' = A, the eigenvalues of B and H reciprocal, the sign rule.
Bounds (the root tests'): 1e-11 relative in the 2-norm for B and for eigenvalues, times cond(B) for H; for the
parallel sets every error is relative to max |lambda| and multiplied by cond of the unit-column Gram.  Then the
plan of the basis pass, walked exhaustively by tests/qn_basis_plan_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_qn_root_cpu import CASES, _dense_b, _p, _pairs

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-11


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_eig_shim")
    so = str(out / "libqn_eig_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_eig_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.es_cut.restype = C.c_double
    lib.es_eig_n.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                             C.c_void_p]
    return lib


def _eig(shim, mode, S, Y, col, theta, sy, ss, m):
    """(rc, W, r, lambda, C): the shim on the pair set; W = [S, Y], C the 2col x r coefficient columns"""
    n = S.shape[0]
    wt = np.zeros((m, m), order="F")
    assert shim.es_formt(m, _p(wt), _p(sy), _p(ss), col, C.c_double(theta)) == 0
    sty = np.asfortranarray(S.T @ Y)
    yty = np.asfortranarray(Y.T @ Y)
    dg = np.ascontiguousarray(np.diag(sty))
    W = np.hstack([S, Y])
    G = np.asfortranarray(W.T @ W)
    d = 2 * col
    nm, cf = np.zeros((d, d), order="F"), np.zeros((d, d), order="F")
    lam = np.zeros(d)
    r = np.zeros(1, np.int32)
    rc = shim.es_eig(mode, m, _p(sy), _p(wt), col, C.c_double(theta), _p(sty), _p(yty), _p(dg), _p(G),
                     C.c_int64(min(d, n)), _p(nm), _p(r), _p(lam), _p(cf))
    return rc, W, int(r[0]), lam[:int(r[0])].copy(), cf[:, :int(r[0])].copy()


def _check_sign(cf):
    for j in range(cf.shape[1]):
        c = cf[:, j]
        big = int(np.argmax(np.abs(c)))  # (the first of equals)
        assert c[big] > 0.0, (j, big, c[big])


def _check(shim, tag, S, Y, col, theta, sy, ss, m, gfac=1.0, rank_below=False):
    """both modes of one pair set; gfac: the factor cond(G_scaled) of the parallel sets (1 otherwise), with which
    every error is taken relative to max |lambda|"""
    n = S.shape[0]
    B = _dense_b(S, Y, theta)
    H = np.linalg.inv(B)
    cond = np.linalg.cond(B)
    lams = []
    for mode, alpha, A, scale in ((0, theta, B, 1.0), (1, 1.0 / theta, H, cond)):
        rc, W, r, lam, cf = _eig(shim, mode, S, Y, col, theta, sy, ss, m)
        assert rc == 0
        assert r <= min(2 * col, n), (r, col, n)
        if rank_below:
            assert r < 2 * col, r
        assert np.all(np.diff(lam) >= 0.0)
        assert np.all(np.abs(lam - alpha) > shim.es_cut() * alpha)
        _check_sign(cf)
        ref = np.linalg.eigvalsh(A)
        lmax = np.abs(ref).max()
        bound = TOL * scale * gfac
        got = np.sort(np.concatenate([lam, np.full(n - r, alpha)]))
        e_val = np.abs(got - ref).max() / lmax
        U = W @ cf
        e_orth = np.abs(U.T @ U - np.eye(r)).max() if r else 0.0
        e_res = np.linalg.norm(A @ U - U * lam, 2) / lmax if r else 0.0
        e_rec = np.linalg.norm(alpha * np.eye(n) + (U * (lam - alpha)) @ U.T - A, 2) / np.linalg.norm(A, 2)
        print("%s mode %d: r %d of %d, eigenvalues %.2e, U'U - I %.2e, AU - UL %.2e, reconstruction %.2e "
              "(bound %.2e, cond %.2e)" % (tag, mode, r, 2 * col, e_val, e_orth, e_res, e_rec, bound, cond))
        assert e_val <= bound and e_orth <= bound and e_res <= bound and e_rec <= bound
        lams.append(got)
    e_inv = np.abs(lams[0] * lams[1][::-1] - 1.0).max()
    print("%s: |lambda_B lambda_H - 1| = %.2e" % (tag, e_inv))
    assert e_inv <= TOL * cond * gfac


@pytest.mark.parametrize("n,m,npairs", CASES)
def test_spectrum_against_dense_model(shim, n, m, npairs):
    rng = np.random.default_rng(1000 * n + npairs)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs)
    _check(shim, "n %d m %d" % (n, m), S, Y, col, theta, sy, ss, m)


@pytest.mark.parametrize("shrink", [0.3, 0.1])
def test_pairs_of_a_converging_run(shim, shrink):
    """steps that shrink by 0.3 (17 pairs) or 0.1 (10 pairs) per pair: the same bounds as for pairs of one size"""
    n, m = 70, 17 if shrink == 0.3 else 10
    rng = np.random.default_rng(11)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, m, shrink=shrink)
    _check(shim, "shrink %g" % shrink, S, Y, col, theta, sy, ss, m)


@pytest.mark.parametrize("eps", [1e-6, 1e-9])
def test_nearly_parallel_pairs(shim, eps):
    """the last pair parallel to the one before it up to eps: its directions fall under the cut (r < 2col), the
    others keep their accuracy -- no division by G"""
    n, m, npairs = 60, 6, 6
    rng = np.random.default_rng(5)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs, parallel=eps)
    W = np.hstack([S, Y])
    Ws = W / np.linalg.norm(W, axis=0)
    gfac = np.linalg.cond(Ws.T @ Ws)
    assert gfac >= 1e10
    _check(shim, "parallel %g" % eps, S, Y, col, theta, sy, ss, m, gfac=gfac, rank_below=True)


@pytest.mark.parametrize("n,col", [(1, 1), (3, 2), (3, 3)])
def test_fewer_rows_than_columns(shim, n, col):
    rng = np.random.default_rng(77 + 10 * n + col)
    S, Y, c, theta, sy, ss = _pairs(rng, n, col, col)
    assert c == col and 2 * col > n
    _check(shim, "n %d col %d" % (n, col), S, Y, col, theta, sy, ss, col)


def _driven_pairs(po, n, m, iters):
    """the pairs of the plain-C oracle's run of the bounded Rosenbrock problem at its NEW_X return number `iters`: the
    states of tests/test_gpu_qn_eig.py -- updates that nearly agree with the model they update, and at many pairs a
    unit-column Gram that is numerically singular"""
    p = po.problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)
    snaps = []
    po.run(po.Engine("oracle"), p, max_iter=iters,
           snapshot=lambda k, s: snaps.append(s.copy()) if s.task_s.startswith("NEW_X") else None)
    s = snaps[-1]
    head, col, theta = int(s.isave[26]), int(s.isave[27]), float(s.dsave[0])
    cols = [(head - 1 + j) % m for j in range(col)]
    S, Y = s.wa[:m * n].reshape(m, n)[cols].T.copy(), s.wa[m * n:2 * m * n].reshape(m, n)[cols].T.copy()
    sy, ss = np.zeros((col, col), order="F"), np.zeros((col, col), order="F")
    sy[:, :], ss[:, :] = np.tril(S.T @ Y), np.triu(S.T @ S)
    return S, Y, col, theta, sy, ss


@pytest.mark.parametrize("n,m,iters", [(65, 10, 14), (257, 11, 14), (257, 16, 20), (1000, 17, 20), (1000, 33, 34)])
def test_pairs_of_driven_runs(oracle_built, shim, n, m, iters):
    """the bounds of the GPU tests on the host algebra alone: |A U - U Lambda|_F <= 1e-10 |B| |U| for B and 1e-10
    cond |U Lambda| for H on every returned vector, U'U - I <= 1e-10 cond |U| on the vectors at least 1e-3 alpha off
    the bulk value.  (c = (N P V)_i / delta_i alone gives 1.9e-7 against 1.2e-7 at 33 pairs, 1.6e-7 against 8.9e-8 at
    16 and 8.8e-8 against 7.1e-8 at 11; with the step of inverse iteration 7e-9, 7e-9 and 3e-10.)"""
    S, Y, col, theta, sy, ss = _driven_pairs(oracle_built, n, m, iters)
    assert col == m
    B = _dense_b(S, Y, theta)
    cond, nb = np.linalg.cond(B), np.linalg.norm(B, 2)
    for mode, alpha, A in ((0, theta, B), (1, 1.0 / theta, np.linalg.inv(B))):
        rc, W, r, lam, cf = _eig(shim, mode, S, Y, col, theta, sy, ss, col)
        assert rc == 0 and 1 <= r <= 2 * col
        U = W @ cf
        res = np.linalg.norm(A @ U - U * lam)
        bound = 1e-10 * nb * np.linalg.norm(U) if mode == 0 else 1e-10 * cond * np.linalg.norm(U * lam)
        sep = np.abs(lam - alpha) >= 1e-3 * alpha
        orth = np.linalg.norm(U[:, sep].T @ U[:, sep] - np.eye(int(sep.sum())))
        print("n %d col %d mode %d: r %d, |AU - UL| %.2e (bound %.2e), U'U - I on %d separated %.2e (bound %.2e)"
              % (n, col, mode, r, res, bound, int(sep.sum()), orth, 1e-10 * cond * np.sqrt(sep.sum())))
        assert res <= bound and orth <= 1e-10 * cond * np.sqrt(sep.sum())
        _check_sign(cf)


def test_not_positive_definite_refused(shim):
    """A = I + w (-3) w' with |w| = 1 has the eigenvalue -2: refused (-2), as the root refuses it"""
    g = np.asfortranarray(np.eye(2))
    nm = np.asfortranarray(np.diag([-3.0, 0.5]))
    cf, lam, r = np.zeros((2, 2), order="F"), np.zeros(2), np.ones(1, np.int32)
    assert shim.es_eig_n(2, C.c_double(1.0), _p(g), _p(nm), 2, _p(r), _p(lam), _p(cf)) == -2 and r[0] == 0
    nm = np.asfortranarray(np.diag([3.0, 0.5]))
    assert shim.es_eig_n(2, C.c_double(1.0), _p(g), _p(nm), 2, _p(r), _p(lam), _p(cf)) == 0 and r[0] == 2
    assert np.allclose(lam, [1.5, 4.0], rtol=0, atol=1e-15)
    assert np.allclose(cf, [[0.0, 1.0], [1.0, 0.0]], rtol=0, atol=1e-15)


def test_bulk_directions_are_cut(shim):
    """delta = 1e-9 alpha is bulk, delta = 1e-7 alpha is returned; no pairs: r = 0"""
    g = np.asfortranarray(np.eye(2))
    nm = np.asfortranarray(np.diag([2e-9, 2e-7]))
    cf, lam, r = np.zeros((2, 2), order="F"), np.zeros(2), np.zeros(1, np.int32)
    assert shim.es_eig_n(2, C.c_double(2.0), _p(g), _p(nm), 2, _p(r), _p(lam), _p(cf)) == 0
    assert r[0] == 1 and lam[0] == 2.0 + 2e-7 and np.allclose(cf[:, 0], [0.0, 1.0], rtol=0, atol=1e-15)
    z = np.zeros(1)
    r[0] = 5
    assert shim.es_eig_n(0, C.c_double(2.0), _p(z), _p(z), 0, _p(r), _p(z), _p(z)) == 0 and r[0] == 0


def test_basis_plan_walk(tmp_path):
    exe = str(tmp_path / "qn_basis_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HERE, "qn_basis_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
