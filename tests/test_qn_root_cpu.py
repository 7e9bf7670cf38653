"""CPU tests of the host algebra behind the square roots, log-determinants and draws of the curvature model
(lbfgsb_hip_qn_apply's root modes, lbfgsb_hip_qn_logdet, lbfgsb_hip_qn_draw): the cyclic Jacobi eigensolver, the
matrix C of A^(1/2) = sqrt(alpha) I + [S, Y] C [S, Y]' and the log-det sum against dense numpy models built by the
recursive BFGS updates (the pair sets of tests/test_qn_host_cpu.py plus one of 64 pairs), nearly parallel pairs, an
indefinite model, and the Philox4x32-10 generator's known answers and uniforms -- all through a g++-built doorway
(tests/qn_root_shim.cpp).  Then, from the built library's code objects: no scratch in any kernel of the draws."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_root_shim")
    so = str(out / "libqn_root_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_root_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.rs_uniforms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.rs_uniforms.restype = None
    lib.rs_root_n.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pairs(rng, n, m, npairs, parallel=None, shrink=1.0):
    """as tests/test_qn_host_cpu.py::_pairs; parallel = eps: the last s is the one before it up to eps; shrink: every
    step is that much shorter than the one before it, as the steps of a converging run are"""
    A = rng.standard_normal((n, n))
    A = A @ A.T / n + np.eye(n)
    S, Y = [], []
    for k in range(npairs):
        s = rng.standard_normal(n) * shrink ** k
        if parallel is not None and k == npairs - 1:
            s = S[-1] + parallel * s
        S.append(s)
        Y.append(A @ s + (0.0 if parallel is not None else 1e-3 * shrink ** k) * rng.standard_normal(n))
    col = min(npairs, m)
    S, Y = np.array(S[-col:]).T, np.array(Y[-col:]).T
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


def _root(shim, mode, S, Y, col, theta, sy, ss, m):
    wt = np.zeros((m, m), order="F")
    assert shim.rs_formt(m, _p(wt), _p(sy), _p(ss), col, C.c_double(theta)) == 0
    sty = np.asfortranarray(S.T @ Y)
    yty = np.asfortranarray(Y.T @ Y)
    dg = np.ascontiguousarray(np.diag(sty))
    W = np.hstack([S, Y])
    G = np.asfortranarray(W.T @ W)
    d = 2 * col
    nm, cm = np.zeros((d, d), order="F"), np.zeros((d, d), order="F")
    ls = np.zeros(1)
    rc = shim.rs_root(mode, m, _p(sy), _p(wt), col, C.c_double(theta), _p(sty), _p(yty), _p(dg), _p(G), _p(nm),
                      _p(cm), _p(ls))
    return rc, W, cm, float(ls[0])


CASES = [(12, 1, 1), (12, 3, 2), (20, 5, 5), (40, 10, 17), (70, 17, 30), (80, 32, 32), (90, 32, 45), (300, 64, 80)]


@pytest.mark.parametrize("n,m,npairs", CASES)
def test_root_and_logdet_against_dense_model(shim, n, m, npairs):
    rng = np.random.default_rng(1000 * n + npairs)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs)
    B = _dense_b(S, Y, theta)
    H = np.linalg.inv(B)
    cond = np.linalg.cond(B)
    lds = []
    for mode, alpha, A, scale in ((0, theta, B, 1.0), (1, 1.0 / theta, H, cond)):
        rc, W, cm, ls = _root(shim, mode, S, Y, col, theta, sy, ss, m)
        assert rc == 0
        assert np.array_equal(cm, cm.T)
        R = np.sqrt(alpha) * np.eye(n) + W @ cm @ W.T
        err = np.linalg.norm(R @ R - A, 2) / np.linalg.norm(A, 2)
        print("mode %d: |R^2 - A| / |A| = %.3e (cond %.2e)" % (mode, err, cond))
        assert err <= 1e-11 * scale
        ld = n * np.log(alpha) + ls
        sign, ref = np.linalg.slogdet(A)
        assert sign == 1.0
        print("mode %d: log det %.15e, slogdet %.15e" % (mode, ld, ref))
        assert abs(ld - ref) <= 1e-10 * n
        lds.append(ld)
    assert abs(lds[0] + lds[1]) <= 1e-10 * n


def test_nearly_parallel_pairs(shim):
    """two columns of S parallel to 1e-7: cond(G) >= 1e14, and the root of B holds the same bound (no division by G)"""
    n, m, npairs = 60, 6, 6
    rng = np.random.default_rng(5)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs, parallel=1e-7)
    W = np.hstack([S, Y])
    assert np.linalg.cond(W.T @ W) >= 1e14
    B = _dense_b(S, Y, theta)
    rc, W, cm, ls = _root(shim, 0, S, Y, col, theta, sy, ss, m)
    assert rc == 0
    R = np.sqrt(theta) * np.eye(n) + W @ cm @ W.T
    err = np.linalg.norm(R @ R - B, 2) / np.linalg.norm(B, 2)
    print("|R^2 - B| / |B| = %.3e" % err)
    assert err <= 1e-11


def test_pairs_of_a_converging_run(shim):
    """steps that shrink by 0.3 per pair (17 pairs: a factor 2e8 between the oldest and the newest, 4e16 between the
    entries of their Gram): the same bounds as for pairs of one size"""
    n, m, npairs = 70, 17, 17
    rng = np.random.default_rng(11)
    S, Y, col, theta, sy, ss = _pairs(rng, n, m, npairs, shrink=0.3)
    B = _dense_b(S, Y, theta)
    cond = np.linalg.cond(B)
    for mode, alpha, A, scale in ((0, theta, B, 1.0), (1, 1.0 / theta, np.linalg.inv(B), cond)):
        rc, W, cm, ls = _root(shim, mode, S, Y, col, theta, sy, ss, m)
        assert rc == 0
        R = np.sqrt(alpha) * np.eye(n) + W @ cm @ W.T
        err = np.linalg.norm(R @ R - A, 2) / np.linalg.norm(A, 2)
        print("mode %d: |R^2 - A| / |A| = %.3e (cond %.2e)" % (mode, err, cond))
        assert err <= 1e-11 * scale
        assert abs(n * np.log(alpha) + ls - np.linalg.slogdet(A)[1]) <= 1e-10 * n


def test_not_positive_definite_refused(shim):
    """A = I + w (-3) w' with |w| = 1 has the eigenvalue -2: refused (-2), no root of a negative number"""
    g = np.asfortranarray(np.eye(2))
    nm = np.asfortranarray(np.diag([-3.0, 0.5]))
    cm = np.zeros((2, 2), order="F")
    ls = np.zeros(1)
    assert shim.rs_root_n(2, C.c_double(1.0), _p(g), _p(nm), _p(cm), _p(ls)) == -2
    nm = np.asfortranarray(np.diag([3.0, 0.5]))
    assert shim.rs_root_n(2, C.c_double(1.0), _p(g), _p(nm), _p(cm), _p(ls)) == 0
    assert abs(ls[0] - np.log(4.0 * 1.5)) <= 1e-14
    assert np.allclose(cm, np.diag([1.0, np.sqrt(1.5) - 1.0]), rtol=0, atol=1e-15)


def test_no_pairs(shim):
    z = np.zeros(1)
    ls = np.ones(1)
    assert shim.rs_root_n(0, C.c_double(2.0), _p(z), _p(z), _p(z), _p(ls)) == 0
    assert ls[0] == 0.0  # log det A = n log alpha alone


@pytest.mark.parametrize("d", [2, 20, 128])
def test_jacobi_against_eigh(shim, d):
    rng = np.random.default_rng(d)
    for trial in range(2):
        A = rng.standard_normal((d, d))
        A = A + A.T
        if trial == 1:  # rank-deficient, as a Gram of dependent columns is
            X = rng.standard_normal((d, max(1, d // 2)))
            A = X @ X.T
        a = np.asfortranarray(A.copy())
        v, w = np.zeros((d, d), order="F"), np.zeros(d)
        sweeps = shim.rs_jacobi(d, _p(a), _p(v), _p(w))
        assert 0 <= sweeps < 30, sweeps
        nrm = np.linalg.norm(A, 2)
        order = np.argsort(w)
        assert np.abs(w[order] - np.linalg.eigvalsh(A)).max() <= 1e-13 * nrm
        assert np.abs(v.T @ v - np.eye(d)).max() <= 1e-13
        assert np.abs(v @ np.diag(w) @ v.T - A).max() <= 1e-13 * nrm


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers(shim):
    for ctr, key, want in KNOWN:
        c, k, o = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        shim.rs_philox(_p(c), _p(k), _p(o))
        assert tuple(int(x) for x in o) == want, [hex(int(x)) for x in o]


def test_uniforms_of_four_counters(shim):
    """u = ((w0 2^32 + w1 >> 12) + 0.5) 2^-52 and v = (w2 2^32 + w3 >> 12) 2^-52 of counter (row lo, row hi, pair lo,
    pair hi) under key (seed lo, seed hi), against the raw words"""
    for seed, row, pair in ((0, 0, 0), (1, 5, 0), ((1 << 40) + 12345, (1 << 33) + 7, 3),
                            (0xffffffffffffffff, 0xffffffffffffffff, 0xffffffffffffffff)):
        c = np.array([row & 0xffffffff, row >> 32, pair & 0xffffffff, pair >> 32], np.uint32)
        k = np.array([seed & 0xffffffff, seed >> 32], np.uint32)
        o = np.zeros(4, np.uint32)
        shim.rs_philox(_p(c), _p(k), _p(o))
        a = (int(o[0]) << 32) | int(o[1])
        b = (int(o[2]) << 32) | int(o[3])
        u, v = np.zeros(1), np.zeros(1)
        shim.rs_uniforms(seed, row, pair, _p(u), _p(v))
        assert u[0] == ((a >> 12) + 0.5) / 2.0 ** 52 and 0.0 < u[0] < 1.0
        assert v[0] == (b >> 12) / 2.0 ** 52 and 0.0 <= v[0] < 1.0
    # the all-zero counter and key, from the known answer above
    shim.rs_uniforms(0, 0, 0, _p(u), _p(v))
    assert u[0] == ((0x6627e8d5e169c58d >> 12) + 0.5) / 2.0 ** 52 and v[0] == (0xbc57ac4c9b00dbd8 >> 12) / 2.0 ** 52


def test_draw_kernels_use_no_scratch():
    """every qn_wtz_kernel / qn_draw_kernel instantiation in the built library: no private segment, registers within
    the file (read from the code objects, as tests/test_code_objects_cpu.py does)"""
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(ROOT, "profiles", "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.collect([os.path.join(ROOT, "lbfgsb_amd", "liblbfgsb_hip.so")])
    for name in ("qn_wtz_kernel<", "qn_draw_kernel<"):
        mine = [r for r in rows if kr.short(r["kernel"]).startswith(name)]
        # fp64: 3 tiles x K {1, 2, 4 | 1, 2} x NT, natural order (V = 1; V = 2 where 2 MC K <= 20) and the layout; fp32
        assert len(mine) >= 60, (name, len(mine))
        bad = [(kr.short(r["kernel"]), r["scratch"]) for r in mine if r["scratch"] != 0 or r["dyn_stack"] == "true"]
        assert not bad, bad
        assert all(r["vgpr"] <= 512 for r in mine)
