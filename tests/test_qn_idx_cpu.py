"""CPU tests of the host side of the entries at index lists (lbfgsb_hip_qn_block / qn_cols and the shifted twins):
qn_entries and qn_shift_entries of host_dense.hpp, and the index check and the chunk plan of qn_idx.hpp, through a
g++-built doorway (tests/qn_idx_shim.cpp).  The pairs are BFGS pairs of a random SPD quadratic
(tests/test_qn_root_cpu.py, _pairs), n = 300, col in {0, 1, 3, 10, 17, 40}; the gathered rows are the rows of the
numpy S and Y at the indices.
  The plain block against the dense B and inv(B) at np.ix_(ia, ib), within 1e-12 cond(B) max|ref|.
  The shifted block against the inverse of the dense free block of B + mu I + D with half the rows pinned, within
  1e-12 cond max|ref|; pinned rows and columns exactly +0.
  ib = ia: symmetric bit for bit.  Repeated indices: repeated rows and columns.
  The chunk plan covers every list exactly once and in order for every k <= 300, col <= 64 and buffer capacity; the
  index check refuses -1 and n_global and accepts 0 and n_global - 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_qn_root_cpu import _dense_b, _p, _pairs

HERE = os.path.dirname(os.path.abspath(__file__))
N = 300
COLS = [0, 1, 3, 10, 17, 40]
MU = 0.3


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_idx_shim")
    so = str(out / "libqn_idx_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_idx_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qi_bad.restype = C.c_int64
    lib.qi_bad.argtypes = [C.c_int64, C.c_void_p, C.c_int64]
    lib.qi_walk.argtypes = [C.c_int64, C.c_int, C.c_int64]
    lib.qi_walk_all.restype = C.c_int64
    lib.qi_walk_all.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.qi_entries.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_int64]
    lib.qi_shift_entries.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int64]
    return lib


@pytest.fixture(scope="module")
def sets():
    """per col: the pairs and the dense references, made once"""
    out = {}
    for col in COLS:
        rng = np.random.default_rng(4000 + col)
        if col == 0:
            z = np.zeros((N, 0))
            S, Y, theta, sy, ss, m = z, z.copy(), 1.7, np.zeros((1, 1), order="F"), np.zeros((1, 1), order="F"), 1
        else:
            S, Y, c, theta, sy, ss = _pairs(rng, N, col, col)
            assert c == col
            m = col
        B = _dense_b(S, Y, theta)
        dd = rng.uniform(0.0, 10.0, N)
        free = np.ones(N, bool)
        free[::2] = False
        w = np.where(free, 1.0 / (theta + MU + dd), 0.0)
        A = (B + np.diag(MU + dd))[np.ix_(free, free)]
        sig = np.zeros((N, N))
        sig[np.ix_(free, free)] = np.linalg.inv(A)
        out[col] = dict(S=S, Y=Y, theta=theta, sy=sy, ss=ss, m=m, B=B, H=np.linalg.inv(B), cond=np.linalg.cond(B),
                        w=w, free=free, sig=sig, cond_a=np.linalg.cond(A))
    return out


def _lists(col):
    """two lists over pinned (even) and free (odd) rows, unsorted, the first with a repeated index"""
    rng = np.random.default_rng(77 + col)
    ia = np.concatenate([[0, N - 1, 1, N - 2], rng.choice(N, 9, replace=False)]).astype(np.int64)
    ia = np.concatenate([ia, ia[[5]]])  # (one row repeated)
    ib = np.concatenate([[N - 1, 3], rng.choice(N, 7, replace=False), ia[[2]]]).astype(np.int64)
    return ia, ib


def _rows(s, idx):
    return np.asfortranarray(np.hstack([s["S"], s["Y"]])[idx, :].reshape(len(idx), -1))


def _block(shim, s, col, mode, ia, ib):
    m, S, Y = s["m"], s["S"], s["Y"]
    wt = np.zeros((m, m), order="F")
    if col:
        assert shim.qi_formt(m, _p(wt), _p(s["sy"]), _p(s["ss"]), col, C.c_double(s["theta"])) == 0
    sty, yty = np.asfortranarray(S.T @ Y), np.asfortranarray(Y.T @ Y)
    if not col:
        sty = yty = np.zeros((1, 1), order="F")
    dg = np.ascontiguousarray(np.diag(sty))
    ra = _rows(s, ia)
    rb = ra if ib is None else _rows(s, ib)
    kb = len(ia) if ib is None else len(ib)
    a = np.full((len(ia), kb), np.nan, order="F")
    rc = shim.qi_entries(mode, m, _p(s["sy"]), _p(wt), col, s["theta"], _p(sty), _p(yty), _p(dg), _p(ra), len(ia),
                         _p(ia), _p(rb), kb, None if ib is None else _p(ib), _p(a), len(ia))
    assert rc == 0
    return a


def _shift_block(shim, s, col, ia, ib):
    m, S, Y, w = s["m"], s["S"], s["Y"], s["w"]
    W = np.hstack([S, Y])
    gw = np.asfortranarray(W.T @ (w[:, None] * W)) if col else np.zeros((1, 1), order="F")
    sts = np.asfortranarray(S.T @ S) if col else np.zeros((1, 1), order="F")
    ra, wa = _rows(s, ia), np.ascontiguousarray(w[ia])
    rb, wb = (ra, wa) if ib is None else (_rows(s, ib), np.ascontiguousarray(w[ib]))
    kb = len(ia) if ib is None else len(ib)
    a = np.full((len(ia), kb), np.nan, order="F")
    rc = shim.qi_shift_entries(col, s["theta"], _p(s["sy"]), m, _p(sts), _p(gw), _p(ra), _p(wa), len(ia), _p(ia),
                               _p(rb), _p(wb), kb, None if ib is None else _p(ib), _p(a), len(ia))
    assert rc == 0
    return a


@pytest.mark.parametrize("col", COLS)
def test_block_against_dense(shim, sets, col):
    s = sets[col]
    ia, ib = _lists(col)
    for mode, A in ((0, s["B"]), (1, s["H"])):
        for jb in (ib, None):
            got = _block(shim, s, col, mode, ia, jb)
            ref = A[np.ix_(ia, ia if jb is None else jb)]
            err, bound = np.abs(got - ref).max(), 1e-12 * s["cond"] * np.abs(ref).max()
            print("col %d mode %d %s: off by %.2e (bound %.2e)" % (col, mode, "rect" if jb is not None else "square",
                                                                  err, bound))
            assert err <= bound
            if jb is None:
                assert np.array_equal(got, got.T)  # (bit for bit)
                assert np.array_equal(got[-1, :], got[5, :]) and np.array_equal(got[:, -1], got[:, 5])
            else:
                assert np.array_equal(got[-1, :], got[5, :])


@pytest.mark.parametrize("col", COLS)
def test_shift_block_against_dense(shim, sets, col):
    s = sets[col]
    ia, ib = _lists(col)
    for jb in (ib, None):
        got = _shift_block(shim, s, col, ia, jb)
        jbb = ia if jb is None else jb
        ref = s["sig"][np.ix_(ia, jbb)]
        err, bound = np.abs(got - ref).max(), 1e-12 * s["cond_a"] * np.abs(ref).max()
        print("col %d %s: off by %.2e (bound %.2e)" % (col, "rect" if jb is not None else "square", err, bound))
        assert err <= bound
        pa, pb = ~s["free"][ia], ~s["free"][jbb]
        assert pa.any() and pb.any() and (~pa).any() and (~pb).any()
        pinned = got[pa, :], got[:, pb]
        for blk in pinned:
            assert np.all(blk == 0.0) and not np.signbit(blk).any()
        if jb is None:
            assert np.array_equal(got, got.T)
            assert np.array_equal(got[-1, :], got[5, :]) and np.array_equal(got[:, -1], got[:, 5])


def test_chunks_cover_every_list(shim):
    walks = np.zeros(1, np.int64)
    bad = shim.qi_walk_all(300, 64, _p(walks))
    print("%d walks, %d bad" % (walks[0], bad))
    assert walks[0] > 1_000_000 and bad == 0
    # every capacity of one shape, not only the ends of each count, and a buffer that holds no row
    for cap in range(21, 21 * 40):
        assert shim.qi_walk(37, 21, cap) == -(-37 // (cap // 21))
    assert shim.qi_walk(5, 21, 20) == -1  # (no chunk: nothing is covered)
    # the library's own buffer holds a row at the largest memory, with the weight along
    assert shim.qi_walk(shim.qi_maxk(), 2 * 1024 + 1, shim.qi_buf()) > 0


def test_index_check(shim):
    n = 4099
    for idx, bad in (([0], -1), ([n - 1], -1), ([0, n - 1, 5, 5], -1), ([-1], 0), ([n], 0), ([3, n - 1, n], 2),
                     ([3, -1, n], 1), ([2 ** 40], 0), ([-2 ** 62], 0)):
        a = np.array(idx, np.int64)
        assert shim.qi_bad(len(a), _p(a), n) == bad
