"""Gram matrices of the curvature model on blocks of vectors (lbfgsb_hip_qn_gram) without a GPU: the two new kernels
read from the code objects of the built library (profiles/scripts/kernel_resources.py, as tests/test_qn_quad_cpu.py
does) -- every instantiation of qn_wtg_kernel and qn_dtd_kernel present, none with a private segment or a dynamic
stack, and at the shapes DESIGN.md section 10d quotes (fp64, 10 columns) the Gram pass at the waves per SIMD of the
quadratic form's pass -- and the host combination G = alpha D'D + P'N P (host_dense.hpp, qn_gram_combine) against
numpy through a shim of its own (tests/qn_gram_shim.cpp)."""
import ctypes as C
import importlib.util
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def kernels():
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(ROOT, "profiles", "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.collect([os.path.join(ROOT, "lbfgsb_amd", "liblbfgsb_hip.so")])
    return {kr.short(r["kernel"]): r for r in rows}


def _wtg_names():
    """(T, MC, K, V, CW, NT, CEN) of the dispatch in k_qn_common.hpp: tiles of 5, 10, 16 columns, blocks of 2 and 4
    vectors (4 up to 10 columns; one vector is qn_wtd_kernel's DD), one or two rows per lane in natural order, the
    layout for fp64 up to 10 columns, both cache policies, with and without a center"""
    for t, mc in itertools.product(("double", "float"), (5, 10, 16)):
        for k in (2, 4) if mc <= 10 else (2,):
            shapes = [(1, "false"), (2, "false")] + ([(1, "true")] if t == "double" and mc <= 10 else [])
            for (v, cw), nt, cen in itertools.product(shapes, ("false", "true"), ("false", "true")):
                yield "qn_wtg_kernel<%s, %d, %d, %d, %s, %s, %s>" % (t, mc, k, v, cw, nt, cen)


def _dtd_names():
    """(T, KA, KB, V, NT, CEN): every pair of piece widths, one or two rows per lane"""
    for t, ka, kb, v, nt, cen in itertools.product(("double", "float"), (1, 2, 4), (1, 2, 4), (1, 2),
                                                   ("false", "true"), ("false", "true")):
        yield "qn_dtd_kernel<%s, %d, %d, %d, %s, %s>" % (t, ka, kb, v, nt, cen)


@pytest.mark.parametrize("kernel,names,count", [("qn_wtg_kernel", _wtg_names, 96), ("qn_dtd_kernel", _dtd_names, 144)])
def test_gram_kernels_present_and_without_scratch(kernels, kernel, names, count):
    want = set(names())
    have = {name for name in kernels if name.startswith(kernel + "<")}
    assert len(want) == count
    assert have == want, (sorted(want - have)[:5], sorted(have - want)[:5])  # (no K = 1 copy of qn_wtd's DD)
    bad = [(name, kernels[name]["scratch"], kernels[name]["dyn_stack"]) for name in sorted(have)
           if kernels[name]["scratch"] != 0 or kernels[name]["dyn_stack"] == "true"]
    assert not bad, bad
    assert all(kernels[name]["vgpr"] <= 512 for name in have)


def test_gram_pass_at_the_headline_shapes(kernels):
    """fp64, a tile of 10 columns: K = 4 with one row per lane in natural order and on the layout, K = 2 with two
    rows per lane.  The K (K + 1) / 2 - K more accumulators (6 at K = 4, 1 at K = 2) cost two registers each and no
    wave per SIMD against qn_wtd_kernel<..., CEN, DD = true> of the same shape."""
    for k, v, cw in ((4, 1, "false"), (4, 1, "true"), (2, 2, "false")):
        head = "double, 10, %d, %d, %s" % (k, v, cw)
        for nt, cen in itertools.product(("false", "true"), repeat=2):
            a = kernels["qn_wtd_kernel<%s, %s, %s, true>" % (head, nt, cen)]
            b = kernels["qn_wtg_kernel<%s, %s, %s>" % (head, nt, cen)]
            print(head, nt, cen, "qn_wtd vgpr %d waves %d, qn_wtg vgpr %d waves %d"
                  % (a["vgpr"], a["waves_per_simd"], b["vgpr"], b["waves_per_simd"]))
            assert b["waves_per_simd"] == a["waves_per_simd"], (head, nt, cen)
            assert 0 <= b["vgpr"] - a["vgpr"] <= 2 * (k * (k + 1) // 2 - k) + 4, (head, nt, cen, a["vgpr"], b["vgpr"])


# ---------------------------------------------------------------- the host combination
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_gram_shim")
    so = str(out / "libqn_gram_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_gram_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qgs_combine.argtypes = [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_int64]
    lib.qgs_combine_failing.argtypes = [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_int64]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("d2", [0, 2, 20, 34])
@pytest.mark.parametrize("k", [1, 3, 9])
def test_host_combination_against_numpy(shim, d2, k):
    """random symmetric N, P and a D'D of which only the upper triangle is handed over (the lower one is poisoned).
    Tolerance: g_ab is one product N p_b (2col terms a row), one inner product of 2col terms, one multiplication and
    one addition, numpy's reference the same: 2 (2 (2col) + 2) u times the sum of the absolute values of the terms,
    u = 2^-53 (the standard bound of a recursive inner product, both sides)."""
    rng = np.random.default_rng(100 * d2 + k)
    col, alpha, ldg = d2 // 2, 0.37, k + 2
    nm = rng.standard_normal((d2, d2))
    nm = np.asfortranarray(nm + nm.T)
    p = np.asfortranarray(rng.standard_normal((d2, k)))
    dm = rng.standard_normal((k + 5, k))
    dtd_full = dm.T @ dm
    dtd = np.asfortranarray(np.triu(dtd_full) + np.tril(np.full((k, k), np.nan), -1))
    g = np.full((ldg, k), -7.0, order="F")
    assert shim.qgs_combine(col, k, alpha, _p(nm), _p(p), _p(dtd), k, _p(g), ldg) == 0
    assert np.all(g[k:] == -7.0)                                   # the padding rows are not touched
    got = g[:k]
    assert np.array_equal(got, got.T) and np.all(np.isfinite(got))  # symmetric bit for bit
    ref = alpha * dtd_full + p.T @ nm @ p
    mag = alpha * np.abs(dtd_full) + np.abs(p).T @ np.abs(nm) @ np.abs(p)
    tol = 2.0 * (2 * d2 + 2) * 2.0 ** -53 * mag
    err = np.abs(got - ref)
    print("2col %d k %d: max |g - ref| / tolerance = %.3f" % (d2, k, (err / tol).max()))
    assert np.all(err <= tol)
    if d2 == 0:
        assert np.array_equal(np.triu(got), np.triu(alpha * dtd_full))


def test_host_combination_leaves_g_alone_on_failure(shim):
    col, k = 3, 4
    p = np.asfortranarray(np.ones((2 * col, k)))
    dtd = np.asfortranarray(np.eye(k))
    g = np.full((k, k), -7.0, order="F")
    assert shim.qgs_combine_failing(col, k, 1.0, _p(p), _p(dtd), k, 2, _p(g), k) == 7
    assert np.all(g == -7.0)
    assert shim.qgs_combine_failing(col, k, 1.0, _p(p), _p(dtd), k, 99, _p(g), k) == 0
    assert np.array_equal(g, np.eye(k) + 2.0 * col)
