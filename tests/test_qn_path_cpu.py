"""CPU tests of the host algebra behind the model along a path of shifts (lbfgsb_hip_qn_path_*; host_dense.hpp,
qn_path_factor, qn_path_shift, qn_path_eval and qn_path_secular) through a g++-built doorway (tests/qn_path_shim.cpp).
The pairs are tests/test_qn_shift_cpu.py's (BFGS pairs of a random SPD quadratic, n = 300, col in {0, 1, 3, 10, 17,
40}), with no pins and with half the rows pinned; the shifts are mu in {-lambda_min(B_FF) / 2, 0, 0.3, 5, 1e4 theta}.
With A = B_FF + mu I dense in numpy:
  the coefficients within 1e-12 cond(K) of a dense solve with K, the solve w o (v + R c) within 1e-12 cond(A);
  log det within 1e-10 n of slogdet;
  ||x||^2, v'x and x'A^-1 x within 4e-12 cond(A) relative (that file's family, the factor 2 for a squared quantity);
  the factor is qn_shift_factor's on the explicitly weighted Gram bit for bit when w is a power of two;
  mu below -lambda_min is info 2, theta + mu <= 0 info 1;
  the secular iteration: mu = 0 exactly when Delta >= ||x(0)||, else | ||x|| - Delta | <= rtol Delta, mu against a
  bisection on the spectrum in np.longdouble, the evaluations under max_it, the adjacent-doubles exit at rtol = 1e-17.
The same code runs once more as a program of its own under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_qn_root_cpu import _dense_b, _p
from test_qn_shift_cpu import COLS, N, _dense_k, _set

HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = [2.0, 1.0, 0.9, 0.1, 1e-3, 1e-9]
D = C.c_double


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_path_shim")
    so = str(out / "libqn_path_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_path_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    for f in (lib.qp_factor, lib.qp_shift_factor, lib.qp_shift, lib.qp_eval, lib.qp_secular):
        f.restype = C.c_int
    return lib


class Case:
    """the pairs, the free rows, and what qn_path_set would hold: G_F, the blocks of M^-1, log |det M^-1|"""

    def __init__(self, shim, col, pin):
        rng = np.random.default_rng(1000 * col + pin)
        self.S, self.Y, self.col, self.theta, sy, ss, m = _set(rng, col)
        col = self.col
        self.free = np.ones(N, bool)
        if pin:
            self.free[::2] = False
        self.nf = int(self.free.sum())
        self.R = np.hstack([self.S, self.Y])
        RF = self.R[self.free]
        self.RF = RF
        d = max(2 * col, 1)
        self.gf = np.zeros((d, d), order="F")
        if col:
            g = RF.T @ RF.copy()  # (two arrays: gemm, as the weighted Gram below -- not syrk)
            self.gf[:] = 0.5 * (g + g.T)
        self.sy = np.asfortranarray(sy[:max(col, 1), :max(col, 1)])
        self.sts = np.asfortranarray(self.S.T @ self.S) if col else np.zeros((1, 1), order="F")
        km = np.zeros((d, d), order="F")
        ldm = D(0.0)
        assert shim.qp_shift_factor(col, D(self.theta), _p(self.sy), _p(self.sts), None, _p(km), C.byref(ldm)) == 0
        self.ldm = ldm.value
        self.A0 = _dense_b(self.S, self.Y, self.theta)[np.ix_(self.free, self.free)]
        self.lam = np.linalg.eigvalsh(self.A0)
        self.v = rng.standard_normal(N)
        self.p = np.ascontiguousarray(RF.T @ self.v[self.free]) if col else np.zeros(1)
        self.vv = float(self.v[self.free] @ self.v[self.free])

    def mus(self):
        return [-0.5 * self.lam[0], 0.0, 0.3, 5.0, 1e4 * self.theta]

    def shift(self, shim, mu):
        """(info, w, kf, log det)"""
        d = max(2 * self.col, 1)
        kf = np.zeros((d, d), order="F")
        w, ld = D(0.0), D(0.0)
        info = shim.qp_shift(self.col, D(self.theta), D(mu), _p(self.sy), _p(self.sts), _p(self.gf), D(self.nf),
                             D(self.ldm), _p(kf), C.byref(w), C.byref(ld))
        return info, w.value, kf, ld.value

    def eval(self, shim, mu):
        """(c, ||x||^2, v'x, x'A^-1 x, w)"""
        info, w, kf, _ = self.shift(shim, mu)
        assert info == 0
        if self.col == 0:
            return np.zeros(0), w * w * self.vv, w * self.vv, w ** 3 * self.vv, w
        c, out = np.zeros(2 * self.col), np.zeros(3)
        assert shim.qp_eval(self.col, D(self.theta), _p(kf), D(w), _p(self.p), D(self.vv), _p(self.gf), _p(c),
                            _p(out)) == 0
        return c, out[0], out[1], out[2], w

    def secular(self, shim, delta, rtol, max_it):
        """(rc, mu, ||x||, iters)"""
        out = np.zeros(3)
        it = C.c_int(0)
        rc = shim.qp_secular(self.col, D(self.theta), _p(self.sy), _p(self.sts), _p(self.gf), _p(self.p), D(self.vv),
                             D(delta), D(rtol), max_it, _p(out), C.byref(it))
        return rc, out[0], np.sqrt(out[1]), it.value


@pytest.fixture(scope="module")
def cases(shim):
    return {(col, pin): Case(shim, col, pin) for col in COLS for pin in (False, True)}


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_factor_and_eval_against_dense(shim, cases, col, pin):
    cs = cases[(col, pin)]
    col, fr = cs.col, cs.free
    for mu in cs.mus():
        A = cs.A0 + mu * np.eye(cs.nf)
        cond = np.linalg.cond(A)
        info, w, kf, ld = cs.shift(shim, mu)
        assert info == 0
        sign, ref_ld = np.linalg.slogdet(A)
        print("col %d pin %d mu %.3e: log det %.12e against %.12e (bound %.1e)" % (col, pin, mu, ld, ref_ld, 1e-10 * N))
        assert sign > 0 and abs(ld - ref_ld) <= 1e-10 * N
        c, n2, vx, xbx, w = cs.eval(shim, mu)
        if col:
            wv = np.where(fr, w, 0.0)
            K = _dense_k(cs.S, cs.Y, cs.theta, wv)
            stv, ytv = cs.S.T @ (wv * cs.v), cs.Y.T @ (wv * cs.v)
            z = np.linalg.solve(K, np.concatenate([ytv, cs.theta * stv]))
            ref_c = np.concatenate([cs.theta * z[col:], z[:col]])
            e_c, b_c = np.linalg.norm(c - ref_c), 1e-12 * np.linalg.cond(K) * np.linalg.norm(ref_c)
            print("  coefficients off by %.2e (bound %.2e)" % (e_c, b_c))
            assert e_c <= b_c
        x = w * (cs.v[fr] + (cs.RF @ c if col else 0.0))
        ref = np.linalg.solve(A, cs.v[fr])
        err = np.linalg.norm(x - ref)
        print("  solve off by %.2e (bound %.2e, cond %.2e)" % (err, 1e-12 * cond * np.linalg.norm(ref), cond))
        assert err <= 1e-12 * cond * np.linalg.norm(ref)
        refl = ref.astype(np.longdouble)
        for name, got, want in (("x'x", n2, float(refl @ refl)), ("v'x", vx, float(cs.v[fr].astype(np.longdouble) @ refl)),
                                ("x'A^-1 x", xbx, float(refl @ np.linalg.solve(A, ref).astype(np.longdouble)))):
            print("  %s %.15e against %.15e (relative bound %.1e)" % (name, got, want, 4e-12 * cond))
            assert abs(got - want) <= 4e-12 * cond * abs(want), name


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS[1:])
def test_factor_is_qn_shift_factor_on_the_weighted_gram(shim, cases, col, pin):
    """w a power of two: R_F' diag(w) R_F is w G_F exactly, and the two routes run the same arithmetic"""
    cs = cases[(col, pin)]
    d = 2 * col
    for w in (2.0 ** -3, 2.0 ** -11, 4.0):
        g = (cs.RF * w).T @ cs.RF.copy()
        gw = np.asfortranarray(0.5 * (g + g.T))
        k1, k2 = np.zeros((d, d), order="F"), np.zeros((d, d), order="F")
        l1, l2 = D(0.0), D(0.0)
        r1 = shim.qp_factor(col, D(cs.theta), _p(cs.sy), _p(cs.sts), _p(cs.gf), D(w), _p(k1), C.byref(l1))
        r2 = shim.qp_shift_factor(col, D(cs.theta), _p(cs.sy), _p(cs.sts), _p(gw), _p(k2), C.byref(l2))
        assert r1 == r2
        assert k1.tobytes() == k2.tobytes() and l1.value == l2.value


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_bad_shifts_are_told_apart(shim, cases, col, pin):
    cs = cases[(col, pin)]
    for mu in (-cs.theta, -2.0 * cs.theta, float("nan"), float("inf")):
        assert cs.shift(shim, mu)[0] == 1
    if cs.lam[0] < cs.theta * (1.0 - 1e-6):  # (B_FF has an eigenvalue below theta: some shift keeps theta + mu > 0)
        mu = -0.5 * (cs.lam[0] + cs.theta)
        assert cs.theta + mu > 0 and cs.lam[0] + mu < 0
        assert cs.shift(shim, mu)[0] == 2
    assert cs.shift(shim, -0.5 * cs.lam[0])[0] == 0


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_secular_iteration(shim, cases, col, pin):
    """The reference shift: bisection on ||x(mu)||^2 = sum_i (q_i'v)^2 / (lambda_i + mu)^2 in np.longdouble, from the
    spectrum of B_FF.  The bound on mu: d||x|| / d mu = -x'A^-1 x / ||x|| and x'A^-1 x >= ||x||^2 / (lambda_max + mu),
    so an error e in ||x|| moves mu by at most e (lambda_max + mu) / ||x||; the iteration stops with e <= rtol Delta,
    and the evaluated norm itself is within 2e-12 cond of the true one (half the bound of its square above): together
    (rtol + 2e-12 cond) (lambda_max + mu) -- rtol cond relative to lambda_min + mu."""
    cs = cases[(col, pin)]
    lam, Q = np.linalg.eigh(cs.A0)
    qv = (Q.T @ cs.v[cs.free]).astype(np.longdouble)
    laml = lam.astype(np.longdouble)

    def norm_at(mu):
        return np.sqrt(np.sum((qv / (laml + mu)) ** 2))

    x0 = float(norm_at(np.longdouble(0)))
    _, n2, _, _, _ = cs.eval(shim, 0.0)
    assert abs(np.sqrt(n2) - x0) <= 2e-12 * np.linalg.cond(cs.A0) * x0
    x0 = float(np.sqrt(n2))  # (the ratio 1 is exact for the norm the iteration sees)
    for ratio in RATIOS:
        delta = ratio * x0
        for rtol in (1e-6, 1e-10):
            rc, mu, nx, iters = cs.secular(shim, delta, rtol, 100)
            print("col %d pin %d ratio %g rtol %g: rc %d mu %.6e ||x|| %.15e iters %d" % (col, pin, ratio, rtol, rc, mu,
                                                                                        nx, iters))
            assert iters <= 100 and rc != 3
            if ratio >= 1.0:
                assert rc == 0 and mu == 0.0 and iters == 1
                continue
            assert rc in (1, 2) and mu > 0.0
            assert abs(nx - delta) <= rtol * delta
            lo, hi = np.longdouble(0), np.longdouble(1)
            while norm_at(hi) > delta:
                hi *= 2
            for _ in range(200):
                mid = (lo + hi) / 2
                if norm_at(mid) > delta:
                    lo = mid
                else:
                    hi = mid
            ref = float(hi)
            cond = (lam[-1] + ref) / (lam[0] + ref)
            bound = (rtol + 2e-12 * cond) * (lam[-1] + ref)
            print("    mu against the bisection %.15e: off by %.2e (bound %.2e)" % (ref, abs(mu - ref), bound))
            assert abs(mu - ref) <= bound
        rc, mu, nx, iters = cs.secular(shim, delta, 1e-17, 400)
        print("col %d pin %d ratio %g rtol 1e-17: rc %d iters %d" % (col, pin, ratio, rc, iters))
        if ratio >= 1.0:
            assert rc == 0
        else:
            assert rc == 2 or (rc == 1 and nx == delta)
            assert nx <= delta * (1.0 + 1e-10)


@pytest.mark.parametrize("pin", [False, True])
@pytest.mark.parametrize("col", COLS)
def test_secular_iteration_out_of_evaluations(shim, cases, col, pin):
    """max_it in {1, 2, 3}: what is handed out is inside the region (codes 0 .. 3: ||x|| <= delta to rtol, code 3 the
    upper end of the bracket) or the call says that it has nothing (code 4: no evaluation reached ||x|| <= delta) --
    never a shift with ||x|| > delta under a code that a caller would take for a step"""
    cs = cases[(col, pin)]
    _, n2, _, _, _ = cs.eval(shim, 0.0)
    x0 = float(np.sqrt(n2))
    seen = set()
    for ratio in RATIOS:
        delta = ratio * x0
        for max_it in (1, 2, 3):
            rc, mu, nx, iters = cs.secular(shim, delta, 1e-10, max_it)
            seen.add(rc)
            assert iters <= max_it
            if ratio >= 1.0:
                assert rc == 0 and mu == 0.0
            elif rc == 4:
                assert nx > delta  # (reported: the solver refuses, nothing is written)
            else:
                assert rc in (1, 2, 3) and mu > 0.0 and nx <= delta * (1.0 + 1e-10)
                if rc == 3:  # the upper end: inside, not on the boundary to rtol
                    _, n2m, _, _, _ = cs.eval(shim, mu)
                    assert np.sqrt(n2m) == nx and nx < delta
            if ratio < 1.0 and max_it == 1:
                assert rc == 4 and mu == 0.0  # (one evaluation, at mu = 0, outside the region)
    assert 4 in seen


def test_host_algebra_under_sanitizers(tmp_path):
    """tests/qn_path_shim.cpp as a program of its own (-DQN_PATH_MAIN), built with AddressSanitizer and UBSan: the
    factor, the evaluation and the secular iteration on pairs the program makes, with and without pins"""
    exe = str(tmp_path / "qn_path_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DQN_PATH_MAIN", os.path.join(HERE, "qn_path_shim.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "qn_path host algebra: 0 failures" in r.stdout, r.stdout[-1500:]
