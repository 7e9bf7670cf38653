"""Eigenvalues and eigenvectors of the curvature model on the device (lbfgsb_hip_qn_eig / lbfgsb_hip_qn_eigvec;
DeviceSolver.qn_eig / qn_eigvec, QnOperator.eigvalsh / eigh / cond): states from driven runs as in
tests/test_gpu_qn_root.py, the dense numpy model from export_state.  Eigenvalues against eigvalsh, U'U = I,
A U = U Lambda and the reconstruction alpha I + U diag(lambda - alpha) U' = A on the device vectors, qn_apply(U) =
U Lambda and qn_apply(U, other mode) = U / Lambda on the device, at row counts around a wave (1 ... 1000) and pair
counts at every tile capacity and across two and three tiles; the basis pass against the expansion route (option
"qn_basis"), the tile-local layout, a REAL32 context, one size at which no dense model fits, runs that call the
entries at every return bit-identical to runs that do not, and the refusals.

Bounds (those of test_gpu_qn_root.py::_check_root): an error of A X is at most 1e-10 |B| |X| for A = B and
1e-10 cond(B) |ref| for A = H (Frobenius norms of the blocks); U'U - I of a block of vectors at most 1e-10 cond(B) |U|.
They hold as they stand for A U = U Lambda on every returned vector, for the r returned eigenvalues, and for U'U - I
on the vectors whose eigenvalue lies at least 1e-3 alpha off the bulk value alpha.  What the cut itself implies is
allowed for and nothing else:
  the n - r entries of the spectrum that are filled in with alpha may be off by LBFGSB_QN_EIG_CUT alpha, which is what
  a direction under the cut is by definition; the reconstruction lacks those c = min(2col, n) - r directions and may
  be off by CUT alpha c^(1/2) more (nothing where none was cut);
  U'U - I over ALL returned vectors -- a vector whose eigenvalue is delta_i away from the (n - r)-dimensional bulk
  eigenspace is determined by data with relative rounding eps only up to eps |A| / |delta_i| (Davis-Kahan; the
  header states it), and a vector is a sum of at most 64 products per row: with e_i the part of u_i off its direction,
  |e_i| <= 64 eps |A| / |delta_i|, entry (i, j) is u_j'e_i + u_i'e_j, so |U'U - I|_F <= 1e-10 cond(B) |U| + 2 * 64 eps
  |A| (sum_i delta_i^-2)^(1/2).
The coefficients behind the entrywise bounds (64 eps sum_c |coef_c| |W_ic|) and the REAL32 reference come from the
host algebra through tests/qn_eig_shim.cpp on the exported state, with numpy's own sums -- never from the vectors
under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_qn_root import (RUNS, _cond_and_norm, _drive, _first_return, _model, _problem, _slow_quadratic,
                              _wrapped)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -101, -104
EPS = 2.0 ** -53
CUT = 1e-8  # LBFGSB_QN_EIG_CUT
SEP = 1e-3  # |delta_i| >= SEP alpha: the vectors held to the bounds of _check_root as they stand
HERE = os.path.dirname(os.path.abspath(__file__))


def _orth_bound(cond, na, lam, alpha, unorm):
    """the bound on |U'U - I| of the module docstring; na = |A|_2"""
    return 1e-10 * cond * unorm + 2.0 * 64.0 * EPS * na * float(np.sqrt(np.sum((lam - alpha) ** -2.0)))


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def _fro(a):
    return float(np.linalg.norm(a))


def _spectrum(sol, inverse):
    bulk, lam = sol.qn_eig(inverse=inverse)
    return bulk, lam, len(lam)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("qn_eig_shim_gpu")
    so = str(out / "libqn_eig_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "qn_eig_shim.cpp"), "-o", so])
    return C.CDLL(so)


def _host_coef(shim, wa, n, m, head, col, theta, inverse, ss_of_pairs=False):
    """(W, lambda, C) of an exported state by the host algebra in numpy's sums: W = [S, Y] (n x 2col, ring order), the
    eigenvalues off the bulk value and their coefficient columns C (2col x r), U = W C.  Sy, Ss and Wt are the exported
    ones (what the context's N is built from), S'Y, Y'Y and theta's Gram numpy's; theta None: y'y / s'y of the newest
    pair, as a context that imported the state forms it; ss_of_pairs: S'S of G numpy's too (REAL32 contexts)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    wa = wa.astype(np.float64)
    cols = [(head - 1 + j) % m for j in range(col)]
    S, Y = wa[:m * n].reshape(m, n)[cols].T.copy(), wa[m * n:2 * m * n].reshape(m, n)[cols].T.copy()
    off = 2 * m * n
    sy = np.asfortranarray(wa[off:off + m * m].reshape(m, m, order="F"))
    ss = np.asfortranarray(wa[off + m * m:off + 2 * m * m].reshape(m, m, order="F"))
    sty, yty = np.asfortranarray(S.T @ Y), np.asfortranarray(Y.T @ Y)
    assert np.abs(np.tril(sty) - sy[:col, :col]).max() <= 1e-5 * np.abs(sty).max()  # (the layout of wa as read here)
    assert np.abs(np.triu(S.T @ S) - ss[:col, :col]).max() <= 1e-5 * np.abs(S.T @ S).max()
    if theta is None:
        theta = float(yty[col - 1, col - 1] / sy[col - 1, col - 1])
    wt = np.asfortranarray(wa[off + 2 * m * m:off + 3 * m * m].reshape(m, m, order="F"))  # (formt's factor, as exported)
    sss = S.T @ S if ss_of_pairs else np.triu(ss[:col, :col]) + np.triu(ss[:col, :col], 1).T
    W = np.hstack([S, Y])
    G = np.asfortranarray(np.block([[sss, sty], [sty.T, yty]]))
    dg = np.ascontiguousarray(np.diag(sy)[:col])
    d = 2 * col
    nm, cf, lam, r = np.zeros((d, d), order="F"), np.zeros((d, d), order="F"), np.zeros(d), np.zeros(1, np.int32)
    rc = shim.es_eig(1 if inverse else 0, m, p(sy), p(wt), col, C.c_double(theta), p(sty), p(yty), p(dg), p(G),
                     C.c_int64(min(d, n)), p(nm), p(r), p(lam), p(cf))
    assert rc == 0, rc
    return W, lam[:int(r[0])].copy(), cf[:, :int(r[0])].copy()


def _match(lam, lam_ref):
    """for every eigenvalue of lam the index of the nearest one of lam_ref"""
    return np.array([int(np.argmin(np.abs(lam_ref - v))) for v in lam], dtype=int)


def _entry_bound(W, cf):
    """64 eps sum_c |coef_c| |W_ic| for the vectors W cf, as rows (k, n)"""
    return 64.0 * EPS * (np.abs(W) @ np.abs(cf)).T


def _check_eig(env, shim, sol, routes=True):
    """every check of one state on both modes; returns (col, r of B)"""
    torch = env["torch"]
    n = sol.n
    wa, _ = sol.export_state()
    B, col, theta, W = _model(sol, wa)
    cond, nb = _cond_and_norm(B, theta, W)
    H = np.linalg.inv(B)
    ref_b = np.linalg.eigvalsh(B)
    out_r = 0
    for inverse, alpha, A in ((False, theta, B), (True, 1.0 / theta, H)):
        # |A X - ref| <= opb(is_h, X, ref)
        opb = lambda is_h, X, ref: 1e-10 * cond * _fro(ref) if is_h else 1e-10 * nb * _fro(X)
        bulk, lam, r = _spectrum(sol, inverse)
        assert bulk == alpha and r <= min(2 * col, n)
        assert np.all(np.diff(lam) >= 0.0)
        want = 1.0 / ref_b[::-1] if inverse else ref_b
        bound = 1e-10 * cond * np.abs(want).max() if inverse else 1e-10 * nb
        err = max([np.abs(want - v).min() for v in lam], default=0.0)  # each returned one against the nearest
        vals, fill = np.concatenate([lam, np.full(n - r, alpha)]), np.concatenate([np.zeros(r), np.ones(n - r)])
        o = np.argsort(vals, kind="stable")
        print("n %d col %d inverse %s: r %d, eigenvalues %.3e (bound %.3e, cond %.2e), with alpha filled in %.3e"
              % (n, col, inverse, r, err, bound, cond, np.abs(vals[o] - want).max()))
        assert err <= bound
        assert np.all(np.abs(vals[o] - want) <= bound + CUT * alpha * fill[o])  # (CUT alpha for the filled-in only)
        op = sol.qn_operator(inverse=inverse)
        b2, l2 = op.eigvalsh()
        assert b2 == bulk and np.array_equal(l2, lam)
        ev = np.concatenate([lam, [alpha] if n > r else []])
        assert op.cond() == ev.max() / ev.min()
        if not inverse:
            out_r = r
        if r == 0:
            continue
        Ut = sol.qn_eigvec(inverse=inverse)  # k = r
        assert tuple(Ut.shape) == (r, n)
        U = Ut.cpu().numpy().astype(np.float64)
        na = np.abs(want).max()
        e_orth, b_orth = _fro(U @ U.T - np.eye(r)), _orth_bound(cond, na, lam, alpha, _fro(U))
        e_res, b_res = _fro(U @ A - lam[:, None] * U), opb(inverse, U, lam[:, None] * U)
        rec = alpha * np.eye(n) + (U.T * (lam - alpha)) @ U
        e_rec, b_rec = _fro(rec - A), opb(inverse, U, A) + CUT * alpha * np.sqrt(min(2 * col, n) - r)
        sep = np.abs(lam - alpha) >= SEP * alpha
        e_sep, b_sep = _fro(U[sep] @ U[sep].T - np.eye(int(sep.sum()))), 1e-10 * cond * _fro(U[sep])
        print("   U'U - I %.3e (%.3e), on the %d separated %.3e (%.3e), AU - UL %.3e (%.3e), reconstruction %.3e (%.3e)"
              % (e_orth, b_orth, int(sep.sum()), e_sep, b_sep, e_res, b_res, e_rec, b_rec))
        assert e_sep <= b_sep and e_orth <= b_orth and e_res <= b_res and e_rec <= b_rec
        lt = torch.from_numpy(lam).cuda()[:, None]
        au, ul = sol.qn_apply(Ut, inverse=inverse).cpu().numpy(), (lt * Ut).cpu().numpy()
        iu, uil = sol.qn_apply(Ut, inverse=not inverse).cpu().numpy(), (Ut / lt).cpu().numpy()
        e1, b1 = _fro(au - ul), opb(inverse, U, ul)
        e2, b2 = _fro(iu - uil), opb(not inverse, U, uil)
        print("   device: A U - U L %.3e (%.3e), A^-1 U - U / L %.3e (%.3e)" % (e1, b1, e2, b2))
        assert e1 <= b1 and e2 <= b2
        _, _, vecs = op.eigh()
        assert torch.equal(vecs, Ut)
        # k = 1 and k = 3: the same arithmetic per output, whatever the others are
        assert torch.equal(sol.qn_eigvec(which=[r - 1], inverse=inverse)[0], Ut[r - 1])
        three = [0, r // 2, r - 1]
        assert torch.equal(sol.qn_eigvec(which=three, inverse=inverse), Ut[three])
        if routes:  # the expansion route, 4 vectors a pass: the same products summed in another order
            sol.set_option("qn_basis", 0)
            try:
                U0 = sol.qn_eigvec(inverse=inverse).cpu().numpy()
                U03 = sol.qn_eigvec(which=three, inverse=inverse).cpu().numpy()
            finally:
                sol.set_option("qn_basis", 1)
            Wh, lam_h, cf_h = _host_coef(shim, wa, n, sol.m, int(sol.isave[26]), col, theta, inverse)
            eb = _entry_bound(Wh, cf_h[:, _match(lam, lam_h)])
            print("   qn_basis 0 / 1: max |delta| %.3e, max of bound %.3e" % (np.abs(U0 - U).max(), eb.max()))
            assert np.all(np.abs(U0 - U) <= eb) and np.all(np.abs(U03 - U[three]) <= eb[three])
    return col, out_r


SHAPES = [(1, 1), (63, 5), (64, 6), (65, 10), (257, 11), (257, 16), (1000, 17), (1000, 33)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_spectrum_and_vectors_fp64(env, shim, n, m):
    """col = 0 (FG_START), a partly filled ring and a full ring whose head has wrapped"""
    la = env["la"]
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)  # (no early stop: the ring fills and wraps)
    sol = la.DeviceSolver(n, m)
    seen = {}
    try:
        def at(s, t):
            col = int(s.isave[27])
            if not (t.startswith("NEW_X") or t.startswith("FG_START")):
                return
            tag = "empty" if col == 0 else ("wrapped" if _wrapped(s) else ("full" if col == m else "part"))
            if tag in seen or (tag == "full" and m > 1) or (tag == "part" and col < max(1, m // 2)):
                return
            seen[tag] = _check_eig(env, shim, s)
        _drive(env, sol, p, max_iter=4 * m + 40, at_return=at, until=lambda s: "wrapped" in seen)
    finally:
        sol.close()
    assert seen.get("empty") == (0, 0), seen
    if n > 1:
        assert "wrapped" in seen and seen["wrapped"][0] == m and seen["wrapped"][1] >= 1, seen
        assert "part" in seen or m == 1, seen
    print("checked states (col, r):", seen)  # (one row: whatever states the run passes through, r <= 1)


def test_which_with_repeats_and_padded_rows(env):
    la, torch = env["la"], env["torch"]
    n, m = 257, 11
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)
    sol = la.DeviceSolver(n, m)
    try:
        _drive(env, sol, p, max_iter=4 * m + 40, until=_wrapped)
        assert _wrapped(sol)
        for inverse in (False, True):
            _, lam, r = _spectrum(sol, inverse)
            assert r >= 4
            U = sol.qn_eigvec(inverse=inverse)
            which = [r - 1, r - 1, 2, 0]
            ldo = n + 5
            buf = torch.full((len(which), ldo), -7.0, dtype=torch.float64, device="cuda")
            got = sol.qn_eigvec(which=which, out=buf[:, :n], inverse=inverse)
            assert got.data_ptr() == buf.data_ptr()
            assert torch.equal(buf[:, :n], U[which])
            assert bool((buf[:, n:] == -7.0).all())
            one = torch.full((ldo,), -7.0, dtype=torch.float64, device="cuda")
            sol.qn_eigvec(which=[1], out=one[:n], inverse=inverse)
            assert torch.equal(one[:n], U[1]) and bool((one[n:] == -7.0).all())
    finally:
        sol.close()


def test_large_problem_identities(env):
    """n = 200 003, m = 10: no dense model.  cond(B) and |B| from the Rayleigh quotient of B on an orthonormal basis
    of span(W) through qn_apply (B is theta I on the complement); then the qn_apply identities, U U' = I by torch
    products and log det A = n log alpha + sum_i log(lambda_i / alpha) against qn_logdet"""
    la, torch = env["la"], env["torch"]
    n, m = 200_003, 10
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0)
    sol = la.DeviceSolver(n, m)
    try:
        _drive(env, sol, p, max_iter=4 * m + 40, until=_wrapped)
        assert _wrapped(sol)
        wa, _ = sol.export_state()
        head, col, theta = int(sol.isave[26]), int(sol.isave[27]), float(sol.dsave[0])
        cols = [(head - 1 + j) % m for j in range(col)]
        W = np.concatenate([wa[:m * n].reshape(m, n)[cols], wa[m * n:2 * m * n].reshape(m, n)[cols]]).T
        Q, _ = np.linalg.qr(W)
        Qt = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda()
        ev = np.concatenate([[theta], np.linalg.eigvalsh((Qt @ sol.qn_apply(Qt).T).cpu().numpy())])
        cond, nb = ev.max() / ev.min(), ev.max()
        for inverse in (False, True):
            alpha = 1.0 / theta if inverse else theta
            bulk, lam, r = _spectrum(sol, inverse)
            assert bulk == alpha and 1 <= r <= 2 * col
            U = sol.qn_eigvec(inverse=inverse)
            lt = torch.from_numpy(lam).cuda()[:, None]
            nu = float(torch.linalg.norm(U))
            opb = lambda is_h, ref: 1e-10 * cond * float(torch.linalg.norm(ref)) if is_h else 1e-10 * nb * nu
            e1 = float(torch.linalg.norm(sol.qn_apply(U, inverse=inverse) - lt * U))
            e2 = float(torch.linalg.norm(sol.qn_apply(U, inverse=not inverse) - U / lt))
            e3 = float(torch.linalg.norm(U @ U.T - torch.eye(r, dtype=torch.float64, device="cuda")))
            b3 = _orth_bound(cond, 1.0 / ev.min() if inverse else nb, lam, alpha, nu)
            Us = U[torch.from_numpy(np.abs(lam - alpha) >= SEP * alpha).cuda()]
            e4 = float(torch.linalg.norm(Us @ Us.T - torch.eye(len(Us), dtype=torch.float64, device="cuda")))
            assert e4 <= 1e-10 * cond * float(torch.linalg.norm(Us)), e4
            print("inverse %s: r %d, A U - U L %.3e (%.3e), A^-1 U - U / L %.3e (%.3e), U U' - I %.3e (%.3e)"
                  % (inverse, r, e1, opb(inverse, lt * U), e2, opb(not inverse, U / lt), e3, b3))
            assert e1 <= opb(inverse, lt * U) and e2 <= opb(not inverse, U / lt) and e3 <= b3
            ld = n * np.log(alpha) + float(np.sum(np.log(lam / alpha)))
            assert abs(ld - sol.qn_logdet(inverse=inverse)) <= 1e-10 * n
    finally:
        sol.close()


def test_layout_read_as_it_is(env, shim):
    """compact_w on and the layout packed: the eigenvalues and the vectors of the packed context against those of a
    natural-order context that imported its state -- every separated vector lies in the span of the plain context's
    vectors, and equals the plain one entry by entry where its eigenvalue is SEP alpha away from every other one:
    beyond the entry bound only what _check_root's norm allows, 1e-10 cond |u| -- and the packed vectors satisfy the
    plain context's qn_apply identities"""
    la, torch = env["la"], env["torch"]
    n, m = 4099, 5
    p = _problem(env, "rosenbrock", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": 1, "compact_min_rows": 0})
    got = {}
    try:
        def at(s, t):
            if got or not t.startswith("NEW_X") or int(s.isave[27]) < m or not s.compact_stats()[2]:
                return
            before = s.compact_stats()
            assert before[2] and before[3]  # packed now, and eligible
            for inverse in (False, True):
                got[inverse] = (s.qn_eig(inverse=inverse), s.qn_eigvec(inverse=inverse).clone())
                s.set_option("qn_basis", 0)
                got[inverse] += (s.qn_eigvec(inverse=inverse).clone(),)
                s.set_option("qn_basis", 1)
                assert torch.equal(got[inverse][1], s.qn_eigvec(inverse=inverse))  # reproducible bit for bit
            assert s.compact_stats() == before
            got["wa"], got["iwa"] = s.export_state()
            got["isave"], got["theta"] = s.isave.copy(), float(s.dsave[0])
        _drive(env, sol, p, max_iter=40, at_return=at, until=lambda s: bool(got))
    finally:
        sol.close()
    assert got, "the layout never packed"
    plain = la.DeviceSolver(n, m)
    try:
        plain.import_state(got["wa"], got["iwa"], got["isave"])
        plain.isave[:] = got["isave"]
        plain.dsave[0] = got["theta"]  # (what _model reads; the context itself forms theta from the Gram)
        B, col, theta, W = _model(plain, got["wa"])
        cond, nb = _cond_and_norm(B, theta, W)
        for inverse in (False, True):
            (bulk, lam), U, U0 = got[inverse]
            b2, l2 = plain.qn_eig(inverse=inverse)
            assert len(l2) == len(lam) and abs(b2 - bulk) <= 1e-13 * bulk
            assert np.abs(l2 - lam).max() <= 1e-13 * np.abs(lam).max()
            lt = torch.from_numpy(lam).cuda()[:, None]
            for is_h, ref in ((inverse, lt * U), (not inverse, U / lt)):
                err = float(torch.linalg.norm(plain.qn_apply(U, inverse=is_h) - ref))
                bound = 1e-10 * cond * float(torch.linalg.norm(ref)) if is_h else 1e-10 * nb * float(torch.linalg.norm(U))
                assert err <= bound, (inverse, is_h, err, bound)
            Uh = U.cpu().numpy()
            Wh, lam_h, cf_h = _host_coef(shim, got["wa"], n, m, int(got["isave"][26]), col, theta, inverse)
            eb = _entry_bound(Wh, cf_h[:, _match(lam, lam_h)])
            assert np.all(np.abs(U0.cpu().numpy() - Uh) <= eb)
            e_orth = _fro(Uh @ Uh.T - np.eye(len(lam)))
            na = cond / nb if inverse else nb
            assert e_orth <= _orth_bound(cond, na, lam, bulk, _fro(Uh))
            sep = np.abs(lam - bulk) >= SEP * bulk
            assert _fro(Uh[sep] @ Uh[sep].T - np.eye(int(sep.sum()))) <= 1e-10 * cond * _fro(Uh[sep])
            # the packed vectors against the natural-order context's own
            Un = plain.qn_eigvec(inverse=inverse).cpu().numpy()
            ev = np.concatenate([lam, [bulk]])
            for i in np.flatnonzero(sep):
                out_of_span = np.linalg.norm(Uh[i] - Un.T @ (Un @ Uh[i]))
                assert out_of_span <= 1e-10 * cond, (i, out_of_span)
                if np.abs(np.delete(ev, i) - ev[i]).min() >= SEP * bulk:
                    assert Uh[i] @ Un[i] > 0.0  # (the sign rule: the same coefficients up to rounding)
                    excess = np.maximum(np.abs(Uh[i] - Un[i]) - eb[i], 0.0)
                    print("inverse %s vector %d: |packed - plain| %.3e, beyond the entry bound %.3e"
                          % (inverse, i, np.linalg.norm(Uh[i] - Un[i]), np.linalg.norm(excess)))
                    assert np.linalg.norm(excess) <= 1e-10 * cond
    finally:
        plain.close()


def test_real32_vectors(env, shim):
    """a REAL32 context: fp32 outputs, fp64 sums rounded on store.  The state of an fp32 run is exported and imported
    into an fp32 context, so that the context's model is the one of the exported state (the host matrices of a
    running fp32 context are not the exported fp32 ones).  The fp64 reference is U64 = W C in numpy from the exported
    fp32 pairs, C by the host algebra on the exported state (tests/qn_eig_shim.cpp) -- nothing of the device.  For
    every vector |u32 - u64| <= 2^-23 |u64| + 64 eps sum_c |coef_c| |W_ic| entry by entry, and what exceeds it at most
    1e-10 cond |u64| in the norm (the fp64 bound of _check_root: the context's Gram and numpy's differ in the order of
    their sums).  A vector less than SEP alpha off the bulk value or off another eigenvalue cannot be compared so in a
    REAL32 context: the Ss a context holds agrees with its stored fp32 pairs to fp32 rounding only, so such a vector is
    determined to 2^-24 |A| / |delta_i| (on the GPU: |u| = 0.992 and |A u - lambda u| = 1.4e-4 |A| for the one vector of
    this state that is 1e-5 alpha off the bulk value).  Those are checked to lie in the span of the exported pairs to
    the rounding of the store; at least half of the vectors must be compared entry by entry."""
    la, torch = env["la"], env["torch"]
    n, m = 257, 10
    p = env["po"].problem_rosenbrock(n, m, factr=0.0, pgtol=0.0, real=np.float32)
    sol = la.DeviceSolver(n, m, real32=True)
    try:
        _drive(env, sol, p, max_iter=4 * m + 40, until=_wrapped)
        assert _wrapped(sol)
        wa, iwa = sol.export_state()
        isave = sol.isave.copy()
    finally:
        sol.close()
    assert wa.dtype == np.float32
    head, col = int(isave[26]), int(isave[27])
    s32 = la.DeviceSolver(n, m, real32=True)
    try:
        s32.import_state(wa, iwa, isave)
        s32.isave[:] = isave
        for inverse in (False, True):
            bulk, lam = s32.qn_eig(inverse=inverse)
            W, lam_h, cf_h = _host_coef(shim, wa, n, m, head, col, None, inverse, ss_of_pairs=True)
            r = len(lam)
            assert r >= 1 and len(lam_h) == r and np.abs(lam_h - lam).max() <= 1e-10 * np.abs(lam).max()
            U32t = s32.qn_eigvec(inverse=inverse)
            assert U32t.dtype == torch.float32 and tuple(U32t.shape) == (r, n)
            U32 = U32t.cpu().numpy().astype(np.float64)
            U64 = (W @ cf_h).T
            s32.dsave[0] = 1.0 / bulk if inverse else bulk  # (what _model reads)
            B, _, theta, Wm = _model(s32, wa)
            cond, _ = _cond_and_norm(B, theta, Wm)
            eb = 2.0 ** -23 * np.abs(U64) + _entry_bound(W, cf_h)
            ev = np.concatenate([lam, [bulk]])
            worst, compared = 0.0, 0
            for i in range(r):
                if np.abs(np.delete(ev, i) - ev[i]).min() >= SEP * bulk:
                    assert U32[i] @ U64[i] > 0.0
                    excess = np.maximum(np.abs(U32[i] - U64[i]) - eb[i], 0.0)
                    worst, compared = max(worst, float(np.linalg.norm(excess))), compared + 1
                    assert np.linalg.norm(excess) <= 1e-10 * cond * np.linalg.norm(U64[i]), (i, lam[i])
                else:  # in the span of the exported pairs up to the rounding of the store, |e_k| <= 2^-24 |u_k|
                    u, nu = U32[i], np.linalg.norm(U32[i])
                    off = np.linalg.norm(u - W @ np.linalg.lstsq(W, u, rcond=None)[0])
                    assert off <= 2.0 ** -23 * nu + 1e-10 * cond * nu, (i, off)
            print("fp32, inverse %s: %d of %d vectors entry by entry, worst excess %.3e" % (inverse, compared, r, worst))
            assert 2 * compared >= r
    finally:
        s32.close()


def _both_entries(sol, torch, n):
    res = []
    for inverse in (False, True):
        bulk, lam = sol.qn_eig(inverse=inverse)
        res += [np.array([bulk]), lam]
        if len(lam):
            res.append(sol.qn_eigvec(inverse=inverse).cpu().numpy())
    return res


@pytest.mark.parametrize("name", list(RUNS))
def test_run_does_not_notice(env, name):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    cfg = RUNS[name]
    n, m = 4099, 7
    p = _problem(env, "rosenbrock", n, m)
    iters = 30
    outs = []
    counts = {"ok": 0, "refused": 0}
    sentinel = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    for touch in (False, True):
        sol = la.DeviceSolver(n, m, **cfg.get("ctor", {}))
        try:
            def at(s, t):
                try:
                    _both_entries(s, torch, n)
                    counts["ok"] += 1
                except la.LbfgsbError as e:
                    assert "-104" in str(e), e  # E_STATE: a deferred set-up or a parked f
                    counts["refused"] += 1
                    r, bulk = C.c_int32(-5), C.c_double(-5.0)
                    assert lib.lbfgsb_hip_qn_eig(s.h, 0, 0, C.byref(r), C.byref(bulk), None) == E_STATE
                    assert lib.lbfgsb_hip_qn_eigvec(s.h, 0, 1, None, sentinel.data_ptr(), n) == E_STATE
                    assert r.value == -5 and bulk.value == -5.0 and bool((sentinel == -7.0).all())
            rows, _ = _drive(env, sol, p, iters, at_return=at if touch else None, pp=cfg["pp"],
                             builtin=cfg.get("builtin"), deferred_f=cfg.get("deferred_f", False))
            wa, iwa = sol.export_state()
            outs.append((rows, wa.tobytes(), iwa.tobytes(), sol.compact_stats()))
        finally:
            sol.close()
    assert counts["ok"] > iters
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert outs[0][3] == outs[1][3]
    if name in ("defer", "builtin_deferred_f"):
        assert counts["refused"] > 0


def test_refusals_and_arguments(env):
    la, torch = env["la"], env["torch"]
    lib = la.load_library()
    n, m = 300, 5
    p = _problem(env, "rosenbrock", n, m)
    out = torch.full((3 * n,), -7.0, dtype=torch.float64, device="cuda")
    r, bulk = C.c_int32(-5), C.c_double(-5.0)
    lam = (C.c_double * 16)(*([-5.0] * 16))
    which = lambda *v: (C.c_int32 * len(v))(*v)
    eig = lambda s, mode=0, cap=0, pr=C.byref(r), pb=C.byref(bulk), pl=None: \
        lib.lbfgsb_hip_qn_eig(s.h, mode, cap, pr, pb, pl)
    vec = lambda s, mode=0, k=1, w=None, o=out.data_ptr(), ldo=n: lib.lbfgsb_hip_qn_eigvec(s.h, mode, k, w, o, ldo)
    untouched = lambda: bool((out == -7.0).all()) and r.value == -5 and bulk.value == -5.0 and lam[0] == -5.0
    sol = la.DeviceSolver(n, m)
    try:
        assert eig(sol) == E_STATE and vec(sol) == E_STATE and untouched()  # no run
        _first_return(env, sol)
        assert eig(sol, cap=16, pl=lam) == 0 and r.value == 0 and bulk.value == 1.0 and lam[0] == -5.0  # no pair
        assert vec(sol) == E_ARG and bool((out == -7.0).all())  # (no index is inside 0 .. r - 1)
        assert len(sol.qn_eigvec()) == 0 and sol.qn_operator().cond() == 1.0
    finally:
        sol.close()
    r.value, bulk.value = -5, -5.0
    sol = la.DeviceSolver(n, m)
    try:
        _drive(env, sol, p, max_iter=8)
        for mode in (2, 3, 4, 5, -1):
            assert eig(sol, mode=mode) == E_ARG and vec(sol, mode=mode) == E_ARG
        assert eig(sol, pr=None) == E_ARG and eig(sol, pb=None) == E_ARG
        assert eig(sol, cap=-1) == E_ARG and eig(sol, cap=2) == E_ARG  # (cap > 0 without h_lambda)
        assert untouched()
        assert eig(sol) == 0 and 1 <= r.value <= 2 * m and bulk.value == float(sol.dsave[0]) and lam[0] == -5.0
        rr = r.value
        assert eig(sol, cap=1, pl=lam) == 0 and lam[0] != -5.0 and lam[1] == -5.0  # min(r, cap) values
        lam[0] = -5.0
        assert vec(sol, k=0) == E_ARG and vec(sol, k=129) == E_ARG and vec(sol, ldo=n - 1) == E_ARG
        assert vec(sol, o=None) == E_ARG
        assert vec(sol, k=2, w=which(0, rr)) == E_ARG and vec(sol, k=2, w=which(-1, 0)) == E_ARG
        assert vec(sol, k=rr + 1) == E_ARG  # (NULL h_which: 0 .. k - 1)
        assert bool((out == -7.0).all())
        assert vec(sol, k=3, w=which(rr - 1, 0, rr - 1)) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:n], out[2 * n:]) and bool((out[:n] != -7.0).any())
        # k = 128 outputs in one launch (repeats)
        big = torch.empty((128, n), dtype=torch.float64, device="cuda")
        sol.qn_eigvec(which=[j % rr for j in range(128)], out=big)
        assert torch.equal(big[rr:2 * rr], big[:rr])
        # a model that is not positive definite: the newest pair with s'y < 0 (as qn_logdet refuses it)
        wa, iwa = sol.export_state()
        isave = sol.isave.copy()
        wa[m * n:2 * m * n] *= -1.0
        wa[2 * m * n:2 * m * n + m * m] *= -1.0
    finally:
        sol.close()
    out.fill_(-7.0)
    r.value, bulk.value = -5, -5.0
    sol = la.DeviceSolver(n, m)
    try:
        sol.import_state(wa, iwa, isave)
        sol.isave[:] = isave
        val = C.c_double(0.0)
        assert lib.lbfgsb_hip_qn_logdet(sol.h, 1, C.byref(val)) == E_STATE
        assert eig(sol, mode=1) == E_STATE and vec(sol, mode=1) == E_STATE and untouched()
    finally:
        sol.close()
    # 65 stored pairs: beyond LBFGSB_QN_ROOT_MAXCOL
    sol = la.DeviceSolver(1000, 70)
    try:
        _, t = _drive(env, sol, _slow_quadratic(env, 1000, 70), max_iter=400, until=lambda s: int(s.isave[27]) == 65)
        assert int(sol.isave[27]) == 65, t
        o = torch.full((1000,), -7.0, dtype=torch.float64, device="cuda")
        for mode in (0, 1):
            assert eig(sol, mode=mode) == E_ARG
            assert lib.lbfgsb_hip_qn_eigvec(sol.h, mode, 1, None, o.data_ptr(), 1000) == E_ARG
        assert r.value == -5 and bulk.value == -5.0 and bool((o == -7.0).all())
    finally:
        sol.close()
