"""Every switch of the curvature-model passes at small shapes: the qn_* entries of DeviceSolver on states with a chosen
col and head (tests/_qn_synth.py, taken in through import_state) and on packed states from a run, under the options
"nt" 0 / 1, "wgrid" 0 / 1, "qn_basis" 0 / 1 and with operands 16-byte aligned or offset by one element, against the
extended-precision reference of tests/_qn_truth.py within the bound derived there -- |out - ref| <= bound entry by
entry, no further constant.  The worst err / bound per entry family and real kind is printed by the last test
(profiles/qn_switch_ratios.txt is that table from an MI355X).

Roots are checked by their definition: the columns R e_i of qn_apply(sqrt=True) are collected, R must be symmetric, R R
must equal the reference A and eigvalsh(R) > 0 -- the positive definite root is unique.  QnShifted.sqrt likewise with
L L' = Sigma.  Other switch settings and the draws are then held to that checked R (or L) as the reference operator.
Draws: draw - mean = scale R z with z the numpy Philox reference of tests/test_gpu_qn_root.py; the device's z differs
from it by the elementary functions alone: log, sqrt, sincospi and their numpy twins are each within 2 ulp, so
|dz| <= 8 u |z| + (4 pi + 4) u r, r = sqrt(-2 log u) = hypot of the two deviates of a generator pair (the argument
2 pi v of numpy's sin carries the rounding of 2 pi and of the product); R |dz| is added to the bound.
Eigenpairs: with c the coefficients of an eigenvector in the [S, Y] basis, the expansion errs by e_i <= gamma_(d+2)
|W_i| |c| (+ 2^-24 |u_i| in REAL32, and 2^-24 |W_i| |c| for every column tile whose partial output is stored and read
back) and the host's symmetric eigensolver is backward stable to eta (|A|_2 relative), so
|A u - lambda u|_2 <= 2 |A|_2 (eta + |e|_2), | |u|_2 - 1 | and |u_a'u_b| <= 2 (eta + |e|_2), and the eigenvalues are
within (eta + gamma_n) lambda_max of eigvalsh of the reference rounded to fp64.

Case -> instantiation (read off QN_DISPATCH_MC / _K / _CW / _BOOL in k_qn_common.hpp and the launch_* of each file).
  MC     5: col in {0, 1, 5}; 10: {6, 10}; 16: {11, 16}; then the second and third tile: 17 = 16 + MC 5, 21 = 16 + 5,
         27 = 16 + MC 16 (11 columns), 32 = 16 + 16, 33 = 16 + 16 + MC 5 (1 column); head != 1 in one state per class.
  K      vector counts 1, 2, 3 = 2 + 1, 4, 5 = 4 + 1, 9 = 4 + 4 + 1 give K in {1, 2, 4} on MC 5 / 10 and {1, 2} on MC 16
         (qn_kmax); every switch setting keeps k = 3 and 5, so K = 1, 2 and 4 each meet both NT values.
  V      every W'v, expansion and draw launch takes two rows per lane only if 2 MC K <= 20 and every operand it loads
         or stores is aligned for two elements (`vec2` in launch_qn_wtv / _wtd / _wtg / _expand / _draw and their
         qn_shift twins; qn_wtz and qn_shift_wtz load no operand, for them the size rule alone or with the weights).
         So V = 2 exists for (MC 5, K = 1), (MC 5, K = 2) and (MC 10, K = 1) only -- col 0, 1, 5 and the last tile
         of 17, 21, 33 with pieces of 1 and 2 vectors, col 6 and 10 with pieces of 1 -- and these classes run with
         both V: aligned operands with an even row stride give V = 2, operands one element off V = 1
         (all_aligned_for).  Every other class (K = 4, MC 10 with K = 2, MC 16), the Gram pass (VSLOT), CW, qn_diag,
         qn_basis and qn_cols are V = 1 whatever the alignment; there the offset operands change only the addresses.
         qn_dtd (k = 5 in qn_gram) has no size rule: V2 by alignment alone.  n = 259 and 63 are odd, so a V = 2
         loop ends in a scalar tail.
  NT     option "nt" 0 / 1 in every state.
  CW     true in the states taken from a run with compact_w on (fp64, m = 5 and 10), asserted through compact_stats().
  grid   option "wgrid" 1 at n = 1027: one workgroup takes two full trips, a partial one and the tail; qn_basis_kernel
         and qn_cols_kernel take three 512-row trips.
         Under both, every entry runs, the roots and the draws included: at n = 1027 the collected root is held to
         its definition on ten vectors (R (R v) = A v, L (L'v) = Sigma v) instead of entry by entry.
  file / kernels                                     reached through                               further switches
  k_qn.hip         qn_wtv  qn_expand  qn_diag        qn_apply (B, H, roots), qn_diag, the Gram      VSLOT (the Gram pass)
                   qn_wtd  qn_wtg  qn_dtd            qn_quad / qn_logpdf, qn_gram (k = 4, then 5)   CEN (center), DD, GG
  k_qn_draw.hip    qn_wtz  qn_wtzz  qn_draw          qn_draw (first = 0 and 3, return_logpdf)       ZZ (with logpdf)
  k_qn_eig.hip     qn_basis                          qn_eigvec k = 1, 17, 128, "qn_basis" 0 / 1     ACC (tiles 2, 3), R
  k_qn_idx.hip     qn_rows  qn_cols                  qn_rows, qn_block, qn_cols k = 1, 17, 128      ACC, WGT (shifted)
  k_qn_shift.hip   qn_shift_w  _wtv  _expand  _diag  qn_shift: solve, sqrt, diag, logdet            ROOT (sqrt), VSLOT
  k_qn_shift_draw.hip  qn_shift_wtz  _wtzz  _draw  _wtd   sample (log_prob), quad, log_prob          ZZ, CEN, DD
Each file runs in fp64 and REAL32 (REAL32: the dyadic family at every col, the generic one at col 5, 10, 17)."""
import functools

import numpy as np
import pytest

import _qn_synth as qs
import _qn_truth as qt
from test_gpu_qn_root import _drive, _problem, z_ref

pytestmark = pytest.mark.gpu

LD = qt.LD
U, U32 = qt.U, qt.U32
COLS = (0, 1, 5, 6, 10, 11, 16, 17, 21, 27, 32, 33)
MU, SCALE, SEED = 0.3, 0.7, 2 ** 40 + 77


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lbfgsb_amd.load_library()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


# ------------------------------------------------------------------------------------------------ operands
def _ld(n):
    return (n + 3) // 4 * 4  # (an even row stride, so that every row of an aligned block is aligned)


def _dev(env, a, real, off):
    """a (n,) or (k, n) numpy array as a device tensor in `real`: rows _ld(n) apart, the first element 16-byte aligned
    (off = 0) or one element past that (off = 1)"""
    torch = env["torch"]
    a = np.asarray(a, real)
    n = a.shape[-1]
    k = 1 if a.ndim == 1 else a.shape[0]
    buf = torch.full((k * _ld(n) + 4,), float("nan"), dtype=torch.float32 if real == np.float32 else torch.float64,
                     device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + k * _ld(n)].view(k, _ld(n))[:, :n]
    t.copy_(torch.from_numpy(np.atleast_2d(a)))
    assert t.data_ptr() % 16 == off * a.itemsize
    return t[0] if a.ndim == 1 else t


def _out(env, k, n, real, off):
    return _dev(env, np.full((k, n) if k else (n,), np.nan), real, off)


def _np(t):
    return t.cpu().numpy()


def _kind(real):
    return "fp32" if real == np.float32 else "fp64"


# ------------------------------------------------------------------------------------------------ references
_TRUTHS = {}


def _truth(key, make):
    if key not in _TRUTHS:
        _TRUTHS[key] = make()
    return _TRUTHS[key]


def _shift_d(n, real):
    """every third row and a run of 40 rows across the layout tile boundary at 128 pinned"""
    d = np.linspace(0.0, 3.0, n).astype(real)
    d[::3] = np.inf
    d[110:150] = np.inf  # (n = 63: every third row only)
    return d


def _shift_truth(tr, d):
    """the shifted reference of a state, made once (against the recursion: in REAL32 with the fp32 allowance)"""
    if not hasattr(tr, "shift_op"):
        tr.shift_op = tr.shifted(d, MU, rec=True)
    return tr.shift_op


def _root_op(env, tr, apply_fn, a, l, r, top, real, tag, free=None, symmetric=True):
    """the checked root of the operator `top`: its dense matrix from n applies at the default switches, as an Op of
    the given shape.  R R (or L L') is held to top.A entry by entry; at n > 400, where that product in longdouble
    takes ten seconds, on six random and four unit vectors instead: R (R v) = A v."""
    n = tr.n
    E = np.eye(n, dtype=real)
    R = np.zeros((n, n), LD)
    for i0 in range(0, n, 64):  # (R e_i, 64 columns a call)
        R[:, i0:i0 + 64] = _np(apply_fn(_dev(env, E[i0:i0 + 64], real, 0))).astype(LD).T
    rows = None if free is None else np.flatnonzero(free)
    if free is not None:
        assert qt.pos_zero(R[~free].astype(np.float64)).all() and not R[:, ~free].any()
    N = qt.middle(R, a, l, r, tr.W, rows=rows) if tr.col and (rows is None or rows.size) else np.zeros((2 * tr.col,) * 2, LD)
    op = qt.Op(tr.W, N, a, l, r, A=R, g=tr.g, extra=0 if free is None else 8, free=free)
    bR = op.bound_apply(E.astype(np.float64), real, ref=R.T).T  # (entry [i, j] of R: row i of the apply to e_j)
    Ra = np.abs(R.astype(np.float64))
    if symmetric:
        qt.check("%s symmetry %s" % (tag, _kind(real)), R, R.T, bR + bR.T)
        ev = np.linalg.eigvalsh(((R + R.T) / 2).astype(np.float64))
        assert ev[0] > 0.0
    Rt, bRt, Rat = (R, bR, Ra) if symmetric else (R.T, bR.T, Ra.T)
    if n <= 400:
        V = np.eye(n)
    else:
        V = np.concatenate([_vectors(n, 6, np.float64, 11), np.eye(n)[[0, 127, 128, n - 1]]])
    Va = np.abs(V).T                                   # (n, k)
    prod = R @ (Rt @ V.T.astype(LD))
    pb = Ra @ (bRt @ Va) + bR @ (Rat @ Va)             # |R^ R^' - R R'| |v| to first order, R^ within bR of R
    target = top.A if n <= 400 else top.apply(V).T  # (V = I: the matrix itself)
    qt.check("%s by definition %s" % (tag, _kind(real)), prod, target, pb + top.bound_apply(V).T)
    return op


# ------------------------------------------------------------------------------------------------ the entries
def _vectors(n, k, real, salt):
    return np.random.default_rng(1000 * n + 10 * k + salt).standard_normal((k, n)).astype(real)


@functools.lru_cache(maxsize=None)
def _z(n, first, k):
    """(z, dz): the reference deviates of samples first .. first + k - 1 and the allowance for the device's"""
    z = np.array([z_ref(SEED, 0, n, s) for s in range(first, first + k)])
    zp = np.array([z_ref(SEED, 0, n, s ^ 1) for s in range(first, first + k)])
    return z, 8 * U * np.abs(z) + (4 * np.pi + 4) * U * np.hypot(z, zp)


def _check_plain(env, sol, tr, real, nt, off, ks, roots, tagx=""):
    """the entries of the plain model under one switch setting"""
    n, col = tr.n, tr.col
    kd = _kind(real) + tagx
    dev = lambda a: _dev(env, a, real, off)  # noqa: E731
    ops = {False: ((tr.B, ""), (tr.B_rec, " (recursion)")) if tr.real32 is not None else ((tr.B, ""),),
           True: ((tr.H, ""),)}
    for inverse in (False, True):
        nm = "H" if inverse else "B"
        alpha = 1 / tr.theta if inverse else tr.theta
        for k in ks:
            V = _vectors(n, k, real, 1)
            out = _np(sol.qn_apply(dev(V), out=_out(env, k, n, real, off), inverse=inverse))
            assert out.dtype == real
            for op, note in ops[inverse]:
                ref = op.apply(V)
                qt.check("qn_apply %s%s %s" % (nm, note, kd), out, ref, op.bound_apply(V, real, ref))
            if roots is not None:
                rop = roots[inverse]
                ref = rop.apply(V)
                out = _np(sol.qn_apply(dev(V), out=_out(env, k, n, real, off), inverse=inverse, sqrt=True))
                qt.check("qn_apply sqrt %s %s" % (nm, kd), out, ref, _rb(rop, V, real, ref))
        op = ops[inverse][-1][0]  # (what holds against the recursion)
        if col <= 32:
            out = _np(sol.qn_diag(out=_out(env, 0, n, real, off), inverse=inverse))
            ref = np.diag(op.A)
            qt.check("qn_diag %s %s" % (nm, kd), out, ref,
                     op.bound_diag() + (U32 * np.abs(ref.astype(np.float64)) if real == np.float32 else 0.0))
        ld_ref = -tr.logdet_b if inverse else tr.logdet_b
        ld_bound = op.bound_logdet(n * abs(float(np.log(alpha))), tr.cond)
        if col <= 64:
            qt.check("qn_logdet %s" % kd, sol.qn_logdet(inverse=inverse), ld_ref, ld_bound)
        c = _vectors(n, 1, real, 2)[0]
        for k in ks:
            V = _vectors(n, k, real, 3)
            for center in (None, c):
                Dv = V.astype(LD) - (0 if center is None else center.astype(LD))
                # (d = v - center is formed in fp64 on the device, exactly for fp32 operands: one rounding, 2 gamma_1)
                Dabs = np.abs(Dv).astype(np.float64) * (1 + 2 * U)
                cen = None if center is None else dev(center)
                ref = np.diag(op.quad(Dv))
                bq = np.diag(op.bound_quad(Dabs)) + 4 * U * np.diag(op.bound_quad(Dabs)) \
                    + (0 if center is None else 2 * U * 2 * _absquad(op, Dabs))
                q = sol.qn_quad(dev(V), center=cen, inverse=inverse)
                qt.check("qn_quad %s %s" % (nm, kd), q, ref, bq)
                if col <= 64:
                    # covariance A: the quadratic form of A^-1, the log det of A
                    iop = ops[not inverse][-1][0]
                    refq = np.diag(iop.quad(Dv)) / LD(SCALE) ** 2
                    bqi = (np.diag(iop.bound_quad(Dabs)) * (1 + 4 * U)
                           + (0 if center is None else 4 * U * _absquad(iop, Dabs))
                           ) / SCALE ** 2
                    terms = [n * np.log(2 * LD(np.pi)), 2 * n * np.log(LD(SCALE)), ld_ref]
                    ref = -(sum(terms) + refq) / 2
                    bl = 0.5 * (ld_bound + bqi) + qt.gamma(6) * (sum(abs(float(t)) for t in terms)
                                                                  + np.abs(refq).astype(np.float64))
                    lp = sol.qn_logpdf(dev(V), mean=cen, scale=SCALE, inverse=inverse)
                    qt.check("qn_logpdf %s %s" % (nm, kd), lp, ref, bl)
        for k in (4, 5):
            V = _vectors(n, k, real, 4)
            G = sol.qn_gram(dev(V), inverse=inverse)
            assert np.array_equal(G, G.T)
            qt.check("qn_gram %s %s" % (nm, kd), G, op.quad(V), op.bound_quad(V) * (1 + 4 * U))
        # index lists
        idx = np.array([n - 1, 0, 63, 64, 128, 0, n // 2], np.int64) % n
        blk = sol.qn_block(idx, inverse=inverse)
        assert np.array_equal(blk, blk.T)
        qt.check("qn_block %s %s" % (nm, kd), blk, op.A[np.ix_(idx, idx)], op.bound_block(idx, idx))
        ib = np.array([1, n - 2], np.int64)
        qt.check("qn_block %s %s" % (nm, kd), sol.qn_block(idx, ib, inverse=inverse), op.A[np.ix_(idx, ib)],
                 op.bound_block(idx, ib))
        for k in (1, 17, 128):
            ix = np.random.default_rng(k).integers(0, n, k)
            out = _np(sol.qn_cols(ix, out=_out(env, k, n, real, off), inverse=inverse))
            E = np.eye(n)[ix]
            ref = op.apply(E)
            qt.check("qn_cols %s %s" % (nm, kd), out, ref, op.bound_apply(E, real, ref))
        # the spectrum
        if 0 < col <= 64:
            _check_eig(env, sol, tr, op, real, off, inverse, kd)
        # draws
        if roots is not None:
            _check_draws(env, sol, tr, roots[inverse], op, real, off, inverse, kd, ld_ref, ld_bound)
    if col:
        ridx = np.array([0, n - 1, 64, 0], np.int64) % n
        rows = sol.qn_rows(ridx)
        want = tr.W[ridx].astype(np.float64)
        assert rows.shape == want.shape and np.array_equal(rows, want)  # (the stored values, bit for bit)


def _rb(rop, V, real, ref=None):
    """the bound of an apply of a checked root against its collected matrix: the root's own bound for the matrix and
    for the apply (2 x), and in REAL32 the store of every collected entry (2^-24 |R| |v|) and of the output"""
    b = 2 * rop.bound_apply(V, real, ref)
    if real == np.float32:
        b = b + U32 * (np.abs(np.asarray(V, np.float64)) @ np.abs(rop.A.astype(np.float64)).T)
    return b


def _absquad(op, D):
    """d'|A| d for every row d of D: the allowance of a rounded v - center"""
    if not hasattr(op, "absA"):
        op.absA = np.abs(op.A).astype(np.float64)
    return np.einsum("ki,ij,kj->k", D, op.absA, D)


def _check_eig(env, sol, tr, op, real, off, inverse, kd):
    n, d = tr.n, 2 * tr.col
    nm = "H" if inverse else "B"
    bulk, lam = sol.qn_eig(inverse=inverse)
    alpha = 1 / tr.theta if inverse else tr.theta
    assert abs(bulk - float(alpha)) <= qt.gamma(n + 2) * float(alpha)
    ev = np.linalg.eigvalsh(op.A.astype(np.float64))
    a2 = float(ev[-1])
    r = len(lam)
    assert 0 < r <= min(d, n) and np.all(np.diff(lam) >= 0)
    # the n - r eigenvalues at the bulk value taken out of eigvalsh's list, the others matched in order
    rest = list(ev)
    for _ in range(n - r):
        rest.pop(int(np.argmin(np.abs(np.array(rest) - float(alpha)))))
    qt.check("qn_eig %s %s" % (nm, kd), lam, np.array(rest), (op.eta + qt.gamma(n)) * a2)
    for k, basis in ((1, 1), (17, 1), (128, 1), (17, 0)):
        sol.set_option("qn_basis", basis)
        which = np.random.default_rng(k).integers(0, r, k).astype(np.int32)
        Uv = _np(sol.qn_eigvec(which, out=_out(env, k, n, real, off), inverse=inverse)).astype(np.float64)
        c = np.linalg.lstsq(tr.W.astype(np.float64), Uv.T, rcond=None)[0]  # (d, k)
        wc = np.abs(tr.W.astype(np.float64)) @ np.abs(c)
        e = qt.gamma(d + 2) * wc + (U32 * (np.abs(Uv.T) + (op.tiles - 1) * wc) if real == np.float32 else 0)
        tol = 2 * (op.eta + np.sqrt((e ** 2).sum(axis=0)))  # (k,)
        res = (op.A.astype(np.float64) @ Uv.T) - Uv.T * lam[which]
        qt.check("qn_eigvec residual %s %s" % (nm, kd), np.sqrt((res ** 2).sum(axis=0)), 0.0, a2 * tol)
        G = Uv @ Uv.T
        same = which[:, None] == which[None, :]
        qt.check("qn_eigvec orthonormal %s %s" % (nm, kd), G, same.astype(np.float64),
                 np.where(same, tol[:, None] + tol[None, :], np.inf))  # (distinct numbers: below)
        gap_ok = np.abs(lam[which][:, None] - lam[which][None, :]) > 0
        qt.check("qn_eigvec orthonormal %s %s" % (nm, kd), np.where(gap_ok & ~same, G, 0.0), 0.0,
                 tol[:, None] + tol[None, :])
    sol.set_option("qn_basis", 1)


def _check_draws(env, sol, tr, rop, op, real, off, inverse, kd, ld_ref, ld_bound):
    n = tr.n
    nm = "H" if inverse else "B"
    mean = _vectors(n, 1, real, 5)[0]
    Ra = np.abs(rop.A.astype(np.float64))
    for first, k in ((0, 5), (3, 4)):
        z, dz = _z(n, first, k)
        for mv in (None, mean):
            out, logp = sol.qn_draw(k, SEED, first=first, mean=None if mv is None else _dev(env, mv, real, off),
                                    scale=SCALE, inverse=inverse, out=_out(env, k, n, real, off), return_logpdf=True)
            out = _np(out)
            rz = SCALE * rop.apply(z)
            ref = rz + (0 if mv is None else mv.astype(LD))
            b = SCALE * (_rb(rop, z, real) + dz @ Ra.T) + 4 * U * (np.abs(rz).astype(np.float64)
                                                                        + (0 if mv is None else np.abs(mv)))
            if real == np.float32:  # (the store of every tile's partial draw carries the mean)
                b = b + U32 * (np.abs(ref).astype(np.float64) + (0 if mv is None else rop.tiles * np.abs(mv)))
            qt.check("qn_draw %s %s" % (nm, kd), out, ref, b)
            zz = (z.astype(LD) ** 2).sum(axis=1)
            terms = [n * np.log(2 * LD(np.pi)), 2 * n * np.log(LD(SCALE)), ld_ref]
            lref = -(sum(terms) + zz) / 2
            bl = 0.5 * (ld_bound + qt.gamma(n + 2) * zz.astype(np.float64) + 2 * (np.abs(z) * dz).sum(axis=1)) \
                + qt.gamma(6) * (sum(abs(float(t)) for t in terms) + zz.astype(np.float64))
            qt.check("qn_draw logpdf %s %s" % (nm, kd), logp, lref, bl)
            plain = _np(sol.qn_draw(k, SEED, first=first, mean=None if mv is None else _dev(env, mv, real, off),
                                    scale=SCALE, inverse=inverse, out=_out(env, k, n, real, off)))
            assert np.array_equal(plain, out)  # (the same bits with and without the density)


def _check_shift(env, sol, tr, real, nt, off, ks, lop, tagx=""):
    """the entries of the model plus a diagonal under one switch setting; lop: the checked factor L (or None)"""
    n, col = tr.n, tr.col
    kd = _kind(real) + tagx
    dev = lambda a: _dev(env, a, real, off)  # noqa: E731
    d = _shift_d(n, real)
    op = _shift_truth(tr, d)
    free = op.free
    sh = sol.qn_shift(dev(d), MU)
    assert sh.pinned == int((~free).sum())
    f32 = (lambda ref: U32 * np.abs(np.asarray(ref, np.float64))) if real == np.float32 else (lambda ref: 0.0)
    for k in ks:
        V = _vectors(n, k, real, 6)
        out = _np(sh.solve(dev(V), out=_out(env, k, n, real, off)))
        assert qt.pos_zero(out[:, ~free]).all()
        ref = op.apply(V)
        qt.check("shift solve %s" % kd, out, ref, op.bound_apply(V, real, ref))
        if lop is not None:
            out = _np(sh.sqrt(dev(V), out=_out(env, k, n, real, off)))
            assert qt.pos_zero(out[:, ~free]).all()
            ref = lop.apply(V)
            qt.check("shift sqrt %s" % kd, out, ref, _rb(lop, V, real, ref))
    if col <= 32:
        out = _np(sh.diag(out=_out(env, 0, n, real, off)))
        assert qt.pos_zero(out[~free]).all()
        ref = np.diag(op.A)
        qt.check("shift diag %s" % kd, out, ref, op.bound_diag() + f32(ref))
    ld_bound = op.bound_logdet(op.sum_abs_log, op.cond_a)
    qt.check("shift logdet %s" % kd, sh.logdet(), op.logdet, ld_bound)
    c = _vectors(n, 1, real, 7)[0]
    nf = int(free.sum())
    for k in ks:
        V = _vectors(n, k, real, 8)
        for center in (None, c):
            Dv = V.astype(LD) - (0 if center is None else center.astype(LD))
            Dabs = np.abs(Dv).astype(np.float64) * (1 + 2 * U)
            cen = None if center is None else dev(center)
            ref = np.diag(op.fwd.quad(Dv))
            bq = np.diag(op.fwd.bound_quad(Dabs)) * (1 + 4 * U) \
                + (0 if center is None else 4 * U * _absquad(op.fwd, Dabs))
            qt.check("shift quad %s" % kd, sh.quad(dev(V), center=cen), ref, bq)
            terms = [nf * np.log(2 * LD(np.pi)), 2 * nf * np.log(LD(SCALE)), -op.logdet]
            refq = ref / LD(SCALE) ** 2
            lref = -(sum(terms) + refq) / 2
            bl = 0.5 * (ld_bound + bq / SCALE ** 2) + qt.gamma(6) * (sum(abs(float(t)) for t in terms)
                                                                     + np.abs(refq).astype(np.float64))
            qt.check("shift log_prob %s" % kd, sh.log_prob(dev(V), mean=cen, scale=SCALE), lref, bl)
    idx = np.array([n - 1, 0, 1, 63, 64, 127, 128, 1, n // 2], np.int64) % n
    blk = sh.block(idx)
    assert np.array_equal(blk, blk.T)
    pin = ~free[idx]
    assert qt.pos_zero(blk[pin]).all() and qt.pos_zero(blk[:, pin]).all()
    qt.check("shift block %s" % kd, blk, op.A[np.ix_(idx, idx)], op.bound_block(idx, idx))
    for k in (1, 17, 128):
        ix = np.random.default_rng(k + 1).integers(0, n, k)
        out = _np(sh.columns(ix, out=_out(env, k, n, real, off)))
        assert qt.pos_zero(out[:, ~free]).all() and qt.pos_zero(out[~free[ix]]).all()
        E = np.eye(n)[ix]
        ref = op.apply(E)
        qt.check("shift columns %s" % kd, out, ref, op.bound_apply(E, real, ref))
    if lop is not None:
        mean = _vectors(n, 1, real, 9)[0]
        La = np.abs(lop.A.astype(np.float64))
        for first, k in ((0, 5), (3, 4)):
            z, dz = _z(n, first, k)
            for mv in (None, mean):
                out, logp = sh.sample(k, SEED, first=first, mean=None if mv is None else dev(mv), scale=SCALE,
                                      log_prob=True, out=_out(env, k, n, real, off))
                out = _np(out)
                lz = SCALE * lop.apply(z)
                ref = lz + (0 if mv is None else mv.astype(LD))
                b = SCALE * (_rb(lop, z, real) + dz @ La.T) + 4 * U * (np.abs(lz).astype(np.float64)
                                                                            + (0 if mv is None else np.abs(mv)))
                qt.check("shift sample %s" % kd, out, ref, b + f32(ref) + (0 if mv is None else lop.tiles * f32(mv)))
                if mv is None:
                    assert qt.pos_zero(out[:, ~free]).all()
                else:
                    assert np.array_equal(out[:, ~free], np.broadcast_to(mv[~free], (k, int((~free).sum()))))
                zz = (z[:, free].astype(LD) ** 2).sum(axis=1)
                terms = [nf * np.log(2 * LD(np.pi)), 2 * nf * np.log(LD(SCALE)), -op.logdet]
                lref = -(sum(terms) + zz) / 2
                bl = 0.5 * (ld_bound + qt.gamma(n + 2) * zz.astype(np.float64) + 2 * (np.abs(z) * dz).sum(axis=1)) \
                    + qt.gamma(6) * (sum(abs(float(t)) for t in terms) + zz.astype(np.float64))
                qt.check("shift sample log_prob %s" % kd, logp, lref, bl)
    return sh


def _roots(env, sol, tr, real):
    """the two roots of the plain model and the factor of the shifted one, checked by their definitions"""
    n = tr.n
    roots = {}
    for inverse in (False, True):
        op = (tr.H if inverse else tr.B_rec)
        alpha = 1 / tr.theta if inverse else tr.theta
        roots[inverse] = _root_op(env, tr, lambda v: sol.qn_apply(v, inverse=inverse, sqrt=True), np.sqrt(alpha), 1, 1,
                                  op, real, "root " + ("H" if inverse else "B"))
    d = _shift_d(n, real)
    sop = _shift_truth(tr, d)
    sh = sol.qn_shift(_dev(env, d, real, 0), MU)
    sw = np.sqrt(sop.w)
    lop = _root_op(env, tr, sh.sqrt, sw, sop.w, sw, sop, real, "shift sqrt", free=sop.free, symmetric=False)
    return roots, lop


def _all_switches(env, sol, tr, real, grids=(0,), full_ks=(1, 2, 3, 4, 5, 9)):
    roots, lop = _roots(env, sol, tr, real) if tr.col <= 64 else (None, None)
    for wg in grids:
        sol.set_option("wgrid", wg)
        for nt in (0, 1):
            sol.set_option("nt", nt)
            for off in (0, 1):
                ks = full_ks if (nt, off) == (0, 0) else (3, 5)
                tagx = " packed" if tr.g == 2 else ""
                _check_plain(env, sol, tr, real, nt, off, ks, roots, tagx)
                if tr.col <= 64:
                    _check_shift(env, sol, tr, real, nt, off, ks, lop, tagx)
    sol.set_option("nt", 0)
    sol.set_option("wgrid", 0)


# ------------------------------------------------------------------------------------------------ states by import
def _states():
    out = []
    for col in COLS:
        out.append((259, max(col, 1), col, "dyadic", np.float64))     # m = col, head = 1
        out.append((259, max(col, 1), col, "generic", np.float64))
        out.append((259, max(col, 1), col, "dyadic", np.float32))
    for col in (5, 10, 17):
        out.append((259, col, col, "generic", np.float32))
    out.append((259, 9, 6, "dyadic", np.float64))                    # col < m: the ring partly filled
    for m, npairs in ((5, 8), (10, 17), (16, 21), (17, 20), (33, 40)):  # the ring wrapped: head != 1, one per tile class
        out.append((259, m, npairs, "generic", np.float64))
    for m, npairs in ((10, 17), (33, 40)):
        out.append((259, m, npairs, "dyadic", np.float32))
    out.append((63, 5, 7, "dyadic", np.float64))                     # less than a wave
    out.append((63, 33, 33, "generic", np.float64))
    out.append((63, 17, 17, "dyadic", np.float32))
    return out


def _sid(s):
    n, m, npairs, fam, real = s
    return "n%d-m%d-pairs%d-%s-%s" % (n, m, npairs, fam, _kind(real))


def _import(env, n, m, npairs, fam, real):
    st = qs.synth(n, m, npairs, fam, real)
    S, Y = st.pairs()
    r32 = (st.mats("sy"), st.mats("wt")) if real == np.float32 else None
    theta = None
    if r32 is not None and st.col:
        # the context divides y'y of the newest pair by the s'y it was given: the imported fp32 number (the same
        # value in the dyadic family); the recursion starts from that theta
        y = Y[:, -1].astype(LD)
        theta = (y @ y) / LD(r32[0][st.col - 1, st.col - 1])
    tr = _truth((n, m, npairs, fam, real),
                lambda: qt.Truth(S, Y, theta=theta, real32=r32, sy_exact=fam == "dyadic"))
    sol = env["la"].DeviceSolver(n, m, real32=real == np.float32)
    sol.import_state(st.wa, st.iwa, st.isave)
    return st, tr, sol


@pytest.mark.parametrize("state", _states(), ids=_sid)
def test_imported_state(env, state):
    n, m, npairs, fam, real = state
    st, tr, sol = _import(env, *state)
    try:
        assert tr.col == st.col == min(npairs, m) and (st.head != 1) == (npairs > m > 1)
        _all_switches(env, sol, tr, real)
    finally:
        sol.close()


@pytest.mark.parametrize("col,real", [(10, np.float64), (17, np.float32)], ids=["col10-fp64", "col17-fp32"])
def test_one_workgroup_many_trips(env, col, real):
    """n = 1027 with "wgrid" 1: two full trips, a partial third and the tail; three 512-row trips of the basis and
    cols kernels.  The roots are collected at the default grid and checked by R (R v) = A v on ten vectors."""
    st, tr, sol = _import(env, 1027, col, col + 4, "generic" if real == np.float64 else "dyadic", real)
    try:
        _all_switches(env, sol, tr, real, grids=(1,), full_ks=(1, 4, 9))
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ the packed layout
@pytest.mark.parametrize("ring", ["part", "wrapped"])
@pytest.mark.parametrize("m", [5, 10])
def test_packed_layout(env, m, ring):
    """a state from a run of the mixed-nbd bounded quadratic at n = 1027 with compact_w on: W in the tile-local layout
    (CW = true), with the ring partly filled or after it has wrapped.  export_state puts W back into natural
    order, so the reference reads the pairs through qn_rows, which gathers the stored values from the layout as it
    is; after the entries have run, export_state must give the same pairs bit for bit."""
    la = env["la"]
    n = 1027
    p = _problem(env, "quadratic", n, m)
    sol = la.DeviceSolver(n, m, options={"compact_w": 2, "compact_policy": 2, "compact_min_rows": 0})
    # (compact_policy 2 re-packs in every iteration: the automatic policy packs only once the ring is full)
    seen = {}
    try:
        def at(s, t):
            if not t.startswith("NEW_X") or not s.compact_stats()[2]:
                return
            col, head = int(s.isave[27]), int(s.isave[26])
            tag = "part" if 2 <= col < m else ("wrapped" if col == m and int(s.isave[30]) > m and head > 1 else None)
            if tag != ring or tag in seen:
                return
            before = s.compact_stats()
            rows = s.qn_rows(np.arange(n, dtype=np.int64))
            assert rows.shape == (n, 2 * col)
            S, Y = rows[:, :col].copy(), rows[:, col:].copy()
            tr = qt.Truth(S, Y, theta=float(s.dsave[0]), g=2)
            _all_switches(env, s, tr, np.float64, grids=(0, 1), full_ks=(1, 4, 9))
            assert s.compact_stats() == before and before[2]  # (still packed: the passes read the layout as it is)
            S2, Y2 = qs.ring_pairs(s.export_state()[0], n, m, col, head)
            assert np.array_equal(S, S2) and np.array_equal(Y, Y2)  # (the reference read the pairs of this return)
            seen[tag] = (col, head)
        _drive(env, sol, p, max_iter=6 * m + 20, at_return=at, until=lambda s: bool(seen))
    finally:
        sol.close()
    assert set(seen) == {ring}, seen


def test_zz_ratio_table():
    """prints the worst err / bound of every entry family of this module's run (run with -s to read it)"""
    for tag in sorted(qt.RATIOS):
        print("%-44s %.3g" % (tag, qt.RATIOS[tag]))
