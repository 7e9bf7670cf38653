"""Every output bit of the curvature-model operators (qn_*, qn_shift_*, the index lists) on fixed cases, for comparing
two builds of the library: a refactor of k_qn*.hip / solver_qn*.inl must leave every array as it is.

    LBFGSB_HIP_LIBRARY=/path/to/liblbfgsb_hip.so python profiles/scripts/qn_bits.py --out A.npz   (once per build)
    python profiles/scripts/qn_bits.py --compare A.npz B.npz    (exit 1 at the first array that differs in any byte)

One process runs the built-in bounded quadratic from x = 0 and, at the returns where the number of stored pairs reaches
one of COLS (the tile and piece boundaries of qn_plan.hpp) and once after the ring has wrapped, calls every entry with
inputs from fixed seeds: blocks of 1, 2, 3, 4, 5 and 9 vectors, fp64 and REAL32, the natural and (fp64, m <= 10) the
packed layout, n = 63 (less than a wave) and n = 1537 (twelve layout tiles and a row), every operand and output once
offset by one element, draws from an even and from an odd first sample, a shift with every third row pinned, index
lists with a repeat; and at n = 1 000 003 (the grid is the resident-workgroup count, no longer the row count) m = 10,
fp64, both layouts, k = 4.  An entry that refuses contributes its message; an array of more than 1 MiB contributes the
SHA-256 of its bytes.  Needs the GPU; takes seconds."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

COLS = (0, 1, 5, 6, 10, 11, 16, 17, 33)
KS = (1, 2, 3, 4, 5, 9)


def entries(sol, torch, la, tag, ks, res):
    """call every entry on the pairs of this return; res[tag/...] = the bytes that came out"""
    n, real = sol.n, sol.real
    dt = torch.float32 if real == np.float32 else torch.float64
    rng = np.random.default_rng(12345 + n)

    def put(name, f):
        try:
            v = f()
        except la.LbfgsbError as e:
            v = np.frombuffer(str(e).encode(), np.uint8)
        for i, a in enumerate(v if isinstance(v, tuple) else (v,)):
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            if a.nbytes > 1 << 20:  # (the large size: the SHA-256 of the bytes stands for them)
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
            res["%s/%s/%d" % (tag, name, i)] = a

    def vec(k, off=0):
        """(k, n) standard normals; off: the first element sits `off` elements into its buffer (not 16-byte aligned)"""
        h = rng.standard_normal((k, n)).astype(real)
        buf = torch.zeros(k * n + off, dtype=dt, device="cuda")
        buf[off:] = torch.from_numpy(h).reshape(-1).cuda()
        return buf[off:].view(k, n)

    def out(k, off=0):
        return torch.zeros(k * n + off, dtype=dt, device="cuda")[off:].view(k, n)

    idx = np.array([n - 1, 0, n // 2, 0, n // 3], np.int64)  # (unsorted, 0 twice)
    ib = np.array([1 % n, n - 1], np.int64)
    for inv in (False, True):
        t = "H" if inv else "B"
        put("diag" + t, lambda: sol.qn_diag(inverse=inv))
        put("logdet" + t, lambda: sol.qn_logdet(inverse=inv))
        put("eig" + t, lambda: sol.qn_eig(inverse=inv))
        for basis in (1, 0):
            sol.set_option("qn_basis", basis)
            put("eigvec%s%d" % (t, basis), lambda: sol.qn_eigvec(inverse=inv))
        sol.set_option("qn_basis", 1)
        put("block" + t, lambda: sol.qn_block(idx, inverse=inv))
        put("block2" + t, lambda: sol.qn_block(idx, ib, inverse=inv))
        put("cols" + t, lambda: sol.qn_cols(idx, inverse=inv))
        put("cols_off" + t, lambda: sol.qn_cols(idx, out=out(len(idx), 1), inverse=inv))
    put("rows", lambda: sol.qn_rows(idx))
    d = torch.from_numpy((10.0 * rng.random(n + 1)).astype(real)).cuda()
    d[0::3] = float("inf")
    shifts = [("sh", lambda: sol.qn_shift(d[:n], 0.3)), ("sh_off", lambda: sol.qn_shift(d[1:], 0.3)),
              ("sh0", lambda: sol.qn_shift(None, 0.25))]
    for k in ks:
        for off in ((0, 1) if k == 2 else (0,)):
            o = "k%d%s" % (k, "_off" if off else "")
            v, c = vec(k, off), vec(1, off)[0]
            for inv in (False, True):
                t = o + ("H" if inv else "B")
                put("apply" + t, lambda: sol.qn_apply(v, out(k, off), inverse=inv))
                put("sqrt" + t, lambda: sol.qn_apply(v, out(k, off), inverse=inv, sqrt=True))
                put("quad" + t, lambda: sol.qn_quad(v, c, inverse=inv))
                put("quad0" + t, lambda: sol.qn_quad(v, inverse=inv))
                put("gram" + t, lambda: sol.qn_gram(v, c, inverse=inv))
                put("logpdf" + t, lambda: sol.qn_logpdf(v, c, 0.7, inverse=inv))
                for first in (4, 3):
                    put("draw%s_%d" % (t, first), lambda: sol.qn_draw(k, 99, first, c, 0.7, inv, out(k, off)))
                    put("drawlp%s_%d" % (t, first),
                        lambda: sol.qn_draw(k, 99, first, None, 1.3, inv, out(k, off), True))
    for name, make in shifts:
        try:
            sh = make()
        except la.LbfgsbError as e:
            res["%s/%s/refused" % (tag, name)] = np.frombuffer(str(e).encode(), np.uint8)
            continue
        put(name + "/pinned", lambda: np.int64(sh.pinned))
        put(name + "/logdet", sh.logdet)
        put(name + "/diag", sh.diag)
        put(name + "/block", lambda: sh.block(idx))
        put(name + "/block2", lambda: sh.block(idx, ib))
        put(name + "/cols", lambda: sh.columns(idx))
        for k in (ks if name == "sh" else ks[:2]):
            for off in ((0, 1) if k == 2 else (0,)):
                o = "%s/k%d%s" % (name, k, "_off" if off else "")
                v, c = vec(k, off), vec(1, off)[0]
                put(o + "solve", lambda: sh.solve(v, out(k, off)))
                put(o + "sqrt", lambda: sh.sqrt(v, out(k, off)))
                put(o + "quad", lambda: sh.quad(v, c))
                put(o + "quad0", lambda: sh.quad(v))
                put(o + "logp", lambda: sh.log_prob(v, c, 0.7))
                for first in (4, 3):
                    put("%ssample_%d" % (o, first), lambda: sh.sample(k, 99, first, c, 0.7, out=out(k, off)))
                    put("%ssamplelp_%d" % (o, first), lambda: sh.sample(k, 99, first, None, 1.3, True, out(k, off)))


def run_case(torch, la, n, m, real32, compact_w, cols, ks, res):
    tag0 = "n%d_m%d_%s_cw%d" % (n, m, "r32" if real32 else "f64", compact_w)
    sol = la.DeviceSolver(n, m, real32=real32, options={"compact_w": compact_w})
    try:
        dt = torch.float32 if real32 else torch.float64
        x = torch.zeros(n, dtype=dt, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        seen, wrapped = set(), False
        for _ in range(40 * (m + 4)):
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            col, it = int(sol.isave[27]), int(sol.isave[29])
            if t.startswith("NEW_X") or (t.startswith("FG_START") and col == 0):
                wrap = col == m and it >= m + 3 and not wrapped
                if (col in cols and col not in seen) or wrap:
                    seen.add(col)
                    wrapped = wrapped or wrap
                    entries(sol, torch, la, "%s_col%d%s" % (tag0, col, "w" if wrap else ""), ks, res)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or wrapped or it > m + 4:
                break
        res[tag0 + "/end"] = np.frombuffer(t.encode(), np.uint8)
        res[tag0 + "/x"] = np.frombuffer(hashlib.sha256(x.cpu().numpy().tobytes()).digest(), np.uint8)
        print("%s: pairs %s%s, ended at %r"
              % (tag0, sorted(seen), " and the wrapped ring" if wrapped else "", t.strip()))
    finally:
        sol.close()


def compare(a, b):
    A, B = np.load(a), np.load(b)
    for k in sorted(set(A.files) | set(B.files)):
        if k not in A.files or k not in B.files:
            print("qn_bits: %s is in one file only" % k)
            return 1
        x, y = A[k], B[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            print("qn_bits: %s differs" % k)
            return 1
    print("qn_bits: %d arrays, all equal" % len(A.files))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="qn_bits.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--big", type=int, default=1_000_003, help="the large size (0: skip it)")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "qn_bits.py runs on the MI355X"
    print("library:", lbfgsb_amd.capi.lib_path())
    res = {}
    for n in (63, 1537):
        run_case(torch, lbfgsb_amd, n, 33, False, 0, COLS, KS, res)
        run_case(torch, lbfgsb_amd, n, 33, True, 0, COLS, KS, res)
        run_case(torch, lbfgsb_amd, n, 10, False, 2, COLS, KS, res)
    if a.big:
        for cw in (0, 2):
            run_case(torch, lbfgsb_amd, a.big, 10, False, cw, (10,), (4,), res)
    np.savez(a.out, **res)
    print("qn_bits: %d arrays -> %s" % (len(res), a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
