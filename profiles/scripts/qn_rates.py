"""Rates of the curvature-model operator (lbfgsb_hip_qn_apply / qn_diag) at the headline size: n = 1e8, m = 10,
fp64, the separable bounded quadratic on the device, in natural row order (compact_w = 0) and on the packed
tile-local layout after a bench-like warm-up (compact_w = 1).  Prints one JSON line: ms per call of B v, H v with the
Gram cached, H v with a stale Gram, a block of k = 4 (B and H), diag(H), and the algorithmic bytes per row of each
kernel.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
usage: python profiles/scripts/qn_rates.py [--n N] [--iters K] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402


def run(n, m, iters, reps, options):
    sol = lbfgsb_amd.DeviceSolver(n, m, options=options)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        for _ in range(10 * iters):
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
                break
        assert t.startswith("NEW_X") and int(sol.isave[27]) == m, t
        v = torch.randn(n, dtype=torch.float64, device="cuda")
        v4 = torch.randn(4, n, dtype=torch.float64, device="cuda")
        out, out4 = torch.empty_like(v), torch.empty_like(v4)

        def timed(f):
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3

        res = dict(compact_stats=list(sol.compact_stats()))
        res["Bv_ms"] = timed(lambda: sol.qn_apply(v, out))
        res["Hv_ms"] = timed(lambda: sol.qn_apply(v, out, inverse=True))
        res["Bv_k4_ms"] = timed(lambda: sol.qn_apply(v4, out4))
        res["Hv_k4_ms"] = timed(lambda: sol.qn_apply(v4, out4, inverse=True))
        res["diagH_ms"] = timed(lambda: sol.qn_diag(out, inverse=True))
        # a stale Gram: re-import the exported state (a new pair generation) in front of each timed call
        wa, iwa = sol.export_state()
        isave = sol.isave.copy()
        stale = []
        for _ in range(max(1, reps // 4)):
            sol.import_state(wa, iwa, isave)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sol.qn_apply(v, out, inverse=True)
            torch.cuda.synchronize()
            stale.append((time.perf_counter() - t0) * 1e3)
        res["Hv_stale_gram_ms"] = float(np.median(stale))
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_rates.py measures on the MI355X"
    m, e = a.m, 8
    line = dict(metric="qn operator ms per call", n=a.n, m=m, dtype="f64",
                # algorithmic bytes per row (fp64): W'V reads 2m W entries + k vectors; expand reads 2m + k and
                # writes k; diag reads 2m and writes 1; the Gram is m W'V passes with the Y columns as vectors
                bytes_per_row=dict(wtv_k1=(2 * m + 1) * e, wtv_k4=(2 * m + 4) * e, expand_k1=(2 * m + 2) * e,
                                   expand_k4=(2 * m + 8) * e, diag=(2 * m + 1) * e),
                natural=run(a.n, m, a.iters, a.reps, {"compact_w": 0}),
                packed=run(a.n, m, a.iters, a.reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
