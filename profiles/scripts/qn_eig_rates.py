"""Rates of the eigenvectors of the curvature model (lbfgsb_hip_qn_eigvec) at the headline size: n = 1e8, m = 10 with
full memory, fp64, all k = r vectors (20 when no direction falls under the cut), in natural row order (compact_w = 0)
and on the packed tile-local layout after a bench-like warm-up (compact_w = 1).  In one process per layout, hipEvent
times around each call, the median of `reps` calls after a warm-up call:
  qn_eigvec by the basis pass (option "qn_basis" = 1);
  qn_eigvec by the expansion route ("qn_basis" = 0: qn_expand, 4 vectors a pass) -- the A/B partner;
  qn_apply (B) at k = 4 -- the yardstick.
Derived: the basis pass's share of 8 TB/s on its algorithmic bytes (2 * 2m reals per row at k = 2m), the expansion
route's share on its own ((2m + 8) reals per row and pass), the yardstick's on its two passes ((2m + 4) + (2m + 8)
reals per row), and the speed-up of the basis pass over the expansion route.  The times are those of the calls: a
repeated qn_eigvec call keeps its coefficients on the device, so it is the launches and the final wait.
Prints one JSON line.
usage: python profiles/scripts/qn_eig_rates.py [--n N] [--iters K] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402

PEAK = 8.0e12  # bytes per second


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
        del x, g, l, u, nbd
        bulk, lam = sol.qn_eig()
        k = len(lam)
        assert k >= 1
        U = torch.empty((k, n), dtype=torch.float64, device="cuda")
        v4 = torch.randn(4, n, dtype=torch.float64, device="cuda")
        out4 = torch.empty_like(v4)

        def timed(f):
            f()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return float(np.median(ms)), float(min(ms)), float(max(ms))

        res = dict(compact_stats=list(sol.compact_stats()), k=k, bulk=bulk, lambda_min=float(lam.min()),
                   lambda_max=float(lam.max()))
        res["basis_ms"], res["basis_min_ms"], res["basis_max_ms"] = timed(lambda: sol.qn_eigvec(out=U))
        sol.set_option("qn_basis", 0)
        res["expand_ms"], res["expand_min_ms"], res["expand_max_ms"] = timed(lambda: sol.qn_eigvec(out=U))
        sol.set_option("qn_basis", 1)
        res["Bv_k4_ms"], _, _ = timed(lambda: sol.qn_apply(v4, out4))
        e = 8
        passes = (k + 3) // 4
        res["basis_share"] = (2 * m + k) * e * n / (res["basis_ms"] * 1e-3) / PEAK
        res["expand_share"] = (passes * 2 * m + 2 * k) * e * n / (res["expand_ms"] * 1e-3) / PEAK
        res["speedup"] = res["expand_ms"] / res["basis_ms"]
        res["Bv_k4_share"] = (4 * m + 12) * e * n / (res["Bv_k4_ms"] * 1e-3) / PEAK
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_eig_rates.py measures on the MI355X"
    line = dict(metric="qn_eigvec ms per call", n=a.n, m=a.m, dtype="f64", peak_bytes_per_s=PEAK,
                natural=run(a.n, a.m, a.iters, a.reps, {"compact_w": 0}),
                packed=run(a.n, a.m, a.iters, a.reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
