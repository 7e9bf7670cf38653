"""Rates of the Gram matrices of the curvature model on blocks of vectors (lbfgsb_hip_qn_gram) at the headline size:
n = 1e8, m = 10, fp64, the separable bounded quadratic on the device, in natural row order (compact_w = 0) and on the
packed tile-local layout after a bench-like warm-up (compact_w = 1).  The routes are called in turn in one process,
each call between two events on the context's stream; the medians of `reps` rounds, with min and max, go into one
JSON line:
  qn_gram (B, with a center) at k = 4 against qn_quad at k = 4: the same bytes, 6 more accumulators;
  qn_gram at k = 4, 8 and 16 against the unfused route to the same matrix: torch.sub into a buffer, qn_apply(D, B),
  torch.matmul(D, (B D)'), the matrix to the host -- the two must agree to 1e-9 |d_a|_B |d_b|_B;
  the cross-block pass (4 x 4, with a center): one call at k = 8 (two passes over W, one cross launch) minus two
  calls at k = 4 on its two halves, round by round -- the launch with its finalize and its fetch; beside it
  torch.matmul of the same two 4 x n blocks on the same stream.
usage: python profiles/scripts/qn_gram_rates.py [--n N] [--iters K] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402

KS = (4, 8, 16)


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
        torch.cuda.synchronize()
        stream = torch.cuda.ExternalStream(sol.stream)  # every route below runs on the context's stream
        with torch.cuda.stream(stream):
            kmax = max(KS)
            v = torch.randn(kmax, n, dtype=torch.float64, device="cuda")
            c = torch.randn(n, dtype=torch.float64, device="cuda")
            d, out = torch.empty_like(v), torch.empty_like(v)
            small = torch.empty((4, 4), dtype=torch.float64, device="cuda")

            def unfused(k):
                torch.sub(v[:k], c, out=d[:k])
                sol.qn_apply(d[:k], out[:k])
                return torch.matmul(d[:k], out[:k].t()).cpu().numpy()

            routes = {"quad_k4": lambda: sol.qn_quad(v[:4], center=c)}
            for k in KS:
                routes["gram_k%d" % k] = lambda k=k: sol.qn_gram(v[:k], center=c)
                routes["unfused_k%d" % k] = lambda k=k: unfused(k)
            routes["gram_k4_twice"] = lambda: (sol.qn_gram(v[:4], center=c), sol.qn_gram(v[4:8], center=c))
            routes["matmul_4x4"] = lambda: torch.matmul(v[:4], v[4:8].t(), out=small)
            times = {name: [] for name in routes}
            for f in routes.values():  # warm-up of every shape (code objects, the cached Gram of the pairs)
                f()
            stream.synchronize()
            for k in KS:  # the same matrix by both routes
                gf, gu = sol.qn_gram(v[:k], center=c), unfused(k)
                na = np.sqrt(np.diag(gu))
                assert np.all(np.abs(gf - gu) <= 1e-9 * np.outer(na, na)), (k, gf, gu)
            for _ in range(reps):
                for name, f in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f()
                    e1.record(stream)
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            times["cross_4x4"] = [a - b for a, b in zip(times["gram_k8"], times["gram_k4_twice"])]
            res = dict(compact_stats=list(sol.compact_stats()))
            for name, ts in times.items():
                res[name + "_ms"] = float(np.median(ts))
                res[name + "_minmax_ms"] = [float(min(ts)), float(max(ts))]
            res["gram_minus_quad_k4_ms"] = res["gram_k4_ms"] - res["quad_k4_ms"]
            for k in KS:
                res["gram_over_unfused_k%d" % k] = res["gram_k%d_ms" % k] / res["unfused_k%d_ms" % k]
            res["cross_4x4_share_of_8TBs"] = 72.0 * n / (res["cross_4x4_ms"] * 1e-3) / 8e12
            res["cross_over_matmul_4x4"] = res["cross_4x4_ms"] / res["matmul_4x4_ms"]
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_gram_rates.py measures on the MI355X"
    m, e = a.m, 8

    def fused(k):  # k / 4 passes over W with the center, a cross pass per pair of blocks
        nb = k // 4
        return nb * (2 * m + 4 + 1) * e + nb * (nb - 1) // 2 * 9 * e

    def unfused(k):  # W'V and expand per block, the product (D and B D once), the subtraction (k + 1 in, k out)
        nb = k // 4
        return nb * ((2 * m + 4) * e + (2 * m + 8) * e) + 2 * k * e + (2 * k + 1) * e
    line = dict(metric="qn gram ms per call", n=a.n, m=m, dtype="f64", reps=a.reps,
                bytes_per_row={"gram_k%d" % k: fused(k) for k in KS} | {"unfused_k%d" % k: unfused(k) for k in KS}
                | {"cross_4x4": 9 * e},
                natural=run(a.n, m, a.iters, a.reps, {"compact_w": 0}),
                packed=run(a.n, m, a.iters, a.reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
