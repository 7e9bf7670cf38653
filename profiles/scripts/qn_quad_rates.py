"""Rates of the quadratic forms and Gaussian log-densities of the curvature model (lbfgsb_hip_qn_quad,
lbfgsb_hip_qn_logpdf, lbfgsb_hip_qn_draw_logpdf) at the headline size: n = 1e8, m = 10, fp64, the separable bounded
quadratic on the device, in natural row order (compact_w = 0) and on the packed tile-local layout after a bench-like
warm-up (compact_w = 1).  The routes are called in turn in one process, each call between two events on the
context's stream; the medians of `reps` rounds, with min and max, go into one JSON line:
  qn_quad (B, with a center) at k = 1 and k = 4 against the unfused route a caller has without it for the same
  numbers: torch.sub into a buffer, qn_apply(D, B), one torch.dot per vector, the k results to the host;
  qn_draw against qn_draw_logpdf at k = 4 (covariance H): the same draws, with and without their densities;
  qn_logpdf at the 4 stored draws, the only route to those densities without qn_draw_logpdf.
usage: python profiles/scripts/qn_quad_rates.py [--n N] [--iters K] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

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
        torch.cuda.synchronize()
        stream = torch.cuda.ExternalStream(sol.stream)  # every route below runs on the context's stream
        with torch.cuda.stream(stream):
            v4 = torch.randn(4, n, dtype=torch.float64, device="cuda")
            c = torch.randn(n, dtype=torch.float64, device="cuda")
            d4, out4, dr4 = torch.empty_like(v4), torch.empty_like(v4), torch.empty_like(v4)

            def unfused(k):
                torch.sub(v4[:k], c, out=d4[:k])
                sol.qn_apply(d4[:k], out4[:k])
                return torch.stack([torch.dot(d4[j], out4[j]) for j in range(k)]).cpu().numpy()

            routes = {
                "quad_k1": lambda: sol.qn_quad(v4[0], center=c),
                "unfused_k1": lambda: unfused(1),
                "quad_k4": lambda: sol.qn_quad(v4, center=c),
                "unfused_k4": lambda: unfused(4),
                "draw_k4": lambda: sol.qn_draw(4, 1, out=dr4),
                "draw_logpdf_k4": lambda: sol.qn_draw(4, 1, out=dr4, return_logpdf=True),
                "logpdf_at_draws_k4": lambda: sol.qn_logpdf(dr4),
            }
            times = {k: [] for k in routes}
            for f in routes.values():  # warm-up of every shape (code objects, the cached Gram and root)
                f()
            stream.synchronize()
            q, qu = sol.qn_quad(v4, center=c), unfused(4)
            assert np.all(np.abs(q - qu) <= 1e-9 * np.abs(qu)), (q, qu)  # the same numbers by both routes
            for _ in range(reps):
                for name, f in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f()
                    e1.record(stream)
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            res = dict(compact_stats=list(sol.compact_stats()))
            for name, ts in times.items():
                res[name + "_ms"] = float(np.median(ts))
                res[name + "_minmax_ms"] = [float(min(ts)), float(max(ts))]
            res["quad_over_unfused_k1"] = res["quad_k1_ms"] / res["unfused_k1_ms"]
            res["quad_over_unfused_k4"] = res["quad_k4_ms"] / res["unfused_k4_ms"]
            res["draw_logpdf_minus_draw_k4_ms"] = res["draw_logpdf_k4_ms"] - res["draw_k4_ms"]
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
    assert torch.cuda.is_available(), "qn_quad_rates.py measures on the MI355X"
    m, e = a.m, 8
    line = dict(metric="qn quad / logpdf ms per call", n=a.n, m=m, dtype="f64", reps=a.reps,
                # algorithmic bytes per row at k = 4 (fp64): the fused pass reads 2m W entries and k vector entries
                # (and the center); the unfused route reads 2m + k (W'V), reads 2m + k and writes k (expand), reads
                # 2k (dots) -- and before them reads k + 1 and writes k (the subtraction)
                bytes_per_row=dict(quad_k4=(2 * m + 4) * e, quad_center=e,
                                   unfused_k4=(2 * m + 4) * e + (2 * m + 8) * e + 8 * e, unfused_sub_k4=9 * e),
                natural=run(a.n, m, a.iters, a.reps, {"compact_w": 0}),
                packed=run(a.n, m, a.iters, a.reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
