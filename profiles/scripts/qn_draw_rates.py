"""Rates of the square roots and draws of the curvature model (lbfgsb_hip_qn_apply's root modes, lbfgsb_hip_qn_draw)
at the headline size: n = 1e8, m = 10, fp64, the separable bounded quadratic on the device, in natural row order
(compact_w = 0) and on the packed tile-local layout after a bench-like warm-up (compact_w = 1).  The routes are
called in turn in one process, each call between two events on the context's stream; the medians of `reps` rounds go
into one JSON line:
  B v against B^(1/2) v at k = 1 and k = 4 (the same kernels: only the host's coefficient map differs);
  qn_draw (k = 4, covariance B) against the unfused route a caller has without it, torch.randn(4, n) on the same
  stream followed by qn_apply(V, B);
  the first root call after a new set of pairs (Gram pass + the host's eigenproblems) against a first H v (Gram pass
  alone).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
usage: python profiles/scripts/qn_draw_rates.py [--n N] [--iters K] [--reps R] [--first-reps F] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402


def run(n, m, iters, reps, first_reps, options):
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
            v = torch.randn(n, dtype=torch.float64, device="cuda")
            v4 = torch.randn(4, n, dtype=torch.float64, device="cuda")
            out, out4, z4 = torch.empty_like(v), torch.empty_like(v4), torch.empty_like(v4)

            def unfused():
                torch.randn(4, n, dtype=torch.float64, device="cuda", out=z4)
                sol.qn_apply(z4, out4)

            routes = {
                "Bv_k1": lambda: sol.qn_apply(v, out),
                "Bsqrt_k1": lambda: sol.qn_apply(v, out, sqrt=True),
                "Bv_k4": lambda: sol.qn_apply(v4, out4),
                "Bsqrt_k4": lambda: sol.qn_apply(v4, out4, sqrt=True),
                "Hsqrt_k4": lambda: sol.qn_apply(v4, out4, sqrt=True, inverse=True),
                "draw_k4": lambda: sol.qn_draw(4, 1, inverse=False, out=out4),
                "unfused_k4": unfused,
                "draw_k1": lambda: sol.qn_draw(1, 1, inverse=False, out=out),
            }
            times = {k: [] for k in routes}
            for f in routes.values():  # warm-up of every shape (code objects, the cached Gram and roots)
                f()
            stream.synchronize()
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
            res["draw_over_unfused_k4"] = res["draw_k4_ms"] / res["unfused_k4_ms"]
            if not first_reps:
                return res
            # a new set of pairs: re-import the exported state in front of each timed call
            wa, iwa = sol.export_state()
            isave = sol.isave.copy()
            first = {"Hv": [], "Bsqrt": []}
            for _ in range(first_reps):
                for name, kw in (("Hv", dict(inverse=True)), ("Bsqrt", dict(sqrt=True))):
                    sol.import_state(wa, iwa, isave)
                    stream.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    sol.qn_apply(v, out, **kw)
                    e1.record(stream)
                    e1.synchronize()
                    first[name].append(e0.elapsed_time(e1))
            res["Hv_first_ms"] = float(np.median(first["Hv"]))        # Gram pass + H v
            res["Bsqrt_first_ms"] = float(np.median(first["Bsqrt"]))  # Gram pass + the host's root + B^(1/2) v
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--first-reps", type=int, default=2, help="timed first calls after new pairs (0: skip)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_draw_rates.py measures on the MI355X"
    m, e = a.m, 8
    line = dict(metric="qn root / draw ms per call", n=a.n, m=m, dtype="f64", reps=a.reps,
                # algorithmic bytes per row (fp64): W'z reads 2m W entries; the draw reads 2m and writes k; the
                # unfused route writes k (randn), reads 2m + k (W'V), reads 2m + k and writes k (expand)
                bytes_per_row=dict(wtz=2 * m * e, draw_k4=(2 * m + 4) * e, fused_k4=(4 * m + 4) * e,
                                   unfused_k4=(4 * m + 16) * e),
                natural=run(a.n, m, a.iters, a.reps, a.first_reps, {"compact_w": 0}),
                packed=run(a.n, m, a.iters, a.reps, a.first_reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
