"""Rates of the entries at index lists (lbfgsb_hip_qn_block / qn_shift_block / qn_cols) at the headline size:
n = 1e8, m = 10, fp64, the separable bounded quadratic on the device, in natural row order (compact_w = 0) and on the
packed tile-local layout after a bench-like warm-up (compact_w = 1).  The routes are called in turn in one process,
each call between two events on the context's stream; the medians of `reps` rounds, with min and max, go into one
JSON line:
  qn_block (H) and qn_shift_block at 64 and 1024 random indices: one gather each, no pass over W;
  qn_cols (H) at 1, 16 and 128 indices: the gather and one pass over W that writes all the columns;
  what the same answers cost without index lists: qn_gram on 64 unit vectors (51 GB of them at n = 1e8) for the
  64 x 64 block, qn_apply on 1 and on 16 unit vectors for the columns (128 of them would be 8 such calls: the unit
  vectors and the outputs of 128 do not fit beside each other).
The two routes must agree: the block to 1e-12 of its largest entry, the columns to 1e-12 in the relative 2-norm.
usage: python profiles/scripts/qn_idx_rates.py [--n N] [--iters K] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402

KCOLS = (1, 16, 128)
KBLOCK = (64, 1024)


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
        rng = np.random.default_rng(11)
        idx = {k: np.sort(rng.choice(n, k, replace=False)).astype(np.int64) for k in set(KCOLS) | set(KBLOCK)}
        stream = torch.cuda.ExternalStream(sol.stream)  # every route below runs on the context's stream
        with torch.cuda.stream(stream):
            d = 10.0 * torch.rand(n, dtype=torch.float64, device="cuda")
            d[::3] = float("inf")
            sh = sol.qn_shift(d, 0.3)
            del d, l, u, nbd, g, x
            big = torch.zeros((max(KCOLS), n), dtype=torch.float64, device="cuda")  # columns, or unit vectors

            def units(k, rows):
                big[:k].zero_()
                big[torch.arange(k, device="cuda"), torch.from_numpy(rows).cuda()] = 1.0

            # the same answers by both routes, then the old routes' times (they need the unit vectors in `big`)
            times = {}

            def clock(name, f):
                f()  # warm-up of the shape (code objects, the cached Gram of the pairs)
                stream.synchronize()
                ts = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f()
                    e1.record(stream)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                times[name] = ts

            res = dict(compact_stats=list(sol.compact_stats()))
            units(64, idx[64])
            gram = sol.qn_gram(big[:64], inverse=True)
            block = sol.qn_block(idx[64], inverse=True)
            res["block_vs_gram_unit_k64"] = float(np.abs(block - gram).max() / np.abs(gram).max())
            assert res["block_vs_gram_unit_k64"] <= 1e-12, res
            clock("gram_unit_k64", lambda: sol.qn_gram(big[:64], inverse=True))
            for k in (1, 16):
                units(k, idx[k])
                ref = sol.qn_apply(big[:k], big[16:16 + k], inverse=True)
                cols = sol.qn_cols(idx[k], big[32:32 + k], inverse=True)
                res["cols_vs_apply_unit_k%d" % k] = float((torch.linalg.norm(cols - ref) / torch.linalg.norm(ref)).item())
                assert res["cols_vs_apply_unit_k%d" % k] <= 1e-12, res
                clock("apply_unit_k%d" % k, lambda k=k: sol.qn_apply(big[:k], big[16:16 + k], inverse=True))
            for k in KBLOCK:
                clock("block_k%d" % k, lambda k=k: sol.qn_block(idx[k], inverse=True))
                clock("shift_block_k%d" % k, lambda k=k: sh.block(idx[k]))
            for k in KCOLS:
                clock("cols_k%d" % k, lambda k=k: sol.qn_cols(idx[k], big[:k], inverse=True))
            clock("shift_cols_k16", lambda: sh.columns(idx[16], big[:16]))
            assert list(sol.compact_stats()) == res["compact_stats"]  # (the layout as it was)
            for name, ts in times.items():
                res[name + "_ms"] = float(np.median(ts))
                res[name + "_minmax_ms"] = [float(min(ts)), float(max(ts))]
            res["gram_unit_over_block_k64"] = res["gram_unit_k64_ms"] / res["block_k64_ms"]
            for k in (1, 16):
                res["apply_unit_over_cols_k%d" % k] = res["apply_unit_k%d_ms" % k] / res["cols_k%d_ms" % k]
            res["apply_unit_8x_k16_over_cols_k128"] = 8.0 * res["apply_unit_k16_ms"] / res["cols_k128_ms"]
            for k in KCOLS:  # the columns pass against its algorithmic bytes: 2 m reals read, k written per row
                res["cols_k%d_TBs" % k] = (2 * m + k) * 8.0 * n / (res["cols_k%d_ms" % k] * 1e-3) / 1e12
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_idx_rates.py measures on the MI355X"
    m, e = a.m, 8
    line = dict(metric="qn entries at index lists, ms per call", n=a.n, m=m, dtype="f64", reps=a.reps,
                device=torch.cuda.get_device_name(0),
                gather_bytes={"block_k%d" % k: k * 2 * m * e for k in KBLOCK},
                bytes_per_row={"cols_k%d" % k: (2 * m + k) * e for k in KCOLS}
                | {"apply_unit_k%d" % k: -(-k // 4) * ((2 * m + 4) * e + (2 * m + 8) * e) for k in (1, 16)}
                | {"gram_unit_k64": 16 * (2 * m + 4) * e + 120 * 8 * e},
                natural=run(a.n, m, a.iters, a.reps, {"compact_w": 0}),
                packed=run(a.n, m, a.iters, a.reps, {"compact_w": 1}))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
