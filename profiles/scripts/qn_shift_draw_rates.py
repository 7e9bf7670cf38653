"""Rates of the draws of the model plus a diagonal (lbfgsb_hip_qn_shift_sqrt / _draw / _draw_logpdf / _quad) at the
headline size: n = 1e8, m = 10, fp64, the separable bounded quadratic on the device, a third of the rows pinned, in
natural row order (compact_w = 0) and on the packed tile-local layout after a bench-like warm-up (compact_w = 1).  Per
layout, from ONE process: ms per call of QnShifted.sample at k = 1 and 4 against the unfused route of the same process,
torch.randn(k, n) plus QnShifted.sqrt; of sqrt against shift_solve at the same k (the same kernels and bytes); and of
sample with log_prob, quad and log_prob at k = 4.  Targets: fused <= unfused, sqrt <= 1.05 x shift_solve.  Every pair
is timed twice, interleaved, and the ratio taken of the two minima, so that a drift of the box shows in both.  Each
layout is measured by a child process of its own under a time limit, and the second one starts only if the first one
ended well.  Writes one JSON line to profiles/qn_shift_draw_rates.json (or --out).
usage: python profiles/scripts/qn_shift_draw_rates.py [--n N] [--iters K] [--reps R] [--out FILE] [--limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(n, m, iters, reps, options):
    import numpy as np
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "qn_shift_draw_rates.py measures on the MI355X"
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
        del l, u, nbd, g
        v = torch.randn(n, dtype=torch.float64, device="cuda")
        v4 = torch.randn(4, n, dtype=torch.float64, device="cuda")
        out, out4 = torch.empty_like(v), torch.empty_like(v4)
        d = 10.0 * torch.rand(n, dtype=torch.float64, device="cuda")
        d[::3] = float("inf")
        sh = sol.qn_shift(d, 0.3)

        def timed(f):
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3

        def unfused(z, o):
            torch.randn(z.shape, dtype=torch.float64, device="cuda", out=z)
            sh.sqrt(z, o)

        res = dict(compact_stats=list(sol.compact_stats()), pinned=sh.pinned)
        pairs = dict(
            sample_k1=(lambda: sh.sample(1, 7, out=out), lambda: unfused(v, out)),
            sample_k4=(lambda: sh.sample(4, 7, out=out4), lambda: unfused(v4, out4)),
            sqrt_k1=(lambda: sh.sqrt(v, out), lambda: sh.solve(v, out)),
            sqrt_k4=(lambda: sh.sqrt(v4, out4), lambda: sh.solve(v4, out4)))
        for name, (new, ref) in pairs.items():
            a = [timed(new), timed(ref), timed(new), timed(ref)]
            res[name + "_ms"], res[name + "_ref_ms"] = min(a[0], a[2]), min(a[1], a[3])
            res[name + "_all_ms"] = a
            res[name + "_ratio"] = res[name + "_ms"] / res[name + "_ref_ms"]
        res["sample_logp_k4_ms"] = timed(lambda: sh.sample(4, 7, out=out4, log_prob=True))
        res["quad_k4_ms"] = timed(lambda: sh.quad(out4))
        res["log_prob_k4_ms"] = timed(lambda: sh.log_prob(out4))
        assert sol.compact_stats()[2] == res["compact_stats"][2]
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qn_shift_draw_rates.json"))
    ap.add_argument("--layout", default="", help="(internal) measure this layout in this process: natural | packed")
    a = ap.parse_args()
    if a.layout:
        print("RESULT " + json.dumps(run(a.n, a.m, a.iters, a.reps, {"compact_w": 1 if a.layout == "packed" else 0})))
        return 0
    m, e = a.m, 8
    line = dict(metric="qn shift draw ms per call", n=a.n, m=m, dtype="f64",
                targets=dict(sample_ratio="<= 1 (fused / unfused)", sqrt_ratio="<= 1.05 (sqrt / shift_solve)"),
                # algorithmic bytes per row (fp64): the weighted W'z pass reads 2m W entries + w; the draw's expansion
                # the same and writes k; the unfused route writes and reads z twice more (randn, W'v, expansion); the
                # quadratic form reads 2m + w + k vectors and writes nothing
                bytes_per_row=dict(wtz=(2 * m + 1) * e, draw_k1=(4 * m + 3) * e, draw_k4=(4 * m + 6) * e,
                                   unfused_k1=(4 * m + 6) * e, unfused_k4=(4 * m + 18) * e,
                                   sqrt_k1=(4 * m + 5) * e, quad_k4=(2 * m + 5) * e))
    for layout in ("natural", "packed"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--layout", layout,
               "--n", str(a.n), "--m", str(m), "--iters", str(a.iters), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            print("qn_shift_draw_rates: the %s step ended with status %d: nothing further is started"
                  % (layout, r.returncode))
            return 1
        line[layout] = json.loads(got[-1][len("RESULT "):])
    s = json.dumps(line)
    print(s)
    with open(a.out, "w") as f:
        f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
