"""Rates of the model plus a diagonal (lbfgsb_hip_qn_shift_set / _solve / _diag) at the headline size: n = 1e8, m = 10,
fp64, the separable bounded quadratic on the device, in natural row order (compact_w = 0) and on the packed tile-local
layout after a bench-like warm-up (compact_w = 1).  Per layout, from ONE process: ms per call of shift_set (d random,
a third of the rows pinned), of shift_solve at k = 1 and 4 and of shift_diag, and as the yardstick of the same run
qn_apply(inverse=True) at k = 1 and 4 and qn_diag(inverse=True); then the ratios solve / H v.  Each layout is measured
by a child process of its own under a time limit, and the second one starts only if the first one ended well.  Writes
one JSON line to profiles/qn_shift_rates.json (or --out).
usage: python profiles/scripts/qn_shift_rates.py [--n N] [--iters K] [--reps R] [--out FILE] [--limit SECONDS]"""
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
    assert torch.cuda.is_available(), "qn_shift_rates.py measures on the MI355X"
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

        def timed(f):
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3

        res = dict(compact_stats=list(sol.compact_stats()))
        res["Hv_ms"] = timed(lambda: sol.qn_apply(v, out, inverse=True))
        res["Hv_k4_ms"] = timed(lambda: sol.qn_apply(v4, out4, inverse=True))
        res["diagH_ms"] = timed(lambda: sol.qn_diag(out, inverse=True))
        res["shift_set_ms"] = timed(lambda: sol.qn_shift(d, 0.3))
        sh = sol.qn_shift(d, 0.3)
        res["pinned"] = sh.pinned
        res["shift_solve_ms"] = timed(lambda: sh.solve(v, out))
        res["shift_solve_k4_ms"] = timed(lambda: sh.solve(v4, out4))
        res["shift_diag_ms"] = timed(lambda: sh.diag(out))
        # once more, interleaved, so that a drift of the box shows in the yardstick too
        res["Hv_again_ms"] = timed(lambda: sol.qn_apply(v, out, inverse=True))
        res["shift_solve_again_ms"] = timed(lambda: sh.solve(v, out))
        res["solve_over_Hv"] = min(res["shift_solve_ms"], res["shift_solve_again_ms"]) / min(res["Hv_ms"],
                                                                                            res["Hv_again_ms"])
        res["solve_over_Hv_k4"] = res["shift_solve_k4_ms"] / res["Hv_k4_ms"]
        res["diag_over_diagH"] = res["shift_diag_ms"] / res["diagH_ms"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qn_shift_rates.json"))
    ap.add_argument("--layout", default="", help="(internal) measure this layout in this process: natural | packed")
    a = ap.parse_args()
    if a.layout:
        print("RESULT " + json.dumps(run(a.n, a.m, a.iters, a.reps, {"compact_w": 1 if a.layout == "packed" else 0})))
        return 0
    m, e = a.m, 8
    line = dict(metric="qn shift ms per call", n=a.n, m=m, dtype="f64",
                # algorithmic bytes per row (fp64): the weights pass reads d and writes w; the weighted W'V reads 2m W
                # entries + k vectors + w; the weighted expansion the same and writes k; the weighted diagonal reads
                # 2m + w and writes 1; shift_set is the weights pass + ceil(2m / 4) weighted W'V passes whose 4 vectors
                # are columns of W that the same trip loads anyway (no bytes of their own)
                bytes_per_row=dict(w=2 * e, wtv_k1=(2 * m + 2) * e, wtv_k4=(2 * m + 5) * e, expand_k1=(2 * m + 3) * e,
                                   expand_k4=(2 * m + 9) * e, diag=(2 * m + 2) * e,
                                   solve_k1=(4 * m + 5) * e, Hv_k1=(4 * m + 3) * e,
                                   set=2 * e + ((2 * m + 3) // 4) * (2 * m + 1) * e))
    for layout in ("natural", "packed"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--layout", layout,
               "--n", str(a.n), "--m", str(m), "--iters", str(a.iters), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            print("qn_shift_rates: the %s step ended with status %d: nothing further is started" % (layout, r.returncode))
            return 1
        line[layout] = json.loads(got[-1][len("RESULT "):])
    s = json.dumps(line)
    print(s)
    with open(a.out, "w") as f:
        f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
