"""Rates of the model along a path of shifts (lbfgsb_hip_qn_path_set / _solve / _trust) at the headline size: n = 1e8,
m = 10, fp64, the separable bounded quadratic on the device, a third of the rows pinned, in natural row order
(compact_w = 0) and on the packed tile-local layout after a bench-like warm-up (compact_w = 1).  Per layout, from ONE
process, after a warm-up call each, the median over --reps synchronised calls of: path_set; path.solve at k = 1, 8 and
64 shifts; path.solve for the scalars alone (the read pass); path.trust; and, as the yardstick of the same run, the
route before it: a loop of qn_shift(d, mu) + solve over the same 8 shifts.  The write pass's own time is taken as
solve(k) minus the read pass, and its fraction of 8 TB/s from 2col*8 + 8 + 1 + 8k bytes per row.  Each layout is
measured by a child process of its own under a time limit, and the second one starts only if the first one ended well.
Writes one JSON line to profiles/qn_path_rates.json (or --out).
usage: python profiles/scripts/qn_path_rates.py [--n N] [--iters K] [--reps R] [--out FILE] [--limit SECONDS]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(n, m, iters, reps, options):
    import numpy as np
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available(), "qn_path_rates.py measures on the MI355X"
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
        del l, u, nbd, g, x
        v = torch.randn(n, dtype=torch.float64, device="cuda")
        out1 = torch.empty(n, dtype=torch.float64, device="cuda")
        status = torch.zeros(n, dtype=torch.int8, device="cuda")
        status[::3] = 1
        d = torch.zeros(n, dtype=torch.float64, device="cuda")
        d[::3] = float("inf")
        mus = np.geomspace(1e-2, 1e2, 64)

        def timed(f):
            f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts)

        res = dict(compact_stats=list(sol.compact_stats()))
        res["path_set_ms"] = timed(lambda: sol.qn_path(status))
        path = sol.qn_path(status)
        res["pinned"] = path.pinned
        res["read_ms"] = timed(lambda: path.solve(v, mus[:8], out=False, norms=True))
        for k in (1, 8, 64):
            out = torch.empty((k, n), dtype=torch.float64, device="cuda")
            res["solve_k%d_ms" % k] = timed(lambda: path.solve(v, mus[:k], out=out))
            del out
        x0 = float(np.sqrt(path.solve(v, [0.0], out=False, norms=True)[1][0]))
        tr = path.trust(v, 0.1 * x0, out=out1)
        res["trust_iters"] = tr.iters
        res["trust_ms"] = timed(lambda: path.trust(v, 0.1 * x0, out=out1))
        res["trust_scalars_ms"] = timed(lambda: path.trust(v, 0.1 * x0, out=False))

        def before():
            for mu in mus[:8]:
                sol.qn_shift(d, float(mu)).solve(v, out1)
        res["shift_route_k8_ms"] = timed(before)
        res["read_again_ms"] = timed(lambda: path.solve(v, mus[:8], out=False, norms=True))
        res["speedup_k8"] = res["shift_route_k8_ms"] / res["solve_k8_ms"]
        e = 8
        for k in (1, 8, 64):
            ms = res["solve_k%d_ms" % k] - min(res["read_ms"], res["read_again_ms"])
            by = 2 * m * e + e + 1 + e * k
            res["expand_k%d" % k] = dict(ms=ms, bytes_per_row=by, of_8TBs=by * n / (ms * 1e-3) / 8e12)
        assert sol.compact_stats()[2] == res["compact_stats"][2]
        return res
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qn_path_rates.json"))
    ap.add_argument("--layout", default="", help="(internal) measure this layout in this process: natural | packed")
    a = ap.parse_args()
    if a.layout:
        print("RESULT " + json.dumps(run(a.n, a.m, a.iters, a.reps, {"compact_w": 1 if a.layout == "packed" else 0})))
        return 0
    m, e = a.m, 8
    line = dict(metric="qn path ms per call (medians)", n=a.n, m=m, dtype="f64",
                # algorithmic bytes per row (fp64): the read pass reads 2m W entries, v and the byte; the write pass the
                # same and writes k; path_set writes the byte from the status byte and runs ceil(2m / 4) masked W'V
                # passes whose 4 vectors are columns of W that the same trip loads anyway
                bytes_per_row=dict(read=2 * m * e + e + 1, write_k1=2 * m * e + 2 * e + 1, write_k8=2 * m * e + 9 * e + 1,
                                   write_k64=2 * m * e + 65 * e + 1, set=2 + ((2 * m + 3) // 4) * (2 * m * e + 1)))
    for layout in ("natural", "packed"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--layout", layout,
               "--n", str(a.n), "--m", str(m), "--iters", str(a.iters), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            print("qn_path_rates: the %s step ended with status %d: nothing further is started" % (layout, r.returncode))
            return 1
        line[layout] = json.loads(got[-1][len("RESULT "):])
    s = json.dumps(line)
    print(s)
    with open(a.out, "w") as f:
        f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
