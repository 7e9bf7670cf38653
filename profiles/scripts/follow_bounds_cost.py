"""Cost of LBFGSB_F_FOLLOW_BOUNDS without edits at the headline size: n = 1e8, m = 10, fp64, the separable bounded
quadratic on the device, with uniform bounds (l, u, nbd read as constants: the comparison streams 20 bytes per row)
and with plain bounds (l with n distinct values: 37 bytes per row).  Runs of the flag off and on alternate on one
device, `--pairs` pairs per variant; each run warms up to iteration `--warm` and times the iterations up to
`--iters` (ms per iteration from NEW_X to NEW_X; comparison passes per iteration from bounds_stats).  The kernel's
own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line.  usage: python profiles/scripts/follow_bounds_cost.py [--n N] [--pairs P] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402


def run(n, m, follow, plain, warm, iters):
    sol = lbfgsb_amd.DeviceSolver(n, m, follow_bounds=follow)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        if plain:
            l -= torch.arange(n, dtype=torch.float64, device="cuda") / n
        nbd = torch.full((n,), 2, dtype=torch.int32, device="cuda")
        t0, it0, st0 = None, 0, (0, 0, 0)
        for _ in range(100 * iters):
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif t.startswith("NEW_X"):
                it = int(sol.isave[29])
                if it == warm:
                    torch.cuda.synchronize()
                    t0, it0, st0 = time.perf_counter(), it, sol.bounds_stats()
                if it >= iters:
                    break
            else:
                break
        assert t.startswith("NEW_X") and t0 is not None, t
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / (int(sol.isave[29]) - it0) * 1e3
        st = sol.bounds_stats()
        entries = (st[0] - st0[0]) / (int(sol.isave[29]) - it0)
        mask = sol.uniform_bounds()
        return dict(ms_per_iter=ms, entries_per_iter=entries, mask=mask)
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--iters", type=int, default=14)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "follow_bounds_cost.py measures on the MI355X"
    res = dict(metric="LBFGSB_F_FOLLOW_BOUNDS cost, no edits, ms per iteration", n=a.n, m=a.m, dtype="f64",
               bytes_per_row=dict(uniform=20, dictionary=21, plain=37))
    for name, plain in (("uniform", False), ("plain", True)):
        off, on, ent = [], [], []
        for _ in range(a.pairs):
            r0 = run(a.n, a.m, False, plain, a.warm, a.iters)
            r1 = run(a.n, a.m, True, plain, a.warm, a.iters)
            off.append(r0["ms_per_iter"])
            on.append(r1["ms_per_iter"])
            ent.append(r1["entries_per_iter"])
        res[name] = dict(flag_off_ms=off, flag_on_ms=on, entries_per_iter=float(np.mean(ent)),
                         mask=r1["mask"], overhead_ms=float(np.median(on) - np.median(off)))
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
