"""Rates of the pairs in and out (lbfgsb_hip_qn_pairs_get / _set / _push) at the headline size: n = 1e8, m = 10, fp64,
the separable bounded quadratic on the device run until the ring is full.  One process, per entry a warm-up call and
the median of 7 timed calls (wall clock around a synchronised call): pairs_get, pairs_set, one accepted push followed
by H v, and, for comparison, the only route without these entries, export_state + import_state through host memory.
Prints one JSON line with the ms per call, the algorithmic bytes per row and the fraction of 8 TB/s.
usage: python profiles/scripts/qn_pairs_rates.py [--n N] [--m M] [--reps R] [--no-export] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402

PEAK = 8.0e12


def timed(f, reps, before=None):
    out = []
    for i in range(reps + 1):  # (the first call is the warm-up)
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if i:
            out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-export", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qn_pairs_rates.py measures on the MI355X"
    n, m, e = a.n, a.m, 8
    sol, model = lbfgsb_amd.DeviceSolver(n, m), lbfgsb_amd.DeviceSolver(n, m)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.from_numpy((np.arange(1, n + 1) % 4).astype(np.int32)).cuda()
        for _ in range(200):
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif not t.startswith("NEW_X") or sol.isave[29] >= m + 6:
                break
        assert t.startswith("NEW_X") and int(sol.isave[27]) == m, t
        S = torch.empty((m, n), dtype=torch.float64, device="cuda")
        Y = torch.empty_like(S)
        res = {}
        res["pairs_get"] = timed(lambda: sol.qn_pairs(out=(S, Y)), a.reps)
        theta = sol.qn_pairs(out=(S, Y))[2]
        res["pairs_set"] = timed(lambda: model.qn_set_pairs(S, Y, theta=theta), a.reps)
        # one accepted push, then H v: the model is reloaded (untimed) in front of each so that every push meets the
        # same full ring
        s1 = 1.0 / (1.0 + (torch.arange(1, n + 1, device="cuda") % 7).to(torch.float64))
        y1 = 2.0 * s1
        v, out = torch.randn(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")

        def push_hv():
            assert model.qn_push_pair(s1, y1) == 1
            model.qn_apply(v, out, inverse=True)
        res["push_then_Hv"] = timed(push_hv, a.reps, before=lambda: model.qn_set_pairs(S, Y, theta=theta))
        model.qn_set_pairs(S, Y, theta=theta)
        res["push"] = timed(lambda: model.qn_push_pair(s1, y1), a.reps)
        res["Hv"] = timed(lambda: model.qn_apply(v, out, inverse=True), a.reps)
        if not a.no_export:
            isave = sol.isave.copy()

            def roundtrip():
                wa, iwa = sol.export_state()
                model.import_state(wa, iwa, isave)
            res["export_import"] = timed(roundtrip, a.reps)
        rows = dict(pairs_get=2 * m * 2 * e, pairs_set=2 * m * 2 * e, push=(2 * m + 2) * e + 4 * e,
                    export_import=2 * (2 * m + 5) * e)
        # (set: the copy alone; its Gram pass reads the 2m columns 2m / 4 times more, (2m + 4) 8 B per row each)
        rows["pairs_set_with_gram"] = rows["pairs_set"] + ((2 * m + 3) // 4) * (2 * m + 4) * e
        for key, b in rows.items():
            if key.split("_with")[0] in res:
                r = res[key.split("_with")[0]]
                r.setdefault("bytes_per_row", {})[key] = b
                r.setdefault("fraction_of_peak", {})[key] = b * n / (r["ms"] * 1e-3) / PEAK
        line = dict(metric="qn pairs ms per call", n=n, m=m, dtype="f64", peak_bytes_per_s=PEAK, reps=a.reps, **res)
    finally:
        sol.close(), model.close()
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
