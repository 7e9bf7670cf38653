"""Rates of the active-set report (lbfgsb_hip_kkt / lbfgsb_hip_kkt_list) at the headline size, n = 1e8, fp64, against
lbfgsb_hip_projgr -- the pass that reads the same 36 bytes per row -- in ONE process, the calls alternating, each
timed with a pair of hipEvents on the context's stream (kernel + fixed-order finalize + the copy of the summary).
The report is timed with no per-row output, with each output alone and with all three (36 / 44 / 44 / 37 / 53 bytes
per row); the list at selections of 1 %, 50 % and 100 % (1 byte read per row in each of the two passes over the
status bytes, 8 bytes written per selected row).  Prints one JSON line: the median ms of each, its share of 8 TB/s on
those bytes, and the ratios the target of DESIGN.md section 12 is stated in.
usage: python profiles/scripts/kkt_rates.py [--n N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lbfgsb_amd  # noqa: E402

PEAK = 8.0e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kkt_rates.py measures on the MI355X"
    n = a.n
    sol = lbfgsb_amd.DeviceSolver(n, 1)
    try:
        gen = torch.Generator(device="cuda").manual_seed(11)
        l = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        u = torch.full((n,), 1.0, dtype=torch.float64, device="cuda")
        x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 3.0 - 1.5
        x.clamp_(-1.0, 1.0)  # a third of the rows at a bound
        g = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        nbd = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda", generator=gen)
        pg, mult = torch.empty_like(x), torch.empty_like(x)
        status = torch.empty(n, dtype=torch.int8, device="cuda")
        idx = torch.empty(n, dtype=torch.int64, device="cuda")
        r = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen)
        sel = {"1pct": (r < 0.01).to(torch.int8), "50pct": (r < 0.5).to(torch.int8),
               "100pct": torch.ones(n, dtype=torch.int8, device="cuda")}
        del r
        torch.cuda.synchronize()
        stream = torch.cuda.ExternalStream(sol.stream)
        lib, h = sol.lib, sol.h
        cnt, val, count, sbg = np.zeros(9, np.int64), np.zeros(4), np.zeros(1, np.int64), np.zeros(1)
        P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        A = lambda v: v.ctypes.data  # noqa: E731

        def kkt(o_pg, o_mu, o_st):
            return lambda: lib.lbfgsb_hip_kkt(h, P(x), P(l), P(u), P(nbd), P(g), 1e-5, P(o_pg), P(o_mu), P(o_st),
                                              A(cnt), A(val))

        calls = {
            "projgr": (lambda: lib.lbfgsb_hip_projgr(h, P(x), P(l), P(u), P(nbd), P(g), A(sbg)), 36.0),
            "kkt_none": (kkt(None, None, None), 36.0),
            "kkt_pg": (kkt(pg, None, None), 44.0),
            "kkt_mult": (kkt(None, mult, None), 44.0),
            "kkt_status": (kkt(None, None, status), 37.0),
            "kkt_all": (kkt(pg, mult, status), 53.0),
        }
        for k, s in sel.items():
            frac = {"1pct": 0.01, "50pct": 0.5, "100pct": 1.0}[k]
            calls["list_" + k] = ((lambda s=s: lib.lbfgsb_hip_kkt_list(h, P(s), 0b00100, P(idx), n, A(count))),
                                  2.0 + 8.0 * frac)
        times = {k: [] for k in calls}
        for rep in range(a.reps + 2):
            for k, (f, _) in calls.items():  # alternating: one call of each per round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = f()
                e1.record(stream)
                e1.synchronize()
                assert rc == 0, (k, rc)
                if rep >= 2:  # (two warm-up rounds)
                    times[k].append(e0.elapsed_time(e1))
        assert val[0] == sbg[0], (val[0], sbg[0])  # the same number as projgr's
        res = {}
        for k, (_, b) in calls.items():
            ms = float(np.median(times[k]))
            res[k] = dict(ms=round(ms, 4), min_ms=round(float(np.min(times[k])), 4), bytes_per_row=b,
                          share_of_8TBs=round(b * n / (ms * 1e-3) / PEAK, 3))
        base, none = res["projgr"]["ms"], res["kkt_none"]["ms"]
        ratios = dict(kkt_none_over_projgr=round(none / base, 3))
        for k, extra in (("kkt_pg", 8.0), ("kkt_mult", 8.0), ("kkt_status", 1.0), ("kkt_all", 17.0)):
            # what the output costs against its bytes at the no-output rate (target: <= 1)
            ratios[k + "_extra_over_bytes"] = round((res[k]["ms"] - none) / (none * extra / 36.0), 3)
        line = dict(metric="kkt report ms per call", n=n, dtype="f64", reps=a.reps, calls=res, ratios=ratios,
                    counts=cnt.tolist())
    finally:
        sol.close()
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
