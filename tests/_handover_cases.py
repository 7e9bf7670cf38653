"""Constructed inputs for the breakpoint hand-over of the update pass (option spec_capture = 1: update_scan_kernel
appends every row whose breakpoint lies in [0, cand_hi] to a list, and the next Cauchy walk takes that list for every
breakpoint up to cand_hi -- solver_provider.inl: spec_queue / spec_land / the first branch of window_fetch).

The STAIRCASE problem: a separable quadratic f = 1/2 sum a_i (x_i - c_i)^2 from x0 = 0 with factr = pgtol = 0, curvatures
over four decades, every minimiser c_i beyond ONE bound of its row, which sits at a random fraction fr_i of the way.
The walk therefore fixes one to a few of the bounded rows per iteration, for dozens of iterations -- short walks behind
an update pass, which is what the hand-over serves.  WHICH rows carry bounds is the case's choice: the last n % 128
rows (of every rank), so that a list that misses the rows behind the last whole layout tile misses every breakpoint.

tests/test_handover_cases_cpu.py pins, from the oracle alone, that the walks of every case do cross breakpoints in the
chosen rows; tests/test_gpu_handover.py and tests/test_gpu_multirank.py run the cases on the device.
"""
import numpy as np

ITERS = 40


def block_rows(n, world, rank):
    """(row0, n_local) of lbfgsb_amd.block_partition"""
    base, rem = divmod(n, world)
    return rank * base + min(rank, rem), base + (1 if rank < rem else 0)


class Case:
    def __init__(self, name, n, m, seed, served, served7, first=None, world=1):
        self.name, self.n, self.m, self.seed, self.world = name, n, m, seed, world
        # walks that a CPU model of the host's rule (chi = factor * last tsum once three walks have been seen, a walk
        # is served if 1.25 dtm <= chi and at most 128 rows have t <= chi) predicts to be served in ITERS iterations,
        # and how many of them with col >= 7: the floor of the CPU test for iterations whose walk crosses breakpoints
        self.served, self.served7 = served, served7
        bounded = np.zeros(n, bool)
        self.tile0 = np.zeros(n, np.int64)      # per row: first row behind the last whole tile of its rank
        for r in range(world):
            row0, nl = block_rows(n, world, r)
            t0 = row0 + (nl // 128 * 128 if first is None else first)
            bounded[t0:row0 + nl] = True
            self.tile0[row0:row0 + nl] = row0 + nl // 128 * 128
        self.bounded = bounded
        self.whole_tiles = world == 1 and n % 128 == 0
        self.tail = first is None               # the bounded rows are exactly those behind the last whole tile

    def arrays(self):
        rng = np.random.default_rng(self.seed)
        n = self.n
        a = 10 ** (4.0 * rng.random(n))
        c = rng.choice([-1., 1.], n) * (1. + rng.random(n))
        fr = 0.05 + 0.9 * rng.random(n)
        l = np.where(c < 0, fr * c, -10.)
        u = np.where(c > 0, fr * c, 10.)
        nbd = np.where(self.bounded, 2, 0).astype(np.int32)
        return a, c, l, u, nbd

    def problem(self, po):
        """-> (pyoracle.Problem, fg(x, g, lo, hi) on a block of rows)"""
        a, c, l, u, nbd = self.arrays()
        n = self.n

        def fg(x, g, lo=0, hi=None):
            hi = n if hi is None else hi
            d = x - c[lo:hi]
            g[:] = a[lo:hi] * d
            return float(0.5 * np.sum(a[lo:hi] * d * d))
        return po.Problem("stair_" + self.name, n, self.m, np.zeros(n), l, u, nbd, 0.0, 0.0, fg, np.float64), fg


# name, n, m, seed, served, of those at col >= 7, first bounded row (None: behind the last whole tile)
CASES = [Case("n255_m10", 255, 10, 2, 9, 7),
         Case("n255_m7", 255, 7, 1, 9, 7),
         Case("n383_m10", 383, 10, 2, 8, 6),
         Case("n256_m10", 256, 10, 7, 7, 6, first=128),    # whole tiles: the pair-shared instantiation itself hands over
         Case("n384_m10", 384, 10, 1, 7, 5, first=256),    # whole tiles
         Case("n255_m3", 255, 3, 2, 5, 0),                 # MC = 5
         Case("n1000_m20", 1000, 20, 2, 15, 0, first=500),
         Case("n510_w2", 510, 10, 2, 10, 0, world=2),
         Case("n700_w3", 700, 10, 2, 11, 0, world=3)]
BY_NAME = {c.name: c for c in CASES}
SINGLE = [c for c in CASES if c.world == 1]


def oracle_walks(po, case, iters=ITERS):
    """The oracle's run of the case -> one record per iteration whose walk ran behind an update pass (iteration >= 2):
    (iteration, col in effect during the walk, nseg, rows whose iwhere went 0 -> 1 / 2 across the call of the walk)"""
    p, _ = case.problem(po)
    n = p.n
    out, last = [], {}

    def snap(k, s):
        iw = s.iwa[n:2 * n].copy()
        if last.get("new_x") and s.task_s.startswith("FG_LN"):     # the call behind a NEW_X return ran the walk
            rows = np.nonzero((last["iw"] == 0) & ((iw == 1) | (iw == 2)))[0]
            out.append((last["iter"] + 1, int(s.isave[27]), int(s.isave[32]), rows))   # (matupd ran in this call too)
        last.update(new_x=s.task_s.startswith("NEW_X"), iw=iw, iter=int(s.isave[29]))
    po.run(po.Engine("oracle"), p, max_iter=iters, snapshot=snap)
    return out
