"""Worker for tests/test_gpu_follow_bounds_sharded.py: `world` processes on cuda:0, one block of rows each, in a
context with LBFGSB_F_FOLLOW_BOUNDS, reductions through a gloo host group ('gloo'), the library's communicator
code path with the shared-memory RCCL stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY), or none ('single', world 1).
Runs the separable quadratic with all four bound types and edits bounds during the run -- rows that one rank
owns, and on the last rank only a new u pointer -- and writes the rows of every NEW_X return, the task sequence
and this rank's x to out_prefix.<rank>.npz.
usage: _follow_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import join, leave, quadratic_rows


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    import lbfgsb_amd
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, follow_bounds=True)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    last0 = lbfgsb_amd.block_partition(n, 3, 2)[0]   # (rows of the last rank of a 3-way split: one owner at 2 and 3)

    def edit_rows(arr, lo, hi, value):               # global rows [lo, hi) that this rank owns
        a, b = max(lo, row0), min(hi, row0 + n_loc)
        if a < b:
            arr[a - row0:b - row0] = value
    rows, tasks, done = [], [], set()
    uu = u
    for _ in range(100000):
        t = sol.setulb(x, l, uu, nbd, g, 0.0, 0.0)
        tasks.append(t[:30])
        it = int(sol.isave[29])
        key = (t[:5], it)
        if key not in done:
            done.add(key)
            if key == ("NEW_X", 3):
                edit_rows(u, 7, 71, -0.25)           # rank 0's rows
            elif key == ("NEW_X", 5) and rank == world - 1:
                uu = u.clone()                        # another pointer, on one rank only
            elif key == ("FG_LN", 7):
                edit_rows(l, last0 + 3, last0 + 50, 0.125)   # the last rank's rows
                edit_rows(nbd, last0 + 60, last0 + 90, 2)
            torch.cuda.synchronize()
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif t.startswith("NEW_X"):
            rows.append((it, int(sol.isave[33]), int(sol.isave[32]), int(sol.isave[37]), float(sol.f[0])))
            if it >= iters:
                break
        else:
            break
    leave(sol, rank, out_prefix, dict(rows=np.array(rows, np.float64), tasks=np.array(tasks), x=x.cpu().numpy(),
                                      stats=np.array(sol.bounds_stats()), row0=row0), state=False)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
