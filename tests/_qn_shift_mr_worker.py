"""Worker for tests/test_gpu_qn_shift_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  The model plus a diagonal at the FG_START return (no pair yet), then the
separable quadratic with all four bound types to iteration `iters` and the shift again, called collectively: the
solves of K vectors, the diagonal, the log det and the pinned count.  Writes them and this rank's exported state to
out_prefix.<rank>.npz.
usage: _qn_shift_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import MU, SEED, cut, join, leave, quadratic_rows, run_to, shift

K = 5


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, partition=cut)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    sl = slice(row0, row0 + n_loc)
    rng = np.random.default_rng(SEED)                               # the same global vectors on every rank
    V = torch.from_numpy(rng.standard_normal((K, n))[:, sl].copy()).to(dev)
    d = torch.from_numpy(shift(n, world)[sl].copy()).to(dev)

    def shifted(tag):
        sh = sol.qn_shift(d, MU)
        return {tag + "_x": sh.solve(V).cpu().numpy(), tag + "_diag": sh.diag().cpu().numpy(),
                tag + "_logdet": np.float64(sh.logdet()), tag + "_pinned": np.int64(sh.pinned)}

    res = {}
    run_to(sol, x, l, u, nbd, g, iters, on_start=lambda: res.update(shifted("s0")))
    res.update(shifted("s1"))
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
