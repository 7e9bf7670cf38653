"""Worker for tests/test_gpu_qn_gram_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly), reductions
through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  The Gram matrix of K vectors around a center at the FG_START return (no pair
yet), then the separable quadratic with all four bound types to iteration `iters` and the matrices of both modes,
called collectively.  Writes the matrices and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_gram_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import cut, join, leave, quadratic_rows, run_to

K, SEED = 5, 23


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, partition=cut)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    sl = slice(row0, row0 + n_loc)
    rng = np.random.default_rng(SEED)                               # the same global vectors on every rank
    cen = torch.from_numpy(rng.standard_normal(n)[sl].copy()).to(dev)
    V = torch.from_numpy(rng.standard_normal((K, n))[:, sl].copy()).to(dev)

    res = {}
    run_to(sol, x, l, u, nbd, g, iters, on_start=lambda: res.update(g0=sol.qn_gram(V, center=cen)))
    res.update(gb=sol.qn_gram(V, center=cen), gh=sol.qn_gram(V, center=cen, inverse=True),
               gn=sol.qn_gram(V, inverse=True))
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
