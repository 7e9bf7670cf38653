"""Worker for tests/test_gpu_qn_root_sharded.py: `world` processes on cuda:0, one block of rows each, reductions
through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  Draws at the FG_START return (no pair yet), runs the separable quadratic with all
four bound types to iteration `iters`, then calls the new entries of the curvature model collectively (log det B,
log det H, 5 draws from sample 3 with a mean and scale 0.5 for both covariances, H^(1/2) V) and writes this rank's
rows of the results and its exported state to out_prefix.<rank>.npz.
usage: _qn_root_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import join, leave, quadratic_rows, run_to

SEED, K, FIRST, SCALE = 2 ** 40 + 12345, 5, 3, 0.5


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    sl = slice(row0, row0 + n_loc)
    rng = np.random.default_rng(17)                                 # the same global vectors on every rank
    mean = torch.from_numpy(rng.standard_normal(n)[sl].copy()).to(dev)
    V = torch.from_numpy(rng.standard_normal((3, n))[:, sl].copy()).to(dev)
    res = {}
    run_to(sol, x, l, u, nbd, g, iters, on_start=lambda: res.update(
        d0=sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE).cpu().numpy(), ld0=sol.qn_logdet()))
    res.update(ldb=sol.qn_logdet(), ldh=sol.qn_logdet(inverse=True),
               db=sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=False).cpu().numpy(),
               dh=sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=True).cpu().numpy(),
               rh=sol.qn_apply(V, sqrt=True, inverse=True).cpu().numpy())
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
