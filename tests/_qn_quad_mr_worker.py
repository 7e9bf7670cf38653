"""Worker for tests/test_gpu_qn_quad_sharded.py: `world` processes on cuda:0, one block of rows each, reductions
through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  Quadratic forms and draw densities at the FG_START return (no pair yet), then the
separable quadratic with all four bound types to iteration `iters` and the entries called collectively: qn_quad of
both modes and qn_logpdf of both covariances at 3 vectors around a mean, 5 draws from sample 3 with their
log-densities for both covariances.  Writes the numbers, this rank's rows of the draws and its exported state to
out_prefix.<rank>.npz.
usage: _qn_quad_mr_worker.py rank world port mode n m iters out_prefix"""
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

    def draws(inverse):
        d, lp = sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=inverse, return_logpdf=True)
        assert torch.equal(d, sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=inverse))
        return d.cpu().numpy(), lp

    res = {}

    def at_start():
        d0, lp0 = draws(True)
        res.update(d0=d0, lp0=lp0, q0=sol.qn_quad(V, center=mean))
    run_to(sol, x, l, u, nbd, g, iters, on_start=at_start)
    db, lpdb = draws(False)
    dh, lpdh = draws(True)
    res.update(qb=sol.qn_quad(V, center=mean), qh=sol.qn_quad(V, center=mean, inverse=True),
               lpb=sol.qn_logpdf(V, mean=mean, scale=SCALE, inverse=False),
               lph=sol.qn_logpdf(V, mean=mean, scale=SCALE, inverse=True),
               db=db, dh=dh, lpdb=lpdb, lpdh=lpdh, ldb=sol.qn_logdet(), ldh=sol.qn_logdet(inverse=True))
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
