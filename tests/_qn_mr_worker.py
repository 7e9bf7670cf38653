"""Worker for tests/test_gpu_qn_sharded.py: `world` processes on cuda:0, one block of rows each, reductions through
a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  Runs the separable quadratic with all four bound types to iteration `iters`,
then calls the curvature-model operator collectively (B V, H V for 3 vectors, diag(B), diag(H)) and writes this
rank's rows of the results, of the exported Ws / Wy and the model's scalars to out_prefix.<rank>.npz.
usage: _qn_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import join, leave, quadratic_rows, run_to


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    run_to(sol, x, l, u, nbd, g, iters)
    V = np.random.default_rng(17).standard_normal((3, n))          # the same global vectors on every rank
    vt = torch.from_numpy(V[:, row0:row0 + n_loc].copy()).to(dev)
    res = dict(bv=sol.qn_apply(vt).cpu().numpy(), hv=sol.qn_apply(vt, inverse=True).cpu().numpy(),
               h1=sol.qn_apply(vt[1].contiguous(), inverse=True).cpu().numpy())
    col = int(sol.isave[27])
    if col <= 32:
        res.update(db=sol.qn_diag().cpu().numpy(), dh=sol.qn_diag(inverse=True).cpu().numpy())
    wa, _ = sol.export_state()
    res.update(ws=wa[:m * n_loc].reshape(m, n_loc), wy=wa[m * n_loc:2 * m * n_loc].reshape(m, n_loc),
               head=int(sol.isave[26]), col=col, theta=float(sol.dsave[0]), row0=row0, V=V)
    leave(sol, rank, out_prefix, res, state=False)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
