"""Worker for tests/test_gpu_qn_path_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  The separable quadratic with all four bound types to iteration `iters`,
then the model over a range of shifts, called collectively under two masks: every third row and a run of 40 rows
across every rank boundary pinned ("cross"), and every row of rank 1 pinned with every third row elsewhere
("rank1").  Per mask: the pinned count, the log det curve, the solves at the shifts with their norms, a trust step.
Writes them and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_path_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import SEED, cut, join, leave, quadratic_rows, run_to, shift

MUS = [0.01, 0.0, 0.3, 5.0, 300.0]
MASKS = ("cross", "rank1")
TRUTH_AT = (2,)   # the shifts (indices into MUS) that the test also holds to the dense truth


def pins(n, world, mask):
    """the global pinned rows of a mask"""
    pin = np.isinf(shift(n, world))
    if mask == "rank1":
        pin = np.zeros(n, bool)
        pin[::3] = True
        r0, nl = cut(n, world, 1)
        pin[r0:r0 + nl] = True
    return pin


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, partition=cut)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    sl = slice(row0, row0 + n_loc)
    v = torch.from_numpy(np.random.default_rng(SEED).standard_normal(n)[sl].copy()).to(dev)
    res = {}
    run_to(sol, x, l, u, nbd, g, iters)
    for mask in MASKS:
        status = torch.from_numpy(np.where(pins(n, world, mask)[sl], 2, 0).astype(np.int8)).to(dev)
        path = sol.qn_path(status)
        ld, info = path.logdet(MUS)
        out, n2, vx = path.solve(v, MUS, norms=True)
        tr = path.trust(v, 0.05 * float(np.sqrt(n2[1])))
        res.update({mask + "_pinned": np.int64(path.pinned), mask + "_logdet": ld, mask + "_info": info,
                    mask + "_x": out.cpu().numpy(), mask + "_n2": n2, mask + "_vx": vx,
                    mask + "_step": tr.step.cpu().numpy(),
                    mask + "_trust": np.array([tr.mu, tr.norm, tr.predicted, float(tr.on_boundary), tr.iters])})
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
