"""Worker for tests/test_gpu_qn_idx_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  The separable quadratic with all four bound types to iteration `iters`,
then the entries at index lists, called collectively with the same global list on every rank: the rows of the pairs,
the blocks of B and H (square and rectangular) and of the model plus a diagonal, and this rank's rows of the columns.
Writes them and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_idx_mr_worker.py rank world port mode n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import MU, cut, join, leave, quadratic_rows, run_to, shift


def lists(n, world):
    """the global list: the rows on both sides of every cut, the first and the last row, ten random rows, one row
    repeated -- unsorted; and a second list for the rectangular blocks"""
    rng = np.random.default_rng(41)
    edges = [cut(n, world, r)[0] for r in range(1, world)]
    ia = [n - 1] + [e + k for e in edges for k in (0, -1, 1, -2)] + [0] + [int(i) for i in rng.choice(n, 10, False)]
    ia.append(ia[3])
    ib = [int(i) for i in rng.choice(n, 6, False)] + [e - 1 for e in edges] + [e for e in edges]
    return np.array(ia, np.int64), np.array(ib, np.int64)


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, partition=cut)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    d = torch.from_numpy(shift(n, world)[row0:row0 + n_loc].copy()).to(dev)
    ia, ib = lists(n, world)

    run_to(sol, x, l, u, nbd, g, iters)
    res = dict(rows=sol.qn_rows(ia))
    for inv, tag in ((False, "b"), (True, "h")):
        res[tag + "_sq"] = sol.qn_block(ia, inverse=inv)
        res[tag + "_rect"] = sol.qn_block(ia, ib, inverse=inv)
        res[tag + "_cols"] = sol.qn_cols(ia, inverse=inv).cpu().numpy()
    sh = sol.qn_shift(d, MU)
    res.update(s_sq=sh.block(ia), s_rect=sh.block(ia, ib), s_cols=sh.columns(ia).cpu().numpy())
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
