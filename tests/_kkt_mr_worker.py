"""Worker for tests/test_gpu_kkt_sharded.py: `world` processes on cuda:0, one block of rows each, reductions through
a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  Loads the global x, l, u, nbd, g the test wrote, calls the active-set report
collectively on this rank's rows (no run is needed) and the ordered list per rank, and writes the summary, this
rank's per-row outputs and its lists to out_prefix.<rank>.npz.
usage: _kkt_mr_worker.py rank world port mode case.npz tol out_prefix"""
import sys

import numpy as np

from _mr_common import join, leave

MASKS = (0b01100, 0b00011, 0b10000, 31)


def run(rank, world, port, mode, case, tol, out_prefix):
    import torch

    data = np.load(case)
    sol, row0, n_loc, dev = join(rank, world, port, mode, data["x"].size, 3)
    sl = slice(row0, row0 + n_loc)
    x, l, u, nbd, g = (torch.from_numpy(data[k][sl].copy()).to(dev) for k in ("x", "l", "u", "nbd", "g"))
    rep = sol.kkt(x, l, u, nbd, g, tol=tol)
    res = dict(cnt=rep.counts, val=rep.values, status=rep.status.cpu().numpy(), pg=rep.pg.cpu().numpy(),
               mult=rep.mult.cpu().numpy(), row0=row0)
    for mask in MASKS:
        codes = [c for c in range(-1, 4) if mask >> (c + 1) & 1]
        res["idx%d" % mask] = sol.kkt_indices(rep.status, codes).cpu().numpy()
    leave(sol, rank, out_prefix, res, state=False)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], a[5], float(a[6]), a[7])
