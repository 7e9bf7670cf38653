"""Worker for tests/test_gpu_qn_pairs_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  No run: every rank loads its rows of the first m - 1 pairs of one dyadic
sequence (tests/_qn_pairs_seq.py) with qn_set_pairs, pushes the next two (the second one wraps the ring), reads the
pairs back and applies H to its rows of two vectors.  Writes them to out_prefix.<rank>.npz.
usage: _qn_pairs_mr_worker.py rank world port mode n m out_prefix"""
import sys

import numpy as np

from _mr_common import cut, join, leave


def vectors(n):
    """dyadic, as the pairs: S'v and Y'v are then exact in any order of summation, so they do not depend on the split"""
    return np.random.default_rng(5).integers(-8, 9, (2, n)).astype(np.float64) / 8.0


def act(sol, pairs, states, m, rows, dev):
    """set m - 1 pairs, push two, get: what every rank (and the one context the test compares with) does"""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    S0, Y0 = states[m - 1].pairs()
    sol.qn_set_pairs(up(S0[rows].T), up(Y0[rows].T))
    stored = [sol.qn_push_pair(up(s[rows]), up(y[rows])) for s, y in pairs[m - 1:m + 1]]
    S, Y, theta = sol.qn_pairs()
    hv = sol.qn_apply(up(vectors(states[0].n)[:, rows]), inverse=True)
    return dict(stored=np.array(stored), S=S.cpu().numpy(), Y=Y.cpu().numpy(), theta=np.float64(theta),
                hv=hv.cpu().numpy(), logdet=np.float64(sol.qn_logdet()))


def run(rank, world, port, mode, n, m, out_prefix):
    from _qn_pairs_seq import sequence

    sol, row0, n_loc, dev = join(rank, world, port, mode, n, m, partition=cut)
    pairs, states = sequence(n, m, m + 1)
    res = act(sol, pairs, states, m, slice(row0, row0 + n_loc), dev)
    res.update(row0=row0, n_loc=n_loc)
    leave(sol, rank, out_prefix, res, state=False)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), a[7])
