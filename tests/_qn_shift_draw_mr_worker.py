"""Worker for tests/test_gpu_qn_shift_draw_sharded.py: `world` processes on cuda:0, one block of rows each (cut
unevenly, the split and the shift of tests/_mr_common.py), reductions through a gloo host group.  The draws and
densities of the model plus a diagonal at the FG_START return (no pair yet), then the separable quadratic with all
four bound types to iteration `iters` and the same again, called collectively: K draws from sample FIRST with their
log-densities, the factor applied to K vectors, their quadratic forms and log-densities, and the pinned count.  Writes
them and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_shift_draw_mr_worker.py rank world port n m iters out_prefix"""
import sys

import numpy as np

from _mr_common import MU, SEED, cut, join, leave, quadratic_rows, run_to, shift

K, FIRST, DRAW_SEED, SCALE = 5, 3, 2 ** 40 + 77, 0.5


def entries(sh, V, mean):
    """every new entry once on this rank's rows (collective on a sharded context)"""
    dr, lp = sh.sample(K, DRAW_SEED, first=FIRST, mean=mean, scale=SCALE, log_prob=True)
    return dict(draws=dr.cpu().numpy(), logp=lp, root=sh.sqrt(V).cpu().numpy(), quad=sh.quad(V, center=mean),
                logq=sh.log_prob(V, mean=mean, scale=SCALE), pinned=np.int64(sh.pinned))


def run(rank, world, port, n, m, iters, out_prefix):
    import torch
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, "gloo", n, m, partition=cut)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    sl = slice(row0, row0 + n_loc)
    rng = np.random.default_rng(SEED)                               # the same global vectors on every rank
    V = torch.from_numpy(rng.standard_normal((K, n))[:, sl].copy()).to(dev)
    mean = torch.from_numpy(rng.standard_normal(n)[sl].copy()).to(dev)
    d = torch.from_numpy(shift(n, world)[sl].copy()).to(dev)

    def tagged(tag):
        return {tag + k: v for k, v in entries(sol.qn_shift(d, MU), V, mean).items()}

    res = {}
    run_to(sol, x, l, u, nbd, g, iters, on_start=lambda: res.update(tagged("s0_")))
    res.update(tagged("s1_"))
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
