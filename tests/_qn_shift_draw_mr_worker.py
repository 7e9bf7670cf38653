"""Worker for tests/test_gpu_qn_shift_draw_sharded.py: `world` processes on cuda:0, one block of rows each (cut
unevenly, the split and the shift of tests/_qn_shift_mr_worker.py), reductions through a gloo host group.  The draws and
densities of the model plus a diagonal at the FG_START return (no pair yet), then the separable quadratic with all
four bound types to iteration `iters` and the same again, called collectively: K draws from sample FIRST with their
log-densities, the factor applied to K vectors, their quadratic forms and log-densities, and the pinned count.  Writes
them and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_shift_draw_mr_worker.py rank world port n m iters out_prefix"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _qn_shift_mr_worker import MU, SEED, cut, shift  # noqa: E402

K, FIRST, DRAW_SEED, SCALE = 5, 3, 2 ** 40 + 77, 0.5


def entries(sh, V, mean):
    """every new entry once on this rank's rows (collective on a sharded context)"""
    dr, lp = sh.sample(K, DRAW_SEED, first=FIRST, mean=mean, scale=SCALE, log_prob=True)
    return dict(draws=dr.cpu().numpy(), logp=lp, root=sh.sqrt(V).cpu().numpy(), quad=sh.quad(V, center=mean),
                logq=sh.log_prob(V, mean=mean, scale=SCALE), pinned=np.int64(sh.pinned))


def run(rank, world, port, n, m, iters, out_prefix):
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    from oracle import pyoracle as po

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    row0, n_loc = cut(n, world, rank)
    sol = lbfgsb_amd.DeviceSolver(n_loc, m, n_global=n, row0=row0, device=0)
    lbfgsb_amd.attach_host_group(sol, rank, world)
    p = po.problem_quadratic(n, m, mixed_nbd=True)
    sl = slice(row0, row0 + n_loc)
    x = torch.from_numpy(p.x0[sl].copy()).to(dev)
    g = torch.zeros_like(x)
    l = torch.from_numpy(p.l[sl].copy()).to(dev)
    u = torch.from_numpy(p.u[sl].copy()).to(dev)
    nbd = torch.from_numpy(p.nbd[sl].astype(np.int32)).to(dev)
    rng = np.random.default_rng(SEED)                               # the same global vectors on every rank
    V = torch.from_numpy(rng.standard_normal((K, n))[:, sl].copy()).to(dev)
    mean = torch.from_numpy(rng.standard_normal(n)[sl].copy()).to(dev)
    d = torch.from_numpy(shift(n, world)[sl].copy()).to(dev)

    res = {}
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG_START"):
            assert int(sol.isave[27]) == 0
            res.update({"s0_" + k: v for k, v in entries(sol.qn_shift(d, MU), V, mean).items()})
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t
    res.update({"s1_" + k: v for k, v in entries(sol.qn_shift(d, MU), V, mean).items()})
    wa, _ = sol.export_state()
    res.update(wa=wa, isave=sol.isave.copy(), head=int(sol.isave[26]), col=int(sol.isave[27]), row0=row0,
               n_loc=n_loc)
    np.savez(out_prefix + ".%d.npz" % rank, **res)
    sol.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
