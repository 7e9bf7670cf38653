"""Worker for tests/test_gpu_qn_quad_sharded.py: `world` processes on cuda:0, one block of rows each, reductions
through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL stand-in
('fakerccl', LBFGSB_RCCL_LIBRARY).  Quadratic forms and draw densities at the FG_START return (no pair yet), then the
separable quadratic with all four bound types to iteration `iters` and the entries called collectively: qn_quad of
both modes and qn_logpdf of both covariances at 3 vectors around a mean, 5 draws from sample 3 with their
log-densities for both covariances.  Writes the numbers, this rank's rows of the draws and its exported state to
out_prefix.<rank>.npz.
usage: _qn_quad_mr_worker.py rank world port mode n m iters out_prefix"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, K, FIRST, SCALE = 2 ** 40 + 12345, 5, 3, 0.5


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    from oracle import pyoracle as po

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    row0, n_loc = lbfgsb_amd.block_partition(n, world, rank)
    sol = lbfgsb_amd.DeviceSolver(n_loc, m, n_global=n, row0=row0, device=0)
    if mode == "gloo":
        lbfgsb_amd.attach_host_group(sol, rank, world)
    else:
        ids = [lbfgsb_amd.DeviceSolver.rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, 0)
        sol.init_rccl(ids[0], rank, world)
        assert "libfake_rccl" in open("/proc/self/maps").read()   # (the stand-in, not the real library)
    p = po.problem_quadratic(n, m, mixed_nbd=True)
    sl = slice(row0, row0 + n_loc)
    x = torch.from_numpy(p.x0[sl].copy()).to(dev)
    g = torch.zeros_like(x)
    l = torch.from_numpy(p.l[sl].copy()).to(dev)
    u = torch.from_numpy(p.u[sl].copy()).to(dev)
    nbd = torch.from_numpy(p.nbd[sl].astype(np.int32)).to(dev)
    rng = np.random.default_rng(17)                                 # the same global vectors on every rank
    mean = torch.from_numpy(rng.standard_normal(n)[sl].copy()).to(dev)
    V = torch.from_numpy(rng.standard_normal((3, n))[:, sl].copy()).to(dev)

    def draws(inverse):
        d, lp = sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=inverse, return_logpdf=True)
        assert torch.equal(d, sol.qn_draw(K, SEED, first=FIRST, mean=mean, scale=SCALE, inverse=inverse))
        return d.cpu().numpy(), lp

    res = {}
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG_START"):
            assert int(sol.isave[27]) == 0
            d0, lp0 = draws(True)
            res.update(d0=d0, lp0=lp0, q0=sol.qn_quad(V, center=mean))
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t
    db, lpdb = draws(False)
    dh, lpdh = draws(True)
    res.update(qb=sol.qn_quad(V, center=mean), qh=sol.qn_quad(V, center=mean, inverse=True),
               lpb=sol.qn_logpdf(V, mean=mean, scale=SCALE, inverse=False),
               lph=sol.qn_logpdf(V, mean=mean, scale=SCALE, inverse=True),
               db=db, dh=dh, lpdb=lpdb, lpdh=lpdh, ldb=sol.qn_logdet(), ldh=sol.qn_logdet(inverse=True))
    wa, _ = sol.export_state()
    res.update(wa=wa, isave=sol.isave.copy(), head=int(sol.isave[26]), col=int(sol.isave[27]), row0=row0,
               n_loc=n_loc)
    np.savez(out_prefix + ".%d.npz" % rank, **res)
    sol.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]), int(a[7]), a[8])
