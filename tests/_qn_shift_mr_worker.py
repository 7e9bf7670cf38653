"""Worker for tests/test_gpu_qn_shift_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  The model plus a diagonal at the FG_START return (no pair yet), then the
separable quadratic with all four bound types to iteration `iters` and the shift again, called collectively: the
solves of K vectors, the diagonal, the log det and the pinned count.  Writes them and this rank's exported state to
out_prefix.<rank>.npz.
usage: _qn_shift_mr_worker.py rank world port mode n m iters out_prefix"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, SEED, MU = 5, 29, 0.3


def shift(n, world):
    """the global d: random in [0, 10], every third row pinned, and a run of 40 pinned rows across every rank boundary"""
    d = np.random.default_rng(SEED + 1).uniform(0.0, 10.0, n)
    d[::3] = np.inf
    for r in range(1, world):
        e = cut(n, world, r)[0]
        d[e - 20:e + 20] = np.inf
    return d


def cut(n, world, rank):
    """(row0, n_local) of an uneven split: the boundaries at the fractions 0.437 (two ranks) or 0.301 and 0.688"""
    edges = [0] + [int(f * n) for f in {2: (0.437,), 3: (0.301, 0.688)}[world]] + [n]
    return edges[rank], edges[rank + 1] - edges[rank]


def run(rank, world, port, mode, n, m, iters, out_prefix):
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    from oracle import pyoracle as po

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    row0, n_loc = cut(n, world, rank)
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
    rng = np.random.default_rng(SEED)                               # the same global vectors on every rank
    V = torch.from_numpy(rng.standard_normal((K, n))[:, sl].copy()).to(dev)
    d = torch.from_numpy(shift(n, world)[sl].copy()).to(dev)

    def shifted(tag):
        sh = sol.qn_shift(d, MU)
        return {tag + "_x": sh.solve(V).cpu().numpy(), tag + "_diag": sh.diag().cpu().numpy(),
                tag + "_logdet": np.float64(sh.logdet()), tag + "_pinned": np.int64(sh.pinned)}

    res = {}
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG_START"):
            assert int(sol.isave[27]) == 0
            res.update(shifted("s0"))
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t
    res.update(shifted("s1"))
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
