"""Worker for tests/test_gpu_qn_idx_sharded.py: `world` processes on cuda:0, one block of rows each (cut unevenly),
reductions through a gloo host group ('gloo') or the library's communicator code path with the shared-memory RCCL
stand-in ('fakerccl', LBFGSB_RCCL_LIBRARY).  The separable quadratic with all four bound types to iteration `iters`,
then the entries at index lists, called collectively with the same global list on every rank: the rows of the pairs,
the blocks of B and H (square and rectangular) and of the model plus a diagonal, and this rank's rows of the columns.
Writes them and this rank's exported state to out_prefix.<rank>.npz.
usage: _qn_idx_mr_worker.py rank world port mode n m iters out_prefix"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _qn_shift_mr_worker import MU, cut, shift  # noqa: E402  (the split and the shift of the shifted model's test)

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
    d = torch.from_numpy(shift(n, world)[sl].copy()).to(dev)
    ia, ib = lists(n, world)

    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t
    res = dict(rows=sol.qn_rows(ia))
    for inv, tag in ((False, "b"), (True, "h")):
        res[tag + "_sq"] = sol.qn_block(ia, inverse=inv)
        res[tag + "_rect"] = sol.qn_block(ia, ib, inverse=inv)
        res[tag + "_cols"] = sol.qn_cols(ia, inverse=inv).cpu().numpy()
    sh = sol.qn_shift(d, MU)
    res.update(s_sq=sh.block(ia), s_rect=sh.block(ia, ib), s_cols=sh.columns(ia).cpu().numpy())
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
