"""Worker for tests/test_gpu_qn_eig_sharded.py: `world` processes on cuda:0, one block of rows each, reductions
through a gloo host group.  Runs the separable quadratic with all four bound types to iteration `iters`, then calls
the eigen-decomposition of the curvature model collectively (lbfgsb_hip_qn_eig / qn_eigvec, both modes, every
vector) and writes the spectra, this rank's rows of the vectors and its exported state to out_prefix.<rank>.npz.
usage: _qn_eig_mr_worker.py rank world port n m iters out_prefix"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(rank, world, port, n, m, iters, out_prefix):
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    from oracle import pyoracle as po

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    row0, n_loc = lbfgsb_amd.block_partition(n, world, rank)
    sol = lbfgsb_amd.DeviceSolver(n_loc, m, n_global=n, row0=row0, device=0)
    lbfgsb_amd.attach_host_group(sol, rank, world)
    p = po.problem_quadratic(n, m, mixed_nbd=True)
    sl = slice(row0, row0 + n_loc)
    x = torch.from_numpy(p.x0[sl].copy()).to(dev)
    g = torch.zeros_like(x)
    l = torch.from_numpy(p.l[sl].copy()).to(dev)
    u = torch.from_numpy(p.u[sl].copy()).to(dev)
    nbd = torch.from_numpy(p.nbd[sl].astype(np.int32)).to(dev)
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t
    res = {}
    for key, inverse in (("b", False), ("h", True)):
        bulk, lam = sol.qn_eig(inverse=inverse)
        res.update({"bulk_" + key: bulk, "lam_" + key: lam,
                    "u_" + key: sol.qn_eigvec(inverse=inverse).cpu().numpy()})
    wa, _ = sol.export_state()
    res.update(wa=wa, isave=sol.isave.copy(), head=int(sol.isave[26]), col=int(sol.isave[27]), row0=row0,
               n_loc=n_loc, theta=float(sol.dsave[0]))
    np.savez(out_prefix + ".%d.npz" % rank, **res)
    sol.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
