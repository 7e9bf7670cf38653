"""The worker side of the "several ranks on one GPU" tests (tests/_*_mr_worker.py; the test side is
tests/_sharded.py): `world` processes on cuda:0, one block of rows each, reductions through a gloo host group
('gloo'), the library's communicator code path with the shared-memory RCCL stand-in ('fakerccl', tests/fake_rccl.cpp
through LBFGSB_RCCL_LIBRARY), an RCCL communicator of one rank ('rccl1') or none ('single', world 1).  A worker joins,
uploads its rows of the separable quadratic with all four bound types, runs to an iteration, calls the entries that
are its own and leaves its results in out_prefix.<rank>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED, MU = 29, 0.3   # of the model plus a diagonal: the seed of its vectors (SEED + 1: of the shift) and its mu


def cut(n, world, rank):
    """(row0, n_local) of an uneven split: the boundaries at the fractions 0.437 (two ranks) or 0.301 and 0.688"""
    edges = [0] + [int(f * n) for f in {2: (0.437,), 3: (0.301, 0.688)}[world]] + [n]
    return edges[rank], edges[rank + 1] - edges[rank]


def shift(n, world):
    """the global d: random in [0, 10], every third row pinned, and a run of 40 pinned rows across every rank boundary"""
    d = np.random.default_rng(SEED + 1).uniform(0.0, 10.0, n)
    d[::3] = np.inf
    for r in range(1, world):
        e = cut(n, world, r)[0]
        d[e - 20:e + 20] = np.inf
    return d


def attach(sol, rank, world, mode):
    """the reductions of the context `sol` as `mode` says (the process group exists)"""
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    if mode == "gloo":
        lbfgsb_amd.attach_host_group(sol, rank, world)
    elif mode == "rccl1":
        assert world == 1
        lbfgsb_amd.attach_rccl(sol, 0, 1, torch.device("cuda", 0))
    elif mode == "fakerccl":
        # the library's communicator code path (ncclAllReduce / ncclAllGather on the solver's stream) with several
        # ranks on ONE GPU
        ids = [lbfgsb_amd.DeviceSolver.rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, 0)
        sol.init_rccl(ids[0], rank, world)
        assert "libfake_rccl" in open("/proc/self/maps").read()   # (the stand-in, not the real library)
    else:
        assert mode == "single" and world == 1, mode


def join(rank, world, port, mode, n, m, partition=None, **solver_kwargs):
    """The process group, this rank's block of the n rows (lbfgsb_amd.block_partition, or `partition` such as cut)
    and its attached context: (sol, row0, n_loc, dev)."""
    import torch
    import torch.distributed as dist
    import lbfgsb_amd
    if mode != "single":
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    row0, n_loc = (partition or lbfgsb_amd.block_partition)(n, world, rank)
    sol = lbfgsb_amd.DeviceSolver(n_loc, m, n_global=n, row0=row0, device=0, **solver_kwargs)
    attach(sol, rank, world, mode)
    return sol, row0, n_loc, torch.device("cuda", 0)


def upload(p, row0, n_loc, dev):
    """this rank's rows of the problem p on the device: x, g, l, u, nbd"""
    import torch
    sl = slice(row0, row0 + n_loc)
    x = torch.from_numpy(p.x0[sl].copy()).to(dev)
    l = torch.from_numpy(p.l[sl].copy()).to(dev)
    u = torch.from_numpy(p.u[sl].copy()).to(dev)
    return x, torch.zeros_like(x), l, u, torch.from_numpy(p.nbd[sl].astype(np.int32)).to(dev)


def quadratic_rows(po, n, m, row0, n_loc, dev):
    """this rank's rows of the separable quadratic with all four bound types: x, g, l, u, nbd"""
    return upload(po.problem_quadratic(n, m, mixed_nbd=True), row0, n_loc, dev)


def run_to(sol, x, l, u, nbd, g, iters, on_start=None):
    """drive the run to the NEW_X return of iteration `iters`; on_start() is called at the FG_START return (no pair
    stored yet)"""
    for _ in range(100000):
        t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if on_start is not None and t.startswith("FG_START"):
            assert int(sol.isave[27]) == 0
            on_start()
        if t.startswith("FG"):
            sol.f[0] = sol.objective(0, x, g)
        elif not t.startswith("NEW_X") or sol.isave[29] >= iters:
            break
    assert t.startswith("NEW_X"), t


def leave(sol, rank, prefix, res, state=True):
    """write res (with this rank's exported state, if `state`) to prefix.<rank>.npz, close the context and leave the
    group"""
    import torch.distributed as dist
    if state:
        wa, _ = sol.export_state()
        res.update(wa=wa, isave=sol.isave.copy(), head=int(sol.isave[26]), col=int(sol.isave[27]),
                   row0=sol.row0, n_loc=sol.n)
    np.savez(prefix + ".%d.npz" % rank, **res)
    sol.close()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
