"""Contexts come and go without the device losing memory: twelve create / run / use / destroy cycles over the shapes
and flags that allocate differently (m = 5, 10 and 40 -- the last one the unfused path of solver_wide.inl -- and
default, LBFGSB_F_REAL32, LBFGSB_F_PARALLEL_GCP, LBFGSB_F_FOLLOW_BOUNDS), each with the operators that bring buffers
and events of their own (qn_apply, qn_draw, qn_gram, kkt, kkt_list, the pass clocks, the return and order events).
This is where hipFree / hipHostFree / hipEventDestroy are paired on the real runtime along the paths that the CPU
harness (tests/cpu_walk/walk_check.cpp) has no kernels for; small leaks are that harness's job, not this test's.

The bound: free device memory after cycle 12 may be lower than after cycle 4 (the end of the first round of flags) by
at most 8 MiB = one fp64 n-vector at this n.  An n-sized buffer leaked once per cycle would show as 64 MiB or more.
Measured on an MI355X: the difference is 4.0 MiB with the buffers owned by one GpuOwner and 4.0 MiB at the commit
before it (the hand-written lists) -- the same twelve readings, one 4 MiB step of the runtime's own after cycle 7 --
so the bound is the 8 MiB as stated, with nothing added for a drift of the parent.
torch's caching allocator is emptied before each reading: what it keeps for the index tensors of kkt_indices,
whose sizes differ from cycle to cycle, is torch's and not the library's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2 ** 20
CYCLES = 12
ITERS = 6
MIB = 1 << 20


def test_twelve_context_cycles_keep_device_memory():
    import torch
    import lbfgsb_amd as la

    dev = torch.device("cuda", 0)
    # the problem and every output, once, in both real kinds: min 1/2 sum of the built-in quadratic over a box, all
    # four bound types
    nbd = (torch.arange(N, device=dev) % 4).to(torch.int32)
    data = {}
    for dt in (torch.float64, torch.float32):
        data[dt] = dict(x=torch.zeros(N, dtype=dt, device=dev), g=torch.zeros(N, dtype=dt, device=dev),
                        l=torch.full((N,), -1.0, dtype=dt, device=dev), u=torch.full((N,), 1.0, dtype=dt, device=dev),
                        v=torch.linspace(-1.0, 1.0, 3 * N, dtype=dt, device=dev).view(3, N).contiguous(),
                        out=torch.empty((3, N), dtype=dt, device=dev), draws=torch.empty((2, N), dtype=dt, device=dev),
                        pg=torch.empty(N, dtype=dt, device=dev), mult=torch.empty(N, dtype=dt, device=dev))
    status = torch.empty(N, dtype=torch.int8, device=dev)
    second = torch.cuda.Stream(device=dev)
    flag_sets = (dict(), dict(real32=True), dict(parallel_gcp=True), dict(follow_bounds=True))
    free_after = []
    for cycle in range(CYCLES):
        m = (5, 10, 40)[cycle % 3]
        kw = flag_sets[cycle % 4]
        t = data[torch.float32 if kw.get("real32") else torch.float64]
        x, g, l, u = t["x"], t["g"], t["l"], t["u"]
        x.zero_()
        sol = la.DeviceSolver(N, m, **kw)
        try:
            sol.pass_clock(1)  # (on before the run: the clocks' event pairs are created by the passes they time)
            while True:
                task = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
                if task.startswith("FG"):
                    sol.f[0] = sol.objective(0, x, g)
                elif not task.startswith("NEW_X") or sol.isave[29] >= ITERS:
                    break
            assert task.startswith("NEW_X") and sol.isave[29] == ITERS, (cycle, m, kw, task)
            sol.qn_apply(t["v"], out=t["out"])
            sol.qn_draw(2, seed=cycle, out=t["draws"])
            gram = sol.qn_gram(t["v"])
            assert np.all(np.isfinite(gram)) and np.all(np.diag(gram) > 0.0), (cycle, m, kw, gram)
            rep = sol.kkt(x, l, u, nbd, g, pg=t["pg"], mult=t["mult"], status=status)
            idx = sol.kkt_indices(status, (1, 2, 3))
            assert idx.numel() == rep.n_lower + rep.n_upper + rep.n_fixed, (cycle, m, kw, rep)
            sol.pass_clock(-1)
            sol.release_to_stream(second.cuda_stream)
            sol.wait_stream(second.cuda_stream)
        finally:
            sol.close()
        del idx, rep
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free_after.append(torch.cuda.mem_get_info()[0])
    lost = free_after[3] - free_after[CYCLES - 1]
    print("free device memory after each cycle, MiB:", [round(f / MIB, 1) for f in free_after])
    print("lower after cycle %d than after cycle 4 by %.1f MiB" % (CYCLES, lost / MIB))
    assert lost <= 8 * MIB, [round(f / MIB, 1) for f in free_after]
