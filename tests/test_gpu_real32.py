"""REAL32 context (BASELINE.json configs[4], reference -DREAL32, lbfgsb_kinds_module.F90:29-37):
fp32 storage and kernels, fp64 partial sums and host algebra.  The reference's REAL32 build
does everything in fp32, so agreement is a tolerance sweep, not bit parity:
f must agree with the REAL64 oracle to ~1e-6 and with the REAL32 oracle to fp32 noise.
One routine deep, with derived bars (bit for bit / 1e-12 of the fp64 sums / 4 x the REAL32 oracle's own error) and at
n = 1 ... 150001 with every fp32 tail: tests/test_gpu_routines_real32.py (helper tests/_r32_truth.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(oracle_built):
    import torch
    import lbfgsb_amd
    assert torch.cuda.is_available()
    return dict(po=oracle_built, torch=torch, la=lbfgsb_amd)


def test_wtv_fp32_storage_fp64_accumulate(env):
    torch, la = env["torch"], env["la"]
    rng = np.random.default_rng(5)
    for n, m in ((1003, 5), (40001, 10), (8193, 20)):
        ws = rng.standard_normal((m, n)).astype(np.float32)
        wy = rng.standard_normal((m, n)).astype(np.float32)
        v = rng.standard_normal(n).astype(np.float32)
        sol = la.DeviceSolver(n, m, real32=True)
        sol.set_w(ws, wy)
        got = sol.wtv(torch.from_numpy(v).cuda(), m, 1)
        want = np.concatenate([wy.astype(np.float64) @ v.astype(np.float64),
                               ws.astype(np.float64) @ v.astype(np.float64)])
        bound = np.concatenate([np.abs(wy).astype(np.float64) @ np.abs(v),
                                np.abs(ws).astype(np.float64) @ np.abs(v)])
        assert np.all(np.abs(got - want) <= 1e-13 * bound)   # products of fp32 are exact in fp64
        sol.close()


def test_real32_trajectory_tolerance_sweep(env):
    po, torch, la = env["po"], env["torch"], env["la"]
    n, m = 1000, 10
    p64 = po.problem_quadratic(n, m)
    p32 = po.problem_quadratic(n, m, real=np.float32)
    f64 = {}
    po.run(po.Engine("oracle"), p64, max_iter=12,
           snapshot=lambda k, s: f64.__setitem__(int(s.isave[29]), float(s.f[0])) if s.task_s.startswith("NEW_X") else None)
    f32 = {}
    po.run(po.Engine("oracle_r32"), p32, max_iter=12,
           snapshot=lambda k, s: f32.__setitem__(int(s.isave[29]), float(s.f[0])) if s.task_s.startswith("NEW_X") else None)
    # host-pointer form with real_bytes = 4, exactly what the Fortran module passes under -DREAL32
    s = po.State.fresh(p32)
    nbd = p32.nbd.astype(np.int32)
    got = {}
    for _ in range(200):
        la.setulb(n, m, s.x, p32.l, p32.u, nbd, s.f, s.g, 0.0, 0.0, s.wa, s.iwa, s.task, -1,
                  s.csave, s.lsave, s.isave, s.dsave)
        t = s.task_s
        if t.startswith("FG"):
            s.f[0] = p32.fg(s.x, s.g)
        elif t.startswith("NEW_X"):
            got[int(s.isave[29])] = float(s.f[0])
            if s.isave[29] >= 12:
                s.task[:] = po.pad60("STOP: enough")
        else:
            break
    assert s.x.dtype == np.float32 and s.dsave.dtype == np.float32
    assert float(s.dsave[4]) == pytest.approx(1.1920929e-07)        # epsmch of REAL32 (:432)
    assert len(got) >= 8
    for it in sorted(got):
        if it in f64:
            assert got[it] == pytest.approx(f64[it], rel=5e-5), ("vs REAL64 oracle", it)
        if it in f32:
            # the all-fp32 reference is itself ~1e-3 away from the fp64 trajectory (979 Cauchy
            # segments accumulated in fp32 in iteration 1): fp32-noise agreement only
            assert got[it] == pytest.approx(f32[it], rel=5e-3), ("vs REAL32 oracle", it)
    # first iterations are identical decisions: tight agreement there
    for it in (1, 2, 3):
        assert got[it] == pytest.approx(f64[it], rel=2e-6)


# ---------------------------------------------------------------------------------------------
# BASELINE.json configs[4] (m = 20, REAL32): one-step parity of the fp32 MC = 20 / 32 kernels.
# Every setulb return of the REAL32 oracle's trajectory is the INPUT state of one GPU call
# (REAL32 context: fp32 storage, fp64 partial sums and host algebra).  The output is compared
# with two CPU results computed from that same state:
#   * the REAL64 oracle fed the state widened to fp64 ("what exact arithmetic on these fp32
#     inputs gives"): the GPU must agree to fp32 STORAGE rounding -- a tolerance sweep records
#     the tightest power of ten that holds per array, and asserts the bar below;
#   * the REAL32 oracle (= the reference's -DREAL32 build, everything in fp32,
#     src/lbfgsb_kinds_module.F90:29-37): agreement to fp32 ARITHMETIC noise.
# Decisions (task, counters, iwhere) must equal at least one of the two -- near convergence the
# all-fp32 line search and the fp64 one can legitimately part ways.
# ---------------------------------------------------------------------------------------------
def _widen(po, s):
    f64 = np.float64
    return po.State(s.n, s.m, s.x.astype(f64), s.g.astype(f64), s.f.astype(f64), s.wa.astype(f64),
                    s.iwa.copy(), s.task.copy(), s.csave.copy(), s.lsave.copy(), s.isave.copy(),
                    s.dsave.astype(f64))


def _gpu_one_call_r32(env, p32, s):
    po, torch, la = env["po"], env["torch"], env["la"]
    sol = la.DeviceSolver(p32.n, p32.m, real32=True, mirror_index=True)
    try:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        x, g = dev(s.x), dev(s.g)
        l, u, nbd = dev(p32.l), dev(p32.u), dev(p32.nbd.astype(np.int32))
        if not s.task_s.startswith("START"):
            sol.import_state(s.wa, s.iwa, s.isave)
        sol.task[:] = s.task
        sol.csave[:] = s.csave
        sol.lsave[:] = s.lsave
        sol.isave[:] = s.isave
        sol.dsave[:] = s.dsave.astype(np.float64)
        sol.f[0] = float(s.f[0])
        sol.setulb(x, l, u, nbd, g, p32.factr, p32.pgtol)
        torch.cuda.synchronize()
        wa, iwa = sol.export_state()
        assert wa.dtype == np.float32
        return po.State(p32.n, p32.m, x.cpu().numpy(), g.cpu().numpy(), sol.f.copy(), wa, iwa,
                        sol.task.copy(), sol.csave.copy(), sol.lsave.copy(), sol.isave.copy(),
                        sol.dsave.copy())
    finally:
        sol.close()


def _relerr(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.max(np.abs(b))) if b.size else 0.0, floor, 1e-300)
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


SWEEP = [10.0 ** -k for k in range(8, 1, -1)]       # 1e-8 ... 1e-2


def _tightest(err):
    for tol in SWEEP:
        if err <= tol:
            return tol
    return float("inf")


R32_CASES = [
    ("quadmix20000_m20", dict(n=20000, m=20, mixed=True), 64),     # MC = 20: configs[4]'s kernels
    ("quad6007_m17", dict(n=6007, m=17, mixed=False), 52),         # MC = 20, col < MC slots unused
    ("quadmix3001_m25", dict(n=3001, m=25, mixed=True), 70),       # col 21...25: the update pass in two parts
    ("quadmix2003_m36", dict(n=2003, m=36, mixed=True), 90),       # m > 32 in REAL32
]


@pytest.mark.parametrize("name,spec,ncalls", R32_CASES, ids=[c[0] for c in R32_CASES])
def test_real32_one_step_parity_m20(env, name, spec, ncalls):
    po = env["po"]
    n, m = spec["n"], spec["m"]
    p32 = po.problem_quadratic(n, m, mixed_nbd=spec["mixed"], real=np.float32)
    p64 = po.problem_quadratic(n, m, mixed_nbd=spec["mixed"])
    e32, e64 = po.Engine("oracle_r32"), po.Engine("oracle")
    snaps = []
    po.run(e32, p32, max_calls=ncalls, snapshot=lambda k, s: snaps.append(s.copy()))
    off = po.wa_offsets(n, m)
    worst64, worst32 = {}, {}
    tested = decided_by_r32_only = 0
    for k in range(len(snaps) - 1):
        s = snaps[k].copy()
        t = s.task_s
        if not (t.startswith("FG") or t.startswith("NEW_X")):
            continue
        if t.startswith("FG"):
            s.f[0] = p32.fg(s.x, s.g)
        got = _gpu_one_call_r32(env, p32, s)
        exp32 = snaps[k + 1]
        exp64 = _widen(po, s)
        po.call(e64, p64, exp64)

        def same_decisions(exp):
            gi, ei = got.isave[21:44].copy(), exp.isave[21:44].copy()
            gi[2] = ei[2] = 0
            return (got.task_s == exp.task_s and np.array_equal(gi, ei)
                    and np.array_equal(got.iwa[n:2 * n], exp.iwa[n:2 * n])
                    and np.array_equal(got.iwa[:n], exp.iwa[:n]))
        ok64, ok32 = same_decisions(exp64), same_decisions(exp32)
        assert ok64 or ok32, "call %d (%s): decisions match neither oracle" % (k, t)
        if not ok64:
            decided_by_r32_only += 1
            continue                       # compared the floats against a different branch otherwise
        tested += 1
        xs = float(np.max(np.abs(exp64.x)))

        def errs(exp, into):
            rows = {"x": _relerr(got.x, exp.x), "g": _relerr(got.g, exp.g), "f": _relerr(got.f, exp.f)}
            for nm in ("z", "r", "d", "t", "xp", "ws", "wy"):
                o, ln = off[nm]
                rows[nm] = _relerr(got.wa[o:o + ln], exp.wa[o:o + ln], floor=xs * 1e-3)
            for kk in (0, 3, 10, 11, 12, 13, 14, 15):          # theta dnorm gd stpmx sbgnrm stp gdold dtd
                rows["dsave%d" % (kk + 1)] = _relerr([got.dsave[kk]], [exp.dsave[kk]], floor=1e-30)
            for kk, v in rows.items():
                into[kk] = max(into.get(kk, 0.0), v)
        errs(exp64, worst64)
        if ok32:                           # (else the all-fp32 run took another branch here)
            errs(exp32, worst32)
    assert tested >= 20 and decided_by_r32_only <= 2, (tested, decided_by_r32_only)
    table = {kk: (_tightest(worst64[kk]), _tightest(worst32[kk])) for kk in worst64}
    print("\n%s: tightest tolerance that holds (vs REAL64-from-same-state, vs REAL32 oracle)" % name)
    for kk, (a64, a32) in table.items():
        print("   %-8s %8.0e %8.0e   (max err %.2e / %.2e)" % (kk, a64, a32, worst64[kk], worst32[kk]))
    # The bars.  Against exact arithmetic on the same fp32 inputs: vectors that are copied or
    # formed by one rounding (g, t, r, xp, the new W columns) agree to fp32 storage rounding
    # (2^-24 = 6e-8 per element); z, x, d pass through theta and K^-1 (the Cauchy point is rounded
    # to fp32 where the REAL64 oracle keeps 53 bits), which amplifies that rounding by the
    # conditioning of the subspace problem -- 8e-6 (m = 17) to 1.1e-4 (m = 20, d) observed.  Against the all-fp32
    # reference build: fp32 ARITHMETIC noise.
    for kk in ("g", "t", "r", "xp", "ws", "wy", "f"):
        assert worst64[kk] <= 1e-6, (kk, worst64[kk])
    for kk in ("x", "z", "d"):
        assert worst64[kk] <= 5e-4, (kk, worst64[kk])
    for kk in ("dsave1", "dsave4", "dsave11", "dsave13", "dsave15", "dsave16"):
        assert worst64[kk] <= 1e-3, (kk, worst64[kk])
    for kk in ("x", "z", "t", "r"):
        assert worst32.get(kk, 0.0) <= 2e-3, (kk, worst32.get(kk))


def test_real32_config5_full_shape_anchors(env):
    """BASELINE.json configs[4] at its stated size: n = 1e8, m = 20, REAL32 (fp32 storage and kernels,
    fp64 accumulators and host algebra), on-device objective, W = 16 GB of fp32 -- run for 26
    iterations, i.e. through the filling of the memory to col = 20 and into the steady state, so that
    the kernels that only exist at this shape run inside the test-suite: the pair-shared update pass
    `update_scan_kernel<float, 20, ..., NEWROW, PAIR>` (509 registers), the col = 20 closed form, the
    MC = 20 storing pass.

    Anchors.  The all-fp32 reference build cannot serve at this size: its sequential fp32 sums of 1e8
    terms stagnate (measured with the real `-DREAL32 -fdefault-integer-8` build, DESIGN.md section 8:
    already at n = 2e5 its first walk has 180,423 segments where the REAL64 reference has 195,351).
    The meaningful reference for "fp32 storage, fp64 accumulation" is the REAL64 reference, and while
    its rows at this very shape are on file (tests/golden/quad_n1e8_m20_ref_rows.json: the REAL64 reference at
    n = 1e8, m = 20, 26 iterations; its iterations 1..11 are those of the m = 10 run, col < 10 not depending
    on m).  Iterations 1-3: integer columns exactly (nseg(it1) = 97,671,921, nfree(it2) = 49,999,496).
    Iterations 4-26: nfg and col exactly, nseg / nfree within 1e-3 relative + 5 (the walk's stopping point
    moves with the 6e-8 storage rounding of x and g: a handful of the 5e7 free variables' breakpoints change
    sides), f to 1e-6.  Then: f monotone to the end, col = 20 reached,
    every subspace step from iteration 2 on through the closed form (two-pass iteration), and the whole
    trajectory -- f and |proj g| included -- bit for bit reproducible from run to run."""
    import json
    import os
    torch, la = env["torch"], env["la"]
    n, m, iters = 100_000_000, 20, 26
    free_b, _tot = torch.cuda.mem_get_info()
    if free_b < 40 * (1 << 30):
        pytest.skip("needs ~30 GB of HBM")

    def run():
        sol = la.DeviceSolver(n, m, real32=True)
        x = torch.zeros(n, dtype=torch.float32, device="cuda")
        g = torch.zeros_like(x)
        l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
        nbd = torch.full((n,), 2, dtype=torch.int32, device="cuda")
        rows = []
        while True:
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
            if t.startswith("FG"):
                sol.f[0] = sol.objective(0, x, g)
            elif t.startswith("NEW_X"):
                rows.append((int(sol.isave[29]), int(sol.isave[33]), int(sol.isave[32]), int(sol.isave[37]),
                             float(sol.f[0]), float(sol.dsave[12]), int(sol.isave[27])))
                if sol.isave[29] >= iters:
                    break
            else:
                break
        counts = sol.path_counts()
        task = sol.task_s
        sol.close()
        del x, g, l, u, nbd
        torch.cuda.empty_cache()
        return rows, counts, task
    rows, (closed_steps, three_steps, _), task = run()
    assert task.startswith("NEW_X") and len(rows) == iters, (task, rows[-1])
    assert rows[0][2] == 97_671_921, rows[0]
    assert rows[1][3] == 49_999_496, rows[1]
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ref10 = json.load(open(os.path.join(gold, "quad_n1e8_m10_ref_rows.json")))["rows"]
    # the REAL64 reference's own rows at THIS shape (n = 1e8, m = 20; profiles/scripts/cpu_ref_full.py --m 20
    # --iters 26, round 6): the steady state with 20 pairs stored -- iterations 12 to 26, the only ones in which
    # update_scan_kernel<float, 20, ..., PAIR> at col = 20 runs -- has reference rows too
    ref = json.load(open(os.path.join(gold, "quad_n1e8_m20_ref_rows.json")))["rows"]
    assert len(ref) == iters and [r["col"] for r in ref][-6:] == [20] * 6
    for a, b in zip(ref[:11], ref10[:11]):           # (col < 10: the two reference runs are the same run)
        assert (a["nfg"], a["nseg"], a["nfree"], a["f"]) == (b["nfg"], b["nseg"], b["nfree"], b["f"])
    for got, want in zip(rows[:3], ref[:3]):
        assert got[:4] == (want["iter"], want["nfg"], want["nseg"], want["nfree"]), (got, want)
    for got, want in zip(rows, ref):                 # all 26 iterations, the REAL32 rules
        assert got[:2] == (want["iter"], want["nfg"]), (got, want)
        assert abs(got[2] - want["nseg"]) <= 1e-3 * want["nseg"] + 5, (got, want)
        assert abs(got[3] - want["nfree"]) <= 1e-3 * want["nfree"] + 5, (got, want)
        assert got[4] == pytest.approx(want["f"], rel=1e-6), (got, want)
        assert got[6] == want["col"], (got, want)
    assert all(b[4] < a[4] for a, b in zip(rows, rows[1:])), [r[4] for r in rows]
    cols = [r[6] for r in rows]
    assert cols[-1] == m and cols[:11] == list(range(0, 11)) and all(b >= a for a, b in zip(cols, cols[1:])), cols
    assert sum(1 for c in cols if c == m) >= 4, cols       # several iterations with the memory full
    # iterations 2.. (col > 0) take the two-pass route; the col = 20 closed form included
    assert closed_steps >= iters - 3 and three_steps <= 2, (closed_steps, three_steps)
    rows2, _, _ = run()
    assert rows2 == rows       # bit for bit, f and |proj g| included
    print("config 5 full shape, last rows:", rows[-3:])


@pytest.mark.parametrize("case", ["driver2_r32", "quad1000_r32"])
def test_reference_real32_trajectory_through_the_host_entry(env, case):
    """The trajectories the REAL reference's -DREAL32 build produced (tests/golden/*_r32_traj.npz, recorded by
    tests/golden/make_golden.py from oracle/_ref) driven through lbfgsb_hip_setulb_host with real_bytes = 4 --
    exactly the call lbfgsb_module.F90 makes under -DREAL32.  The reference does EVERYTHING in fp32, the
    library keeps fp64 partial sums and host algebra, so this is the tolerance sweep of SURVEY.md a19, on
    the reference's own numbers:
      driver2 (n = 25): call by call, task and the counters (iteration, nfg, nseg, nfree) equal the
        reference's for at least the first third of the run (the two part ways near fp32's floor);
      quad1000 (n = 1000): the first walk already counts 979 segments in fp32 sums, so nseg differs from
        the first iteration on; f per iteration and the nfg column are what is compared.
    f to 1e-2 while it is within four decades of its first value (fp32 noise, amplified by the line
    searches), and the run ends where the reference's ended."""
    import os
    po, la = env["po"], env["la"]
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", case + "_traj.npz"))
    n, m = int(z["n"]), int(z["m"])
    if case.startswith("driver2"):
        p = po.problem_rosenbrock(n, m, float(z["factr"]), float(z["pgtol"]), real=np.float32)
        cols = [29, 33, 32, 37]      # iteration, nfg, nseg of the last walk, nfree
    else:
        p = po.problem_quadratic(n, m, real=np.float32)
        cols = [29, 33]
    assert np.array_equal(p.x0, z["x0"]) and np.array_equal(p.l, z["l"]) and np.array_equal(p.nbd, z["nbd"])
    s = po.State.fresh(p)
    nbd = p.nbd.astype(np.int32)
    ncalls = z["f"].shape[0]
    f_top = float(np.max(np.abs(z["f"])))
    agree = 0
    diverged = False
    for k in range(ncalls):
        la.setulb(n, m, s.x, p.l, p.u, nbd, s.f, s.g, p.factr, p.pgtol, s.wa, s.iwa, s.task, -1,
                  s.csave, s.lsave, s.isave, s.dsave)
        t = s.task_s
        tz = bytes(z["task"][k].tobytes()).decode().rstrip()
        if not diverged:
            same = t == tz and all(int(s.isave[c]) == int(z["isave"][k][c]) for c in cols)
            if same:
                fz = float(z["f"][k])
                if abs(fz) >= 1e-4 * f_top:
                    assert abs(float(s.f[0]) - fz) <= 1e-2 * abs(fz), (case, k, float(s.f[0]), fz)
                agree += 1
            else:
                diverged = True
        if t.startswith("FG"):
            s.f[0] = p.fg(s.x, s.g)
        elif not t.startswith("NEW_X"):
            break
    if s.task_s.startswith("FG") or s.task_s.startswith("NEW_X"):
        from lbfgsb_amd import capi
        capi.load_library().lbfgsb_hip_release_host(s.isave.ctypes.data_as(capi.C.c_void_p))
    assert agree >= ncalls // 3, (case, agree, ncalls)
    assert s.dsave.dtype == np.float32 and float(s.dsave[4]) == pytest.approx(1.1920929e-07)
    # the run got where the reference got: f within fp32's reach of the reference's final value
    f_ref_end = float(z["f"][-1])
    assert float(s.f[0]) <= max(2.0 * f_ref_end, 1e-6 * f_top), (float(s.f[0]), f_ref_end)
