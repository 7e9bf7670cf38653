"""The library's HOST code of the generalized Cauchy point -- the exact replay of the breakpoint walk (solver_walk.inl),
the breakpoint provider with its windows, chunked refills, rank merges and the reference's heap order
(solver_provider.inl), fetch()'s reduction over ranks, import / export of the state -- compiled for the CPU from the
product's own solver.hip, over a host stand-in for the HIP runtime and CPU twins of the kernels this phase launches
(tests/cpu_walk/walk_check.cpp), and run under AddressSanitizer + UndefinedBehaviorSanitizer against the oracle's
lbo_cauchy (reference src/lbfgsb.f90:1157-1532, hpsolb :2079-2157) on several hundred states of random bounded
problems: one rank through the routine door, 2 - 5 ranks as host threads (host merge and device merge of the rank
chunks), every walk in index order and in the reference's heap order, row numbers across 2^31 and 2^32; and task
'START' (errclb, the bound dictionary built by reduced probing passes, active) over 1 - 5 ranks.  GPU sanitizers do
not exist on the pool; this is the buffer-heavy host code they would have been wanted for."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_walk_and_provider_under_sanitizers_against_the_oracle():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "walk_check")
    src = os.path.join(HERE, "cpu_walk", "walk_check.cpp")
    csrc = os.path.join(ROOT, "lbfgsb_amd", "csrc")
    deps = [src, os.path.join(ROOT, "oracle", "lbfgsb_oracle.c")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".inl", ".hpp"))]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        obj_o = os.path.join(out, "oracle_plain.o")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "lbfgsb_oracle.c"),
                               "-o", obj_o])
        obj = os.path.join(out, "walk_check.o")
        # (solver.hip is plain host C++ over the launch interface of kernels.hpp: compiled as C++ by g++, HIP's
        #  headers only for their types; kernels without a CPU twin stay unresolved on purpose)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                               "-I/opt/rocm/include", "-c", src, "-o", obj])
        subprocess.check_call(["g++", "-fsanitize=address,undefined", obj, obj_o, "-o", exe, "-lpthread", "-lm", "-ldl",
                               "-Wl,--unresolved-symbols=ignore-all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    mm = re.search(r"walk_check: (\d+) cases, (\d+) failed, (\d+) stationary-point-on-a-breakpoint, (\d+) multi-rank, "
                   r"(\d+) in heap order, (\d+) walks of more than 256 segments, (\d+) segments in all; rank 0: "
                   r"(\d+) full sorts, (\d+) tie splits replayed", r.stdout)
    assert mm, r.stdout[-1500:]
    cases, failed, degenerate, multi, heap, long_walks, _segs, fullsorts, tiesplits = (int(v) for v in mm.groups())
    assert cases >= 200 and failed == 0
    # task 'START' over 1 - 5 rank threads: the bound dictionary's probing loop ends with the same tables after the
    # same number of collectives on every rank, the code bytes decode to each row's own l, u, nbd, a ninth value
    # makes every rank fall back; active's projection
    ms = re.search(r"walk_check: (\d+) START cases over 1-5 ranks, (\d+) failed", r.stdout)
    assert ms and int(ms.group(1)) >= 60 and int(ms.group(2)) == 0, r.stdout[-1500:]
    assert multi >= 100 and heap >= 80 and long_walks >= 10 and fullsorts >= 1 and tiesplits >= 1
    # the one tolerated class (a stationary point that coincides with a breakpoint to the last bit: the decision
    # rests on the rounding of an n-term sum, walk_check.cpp / DESIGN.md section 7) stays rare
    assert degenerate <= max(3, cases // 50), (degenerate, cases)
    # who owns what on the GPU: the stand-in runtime keeps a table of live device pointers, pinned pointers, events
    # and streams and aborts on a free of the wrong kind or a second free (an abort fails the return code above);
    # every allocating call of lbfgsb_make_solver (default flags; MIRROR_INDEX | FOLLOW_BOUNDS), set_ranks,
    # ensure_sel, qn_alloc and kkt_ready has failed once, was reported, left nothing behind once the context was
    # gone, and the repeated call went through; and when the program ends nothing is live
    ma = re.search(r"walk_check: allocation failures: (\d+) allocations counted, (\d+) cases, (\d+) failed", r.stdout)
    assert ma, r.stdout[-1500:]
    counted, sweep_cases, sweep_failed = (int(v) for v in ma.groups())
    assert sweep_failed == 0 and counted >= 100 and sweep_cases >= counted, r.stdout[-1500:]
    ml = re.search(r"walk_check: (\d+) resources live at exit", r.stdout)
    assert ml and int(ml.group(1)) == 0, r.stdout[-1500:]
