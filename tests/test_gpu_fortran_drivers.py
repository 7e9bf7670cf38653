"""The reference's own test programs (test/driver1.f90, driver2.f90, driver3.f90) are
compiled UNCHANGED against lbfgsb_amd/fortran/lbfgsb_module.F90 (the iso_c_binding face of
the HIP library) and their transcripts are compared with the reference's golden outputs
(test/OUTPUTS/output_90_{1,2,3}, iterate.dat; committed under tests/golden/ref_outputs).

Integer columns must match exactly; floats are printed with 4-6 digits and are compared to
that precision while f is above its rounding floor (the goldens themselves differ between
compilers below ~1e-13); timing lines and list-directed spacing are ignored."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the reference's drivers are built from its sources (oracle/Makefile, target fortran_drivers) under oracle/_ref/;
# examples/driver_dev.f90 is the library's own (lbfgsb_amd/fortran/build)
DRIVERS = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "fortran")
BUILD = os.path.join(DRIVERS, "build")
# the same module and drivers compiled with -fdefault-integer-8 (8-byte INTEGER and LOGICAL: n, m, nbd,
# iwa, isave, lsave, iprint), the build BASELINE.md section 3 calls mandatory for n = 1e8
BUILD_I8 = os.path.join(DRIVERS, "build_i8")
BUILDS = [pytest.param(BUILD, id="int32"), pytest.param(BUILD_I8, id="int64")]
GOLD = os.path.join(HERE, "golden", "ref_outputs")

NUM = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([DEde][+-]?\d+)?$")


def tokens(line):
    return line.replace("=", " = ").split()


def is_num(t):
    return bool(NUM.match(t))


def val(t):
    return float(t.upper().replace("D", "E"))


def significant(lines):
    out = []
    for ln in lines:
        s = ln.strip()
        if not s or "time" in s.lower() or "seconds" in s.lower():
            continue
        out.append(s)
    return out


def compare(got, gold, rtol=3e-3, floor=1e-10):
    got, gold = significant(got), significant(gold)
    assert len(got) == len(gold), "line count %d vs %d" % (len(got), len(gold))
    for a, b in zip(got, gold):
        ta, tb = tokens(a), tokens(b)
        assert len(ta) == len(tb), (a, b)
        below_floor = False
        for x, y in zip(ta, tb):
            if x == y:
                continue
            assert is_num(x) and is_num(y), (a, b)
            if "." not in x and "." not in y and "D" not in x.upper() and "E" not in x.upper():
                if below_floor:
                    continue
                assert int(x) == int(y), (a, b)       # integer column
                continue
            vx, vy = val(x), val(y)
            if abs(vy) < floor:
                below_floor = True
                continue
            assert abs(vx - vy) <= rtol * abs(vy), (a, b)


def run_driver(name, cwd, build=BUILD):
    exe = os.path.join(build, name)
    if not os.path.exists(exe):
        pytest.skip("%s not built (needs the reference tree + amdflang at build time)" % exe)
    r = subprocess.run([exe], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("build", BUILDS)
def test_driver1_transcript_and_iteration_file(tmp_path, build):
    out = run_driver("driver1", str(tmp_path), build)
    compare(out, open(os.path.join(GOLD, "output_90_1")).read().splitlines())
    itf = open(os.path.join(str(tmp_path), "driver1_output.txt")).read().splitlines()
    compare(itf, open(os.path.join(GOLD, "iterate.dat")).read().splitlines())
    assert any("CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH" in ln for ln in out)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name,gold", [("driver2", "output_90_2"), ("driver3", "output_90_3")])
def test_driver23_transcripts(tmp_path, name, gold, build):
    out = run_driver(name, str(tmp_path), build)
    want = open(os.path.join(GOLD, gold)).read().splitlines()
    ia = [ln for ln in out if ln.strip().startswith("Iterate")]
    ib = [ln for ln in want if ln.strip().startswith("Iterate")]
    assert len(ia) == len(ib)                       # same number of iterations to the user stop
    checked = 0
    for a, b in zip(ia, ib):
        ta, tb = tokens(a), tokens(b)
        fb = val(tb[7])
        if fb < 1e-9:                               # below this the goldens are compiler noise
            break
        assert ta[1] == tb[1] and ta[4] == tb[4], (a, b)   # iteration number, nfg
        assert abs(val(ta[7]) - fb) <= 1e-4 * fb, (a, b)
        checked += 1
    assert checked >= 20
    assert any("THE PROJECTED GRADIENT IS SUFFICIENTLY SMALL" in ln for ln in out)


@pytest.mark.parametrize("problem,n,m,iprint,iters", [
    ("rosen", 7, 5, 101, 6),       # every vector dump: L, X0, U, Cauchy X, X, G, final X
    ("quadmix", 12, 4, 100, 6),    # per-segment report of the walk, variables entering the free set
    ("quadmix", 12, 4, 99, 6),
])
def test_debug_transcripts_iprint_99_100_101(tmp_path, problem, n, m, iprint, iters):
    """src/lbfgsb.f90's debugging output (iprint >= 99: CAUCHY/SUBSM banners, breakpoint
    counts, the per-segment report, free-set changes, n-vector dumps) against the text the real
    reference printed for the same run (tests/golden/ref_outputs/iprint*.txt, generated by
    tests/golden/make_golden.py; list-directed spacing ignored, numbers to print precision)."""
    worker = os.path.join(HERE, "_iprint_worker.py")
    r = subprocess.run([os.sys.executable, worker, "gpu", problem, str(n), str(m), str(iprint),
                        str(iters)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = open(os.path.join(GOLD, "iprint%d_%s_n%d_m%d.txt" % (iprint, problem, n, m))).read()

    # (breakpoints with EQUAL t: under iprint >= 99 the walk runs in the reference's heap order from
    #  its start, so the "Variable k is fixed." lines come in the reference's own order)
    compare(r.stdout.splitlines(), want.splitlines())


def test_driver1_as_a_plain_c_program(tmp_path):
    """examples/driver1.c: test/driver1.f90 written in C over the host-pointer entry of the C ABI
    (the reference's own argument list), built with the system C compiler and linked against the
    library.  Must reach the reference's result: CONVERGENCE by relative reduction after 23
    iterations, f = 1.08349008343e-09 (test/OUTPUTS/output_90_1)."""
    import shutil
    root = os.path.dirname(HERE)
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "driver1_c")
    subprocess.check_call([cc, "-std=c99", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "driver1.c"), "-L" + os.path.join(root, "lbfgsb_amd"),
                           "-llbfgsb_hip", "-Wl,-rpath," + os.path.join(root, "lbfgsb_amd"), "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    out = r.stdout
    assert "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH" in out, out
    mm = re.search(r"iterations = (\d+)\s+nfg = (\d+)\s+f = (\S+)", out)
    assert mm, out
    assert int(mm.group(1)) == 23 and int(mm.group(2)) == 28, out
    assert abs(float(mm.group(3)) - 1.0834900834300614e-09) <= 1e-6 * 1.0834900834300614e-09, out


# random problems of tests/test_gpu_fuzz.py at one iprint each; what the real reference printed for them is on file
# (tests/golden/ref_outputs/live_*, recorded from oracle/_ref by tests/golden/make_golden.py)
LIVE_CASES = [
    ("fuzz:90001:400:1:13", 1), ("fuzz:90003:60:1:13", 99), ("fuzz:90004:40:1:13", 100), ("fuzz:90005:16:1:13", 101),
    ("fam:linear:91003", 1), ("fam:linear:91002", 99), ("fam:rosenchain:91003", 100), ("fam:scaled:91000", 0),
]


def live_case_name(spec, iprint):
    """file name stem of a LIVE_CASES transcript: <stem>.txt (stdout), <stem>_iterate.txt (the iteration file)"""
    return "live_%s_iprint%d" % (spec.replace(":", "_"), iprint)


@pytest.mark.parametrize("spec,iprint", LIVE_CASES)
def test_transcripts_against_the_live_reference(tmp_path, spec, iprint):
    """Printed output on problems the driver transcripts do not cover: the library through the reference-shaped
    host entry runs a random problem at a given iprint, and its stdout and iteration file are compared word for
    word, numbers to print precision, with what the real reference (oracle/_ref) printed for the same run
    (profiles/scripts/transcript_sweep.py runs hundreds of these; the problems here are ones whose trajectory
    does not leave the reference's by rounding drift)."""
    worker = os.path.join(HERE, "_iprint_worker.py")
    r = subprocess.run([os.sys.executable, worker, "gpu", spec, "0", "0", str(iprint), "25"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    itf = tmp_path / "iterate.dat"
    got = (r.stdout.splitlines(), itf.read_text().splitlines() if itf.exists() else [])
    stem = os.path.join(GOLD, live_case_name(spec, iprint))
    want = (open(stem + ".txt").read().splitlines(), open(stem + "_iterate.txt").read().splitlines())
    assert len(want[0]) > 3
    compare(got[0], want[0])
    compare(got[1], want[1])


def test_device_pointer_example_with_the_callers_own_kernel(tmp_path):
    """examples/bounded_quadratic_dev.hip: a caller that keeps x, g, l, u, nbd on the GPU, evaluates its objective
    with its OWN HIP kernel on the solver's stream and drives lbfgsb_hip_setulb_dev_pp (ping-pong iterate
    buffers) -- built with hipcc against the library, run at n = 200 000, and compared row by row with the
    oracle on the same problem (BASELINE.md section 3's separable bounded quadratic)."""
    from oracle import pyoracle as po
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "bounded_quadratic_dev")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "bounded_quadratic_dev.hip"),
                           "-L" + os.path.join(root, "lbfgsb_amd"), "-llbfgsb_hip",
                           "-Wl,-rpath," + os.path.join(root, "lbfgsb_amd"), "-o", exe])
    n, m, iters = 200_000, 10, 20
    r = subprocess.run([exe, str(n), str(m), str(iters)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    got = [re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?", ln) for ln in r.stdout.splitlines() if ln.startswith("iterate")]
    p = po.problem_quadratic(n, m)
    rows = []
    po.run(po.Engine("oracle"), p, max_iter=iters,
           snapshot=lambda k, s: rows.append((int(s.isave[29]), int(s.isave[33]), int(s.isave[32]), int(s.isave[37]),
                                              float(s.f[0]))) if s.task_s.startswith("NEW_X") else None)
    assert len(got) == len(rows) == iters
    for a, b in zip(got, rows):
        assert [int(v) for v in a[:4]] == list(b[:4]), (a, b)
        assert abs(float(a[4]) - b[4]) <= 1e-10 * abs(b[4]), (a, b)
    assert "STOP: ITERATION LIMIT" in r.stdout


# ---------------------------------------------------------------------------------------------
# The -DREAL32 Fortran face (src/lbfgsb_kinds_module.F90:29-37, README.md:23-35): lbfgsb_module.F90
# compiled with -DREAL32 (wp = real32, real_bytes = 4 handed to the library), the reference's three
# drivers compiled UNCHANGED against it (they take their kind from the module), 4- and 8-byte default
# integers.  The transcripts are compared with what the reference's OWN REAL32 build printed for the
# same programs (tests/golden/ref_outputs/output_r32_*, tests/golden/make_golden_r32_drivers.py).
# The reference does everything in fp32; the library keeps fp32 storage and kernels but fp64 partial
# sums and host algebra, so the bar is the REAL32 tolerance sweep's (tests/test_gpu_real32.py): the
# same decisions while the two agree, f to fp32 noise -- and the behaviour SURVEY.md a19 documents:
# driver1 stops after ONE iteration (factr * epsmch = 1.19 > any relative reduction), driver2 / driver3
# run into fp32's floor near f ~ 1e-12 instead of reaching their |proj g| < 1e-10 stop.
# ---------------------------------------------------------------------------------------------
BUILD_R32 = os.path.join(DRIVERS, "build_r32")
BUILD_R32_I8 = os.path.join(DRIVERS, "build_r32_i8")
BUILDS_R32 = [pytest.param(BUILD_R32, id="real32-int32"), pytest.param(BUILD_R32_I8, id="real32-int64")]


@pytest.mark.parametrize("build", BUILDS_R32)
def test_driver1_real32_stops_after_one_iteration(tmp_path, build):
    out = run_driver("driver1", str(tmp_path), build)
    gold = open(os.path.join(GOLD, "output_r32_1")).read().splitlines()
    # same transcript as the reference's REAL32 build: integer columns exactly, floats to fp32 noise
    compare(out, gold, rtol=2e-4)
    assert any("CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH" in ln for ln in out)
    summary = [tokens(ln) for ln in significant(out) if ln.split()[:1] == ["25"]]
    assert summary and summary[0][1] == "1" and summary[0][2] == "5"      # Tit = 1, Tnf = 5
    itf = open(os.path.join(str(tmp_path), "driver1_output.txt")).read().splitlines()
    compare(itf, open(os.path.join(GOLD, "iterate_r32.dat")).read().splitlines(), rtol=2e-4)
    assert any("Machine precision = 1.192D-07" in ln for ln in itf)


@pytest.mark.parametrize("build", BUILDS_R32)
@pytest.mark.parametrize("name,gold", [("driver2", "output_r32_2"), ("driver3", "output_r32_3")])
def test_driver23_real32_transcripts(tmp_path, name, gold, build):
    out = run_driver(name, str(tmp_path), build)
    want = open(os.path.join(GOLD, gold)).read().splitlines()
    ia = [tokens(ln) for ln in out if ln.strip().startswith("Iterate")]
    ib = [tokens(ln) for ln in want if ln.strip().startswith("Iterate")]
    assert len(ia) >= 20 and len(ib) >= 20
    # while both runs are far above fp32's floor they are the same run: iteration, nfg, f to fp32 noise
    # (the reference's all-fp32 sums against fp64 partial sums, amplified from one line search to the
    #  next: 1e-2 on f until f has lost four decades -- the bar of tests/test_gpu_real32.py)
    f0 = val(ib[0][7])
    same = 0
    for a, b in zip(ia, ib):
        fb = val(b[7])
        if fb < 1e-4 * f0:
            break
        assert a[1] == b[1] and a[4] == b[4], (a, b)
        assert abs(val(a[7]) - fb) <= 1e-2 * fb, (a, b)
        same += 1
    assert same >= 5, same
    # both end at fp32's floor, far from the drivers' |proj g| < 1e-10 stop: f has fallen by > 12 decades
    # and the run ended by itself (ABNORMAL_TERMINATION_IN_LNSRCH / a rounding-level stop), not by the
    # user's test
    f_end = val(ia[-1][7])
    assert f_end <= 1e-10 * f0, (f_end, f0)
    assert f_end >= 0.0
    assert not any("THE PROJECTED GRADIENT IS SUFFICIENTLY SMALL" in ln for ln in out)
    # f decreases monotonically over the printed iterations (no garbage from a mis-sized kind)
    fs = [val(t[7]) for t in ia]
    assert all(b <= a * (1 + 1e-6) for a, b in zip(fs, fs[1:])), fs


# ---------------------------------------------------------------------------------------------
# The Fortran DEVICE-POINTER face (lbfgsb_module: lbfgsb_create / setulb_dev / setulb_dev_pp /
# lbfgsb_objective, extensions beside the unchanged setulb) and examples/driver_dev.f90 -- driver2's loop
# (test/driver2.f90:66-195) on hipMalloc'ed buffers with the built-in quadratic.  The Fortran caller must get
# the very iteration the Python and C callers get -- bit for bit -- and the throughput bench.py reports.
# ---------------------------------------------------------------------------------------------
ROW = re.compile(r"^\s*Iterate\s+(\d+)\s+nfg =\s*(\d+)\s+f =\s*(\S+)\s+\|proj g\| =\s*(\S+)\s+nseg =\s*(\d+)\s+"
                 r"nfree =\s*(\d+)\s+([0-9A-F]{16})\s+([0-9A-F]{16})\s*$")


def run_driver_dev(n, m, iters, warm, mode="pp", compact=False):
    exe = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "fortran", "build", "driver_dev")
    if not os.path.exists(exe):
        pytest.skip("%s not built (needs amdflang at build time)" % exe)
    r = subprocess.run([exe, str(n), str(m), str(iters), str(warm), mode] + (["compact"] if compact else []),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    rows = []
    for ln in r.stdout.splitlines():
        mm = ROW.match(ln)
        if mm:
            rows.append((int(mm.group(1)), int(mm.group(2)), int(mm.group(5)), int(mm.group(6)),
                         int(mm.group(7), 16), int(mm.group(8), 16)))
    rate = re.search(r"RATE n=(\d+) iterations_timed=(\d+) iters_per_sec=\s*(\S+) ms_per_iter=\s*(\S+)", r.stdout)
    assert rate, r.stdout[-1500:]
    return rows, float(rate.group(3)), r.stdout


def python_rows(n, m, iters, warm, pp=True, compact=False):
    """the same run through the Python face: (rows with the bit patterns of f and |proj g|, it/s over the
    iterations warm+1 .. iters, clocked at the NEW_X returns as driver_dev clocks them)"""
    import time
    import numpy as np
    import torch
    import lbfgsb_amd as la
    sol = la.DeviceSolver(n, m, same_stream_objective=pp, defer_lnsrch=pp,
                          options={"compact_w": 1} if compact else None)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    g = torch.zeros_like(x)
    xs, gs = ([x, torch.zeros_like(x)], [g, torch.zeros_like(g)]) if pp else ([x], [g])
    l, u = torch.full_like(x, -1.0), torch.full_like(x, 1.0)
    nbd = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    rows, cur, t0, t1 = [], 0, None, None
    while True:
        if pp:
            t, cur = sol.setulb_pp(xs, l, u, nbd, gs, 0.0, 0.0)
        else:
            t = sol.setulb(x, l, u, nbd, g, 0.0, 0.0)
        if t.startswith("FG"):
            if pp:
                sol.objective(0, xs[cur], gs[cur], deferred=True)
            else:
                sol.f[0] = sol.objective(0, x, g)
        elif t.startswith("NEW_X"):
            it = int(sol.isave[29])
            if it == warm:
                t0 = time.perf_counter()
            if it == iters:
                t1 = time.perf_counter()
            rows.append((it, int(sol.isave[33]), int(sol.isave[32]), int(sol.isave[37]),
                         int(np.float64(sol.f[0]).view(np.int64)), int(np.float64(sol.dsave[12]).view(np.int64))))
            if it >= iters:
                break
        else:
            break
    sol.close()
    del x, g, xs, gs, l, u, nbd
    torch.cuda.empty_cache()
    return rows, (iters - warm) / (t1 - t0)


@pytest.mark.parametrize("mode", ["pp", "classic"])
def test_driver_dev_rows_equal_the_python_path_bit_for_bit(mode):
    """n = 1e6, m = 10, 30 iterations: iteration, nfg, nseg, nfree and the BIT PATTERNS of f and |proj g| at every
    NEW_X return -- the Fortran caller on device pointers (ping-pong + deferred line-search set-up as bench.py
    drives it; the classic in-place entry as an ordinary caller would) against the Python caller of the same
    entry: one library, one iteration, whatever the host language."""
    n, m, iters, warm = 1_000_000, 10, 30, 12
    rows_f, _rate, out = run_driver_dev(n, m, iters, warm, mode)
    rows_p, _ = python_rows(n, m, iters, warm, pp=(mode == "pp"))
    assert len(rows_f) == len(rows_p) == iters, out[-1500:]
    assert rows_f == rows_p
    assert rows_f[0][2] == 976_721 and rows_f[1][3] == 499_997      # SURVEY.md 8c anchors of this problem


def test_driver_dev_reaches_the_bench_throughput_at_n1e8():
    """The headline workload (n = 1e8, m = 10, fp64) from a Fortran program: iterations 13 .. 32 clocked at the
    NEW_X returns, against the Python caller bench.py uses, same box, back to back.  The Fortran face adds a
    few hundred nanoseconds of marshalling per call: its rate must be within 3 % of Python's (in practice it is
    a little faster: no interpreter between the calls)."""
    import torch
    free_b, _tot = torch.cuda.mem_get_info()
    if free_b < 40 * (1 << 30):
        pytest.skip("needs ~30 GB of HBM")
    n, m, iters, warm = 100_000_000, 10, 32, 12
    # (both with the option compact_w, as bench.py runs: lbfgsb_set_option in the Fortran program)
    rows_f, rate_f, out = run_driver_dev(n, m, iters, warm, "pp", compact=True)
    rows_p, rate_p = python_rows(n, m, iters, warm, pp=True, compact=True)
    assert rows_f == rows_p
    assert rows_f[0][2] == 97_671_921 and rows_f[1][3] == 49_999_496
    if rate_f < 0.97 * rate_p:
        # (a box of the pool stalls for tens of ms now and then, and 20 iterations are 0.14 s: one more run of each,
        #  the better of the two counts)
        rate_f = max(rate_f, run_driver_dev(n, m, iters, warm, "pp", compact=True)[1])
        rate_p = max(rate_p, python_rows(n, m, iters, warm, pp=True, compact=True)[1])
    assert rate_f >= 0.97 * rate_p, (rate_f, rate_p)
    print("driver_dev %.2f it/s, python %.2f it/s" % (rate_f, rate_p))
