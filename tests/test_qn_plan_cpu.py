"""The tiling plan of the curvature-model operators (lbfgsb_amd/csrc/qn_plan.hpp: which launches a pass over W is made
of, where each of their sums lands, the scatters out of the fetched sums and the pack of an expansion's coefficients)
is host-only integer bookkeeping, and a mistake in it corrupts results without a fault.  tests/qn_plan_check.cpp walks
it for every col in 0 .. 70 and LBFGSB_MAX_M, every block of 1 .. QN_KMAX vectors, the three carries and the expansion
variant against a naive restatement of the rule; here it is built as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a child process (as tests/test_walk_cpu.py does with the walk).  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_against_a_naive_restatement_under_sanitizers():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "qn_plan_check")
    src = os.path.join(HERE, "qn_plan_check.cpp")
    hdr = os.path.join(os.path.dirname(HERE), "lbfgsb_amd", "csrc", "qn_plan.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "qn_plan_check: 1152 cases, 0 failed" in r.stdout, r.stdout[-1500:]
