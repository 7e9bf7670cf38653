"""The kernels of the quadratic forms and draw densities of the curvature model, read from the code objects of the
built library (profiles/scripts/kernel_resources.py, as tests/test_qn_root_cpu.py does; needs no GPU): every
instantiation of the two new kernels (qn_wtd_kernel, qn_wtzz_kernel) and of the two whose bodies now carry the flags
(qn_wtv_kernel, qn_wtz_kernel) has no private segment and no dynamic stack, every instantiation of the plain
kernels that the launches dispatch to is still there under its name, and at the shapes DESIGN.md section 10c quotes
(fp64, 10 columns) a flagged kernel runs at its plain counterpart's waves per SIMD."""
import importlib.util
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(ROOT, "profiles", "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.collect([os.path.join(ROOT, "lbfgsb_amd", "liblbfgsb_hip.so")])
    return {kr.short(r["kernel"]): r for r in rows}


def _shapes():
    """(T, MC, K, V, CW) of the dispatch in k_qn_common.hpp: tiles of 5, 10, 16 columns, blocks of 1, 2, 4 vectors
    (4 up to 10 columns), one or two rows per lane in natural order, the layout for fp64 up to 10 columns"""
    for t, mc in itertools.product(("double", "float"), (5, 10, 16)):
        for k in (1, 2, 4) if mc <= 10 else (1, 2):
            yield t, mc, k, 1, "false"
            yield t, mc, k, 2, "false"
            if t == "double" and mc <= 10:
                yield t, mc, k, 1, "true"


def _names(kernel, nflags):
    for t, mc, k, v, cw in _shapes():
        for flags in itertools.product(("false", "true"), repeat=nflags):
            if kernel == "qn_wtd_kernel" and flags[1:] == ("false", "false"):
                continue  # (no center, no squared norm: launch_qn_wtd hands that to qn_wtv_kernel)
            yield "%s<%s>" % (kernel, ", ".join([t, str(mc), str(k), str(v), cw] + list(flags)))


@pytest.mark.parametrize("kernel,nflags", [("qn_wtv_kernel", 2), ("qn_wtz_kernel", 1), ("qn_wtd_kernel", 3),
                                           ("qn_wtzz_kernel", 1)])
def test_quad_kernels_present_and_without_scratch(kernels, kernel, nflags):
    """flags after (T, MC, K, V, CW): qn_wtv VSLOT, NT; qn_wtz and qn_wtzz NT; qn_wtd NT, CEN, DD"""
    want = set(_names(kernel, nflags))
    have = {name for name in kernels if name.startswith(kernel + "<")}
    assert want <= have, sorted(want - have)[:5]
    assert len(want) == {2: 152, 1: 76, 3: 228}[nflags]
    if kernel == "qn_wtd_kernel":
        assert have == want, sorted(have - want)[:5]  # no copy of the plain pass under the new name
    bad = [(name, kernels[name]["scratch"], kernels[name]["dyn_stack"]) for name in sorted(have)
           if kernels[name]["scratch"] != 0 or kernels[name]["dyn_stack"] == "true"]
    assert not bad, bad
    assert all(kernels[name]["vgpr"] <= 512 for name in have)



def test_flagged_kernels_at_the_headline_shapes(kernels):
    """fp64, a tile of 10 columns, the shapes a launch picks (two rows per lane at K = 1, one at K = 4, the layout):
    the K squared norms and the center cost a few registers (at most 12) and no wave per SIMD"""
    for k, v, cw in ((1, 2, "false"), (4, 1, "false"), (4, 1, "true")):
        head = "double, 10, %d, %d, %s" % (k, v, cw)
        for nt in ("false", "true"):
            pairs = [(kernels["qn_wtz_kernel<%s, %s>" % (head, nt)], kernels["qn_wtzz_kernel<%s, %s>" % (head, nt)])]
            plain = kernels["qn_wtv_kernel<%s, false, %s>" % (head, nt)]
            pairs += [(plain, kernels["qn_wtd_kernel<%s, %s, %s, %s>" % (head, nt, cen, dd)])
                      for cen, dd in (("true", "true"), ("true", "false"), ("false", "true"))]
            for a, b in pairs:
                assert b["waves_per_simd"] == a["waves_per_simd"], (head, nt)
                assert 0 <= b["vgpr"] - a["vgpr"] <= 12, (head, nt, a["vgpr"], b["vgpr"])
