"""CPU checks of the active-set report (lbfgsb_hip_kkt / lbfgsb_hip_kkt_list): its kernels in the built library's
code objects (no scratch memory; occupancy on record), and the header's LBFGSB_KKT_* indices against the field names
of the Python report."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources():
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(ROOT, "profiles", "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr, kr.collect([os.path.join(ROOT, "lbfgsb_amd", "liblbfgsb_hip.so")])


def test_kkt_kernels_use_no_scratch():
    kr, rows = _resources()
    mine = {kr.short(r["kernel"]): r for r in rows if kr.short(r["kernel"]).startswith("kkt_")}
    table = "; ".join("%s: %d vgpr, %d waves/SIMD" % (k, r["vgpr"], r["waves_per_simd"])
                      for k, r in sorted(mine.items()))
    # the report pass: every subset of the three outputs x vector / scalar rows x the two real kinds
    want = {"kkt_kernel<%s, %d, %s, %s, %s>" % (t, v, a, b, c)
            for t, vs in (("double", (2, 1)), ("float", (4, 1))) for v in vs
            for a in ("true", "false") for b in ("true", "false") for c in ("true", "false")}
    want |= {"kkt_finalize_kernel", "kkt_list_count_kernel", "kkt_list_scan_kernel", "kkt_list_write_kernel"}
    assert set(mine) == want, (set(mine) ^ want, table)
    bad = [k for k, r in mine.items() if r["scratch"] != 0 or r["dyn_stack"] == "true" or r["vgpr_spill"] != 0]
    assert not bad, (bad, table)
    # a streaming pass wants several waves per SIMD to cover the load latency: projgr_kernel runs at 8
    low = [k for k, r in mine.items() if r["waves_per_simd"] < 4]
    assert not low, (low, table)


def test_header_indices_are_the_report_fields():
    from lbfgsb_amd import capi, solver
    hdr = open(os.path.join(ROOT, "include", "lbfgsb_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define LBFGSB_KKT_(\w+) (\d+)", hdr)}
    assert defs.pop("NCNT") == len(capi.KKT_CNT) == 9 and defs.pop("NVAL") == len(capi.KKT_VAL) == 4
    cnt = {k.lower(): v for k, v in defs.items() if k.startswith("N_")}
    val = {k.lower(): v for k, v in defs.items() if not k.startswith("N_")}
    assert cnt == {name: k for k, name in enumerate(capi.KKT_CNT)}
    assert val == {name: k for k, name in enumerate(capi.KKT_VAL)}
    import numpy as np
    rep = solver.KktReport(np.arange(9, dtype=np.int64), np.arange(4, dtype=np.float64) / 2, 0.0, None, None, None)
    for k, name in enumerate(capi.KKT_CNT):
        assert getattr(rep, name) == k
    for k, name in enumerate(capi.KKT_VAL):
        assert getattr(rep, name) == k / 2
    assert capi.PROTOTYPES["lbfgsb_hip_kkt"][1][6].__name__ == "c_double"
    assert len(capi.PROTOTYPES["lbfgsb_hip_kkt"][1]) == 12 and len(capi.PROTOTYPES["lbfgsb_hip_kkt_list"][1]) == 6
