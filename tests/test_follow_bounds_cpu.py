"""LBFGSB_F_FOLLOW_BOUNDS without a GPU: the flag and the new entry points in the header, the library's exports,
the ctypes prototypes and the Python surface."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbfgsb_hip_bounds_changed", "lbfgsb_hip_bounds_stats")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_declares_the_flag_and_the_entry_points():
    h = _read("include", "lbfgsb_hip.h")
    assert re.search(r"LBFGSB_F_FOLLOW_BOUNDS\s*=\s*128\b", h)
    assert re.search(r"int\s+lbfgsb_hip_bounds_changed\s*\(\s*lbfgsb_hip_ctx\s*\*\s*ctx\s*\)\s*;", h)
    d = _read("include", "lbfgsb_hip_debug.h")
    assert re.search(r"int\s+lbfgsb_hip_bounds_stats\s*\(\s*lbfgsb_hip_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*checks\s*,"
                     r"\s*int64_t\s*\*\s*changes\s*,\s*int64_t\s*\*\s*rebuilds\s*\)\s*;", d)
    # the flag does not collide with the others
    vals = [int(v) for v in re.findall(r"LBFGSB_F_\w+\s*=\s*(\d+)", h)]
    assert len(vals) == len(set(vals)) and 128 in vals


def test_library_exports_and_prototypes():
    from lbfgsb_amd import capi
    assert capi.F_FOLLOW_BOUNDS == 128
    for name in NEW:
        assert name in capi.PROTOTYPES, name
    lib = C.CDLL(capi.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_surface():
    import lbfgsb_amd
    sig = inspect.signature(lbfgsb_amd.DeviceSolver.__init__)
    assert "follow_bounds" in sig.parameters and sig.parameters["follow_bounds"].default is False
    assert callable(lbfgsb_amd.DeviceSolver.bounds_changed)
    assert callable(lbfgsb_amd.DeviceSolver.bounds_stats)


def test_null_context_is_refused():
    from lbfgsb_amd import capi
    lib = capi.load_library()
    assert lib.lbfgsb_hip_bounds_changed(None) == capi.E_ARG
    a = C.c_int64()
    assert lib.lbfgsb_hip_bounds_stats(None, C.byref(a), None, None) == capi.E_ARG
