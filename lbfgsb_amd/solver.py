"""Host-side mirror of the reference interface for the hot path.

`setulb(...)` has the reference's argument list (src/lbfgsb.f90:88-89) with numpy
arrays standing in for the Fortran arrays; it calls the C ABI's host-pointer form
exactly as the Fortran shim does.  `DeviceSolver` is the device-resident form used
by bench.py and the parity tests: x, l, u, nbd, g are torch tensors on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from .capi import LbfgsbError, check, load_library

TASK_LEN = 60


def wa_length(n: int, m: int) -> int:
    """reference src/lbfgsb.f90:146"""
    return 2 * m * n + 5 * n + 11 * m * m + 8 * m


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a.data_ptr()))  # torch tensor


def pad60(s: str) -> np.ndarray:
    b = s.encode()[:TASK_LEN]
    return np.frombuffer(b + b" " * (TASK_LEN - len(b)), dtype=np.uint8).copy()


def task_str(a) -> str:
    return bytes(np.asarray(a).tobytes()).decode("ascii", "replace").rstrip()


def setulb(n, m, x, l, u, nbd, f, g, factr, pgtol, wa, iwa, task, iprint, csave, lsave, isave,
           dsave, iteration_file: Optional[str] = None, mirror: bool = False):
    """Reference `setulb` (src/lbfgsb.f90:88).  All arrays are numpy and are updated in
    place: x, g, wa (real kind), f (1 element), iwa/isave/lsave (int32), task/csave
    (60 uint8, blank padded), dsave (real kind).  mirror=True exports the complete
    reference layout of wa/iwa after every return (parity tests)."""
    lib = load_library()
    real_bytes = x.dtype.itemsize
    check(lib.lbfgsb_hip_setulb_host(
        n, m, _p(x), _p(l), _p(u), _p(nbd), _p(f), _p(g), float(factr), float(pgtol), _p(wa),
        _p(iwa), _p(task), int(iprint), _p(csave), _p(lsave), _p(isave), _p(dsave),
        iteration_file.encode() if iteration_file else None, real_bytes, 1 if mirror else 0))


class DeviceSolver:
    """One rank of the device-resident solver.  Tensors stay on the GPU; only the
    60-byte task, f and the isave/dsave scalars cross PCIe."""

    def __init__(self, n_local: int, m: int, n_global: Optional[int] = None, row0: int = 0,
                 real32: bool = False, mirror_index: bool = False, device: int = 0, stream=None,
                 same_stream_objective: bool = False, parallel_gcp: bool = False,
                 exact_ties: bool = True, index_ties: bool = False, options: Optional[dict] = None,
                 defer_lnsrch: bool = False, stream_ordered: bool = False, follow_bounds: bool = False):
        self.lib = load_library()
        # LBFGSB_F_DEFER_LNSRCH returns 'FG_LNSRCH' without waiting for the pass that writes the trial point
        # (it implies LBFGSB_F_NO_RETURN_SYNC): only a caller whose objective runs on the solver's OWN stream
        # may use it -- one that evaluates on torch's current stream would read x while it is being written
        # stream_ordered=True: the objective runs on torch's CURRENT stream and is ordered against the solver's stream
        # with events in both directions -- after every 'FG...' return torch's stream is made to wait for the trial
        # point (lbfgsb_hip_return_event), before every 'FG...' re-entry the solver's stream for g
        # (lbfgsb_hip_wait_stream): no host sync at an FG return either, so such a caller may defer as well.
        # f travels as a device scalar (set_f_device) or as a host float (sol.f[0] = float(...), which syncs torch).
        if defer_lnsrch and not (same_stream_objective or stream_ordered):
            raise ValueError("defer_lnsrch=True needs same_stream_objective=True or stream_ordered=True: the flag "
                             "skips the host sync at every FG_LNSRCH return, so f,g must be evaluated on the "
                             "solver's stream (DeviceSolver.objective / DeviceSolver.stream) or on a stream that is "
                             "ordered behind it with events (stream_ordered)")
        self.same_stream_objective = bool(same_stream_objective)
        self.stream_ordered = bool(stream_ordered) and not self.same_stream_objective
        self.n, self.m = int(n_local), int(m)
        self.device = int(device)
        self.n_global = int(n_global if n_global is not None else n_local)
        self.row0 = int(row0)
        self.real = np.float32 if real32 else np.float64
        flags = (capi.F_REAL32 if real32 else 0) | (capi.F_MIRROR_INDEX if mirror_index else 0)
        flags |= capi.F_NO_RETURN_SYNC if (same_stream_objective or stream_ordered) else 0
        flags |= capi.F_PARALLEL_GCP if parallel_gcp else 0  # opt-in, see include/lbfgsb_hip.h
        # a walk that ends inside a group of equal breakpoints is replayed in the reference's heap
        # order by default; index_ties=True (or exact_ties=False) opts out (include/lbfgsb_hip.h)
        flags |= capi.F_INDEX_TIES if (index_ties or not exact_ties) else 0
        # the caller evaluates f,g on the solver's stream and re-enters with nothing in between: the
        # line-search set-up's sums ride with the next call's fetch (include/lbfgsb_hip.h)
        flags |= capi.F_DEFER_LNSRCH if defer_lnsrch else 0
        # l, u, nbd may be edited between calls: every entry compares them with the snapshot (include/lbfgsb_hip.h)
        flags |= capi.F_FOLLOW_BOUNDS if follow_bounds else 0
        h = C.c_void_p()
        sp = C.c_void_p(int(stream)) if stream else None
        check(self.lib.lbfgsb_hip_create(self.n, self.n_global, self.row0, self.m, flags, device,
                                         sp, C.byref(h)))
        self.h = h
        self.task = pad60("START")
        self.csave = pad60("")
        self.lsave = np.zeros(4, np.int32)
        self.isave = np.zeros(44, np.int32)
        self.dsave = np.zeros(29, np.float64)
        self.f = np.zeros(1, np.float64)
        self._cur = C.c_int32(0)
        self._cur_ref = C.byref(self._cur)
        self._keep = []
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name: str, value: float):
        """measurement / test switch of this context (lbfgsb_hip_set_option)"""
        if name == "defer_lnsrch" and float(value) != 0.0 and not (self.same_stream_objective or self.stream_ordered):
            raise ValueError("option defer_lnsrch needs a context created with same_stream_objective=True or "
                             "stream_ordered=True")
        check(self.lib.lbfgsb_hip_set_option(self.h, name.encode(), float(value)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.lbfgsb_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- multi-GPU ----
    def init_rccl(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(unique_id, 128)
        check(self.lib.lbfgsb_hip_comm_init_rccl(self.h, buf, rank, nranks))

    @staticmethod
    def rccl_unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        check(lib.lbfgsb_hip_rccl_unique_id(buf))
        return buf.raw

    def init_host_reducer(self, allreduce, rank: int, nranks: int, allgather=None):
        """allreduce(np_view, nsum, nmin, nmax) reduces the fp64 view in place over ranks
        (sums | mins | maxes).  allgather(np_uint8_local) -> rank-major concatenation."""
        def _ar(user, buf, nsum, nmin, nmax):
            try:
                k = nsum + nmin + nmax
                view = np.ctypeslib.as_array(buf, shape=(k,))
                allreduce(view, nsum, nmin, nmax)
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1

        def _ag(user, inp, out, nbytes):
            try:
                world = nranks
                src = np.ctypeslib.as_array(C.cast(inp, C.POINTER(C.c_uint8)), shape=(nbytes,))
                dst = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)),
                                            shape=(nbytes * world,))
                dst[:] = allgather(src)
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1
        cb_ar = capi.ALLREDUCE_FN(_ar)
        cb_ag = capi.ALLGATHER_FN(_ag) if allgather is not None else C.cast(None, capi.ALLGATHER_FN)
        self._keep += [cb_ar, cb_ag]
        check(self.lib.lbfgsb_hip_comm_init_host(self.h, cb_ar, cb_ag, None, rank, nranks))

    # ---- setulb, device-pointer form ----
    @property
    def task_s(self) -> str:
        return task_str(self.task)

    def set_task(self, s: str):
        self.task[:] = pad60(s)

    def wait_stream(self, stream=None):
        """Order the solver's stream after everything queued so far on `stream` (default: torch's
        current stream) without blocking the host (lbfgsb_hip_wait_stream)."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        check(self.lib.lbfgsb_hip_wait_stream(self.h, C.c_void_p(int(stream))))

    def release_to_stream(self, stream=None):
        """Make `stream` (default: torch's current stream) wait for everything the last call queued on the solver's
        stream -- the trial point of an 'FG...' return included -- without blocking the host
        (lbfgsb_hip_return_event)."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        check(self.lib.lbfgsb_hip_return_event(self.h, C.c_void_p(int(stream)), 1, None))

    def set_f_device(self, f_dev, stream=None):
        """The objective value as a 0-d / 1-element float64 CUDA tensor produced on `stream` (default: torch's current
        stream): it reaches the host with the next setulb call's own fetch (lbfgsb_hip_f_device) -- no .item()."""
        import torch
        if not (f_dev.is_cuda and f_dev.dtype == torch.float64 and f_dev.numel() == 1):
            raise TypeError("set_f_device needs a one-element float64 CUDA tensor")
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        self._keep_f = f_dev          # (alive until the next call has fetched it)
        check(self.lib.lbfgsb_hip_f_device(self.h, C.c_void_p(f_dev.data_ptr()), C.c_void_p(int(stream)), 1))

    @property
    def stream(self) -> int:
        """the hipStream_t every kernel of this context runs on"""
        return int(self.lib.lbfgsb_hip_get_stream(self.h) or 0)

    # The small caller arrays of a context (task, csave, lsave, isave, dsave, f) live as long as the
    # context and are only ever written in place: their addresses are taken once.  (Per call the wrapper
    # then costs a few microseconds instead of ~20: at n = 1e6 an iteration is 150 us, and the NEW_X
    # return -> re-entry sits on the path during which the device waits for the host.)
    # (The cache is keyed on the array OBJECTS themselves, compared by identity, and keeps them alive: a
    #  replaced array -- sol.isave = saved.copy() in a checkpoint / restore flow -- is always noticed; an id()
    #  alone can be reused by CPython for a new object at another address.)
    _OWN_SPEC = (("f", np.float64, 1), ("task", np.uint8, 60), ("csave", np.uint8, 60), ("lsave", np.int32, 4),
                 ("isave", np.int32, 44), ("dsave", np.float64, 29))

    def _own_ptrs(self):
        arrs = (self.f, self.task, self.csave, self.lsave, self.isave, self.dsave)
        held = getattr(self, "_own_arrs", None)
        if held is None or any(a is not b for a, b in zip(arrs, held)):
            for a, (nm, dt, ln) in zip(arrs, self._OWN_SPEC):
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.size >= ln and a.flags["C_CONTIGUOUS"]
                        and a.flags["WRITEABLE"]):
                    raise TypeError("DeviceSolver.%s must be a writable contiguous %s array of >= %d elements"
                                    % (nm, np.dtype(dt).name, ln))
            self._own_arrs = arrs
            self._own = tuple(a.ctypes.data for a in arrs)
        return self._own

    @staticmethod
    def _addr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def _before_call(self, first):
        """stream ordering of the caller's tensors (include/lbfgsb_hip.h, "Stream ordering")"""
        if isinstance(first, np.ndarray):
            return
        head = bytes(self.task[:5])
        if head == b"START":
            # the solver runs on its own stream: make sure the caller's tensors are materialised
            import torch
            torch.cuda.synchronize()
        elif head[:2] == b"FG" and not self.same_stream_objective:
            # g (and x) were produced on torch's current stream: the solver's stream must not
            # read them before that work is done
            self.wait_stream()

    def setulb(self, x, l, u, nbd, g, factr: float, pgtol: float, iprint: int = -1) -> str:
        self._before_call(x)
        pf, pt, pc, pl, pi, pd = self._own_ptrs()
        a = self._addr
        check(self.lib.lbfgsb_hip_setulb_dev(self.h, a(x), a(l), a(u), a(nbd), pf, a(g), float(factr),
                                             float(pgtol), pt, int(iprint), pc, pl, pi, pd))
        if self.stream_ordered and bytes(self.task[:2]) == b"FG" and not isinstance(x, np.ndarray):
            self.release_to_stream()   # (the caller's stream may read the trial point from here on)
        return self.task_s

    def setulb_pp(self, xs, l, u, nbd, gs, factr: float, pgtol: float, iprint: int = -1):
        """Ping-pong form (lbfgsb_hip_setulb_dev_pp): xs = (x0, x1), gs = (g0, g1) -- two pairs of
        device buffers, x0 holding the starting point.  -> (task, cur): evaluate f, g at xs[cur] into
        gs[cur] on 'FG...'; xs[cur], gs[cur] are the iterate and its gradient on 'NEW_X' and at the end."""
        self._before_call(xs[0])
        pf, pt, pc, pl, pi, pd = self._own_ptrs()
        a = self._addr
        cur = self._cur
        check(self.lib.lbfgsb_hip_setulb_dev_pp(self.h, a(xs[0]), a(xs[1]), a(l), a(u), a(nbd), pf, a(gs[0]),
                                                a(gs[1]), float(factr), float(pgtol), pt, int(iprint), pc, pl,
                                                pi, pd, self._cur_ref))
        if self.stream_ordered and bytes(self.task[:2]) == b"FG":
            self.release_to_stream()   # (the caller's stream may read the trial point from here on)
        return self.task_s, cur.value

    def minimize(self, x, l, u, nbd, g, fg=None, builtin: int = 0, factr: float = 1e7,
                 pgtol: float = 1e-5, max_iter: int = 0, max_fg: int = 0, iprint: int = -1) -> str:
        """The reference's @todo wrapper (src/lbfgsb.f90:36-37): run the reverse-communication
        loop inside the library.  fg(x_ptr, g_ptr) -> global f evaluates the objective on the
        device (raw device pointers as ints); fg=None uses the built-in objective `builtin`."""
        if not isinstance(x, np.ndarray):
            import torch
            torch.cuda.synchronize()
        cb = C.cast(None, capi.FG_FN)
        failure = []
        if fg is not None:
            def _fg(user, xp, gp):
                # the callback must leave g complete, or ordered before the solver's stream
                # (self.wait_stream() / evaluate on self.stream); a Python exception cannot cross
                # the C frame: it is kept, the evaluation reports NaN -- the line search then
                # fails and the loop ends -- and it is raised again below
                if failure:
                    return float("nan")
                try:
                    val = float(fg(xp, gp))
                    if not self.same_stream_objective:
                        self.wait_stream()
                    return val
                except BaseException as e:   # noqa: BLE001
                    failure.append(e)
                    return float("nan")
            cb = capi.FG_FN(_fg)
            self._keep.append(cb)
        check(self.lib.lbfgsb_hip_minimize(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g),
                                           float(factr), float(pgtol), int(max_iter), int(max_fg),
                                           int(iprint), cb, None, int(builtin), _p(self.f),
                                           _p(self.task), _p(self.lsave), _p(self.isave),
                                           _p(self.dsave)))
        if failure:
            raise failure[0]
        return self.task_s

    # ---- state exchange / kernels ----
    def export_state(self):
        wa = np.zeros(wa_length(self.n, self.m), self.real)
        iwa = np.zeros(3 * self.n, np.int32)
        check(self.lib.lbfgsb_hip_export_state(self.h, _p(wa), _p(iwa)))
        return wa, iwa

    def import_state(self, wa, iwa, isave):
        wa = np.ascontiguousarray(wa, self.real)
        iwa = np.ascontiguousarray(iwa, np.int32)
        isave = np.ascontiguousarray(isave, np.int32)
        check(self.lib.lbfgsb_hip_import_state(self.h, _p(wa), _p(iwa), _p(isave)))

    # ---- the curvature model as a device operator (include/lbfgsb_hip.h, lbfgsb_hip_qn_apply / qn_diag) ----
    def _qn_vec(self, t, what):
        import torch
        want = torch.float32 if self.real == np.float32 else torch.float64
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == want):
            raise TypeError("%s must be a CUDA tensor of dtype %s" % (what, want))
        if t.dim() not in (1, 2) or t.shape[-1] != self.n or t.stride(-1) != 1:
            raise ValueError("%s must have shape (n,) or (k, n) with n = %d rows per vector, contiguous per vector"
                             % (what, self.n))
        return t

    def _qn_done(self):
        if self.same_stream_objective or self.stream_ordered:
            self.release_to_stream()  # (out is ordered on the solver's stream only: torch's stream waits for it)

    def qn_apply(self, v, out=None, inverse: bool = False, sqrt: bool = False):
        """out = B v (inverse=False) or H v = B^-1 v (inverse=True) for v of shape (n,) or (k, n): the limited-memory
        model of the last return (or import_state), theta I updated by the stored pairs -- H is exactly the inverse
        of the matrix the solver uses (scipy's hess_inv starts from H0 = I instead).  sqrt=True: the symmetric
        square root B^(1/2) v or H^(1/2) v (at most 64 stored pairs).  Returns out."""
        v = self._qn_vec(v, "v")
        if out is None:
            import torch
            out = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        out = self._qn_vec(out, "out")
        if out.shape != v.shape:
            raise ValueError("out must have the shape of v")
        k = 1 if v.dim() == 1 else v.shape[0]
        ldv = self.n if v.dim() == 1 else v.stride(0)
        ldo = self.n if out.dim() == 1 else out.stride(0)
        self.wait_stream()
        mode = (capi.QN_H_SQRT if inverse else capi.QN_B_SQRT) if sqrt else (capi.QN_H if inverse else capi.QN_B)
        check(self.lib.lbfgsb_hip_qn_apply(self.h, mode, k, v.data_ptr(), ldv, out.data_ptr(), ldo))
        self._qn_done()
        return out

    def qn_diag(self, out=None, inverse: bool = False):
        """diag(B) or diag(H) as an (n,) tensor (at most 32 stored pairs).  Returns out."""
        import torch
        if out is None:
            dt = torch.float32 if self.real == np.float32 else torch.float64
            out = torch.empty(self.n, dtype=dt, device=torch.device("cuda", self.device))
        out = self._qn_vec(out, "out")
        if out.dim() != 1:
            raise ValueError("out must have shape (n,)")
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_diag(self.h, capi.QN_H if inverse else capi.QN_B, out.data_ptr()))
        self._qn_done()
        return out

    def qn_logdet(self, inverse: bool = False) -> float:
        """log det B (inverse=False) or log det H = -log det B over all n_global rows, the same value on every rank
        (collective on sharded contexts; at most 64 stored pairs)."""
        val = C.c_double(0.0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_logdet(self.h, capi.QN_H if inverse else capi.QN_B, C.byref(val)))
        return val.value

    def qn_draw(self, k: int, seed: int, first: int = 0, mean=None, scale: float = 1.0, inverse: bool = True,
                out=None, return_logpdf: bool = False):
        """k draws from N(mean, scale^2 A), A = H (inverse=True) or B, as a (k, n) tensor: row j is mean + scale
        A^(1/2) z_(first + j).  The standard normal z_s is generated on the device inside the passes over W; its
        entry for a row depends on (seed, the global row, s) alone -- not on the sharding or on k.  seed: any
        integer below 2^64.  mean: an (n,) tensor or None.  Returns out; with return_logpdf (out, logp), logp a numpy
        (k,) array of the draws' log-densities under N(mean, scale^2 A) over all rows of all ranks (the draws are
        the same bits either way; float32 solvers: the density of the draw before it is rounded on store)."""
        import torch
        dt = torch.float32 if self.real == np.float32 else torch.float64
        if out is None:
            out = torch.empty((int(k), self.n), dtype=dt, device=torch.device("cuda", self.device))
        out = self._qn_vec(out, "out")
        if (out.dim() == 1 and k != 1) or (out.dim() == 2 and out.shape[0] != k):
            raise ValueError("out must have shape (k, n)")
        if mean is not None:
            mean = self._qn_vec(mean, "mean")
            if mean.dim() != 1:
                raise ValueError("mean must have shape (n,)")
        ldo = self.n if out.dim() == 1 else out.stride(0)
        self.wait_stream()
        if return_logpdf:
            logp = np.zeros(int(k), np.float64)
            check(self.lib.lbfgsb_hip_qn_draw_logpdf(self.h, capi.QN_H if inverse else capi.QN_B, int(k),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(first),
                                                     None if mean is None else mean.data_ptr(), float(scale),
                                                     out.data_ptr(), ldo,
                                                     logp.ctypes.data_as(C.POINTER(C.c_double))))
            self._qn_done()
            return out, logp
        check(self.lib.lbfgsb_hip_qn_draw(self.h, capi.QN_H if inverse else capi.QN_B, int(k),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(first),
                                          None if mean is None else mean.data_ptr(), float(scale), out.data_ptr(),
                                          ldo))
        self._qn_done()
        return out

    def _qn_center(self, c, what):
        if c is None:
            return None
        c = self._qn_vec(c, what)
        if c.dim() != 1:
            raise ValueError("%s must have shape (n,)" % what)
        return c

    def qn_quad(self, v, center=None, inverse: bool = False):
        """(v_j - center)' A (v_j - center) over all rows of all ranks, A = B (inverse=False) or H, for v of shape (n,)
        or (k, n): one pass over the pairs per 4 vectors, nothing written on the device.  center: an (n,) tensor or
        None.  Returns a numpy (k,) array, or a float for a 1-d v.  Any number of stored pairs."""
        v = self._qn_vec(v, "v")
        center = self._qn_center(center, "center")
        k = 1 if v.dim() == 1 else v.shape[0]
        ldv = self.n if v.dim() == 1 else v.stride(0)
        q = np.zeros(k, np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_quad(self.h, capi.QN_H if inverse else capi.QN_B, k, v.data_ptr(), ldv,
                                          None if center is None else center.data_ptr(),
                                          q.ctypes.data_as(C.POINTER(C.c_double))))
        return float(q[0]) if v.dim() == 1 else q

    def qn_gram(self, v, center=None, inverse: bool = False):
        """The k x k matrix (v_a - center)' A (v_b - center) over all rows of all ranks, A = B (inverse=False) or H,
        for v of shape (k, n), k <= 64 (a 1-d v gives (1, 1)): qn_quad's pass with the d_a'd_b of each block of 4
        vectors carried along, and a pass over the vectors alone for two vectors of different blocks.  Returns a
        numpy (k, k) float64 array, symmetric bit for bit; its diagonal is qn_quad's.  With the rows of v the
        functionals c_j and inverse=True it is their covariance C'H C under the Laplace posterior N(x*, H)."""
        v = self._qn_vec(v, "v")
        center = self._qn_center(center, "center")
        k = 1 if v.dim() == 1 else v.shape[0]
        ldv = self.n if v.dim() == 1 else v.stride(0)
        g = np.zeros((k, k), np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_gram(self.h, capi.QN_H if inverse else capi.QN_B, k, v.data_ptr(), ldv,
                                          None if center is None else center.data_ptr(),
                                          g.ctypes.data_as(C.POINTER(C.c_double)), k))
        return g

    def qn_eig(self, inverse: bool = False):
        """(bulk, values): the model A = B (inverse=False) or H is bulk I + U diag(values - bulk) U' with orthonormal
        U -- bulk = theta or 1 / theta with multiplicity n_global - r, values a numpy (r,) array of the other
        eigenvalues in ascending order, r <= min(2 col, n_global) (directions within capi.QN_EIG_CUT * bulk of the
        bulk value count as bulk).  Host algebra on the Gram of the pairs alone: no pass over W beyond that Gram
        pass, the same bits on every rank (collective on sharded contexts; at most 64 stored pairs)."""
        r, bulk = C.c_int32(0), C.c_double(0.0)
        mode = capi.QN_H if inverse else capi.QN_B
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_eig(self.h, mode, 0, C.byref(r), C.byref(bulk), None))
        lam = np.zeros(r.value, np.float64)
        if r.value:
            check(self.lib.lbfgsb_hip_qn_eig(self.h, mode, r.value, C.byref(r), C.byref(bulk),
                                             lam.ctypes.data_as(C.POINTER(C.c_double))))
        return bulk.value, lam

    def qn_eigvec(self, which=None, out=None, inverse: bool = False):
        """The unit eigenvectors of B (inverse=False) or H as a (k, n) tensor of this rank's rows: row j belongs to
        eigenvalue number which[j] of qn_eig's ascending list (repeats allowed; None: all r of them, or the first k of
        an `out` of k rows).  One pass over the pairs per 16 of them writes all k <= 128 vectors.  Returns out."""
        import torch
        dt = torch.float32 if self.real == np.float32 else torch.float64
        if which is None:
            k = out.shape[0] if out is not None and out.dim() == 2 else (1 if out is not None else
                                                                         len(self.qn_eig(inverse)[1]))
            idx = None
        else:
            idx = np.ascontiguousarray(which, np.int32).reshape(-1)
            k = int(idx.size)
        if out is None:
            out = torch.empty((k, self.n), dtype=dt, device=torch.device("cuda", self.device))
            if k == 0:
                return out
        out = self._qn_vec(out, "out")
        if (out.dim() == 1 and k != 1) or (out.dim() == 2 and out.shape[0] != k):
            raise ValueError("out must have shape (k, n)")
        ldo = self.n if out.dim() == 1 else out.stride(0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_eigvec(self.h, capi.QN_H if inverse else capi.QN_B, k,
                                            None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                            out.data_ptr(), ldo))
        self._qn_done()
        return out

    # ---- entries at index lists (include/lbfgsb_hip.h "Entries at index lists") ----
    @staticmethod
    def _qn_idx(idx, what="idx"):
        """an index list as a contiguous host int64 array: numpy arrays, sequences or torch tensors (a device tensor,
        such as kkt_indices returns, is copied to the host)"""
        if hasattr(idx, "detach") and hasattr(idx, "cpu"):
            idx = idx.detach().cpu().numpy()
        a = np.asarray(idx)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("%s must hold integers" % what)
        a = np.ascontiguousarray(a, np.int64).reshape(-1)
        if a.size < 1:
            raise ValueError("%s is empty" % what)
        return a

    def qn_rows(self, idx):
        """The rows of the stored pairs at the global 0-based indices idx as a numpy (k, 2 col) float64 array: entry
        [j, c] is row idx[j] of S (c < col, oldest pair first) or of Y (c >= col), exactly the stored value.  One
        gather, no pass over W; k <= capi.QN_IDX_MAXK.  Collective on sharded contexts: every rank passes the same
        list and receives the same array."""
        idx = self._qn_idx(idx)
        k = int(idx.size)
        buf = np.full((2 * self.m, k), np.nan, np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_rows(self.h, k, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                          buf.ctypes.data_as(C.POINTER(C.c_double)), k))
        written = int(np.count_nonzero(~np.isnan(buf).all(axis=1)))  # (2 col columns were written, no others)
        return np.ascontiguousarray(buf[:written].T)

    def qn_block(self, ia, ib=None, inverse: bool = False):
        """A[ia, ib] for A = B (inverse=False) or H as a numpy (ka, kb) float64 array, from the rows of the pairs at
        the global 0-based indices alone: alpha [ia_a == ib_b] + r_a N r_b'.  ib=None: ib = ia, symmetric bit for
        bit -- with inverse=True the marginal covariance of these parameters under the Laplace posterior N(x*, H).
        Lists may be unsorted and repeat indices; at most capi.QN_IDX_MAXK each, any number of stored pairs.
        Collective on sharded contexts (the same list, the same bits on every rank)."""
        ia = self._qn_idx(ia, "ia")
        ib = None if ib is None else self._qn_idx(ib, "ib")
        ka, kb = int(ia.size), int(ia.size if ib is None else ib.size)
        a = np.zeros((kb, ka), np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_block(self.h, capi.QN_H if inverse else capi.QN_B, ka,
                                           ia.ctypes.data_as(C.POINTER(C.c_int64)), kb,
                                           None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_int64)),
                                           a.ctypes.data_as(C.POINTER(C.c_double)), ka))
        return np.ascontiguousarray(a.T)

    def _qn_cols_out(self, k, out):
        import torch
        dt = torch.float32 if self.real == np.float32 else torch.float64
        if out is None:
            out = torch.empty((k, self.n), dtype=dt, device=torch.device("cuda", self.device))
        out = self._qn_vec(out, "out")
        if (out.dim() == 1 and k != 1) or (out.dim() == 2 and out.shape[0] != k):
            raise ValueError("out must have shape (k, n)")
        return out, (self.n if out.dim() == 1 else out.stride(0))

    def qn_cols(self, idx, out=None, inverse: bool = False):
        """The columns A[:, idx[j]] of B (inverse=False) or H as a (k, n) tensor of this rank's rows, k <= 128: what
        qn_apply gives on unit vectors, without the unit vectors -- the gather of k rows, then one pass over the
        pairs per 16 of them that writes all k columns.  Returns out."""
        idx = self._qn_idx(idx)
        out, ldo = self._qn_cols_out(int(idx.size), out)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_cols(self.h, capi.QN_H if inverse else capi.QN_B, int(idx.size),
                                          idx.ctypes.data_as(C.POINTER(C.c_int64)), out.data_ptr(), ldo))
        self._qn_done()
        return out

    def qn_shift(self, d=None, mu: float = 0.0) -> "QnShifted":
        """The model plus a diagonal, B + mu I + diag(d), as a QnShifted with .solve(v), .logdet(), .diag(), .pinned,
        and .sqrt(v), .sample(k, seed), .quad(v), .log_prob(x) of N(mean, scale^2 (B + mu I + diag(d))^-1).  d: an (n,) tensor of this rank's rows or None (D = 0); an entry +inf pins its row -- the row drops
        out of the matrix, its outputs are +0 -- so d = inf on the rows at bounds gives the model on the free
        variables.  The weights and the factor of the 2col x 2col K are made here (one pass over d, ceil(2 col / 4)
        weighted passes over the pairs) and belong to the pairs of this return: after the next return that stores a
        pair the object raises LbfgsbError ("call qn_shift_set again").  Collective on sharded contexts."""
        if d is not None:
            d = self._qn_vec(d, "d")
            if d.dim() != 1:
                raise ValueError("d must have shape (n,)")
        pinned = C.c_int64(0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_shift_set(self.h, None if d is None else d.data_ptr(), float(mu),
                                               C.byref(pinned)))
        return QnShifted(self, int(pinned.value), float(mu))

    def qn_path(self, status=None, codes=(1, 2, 3)) -> "QnPath":
        """The model on the free rows over a range of shifts, (B_FF + mu I)^-1 for any number of mu, as a QnPath with
        .pinned, .logdet(mus), .solve(v, mus) and .trust(g, delta).  status: an int8 CUDA tensor of n codes as kkt
        writes them, or None (nothing pinned); codes: the status codes to PIN (default: the rows at a lower bound, at
        an upper bound or fixed).  One pass makes the free bytes and counts the pinned rows, ceil(2 col / 4) masked
        passes reduce the Gram of the pairs on the free rows (none without pins: the cached Gram); afterwards a new
        shift costs the host a 2col x 2col factorisation and the device nothing.  Belongs to the pairs of this
        return, as qn_shift's result; independent of it.  Collective on sharded contexts."""
        import torch
        mask = 0
        if status is not None:
            if not (isinstance(status, torch.Tensor) and status.is_cuda and status.dtype == torch.int8
                    and status.dim() == 1 and status.numel() >= self.n and status.is_contiguous()):
                raise TypeError("status must be a contiguous int8 CUDA tensor with n = %d rows" % self.n)
            for c in ([codes] if isinstance(codes, (int, np.integer)) else codes):
                if not -1 <= int(c) <= 3:
                    raise ValueError("status codes are -1 .. 3")
                mask |= 1 << (int(c) + 1)
        pinned = C.c_int64(0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_path_set(self.h, None if status is None else status.data_ptr(), mask,
                                              C.byref(pinned)))
        return QnPath(self, int(pinned.value))

    def qn_logpdf(self, x, mean=None, scale: float = 1.0, inverse: bool = True):
        """log N(x_j; mean, scale^2 A) over all rows of all ranks, the covariance A = H (inverse=True, as qn_draw's
        default) or B, for x of shape (n,) or (k, n): the quadratic form of A^-1 by qn_quad's pass and qn_logdet's
        log det A (at most 64 stored pairs).  Returns a numpy (k,) array, or a float for a 1-d x."""
        x = self._qn_vec(x, "x")
        mean = self._qn_center(mean, "mean")
        k = 1 if x.dim() == 1 else x.shape[0]
        ldx = self.n if x.dim() == 1 else x.stride(0)
        lp = np.zeros(k, np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_logpdf(self.h, capi.QN_H if inverse else capi.QN_B, k, x.data_ptr(), ldx,
                                            None if mean is None else mean.data_ptr(), float(scale),
                                            lp.ctypes.data_as(C.POINTER(C.c_double))))
        return float(lp[0]) if x.dim() == 1 else lp

    # ---- pairs in and out (include/lbfgsb_hip.h "Pairs in and out: a curvature model of the caller's own") ----
    def _qn_pairs_arg(self, a, what, k=None):
        """a (k, n) block of vectors (or (n,) for one) as a CUDA tensor of the context's kind, each vector contiguous;
        a numpy array is copied to the device"""
        import torch
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, self.real)).to(torch.device("cuda", self.device))
        if a.dim() == 2 and a.shape[0] == 0:  # (no pair: nothing is read)
            if a.shape[1] != self.n:
                raise ValueError("%s must have shape (k, n) with n = %d" % (what, self.n))
            return a
        a = self._qn_vec(a, what)
        if k is not None and (1 if a.dim() == 1 else a.shape[0]) != k:
            raise ValueError("%s must hold %d vectors" % (what, k))
        return a

    def qn_pairs(self, out=None):
        """(S, Y, theta): the stored pairs of the last return (or import_state, or of the caller's own model) as two
        (col, n) tensors of this rank's rows, oldest pair first as qn_rows orders them, and theta -- read out of W in
        the layout it is in, device to device; the run does not notice.  out: a pair (S, Y) of tensors of at least col
        rows to write into (the first col rows are returned)."""
        import torch
        col, theta = C.c_int32(0), C.c_double(0.0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_pairs_get(self.h, 0, C.byref(col), C.byref(theta), None, 0, None, 0))
        k = int(col.value)
        dt = torch.float32 if self.real == np.float32 else torch.float64
        if out is None:
            dev = torch.device("cuda", self.device)
            out = (torch.empty((k, self.n), dtype=dt, device=dev), torch.empty((k, self.n), dtype=dt, device=dev))
        S, Y = out
        if k == 0:
            return S[:0], Y[:0], theta.value
        S, Y = self._qn_vec(S, "out[0]"), self._qn_vec(Y, "out[1]")
        if S.dim() != 2 or Y.dim() != 2 or S.shape[0] < k or Y.shape[0] < k:
            raise ValueError("out must be two tensors of shape (>= col, n), col = %d" % k)
        check(self.lib.lbfgsb_hip_qn_pairs_get(self.h, k, C.byref(col), C.byref(theta), S.data_ptr(), S.stride(0),
                                               Y.data_ptr(), Y.stride(0)))
        self._qn_done()
        return S[:k], Y[:k], theta.value

    def qn_set_pairs(self, S, Y, theta=None):
        """Make this context the keeper of a curvature model of the caller's own: S, Y of shape (k, n), k <= m, hold
        the pairs (s_j, y_j) of this rank's rows, oldest first (CUDA tensors of the context's kind; numpy arrays are
        copied to the device).  theta=None: y'y / s'y of the newest pair as the iteration sets it (1.0 with no pair).
        Ends whatever run the context holds -- only a START follows -- and needs none: a DeviceSolver that has never
        run takes pairs and then serves qn_apply, qn_operator(), qn_shift(...) and every other qn_* entry.  Raises
        LbfgsbError (LBFGSB_E_ARG) for a pair with s'y <= 0 or a model that is not positive definite; the context
        then holds no model.  Collective on sharded contexts."""
        S, Y = self._qn_pairs_arg(S, "S"), self._qn_pairs_arg(Y, "Y")
        k = 1 if S.dim() == 1 else int(S.shape[0])
        if (1 if Y.dim() == 1 else int(Y.shape[0])) != k:
            raise ValueError("S and Y must hold the same number of pairs")
        if theta is None:
            theta = 0.0 if k > 0 else 1.0
        lds = self.n if S.dim() == 1 else S.stride(0)
        ldy = self.n if Y.dim() == 1 else Y.stride(0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_pairs_set(self.h, k, S.data_ptr() if k else None, lds,
                                               Y.data_ptr() if k else None, ldy, float(theta)))

    def qn_push_pair(self, s, y, theta=None) -> int:
        """Append one pair to the caller's model (after qn_set_pairs) as the iteration's update does: 1 when it was
        stored (a full ring drops its oldest pair; theta = y'y / s'y unless given), 0 when s'y is not safely positive
        and nothing changed, -1 when the update left the model indefinite and it was reset to the empty one.  One
        pass over the pairs; the next qn_apply needs no Gram pass.  Collective on sharded contexts."""
        s, y = self._qn_pairs_arg(s, "s", 1), self._qn_pairs_arg(y, "y", 1)
        stored = C.c_int32(0)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_qn_pairs_push(self.h, s.data_ptr(), y.data_ptr(),
                                                0.0 if theta is None else float(theta), C.byref(stored)))
        return int(stored.value)

    def qn_operator(self, inverse: bool = True) -> "QnOperator":
        """H (default) or B as a small linear-operator object: hess_inv = sol.qn_operator() after minimize()."""
        return QnOperator(self, inverse)

    # ---- the active set, the multipliers and the projected gradient (include/lbfgsb_hip.h, lbfgsb_hip_kkt) ----
    def kkt(self, x, l, u, nbd, g, tol: float = 0.0, pg=True, mult=True, status=True) -> "KktReport":
        """One pass over x, l, u, nbd, g (device tensors of this rank's rows): the report of include/lbfgsb_hip.h's
        "active set" block.  pg / mult / status: True allocates that per-row output, a tensor is written in place,
        False / None leaves it out (it then costs nothing).  The summary is complete over all ranks."""
        import torch
        want = torch.float32 if self.real == np.float32 else torch.float64
        for name, t in (("x", x), ("l", l), ("u", u), ("g", g)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == want and t.dim() == 1
                    and t.numel() >= self.n and t.is_contiguous()):
                raise TypeError("%s must be a contiguous CUDA tensor of dtype %s with n = %d rows"
                                % (name, want, self.n))
        if not (isinstance(nbd, torch.Tensor) and nbd.is_cuda and nbd.dtype == torch.int32 and nbd.dim() == 1
                and nbd.numel() >= self.n and nbd.is_contiguous()):
            raise TypeError("nbd must be a contiguous int32 CUDA tensor with n = %d rows" % self.n)

        def out_of(o, dt, name):
            if o is None or o is False:
                return None
            if o is True:
                return torch.empty(self.n, dtype=dt, device=x.device)
            if not (isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == dt and o.dim() == 1
                    and o.numel() >= self.n and o.is_contiguous()):
                raise TypeError("%s must be a contiguous CUDA tensor of dtype %s with n = %d rows"
                                % (name, dt, self.n))
            return o
        pg, mult, status = out_of(pg, want, "pg"), out_of(mult, want, "mult"), out_of(status, torch.int8, "status")
        cnt = np.zeros(len(capi.KKT_CNT), np.int64)
        val = np.zeros(len(capi.KKT_VAL), np.float64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_kkt(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), float(tol), _p(pg), _p(mult),
                                      _p(status), _p(cnt), _p(val)))
        return KktReport(cnt, val, float(tol), pg, mult, status)

    def kkt_indices(self, status, codes):
        """The global 0-based indices (row0 + i) of this rank's rows whose status byte is one of `codes` (an int or
        an iterable of the codes -1 .. 3), ascending, as an int64 tensor of exactly the count's length
        (lbfgsb_hip_kkt_list: a counting call, then the list).  status: an int8 CUDA tensor of n codes."""
        import torch
        if not (isinstance(status, torch.Tensor) and status.is_cuda and status.dtype == torch.int8
                and status.dim() == 1 and status.numel() >= self.n and status.is_contiguous()):
            raise TypeError("status must be a contiguous int8 CUDA tensor with n = %d rows" % self.n)
        mask = 0
        for c in ([codes] if isinstance(codes, (int, np.integer)) else codes):
            if not -1 <= int(c) <= 3:
                raise ValueError("status codes are -1 .. 3")
            mask |= 1 << (int(c) + 1)
        count = np.zeros(1, np.int64)
        self.wait_stream()
        check(self.lib.lbfgsb_hip_kkt_list(self.h, _p(status), mask, None, 0, _p(count)))
        idx = torch.empty(int(count[0]), dtype=torch.int64, device=status.device)
        if count[0] > 0:
            check(self.lib.lbfgsb_hip_kkt_list(self.h, _p(status), mask, _p(idx), int(count[0]), _p(count)))
        return idx

    def projgr(self, x, l, u, nbd, g) -> float:
        out = np.zeros(1)
        check(self.lib.lbfgsb_hip_projgr(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), _p(out)))
        return float(out[0])

    # ---- routine doors (include/lbfgsb_hip.h "Routine doors"): one routine of the reference each, on the
    #      state of the context (import_state / export_state); vectors are device tensors ----
    def r_vec_sub(self, a, b, out):
        """out = a - b (level-1 door; src/lbfgsb.f90:720-722, :812-816)"""
        check(self.lib.lbfgsb_hip_vec_sub(self.h, _p(a), _p(b), _p(out)))

    def r_vec_scale(self, alpha, v):
        """v = alpha v (dscal, :822)"""
        check(self.lib.lbfgsb_hip_vec_scale(self.h, float(alpha), _p(v)))

    def r_dot(self, a, b):
        """a'b in fp64, summed over the context's ranks (ddot, :816 / :2196 / :2244 / :2335)"""
        out = np.zeros(1, np.float64)
        check(self.lib.lbfgsb_hip_dot(self.h, _p(a), _p(b), _p(out)))
        return float(out[0])

    def r_active(self, x, l, u, nbd):
        """active :965 -- x projected in place; -> (prjctd, cnstnd, boxed)"""
        out = np.zeros(3, np.int32)
        check(self.lib.lbfgsb_hip_active(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(out)))
        return bool(out[0]), bool(out[1]), bool(out[2])

    def r_errclb(self, l, u, nbd, factr, task=b"START"):
        """errclb :1601 -- -> (task string, info, k)"""
        t = np.frombuffer(task.ljust(60), dtype="S1").copy()
        info, k = np.zeros(1, np.int32), np.zeros(1, np.int64)
        check(self.lib.lbfgsb_hip_errclb(self.h, _p(l), _p(u), _p(nbd), float(factr), _p(t), _p(info), _p(k)))
        return t.tobytes().decode().rstrip(), int(info[0]), int(k[0])

    def r_cauchy(self, x, l, u, nbd, g, theta, col, head, sbgnrm, xcp_out=None):
        """cauchy :1157 -- -> (nseg, info); xcp in the state's z (and in xcp_out)"""
        nseg, info = np.zeros(1, np.int32), np.zeros(1, np.int32)
        check(self.lib.lbfgsb_hip_cauchy(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), float(theta), int(col),
                                         int(head), float(sbgnrm), _p(xcp_out) if xcp_out is not None else None,
                                         _p(nseg), _p(info)))
        return int(nseg[0]), int(info[0])

    def r_freev(self, iter_, cnstnd, updatd):
        """freev :1980 -- -> (nfree, nenter, ileave, wrk)"""
        o = np.zeros(3, np.int64)
        wrk = np.zeros(1, np.int32)
        check(self.lib.lbfgsb_hip_freev(self.h, int(iter_), int(bool(cnstnd)), int(bool(updatd)), _p(o[0:1]),
                                        _p(o[1:2]), _p(o[2:3]), _p(wrk)))
        return int(o[0]), int(o[1]), int(o[2]), bool(wrk[0])

    def r_formk(self, col, head, theta):
        """formk :1681 (inner products from scratch) -- -> info; WN1, WN in the state"""
        info = np.zeros(1, np.int32)
        check(self.lib.lbfgsb_hip_formk(self.h, int(col), int(head), float(theta), _p(info)))
        return int(info[0])

    def r_cmprlb(self, x, g, theta, col, head, cnstnd, r_out):
        """cmprlb :1548 -- r scattered to its rows in r_out -> info"""
        info = np.zeros(1, np.int32)
        check(self.lib.lbfgsb_hip_cmprlb(self.h, _p(x), _p(g), float(theta), int(col), int(head),
                                         int(bool(cnstnd)), _p(r_out), _p(info)))
        return int(info[0])

    def r_subsm(self, x, l, u, nbd, g, r_in, theta, col, head, xhat_out=None):
        """subsm :2676 -- -> (iword, info); the subspace minimiser in the state's z (and xhat_out)"""
        iword, info = np.zeros(1, np.int32), np.zeros(1, np.int32)
        check(self.lib.lbfgsb_hip_subsm(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), _p(r_in), float(theta),
                                        int(col), int(head), _p(xhat_out) if xhat_out is not None else None,
                                        _p(iword), _p(info)))
        return int(iword[0]), int(info[0])

    def r_lnsrlb(self, x, l, u, nbd, g, f, sc, ic, task, csave, isave2, dsave13):
        """lnsrlb :2174 -- sc (8 doubles), ic (7 int32), task / csave (S1[60]), isave2, dsave13 in / out"""
        check(self.lib.lbfgsb_hip_lnsrlb(self.h, _p(x), _p(l), _p(u), _p(nbd), _p(g), float(f), _p(sc), _p(ic),
                                         _p(task), _p(csave), _p(isave2), _p(dsave13)))

    def r_matupd(self, g, stp, dr, dtd, ip):
        """mainlb :812-824 + matupd :2291 -- ip = (iupdat, col, head, itail) int32 in / out -> theta"""
        th = np.zeros(1)
        check(self.lib.lbfgsb_hip_matupd(self.h, _p(g), float(stp), float(dr), float(dtd), _p(ip), _p(th)))
        return float(th[0])

    def set_w(self, ws: np.ndarray, wy: np.ndarray):
        """ws, wy: host arrays of shape (m, n) C-order == Fortran (n, m) column-major."""
        ws = np.ascontiguousarray(ws, self.real)
        wy = np.ascontiguousarray(wy, self.real)
        assert ws.shape == (self.m, self.n) and wy.shape == (self.m, self.n)
        check(self.lib.lbfgsb_hip_set_w(self.h, _p(ws), _p(wy)))

    def set_iwhere(self, iwhere: np.ndarray):
        iw = np.ascontiguousarray(iwhere, np.int32)
        assert iw.shape == (self.n,)
        check(self.lib.lbfgsb_hip_set_iwhere(self.h, _p(iw)))

    def formk_gram(self, col: int, head: int = 1) -> np.ndarray:
        """formk's inner products from scratch (layout: include/lbfgsb_hip.h)"""
        out = np.zeros(2 * col * col + col)
        check(self.lib.lbfgsb_hip_formk_gram(self.h, col, head, _p(out)))
        return out

    def wtv(self, v, col: int, head: int = 1) -> np.ndarray:
        out = np.zeros(2 * col)
        check(self.lib.lbfgsb_hip_wtv(self.h, _p(v), col, head, _p(out)))
        return out

    def wtv_launch(self, v, col: int, head: int = 1):
        check(self.lib.lbfgsb_hip_wtv_launch_only(self.h, _p(v), col, head))

    def wtv_time(self, v, col: int, head: int = 1, reps: int = 20) -> float:
        """average milliseconds of one W'v kernel launch (hipEvents on the solver's stream)"""
        out = np.zeros(1)
        check(self.lib.lbfgsb_hip_wtv_time(self.h, _p(v), col, head, reps, _p(out)))
        return float(out[0])

    def kernel_time(self, which: int, x, g, col: int, head: int = 1, reps: int = 20) -> float:
        """average ms per launch of an in-iteration kernel: 0 = cmprlb_wtv, 1 = formk gram"""
        out = np.zeros(1)
        check(self.lib.lbfgsb_hip_kernel_time(self.h, which, _p(x), _p(g), col, head, reps, _p(out)))
        return float(out[0])

    def sync(self):
        check(self.lib.lbfgsb_hip_sync(self.h))

    def objective(self, kind: int, x, g, deferred: bool = False):
        """Built-in objective on the solver's stream.  deferred=True leaves f on the device: the
        next setulb() call (the FG re-entry) fetches it with its own sums and stores it in
        self.f -- one host sync less per evaluation; returns None then."""
        if deferred:
            check(self.lib.lbfgsb_hip_objective(self.h, kind, self._addr(x), self._addr(g), None))
            return None
        out = np.zeros(1)
        check(self.lib.lbfgsb_hip_objective(self.h, kind, _p(x), _p(g), _p(out)))
        return float(out[0])

    def pass_clock(self, enable: int):
        """In-run hipEvent clocks of the three passes over W (see lbfgsb_hip_pass_clock):
        enable 1 = reset and start, 0 = stop, -1 = read.  -> {name: (ms_total, launches)}"""
        ms = (C.c_double * 3)()
        cnt = (C.c_int64 * 3)()
        check(self.lib.lbfgsb_hip_pass_clock(self.h, int(enable), ms, cnt))
        names = ("cmprlb_wtv", "update_scan", "subsm_update")
        return {nm: (ms[k], cnt[k]) for k, nm in enumerate(names)}

    def path_counts(self):
        """(subspace steps by the two-pass closed form, by the three-pass route, Cauchy walks
        served by the breakpoints the update pass handed over)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.lbfgsb_hip_path_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def uniform_bounds(self) -> int:
        """bit 0 / 1 / 2: l / u / nbd hold one value each and are read as constants by the passes over W"""
        c = C.c_int32()
        check(self.lib.lbfgsb_hip_uniform_bounds(self.h, C.byref(c)))
        return int(c.value)

    def bounds_changed(self):
        """announce an edit of l, u or nbd made since the last setulb call: the next call rebuilds the snapshot
        (lbfgsb_hip_bounds_changed; sharded runs: every rank announces)"""
        check(self.lib.lbfgsb_hip_bounds_changed(self.h))

    def bounds_stats(self):
        """(comparison passes, differences found, snapshot rebuilds) -- lbfgsb_hip_bounds_stats"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.lbfgsb_hip_bounds_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def comm_info(self):
        """(nranks, rank, kind) of the context's communicator; kind 0 none, 1 RCCL (the communicator's own
        ncclCommCount / ncclCommUserRank), 2 host callbacks"""
        a, b, k = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.lbfgsb_hip_comm_info(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return int(a.value), int(b.value), int(k.value)

    def dense_launches(self):
        """option cw_dense: launches of the (storing pass's, update pass's) dense kernel -- lbfgsb_hip_dense_launches"""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.lbfgsb_hip_dense_launches(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ub_launches(self):
        """option cw_ub: launches of the update pass's uniform-bounds form -- lbfgsb_hip_ub_launches"""
        a = C.c_int64(0)
        check(self.lib.lbfgsb_hip_ub_launches(self.h, C.byref(a)))
        return a.value

    def compact_stats(self):
        """option compact_w: (packs, unpacks, packed now, eligible) -- lbfgsb_hip_compact_stats"""
        a, b = C.c_int64(0), C.c_int64(0)
        c, d = C.c_int32(0), C.c_int32(0)
        check(self.lib.lbfgsb_hip_compact_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def collective_time(self, reps: int = 1000):
        """(median_us, min_us) of one host sync of the iteration by itself (lbfgsb_hip_collective_time); a
        collective: every rank calls it"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        check(self.lib.lbfgsb_hip_collective_time(self.h, int(reps), C.byref(a), C.byref(b)))
        return a.value, b.value

    def host_gap(self):
        """(seconds, stretches) the device waited for the host's 2m x 2m algebra between the two passes"""
        a, b = C.c_double(), C.c_int64()
        check(self.lib.lbfgsb_hip_host_gap(self.h, C.byref(a), C.byref(b)))
        return float(a.value), int(b.value)

    def host_segments(self):
        """accumulated host seconds of the stretch between the two passes, by milestone (lbfgsb_hip_host_segments)"""
        a = (C.c_double * 5)()
        check(self.lib.lbfgsb_hip_host_segments(self.h, a))
        return [float(v) for v in a]

    def defer_stats(self):
        """(line-search set-ups whose sums were deferred, of those: requests that had to be re-issued)"""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.lbfgsb_hip_defer_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def tie_splits(self) -> int:
        """setulb calls so far whose Cauchy walk ended inside a group of equal breakpoints"""
        c = C.c_int64()
        check(self.lib.lbfgsb_hip_tie_splits(self.h, C.byref(c)))
        return int(c.value)

    def stats(self):
        a, b, c, w = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        check(self.lib.lbfgsb_hip_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(w)))
        nc, nb = C.c_int64(), C.c_int64()
        check(self.lib.lbfgsb_hip_comm_stats(self.h, C.byref(nc), C.byref(nb)))
        fs = C.c_int64()
        check(self.lib.lbfgsb_hip_freev_skipped(self.h, C.byref(fs)))
        sr = C.c_int64()
        check(self.lib.lbfgsb_hip_skip_stats(self.h, C.byref(sr)))
        rf = C.c_int64()
        check(self.lib.lbfgsb_hip_refresh_count(self.h, C.byref(rf)))
        return dict(launches=a.value, syncs=b.value, cauchy_fullsorts=c.value, wait_seconds=w.value,
                    collectives=nc.value, collective_bytes=nb.value, freev_skipped=fs.value,
                    skip_scans_reused=sr.value, refreshes=rf.value)


class KktReport:
    """What DeviceSolver.kkt returns: the counts and values of lbfgsb_hip_kkt by name (capi.KKT_CNT, capi.KKT_VAL --
    the header's LBFGSB_KKT_* in lower case), the raw arrays as `counts` / `values`, `tol`, and the per-row tensors that
    were asked for (`pg`, `mult`, `status`; None otherwise)."""

    def __init__(self, counts, values, tol, pg, mult, status):
        self.counts, self.values, self.tol = counts, values, tol
        self.pg, self.mult, self.status = pg, mult, status
        for k, name in enumerate(capi.KKT_CNT):
            setattr(self, name, int(counts[k]))
        for k, name in enumerate(capi.KKT_VAL):
            setattr(self, name, float(values[k]))

    def __repr__(self):
        return "KktReport(%s)" % ", ".join(
            ["%s=%d" % (k, getattr(self, k)) for k in capi.KKT_CNT]
            + ["%s=%r" % (k, getattr(self, k)) for k in capi.KKT_VAL])


class QnShifted:
    """What DeviceSolver.qn_shift returns: (B + mu I + diag(d))^-1 on the rows that are not pinned, for the pairs of
    the return it was made at, and the Gaussian N(mean, scale^2 (B + mu I + diag(d))^-1) on them: solve / logdet / diag,
    and sqrt / sample / quad / log_prob.  `pinned` is the number of pinned rows over all ranks.  The context holds ONE
    shift:
    a later qn_shift call replaces the weights this object solves with, and a return that stores a pair makes every
    method raise LbfgsbError with the library's message."""

    def __init__(self, solver: "DeviceSolver", pinned: int, mu: float):
        self.solver, self.pinned, self.mu = solver, pinned, mu

    def solve(self, v, out=None):
        """out = (B + mu I + D)^-1 v for v of shape (n,) or (k, n); pinned rows of out are +0.  Returns out."""
        return self._apply(self.solver.lib.lbfgsb_hip_qn_shift_solve, v, out)

    def logdet(self) -> float:
        """log det of B + mu I + D on the free rows of all ranks (no device pass; the same value on every rank)"""
        val = C.c_double(0.0)
        check(self.solver.lib.lbfgsb_hip_qn_shift_logdet(self.solver.h, C.byref(val)))
        return val.value

    def diag(self, out=None):
        """the diagonal of (B + mu I + D)^-1 as an (n,) tensor, +0 on pinned rows (at most 32 stored pairs)"""
        import torch
        s = self.solver
        if out is None:
            dt = torch.float32 if s.real == np.float32 else torch.float64
            out = torch.empty(s.n, dtype=dt, device=torch.device("cuda", s.device))
        out = s._qn_vec(out, "out")
        if out.dim() != 1:
            raise ValueError("out must have shape (n,)")
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_shift_diag(s.h, out.data_ptr()))
        s._qn_done()
        return out

    def block(self, ia, ib=None):
        """Sigma[ia, ib] of Sigma = (B + mu I + D)^-1 as a numpy (ka, kb) float64 array at global 0-based indices
        (ib=None: ib = ia, symmetric bit for bit): the marginal covariance of these parameters with the pinned rows
        held fixed.  A pinned row or column is exactly +0.  One gather of the rows and weights, no pass over W.
        With kkt_indices: block(solver.kkt_indices(report.status, 0)[:64]) on a shift with d = inf at the bounds."""
        s = self.solver
        ia = s._qn_idx(ia, "ia")
        ib = None if ib is None else s._qn_idx(ib, "ib")
        ka, kb = int(ia.size), int(ia.size if ib is None else ib.size)
        a = np.zeros((kb, ka), np.float64)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_shift_block(s.h, ka, ia.ctypes.data_as(C.POINTER(C.c_int64)), kb,
                                              None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_int64)),
                                              a.ctypes.data_as(C.POINTER(C.c_double)), ka))
        return np.ascontiguousarray(a.T)

    def columns(self, idx, out=None):
        """The columns Sigma[:, idx[j]] as a (k, n) tensor of this rank's rows, k <= 128; pinned rows are +0 and a
        pinned idx[j] gives a row of +0.  Returns out."""
        s = self.solver
        idx = s._qn_idx(idx)
        out, ldo = s._qn_cols_out(int(idx.size), out)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_shift_cols(s.h, int(idx.size), idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                             out.data_ptr(), ldo))
        s._qn_done()
        return out

    def _apply(self, entry, v, out):
        s = self.solver
        v = s._qn_vec(v, "v")
        if out is None:
            import torch
            out = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        out = s._qn_vec(out, "out")
        if out.shape != v.shape:
            raise ValueError("out must have the shape of v")
        k = 1 if v.dim() == 1 else v.shape[0]
        ldv = s.n if v.dim() == 1 else v.stride(0)
        ldo = s.n if out.dim() == 1 else out.stride(0)
        s.wait_stream()
        check(entry(s.h, k, v.data_ptr(), ldv, out.data_ptr(), ldo))
        s._qn_done()
        return out

    def sqrt(self, v, out=None):
        """out = L v for v of shape (n,) or (k, n), L L' = (B + mu I + D)^-1 on the free rows: L = diag(sqrt w) +
        diag(w) [S, Y] C [S, Y]' diag(sqrt w), a factor of the covariance (not its symmetric root), zero on pinned
        rows and columns; pinned rows of out are +0.  With v standard normal, L v is a draw of N(0, (B + mu I +
        D)^-1): the route for quasi-random or antithetic z.  Returns out."""
        return self._apply(self.solver.lib.lbfgsb_hip_qn_shift_sqrt, v, out)

    def sample(self, k: int, seed: int, first: int = 0, mean=None, scale: float = 1.0, log_prob: bool = False,
               out=None):
        """k draws from N(mean, scale^2 (B + mu I + D)^-1) on the free rows as a (k, n) tensor: row j is mean + scale
        L z_(first + j), z_s the standard normal vector of DeviceSolver.qn_draw -- a function of (seed, the global
        row, s) alone, whichever rows are pinned and however the rows are sharded.  A pinned row of a draw is its
        mean (+0 without one).  Returns out; with log_prob (out, logp), logp a numpy (k,) array of the draws'
        log-densities over the free rows of all ranks (the draws are the same bits either way)."""
        import torch
        s = self.solver
        dt = torch.float32 if s.real == np.float32 else torch.float64
        if out is None:
            out = torch.empty((int(k), s.n), dtype=dt, device=torch.device("cuda", s.device))
        out = s._qn_vec(out, "out")
        if (out.dim() == 1 and k != 1) or (out.dim() == 2 and out.shape[0] != k):
            raise ValueError("out must have shape (k, n)")
        mean = s._qn_center(mean, "mean")
        ldo = s.n if out.dim() == 1 else out.stride(0)
        mp = None if mean is None else mean.data_ptr()
        s.wait_stream()
        if log_prob:
            logp = np.zeros(int(k), np.float64)
            check(s.lib.lbfgsb_hip_qn_shift_draw_logpdf(s.h, int(k), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), mp,
                                                        float(scale), out.data_ptr(), ldo,
                                                        logp.ctypes.data_as(C.POINTER(C.c_double))))
            s._qn_done()
            return out, logp
        check(s.lib.lbfgsb_hip_qn_shift_draw(s.h, int(k), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), mp,
                                             float(scale), out.data_ptr(), ldo))
        s._qn_done()
        return out

    def quad(self, v, center=None):
        """(v_j - center)' (B + mu I + D) (v_j - center) over the free rows of all ranks for v of shape (n,) or (k, n):
        one pass per 4 vectors, nothing written on the device; what v and center hold on pinned rows is not used.
        Returns a numpy (k,) array, or a float for a 1-d v."""
        s = self.solver
        v = s._qn_vec(v, "v")
        center = s._qn_center(center, "center")
        k = 1 if v.dim() == 1 else v.shape[0]
        ldv = s.n if v.dim() == 1 else v.stride(0)
        q = np.zeros(k, np.float64)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_shift_quad(s.h, k, v.data_ptr(), ldv, None if center is None else center.data_ptr(),
                                             q.ctypes.data_as(C.POINTER(C.c_double))))
        return float(q[0]) if v.dim() == 1 else q

    def log_prob(self, x, mean=None, scale: float = 1.0):
        """log N(x_j; mean, scale^2 (B + mu I + D)^-1) over the free rows of all ranks for x of shape (n,) or (k, n);
        0 when every row is pinned.  Returns a numpy (k,) array, or a float for a 1-d x."""
        s = self.solver
        x = s._qn_vec(x, "x")
        mean = s._qn_center(mean, "mean")
        k = 1 if x.dim() == 1 else x.shape[0]
        ldx = s.n if x.dim() == 1 else x.stride(0)
        lp = np.zeros(k, np.float64)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_shift_logpdf(s.h, k, x.data_ptr(), ldx, None if mean is None else mean.data_ptr(),
                                               float(scale), lp.ctypes.data_as(C.POINTER(C.c_double))))
        return float(lp[0]) if x.dim() == 1 else lp


class TrustStep:
    """What QnPath.trust returns: step (an (n,) tensor, or None when it was not asked for), mu >= 0, norm = ||step||,
    predicted = the decrease -(g's + s'Bs / 2) the model predicts, on_boundary (mu > 0: the constraint is active) and iters, the
    host evaluations of the secular equation."""

    def __init__(self, step, mu, norm, predicted, on_boundary, iters):
        self.step, self.mu, self.norm, self.predicted = step, mu, norm, predicted
        self.on_boundary, self.iters = on_boundary, iters

    def __repr__(self):
        return "TrustStep(mu=%r, norm=%r, predicted=%r, on_boundary=%r, iters=%r)" % (
            self.mu, self.norm, self.predicted, self.on_boundary, self.iters)


class QnPath:
    """What DeviceSolver.qn_path returns: (B_FF + mu I)^-1 on the rows F that are not pinned, for the pairs of the
    return it was made at and ANY shift mu: logdet, solve and trust take their shifts as host numbers.  `pinned` is the
    number of pinned rows over all ranks.  The context holds one path: a later qn_path call replaces the free rows this
    object works on, and a return that stores a pair makes every method raise LbfgsbError with the library's message."""

    def __init__(self, solver: "DeviceSolver", pinned: int):
        self.solver, self.pinned = solver, pinned

    @staticmethod
    def _mus(mus):
        m = np.ascontiguousarray(np.atleast_1d(np.asarray(mus, np.float64)))
        if m.ndim != 1 or m.size < 1:
            raise ValueError("mus must be a scalar or a 1-d list of at least one shift")
        return m

    def logdet(self, mus):
        """(logdet, info): log det (B_FF + mu_j I) for every shift of mus as a float64 array, NaN where info[j] != 0
        (1: theta + mu_j <= 0 or not finite, 2: not positive definite on the free rows).  Host only: no launch."""
        s = self.solver
        m = self._mus(mus)
        ld = np.full(m.size, np.nan)
        info = np.zeros(m.size, np.int32)
        check(s.lib.lbfgsb_hip_qn_path_logdet(s.h, int(m.size), m.ctypes.data_as(C.POINTER(C.c_double)),
                                              ld.ctypes.data_as(C.POINTER(C.c_double)),
                                              info.ctypes.data_as(C.POINTER(C.c_int32))))
        return ld, info

    def solve(self, v, mus, out=None, norms: bool = False):
        """out[j] = (B_FF + mus[j] I)^-1 v_F for the (n,) tensor v and up to 64 shifts, as a (k, n) tensor; pinned rows
        are +0.  One read pass, then one pass per 16 pairs that writes all k rows of out.  norms=True: returns
        (out, norm2, vx) with the float64 arrays norm2[j] = ||out[j]||^2 and vx[j] = v'out[j] from the host formulas;
        out=False with norms=True makes the read pass alone and returns (None, norm2, vx)."""
        s = self.solver
        v = s._qn_vec(v, "v")
        if v.dim() != 1:
            raise ValueError("v must have shape (n,)")
        m = self._mus(mus)
        k = int(m.size)
        ldo = s.n
        if out is False:
            if not norms:
                raise ValueError("out=False needs norms=True")
            out = None
        else:
            out, ldo = s._qn_cols_out(k, out)
        n2, vx = np.zeros(k), np.zeros(k)
        dp = C.POINTER(C.c_double)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_path_solve(s.h, v.data_ptr(), k, m.ctypes.data_as(dp),
                                             None if out is None else out.data_ptr(), ldo,
                                             n2.ctypes.data_as(dp) if norms else None,
                                             vx.ctypes.data_as(dp) if norms else None))
        s._qn_done()
        return (out, n2, vx) if norms else out

    def trust(self, g, delta: float, rtol: float = 0.0, max_it: int = 0, out=None) -> "TrustStep":
        """The trust-region step of the model on the free rows: step = -(B_FF + mu I)^-1 g_F with mu >= 0, ||step|| <=
        delta and mu (delta - ||step||) = 0 to rtol (0: 1e-10), by a safeguarded Newton iteration on the secular
        equation that runs on the host.  out: an (n,) tensor for the step, None to allocate one, False for the
        scalars alone.  Returns a TrustStep; its step is never outside the region (norm <= delta (1 + rtol)): if max_it evaluations do not get to
        rtol it is the step at the upper end of the bracket (norm < delta), and if they find no shift with norm <= delta
        at all the call raises LbfgsbError (LBFGSB_E_STATE) and writes nothing.  on_boundary says mu > 0."""
        s = self.solver
        g = s._qn_vec(g, "g")
        if g.dim() != 1:
            raise ValueError("g must have shape (n,)")
        if out is False:
            out = None
        else:
            out, _ = s._qn_cols_out(1, out)
        res = np.zeros(4)
        iters = C.c_int32(0)
        s.wait_stream()
        check(s.lib.lbfgsb_hip_qn_path_trust(s.h, g.data_ptr(), float(delta), float(rtol), int(max_it),
                                             None if out is None else out.data_ptr(),
                                             res.ctypes.data_as(C.POINTER(C.c_double)), C.byref(iters)))
        s._qn_done()
        if out is not None and out.dim() == 2:
            out = out[0]
        return TrustStep(out, float(res[0]), float(res[1]), float(res[2]), bool(res[3]), int(iters.value))


class QnOperator:
    """The curvature model of a DeviceSolver's last return as a linear operator on this rank's rows: H = B^-1
    (inverse=True, what scipy's L-BFGS-B returns as hess_inv, but starting from the solver's theta) or B.
    op @ v and op.matvec(v) take an (n,) tensor, op.matmat(V) an (n, k) one (columns are vectors, as in scipy);
    op.diagonal() is diag(A).  Every call reads the solver's state as it is at that moment."""

    def __init__(self, solver: DeviceSolver, inverse: bool = True, root: bool = False):
        self.solver, self.inverse, self.root = solver, bool(inverse), bool(root)
        self.shape = (solver.n, solver.n)
        self.dtype = np.dtype(solver.real)

    def matvec(self, v):
        return self.solver.qn_apply(v, inverse=self.inverse, sqrt=self.root)

    def matmat(self, vs):
        if vs.dim() != 2 or vs.shape[0] != self.shape[1]:
            raise ValueError("matmat takes an (n, k) tensor")
        return self.solver.qn_apply(vs.t().contiguous(), inverse=self.inverse, sqrt=self.root).t()

    def diagonal(self):
        if self.root:
            raise ValueError("qn_diag takes B or H, not a square root")
        return self.solver.qn_diag(inverse=self.inverse)

    def sqrt(self) -> "QnOperator":
        """the symmetric square root A^(1/2) of this operator, with matvec / matmat (at most 64 stored pairs)"""
        if self.root:
            raise ValueError("this operator is a square root already")
        return QnOperator(self.solver, self.inverse, root=True)

    def shifted(self, d=None, mu: float = 0.0) -> "QnShifted":
        """(B + mu I + diag(d))^-1 as a QnShifted (DeviceSolver.qn_shift): the shift is always added to B, whichever
        of B and H this operator is"""
        return self.solver.qn_shift(d=d, mu=mu)

    def path(self, status=None, codes=(1, 2, 3)) -> "QnPath":
        """(B_FF + mu I)^-1 on the rows that `status` and `codes` leave free, over any number of shifts, as a QnPath
        (DeviceSolver.qn_path): the shifts are added to B, whichever of B and H this operator is"""
        return self.solver.qn_path(status=status, codes=codes)

    def logdet(self) -> float:
        """log det A over all rows of all ranks (of a root: half of it)"""
        v = self.solver.qn_logdet(inverse=self.inverse)
        return 0.5 * v if self.root else v

    def sample(self, k: int, seed: int, first: int = 0, mean=None, scale: float = 1.0, log_prob: bool = False):
        """k draws from N(mean, scale^2 A) as a (k, n) tensor (DeviceSolver.qn_draw); log_prob=True: (draws, logp)
        with the draws' log-densities as a numpy (k,) array"""
        if self.root:
            raise ValueError("sample() draws with covariance A: call it on the operator, not on its root")
        return self.solver.qn_draw(k, seed, first=first, mean=mean, scale=scale, inverse=self.inverse,
                                   return_logpdf=log_prob)

    def quad(self, v, center=None):
        """(v - center)' A (v - center) over all rows of all ranks (DeviceSolver.qn_quad)"""
        if self.root:
            raise ValueError("quad() takes B or H, not a square root")
        return self.solver.qn_quad(v, center=center, inverse=self.inverse)

    def gram(self, v, center=None):
        """(v_a - center)' A (v_b - center) as a numpy (k, k) array (DeviceSolver.qn_gram)"""
        if self.root:
            raise ValueError("gram() takes B or H, not a square root")
        return self.solver.qn_gram(v, center=center, inverse=self.inverse)

    def block(self, ia, ib=None):
        """A[ia, ib] at global 0-based index lists as a numpy (ka, kb) array (DeviceSolver.qn_block)"""
        if self.root:
            raise ValueError("block() takes B or H, not a square root")
        return self.solver.qn_block(ia, ib, inverse=self.inverse)

    def columns(self, idx, out=None):
        """the columns A[:, idx[j]] as a (k, n) tensor of this rank's rows (DeviceSolver.qn_cols)"""
        if self.root:
            raise ValueError("columns() takes B or H, not a square root")
        return self.solver.qn_cols(idx, out=out, inverse=self.inverse)

    def marginal(self, idx):
        """the block of this operator at idx: with inverse=True the marginal covariance of those parameters"""
        return self.block(idx)

    def _spectrum(self, what):
        if self.root:
            raise ValueError("%s takes B or H, not a square root" % what)
        return self.solver.qn_eig(inverse=self.inverse)

    def eigvalsh(self):
        """(bulk, values) of DeviceSolver.qn_eig: the eigenvalues off the bulk value, ascending, as a numpy array"""
        return self._spectrum("eigvalsh()")

    def eigh(self):
        """(bulk, values, vectors): A = bulk I + U diag(values - bulk) U', vectors a (r, n) tensor whose rows are the
        orthonormal columns of U on this rank's rows (DeviceSolver.qn_eigvec)"""
        bulk, values = self._spectrum("eigh()")
        return bulk, values, self.solver.qn_eigvec(inverse=self.inverse)

    def cond(self) -> float:
        """the 2-norm condition number max / min over {bulk, values}, with no pass over W beyond the Gram pass (bulk is
        an eigenvalue whenever n_global exceeds the number of values)"""
        bulk, values = self._spectrum("cond()")
        ev = list(values) + ([bulk] if self.solver.n_global > len(values) else [])
        return float(max(ev) / min(ev))

    def log_prob(self, x, mean=None, scale: float = 1.0):
        """log N(x; mean, scale^2 A) with this operator as the covariance (DeviceSolver.qn_logpdf)"""
        if self.root:
            raise ValueError("log_prob() takes the covariance A: call it on the operator, not on its root")
        return self.solver.qn_logpdf(x, mean=mean, scale=scale, inverse=self.inverse)

    def __matmul__(self, v):
        return self.matvec(v) if v.dim() == 1 else self.matmat(v)
