"""The test side of the "several ranks on one GPU" tests: the one launcher of rank processes, the build of the RCCL
stand-in, and the single context that the sharded results are compared with.  The worker side is tests/_mr_common.py.

launch_ranks ends what it started: when a rank fails, or the deadline passes, its collective partners are stopped and
reaped before the error is raised.  After a rank has ended by signal or hung, no later launch of this process starts
anything: nothing may be started on a card after a process on it has aborted, faulted or hung."""
import contextlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

GRACE_S = 3.0           # the partners of a failed rank may still leave on their own for this long
TERM_TO_KILL_S = 2.0   # from terminate() to kill()
POLL_S = 0.05

_faulted = None         # the launch after which nothing more is started (a rank ended by signal, or the deadline passed)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def fake_rccl():
    """Build tests/fake_rccl.cpp (shared-memory stand-in for the RCCL entry points) on demand."""
    so = os.path.join(HERE, "_build", "libfake_rccl.so")
    src = os.path.join(HERE, "fake_rccl.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        # (compiled as HIP: the stand-in launches one tiny kernel -- the stream-side wait of a collective)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-fPIC", "-shared", src, "-o", so, "-lrt", "-lpthread"])
    return so


def _wait_all(procs, seconds):
    end = time.monotonic() + seconds
    while any(p.poll() is None for p in procs) and time.monotonic() < end:
        time.sleep(POLL_S)


def _stop(procs, grace):
    """leave no child running: `grace` seconds to exit on their own, terminate(), TERM_TO_KILL_S later kill(), and
    every one reaped; the ranks that had to be stopped"""
    _wait_all(procs, grace)
    stopped = [r for r, p in enumerate(procs) if p.poll() is None]
    for r in stopped:
        procs[r].terminate()
    _wait_all(procs, TERM_TO_KILL_S)
    for p in procs:
        if p.poll() is None:
            p.kill()
        p.wait()
    return stopped


def launch_ranks(argvs, timeout=300.0, env=None):
    """Start one child per argv list (stdout and stderr inherited) and return once every one has exited 0.  Raises as
    soon as a rank exits otherwise, or when `timeout` seconds have passed -- after the remaining ranks were stopped."""
    global _faulted
    what = "%d x %s" % (len(argvs), " ".join(os.path.basename(a) for a in argvs[0][:2]))
    if _faulted is not None:
        raise RuntimeError("%s: nothing started, because of an earlier launch: %s" % (what, _faulted))
    procs, late, grace = [], False, 0.0
    try:
        for argv in argvs:
            procs.append(subprocess.Popen(argv, env=env))
        deadline = time.monotonic() + timeout
        while True:
            rcs = [p.poll() for p in procs]
            if all(rc == 0 for rc in rcs):
                return
            late = time.monotonic() >= deadline
            if late or any(rc not in (None, 0) for rc in rcs):
                grace = 0.0 if late else GRACE_S
                break
            time.sleep(POLL_S)
    finally:
        stopped = _stop(procs, grace)
    ends = ["rank %d: %d (%s)" % (r, p.returncode, "stopped by the launcher" if r in stopped else "on its own")
            for r, p in enumerate(procs)]
    msg = "%s: %s%s" % (what, "no end after %g s; " % timeout if late else "", ", ".join(ends))
    if late or any(p.returncode < 0 for r, p in enumerate(procs) if r not in stopped):
        _faulted = msg
    raise RuntimeError(msg)


def launch_workers(worker, world, *args, prefix, timeout=300.0, env=None):
    """`world` ranks of tests/<worker> (argv: rank world port *args prefix); what they wrote: every rank's
    prefix.<rank>.npz, or the one JSON that rank 0 of _mr_worker.py writes to `prefix`"""
    port = free_port()
    launch_ranks([[sys.executable, os.path.join(HERE, worker), str(r), str(world), str(port)]
                  + [str(a) for a in args] + [prefix] for r in range(world)], timeout, env)
    if worker == "_mr_worker.py":
        with open(prefix) as fh:
            return json.load(fh)
    return [np.load(prefix + ".%d.npz" % r) for r in range(world)]


def glue(parts, n, m):
    """the per-rank exports (the reference's wa layout over n_local rows, host matrices replicated) as one wa over
    all n rows"""
    nl = [int(p["n_loc"]) for p in parts]
    was = [p["wa"] for p in parts]
    fixed = 11 * m * m
    segs = []
    for blk in range(2):  # Ws, Wy: m columns of n rows
        segs.append(np.concatenate([w[blk * m * k:(blk + 1) * m * k].reshape(m, k) for w, k in zip(was, nl)],
                                   axis=1).ravel())
    segs.append(was[0][2 * m * nl[0]:2 * m * nl[0] + fixed])
    for j in range(5):  # z, r, d, t, xp
        segs.append(np.concatenate([w[2 * m * k + fixed + j * k:2 * m * k + fixed + (j + 1) * k]
                                    for w, k in zip(was, nl)]))
    segs.append(was[0][2 * m * nl[0] + fixed + 5 * nl[0]:])
    wa = np.concatenate(segs)
    assert wa.size == 2 * m * n + fixed + 5 * n + 8 * m
    return wa


@contextlib.contextmanager
def one_context(n, m):
    """ONE context over all n rows at its FG_START return (no pair yet), closed on exit"""
    import torch
    import lbfgsb_amd as la
    one = la.DeviceSolver(n, m)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        nbd = torch.zeros(n, dtype=torch.int32, device="cuda")
        assert one.setulb(x, x.clone(), x.clone(), nbd, g, 0.0, 0.0).startswith("FG_START")
        yield one
    finally:
        one.close()


def import_glued(one, parts, n, m):
    """put the ranks' exported states, glued, into the context `one`; the glued wa"""
    isave = parts[0]["isave"]
    wa = glue(parts, n, m)
    one.import_state(wa, np.zeros(3 * n, np.int32), isave)
    one.isave[:] = isave
    return wa
