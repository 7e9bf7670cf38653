"""Log-determinants, draws and square roots of the curvature model on sharded contexts: 2 and 3 rank processes on
one GPU (a gloo host group, or the library's communicator path with the shared-memory RCCL stand-in of
tests/fake_rccl.cpp), n = 4099 split unevenly.  log det is the same number on every rank; the concatenated draws
equal the draws of ONE context that imported the concatenated state -- a draw is a function of (seed, global row,
sample), not of the sharding -- and are bit-identical while no pair is stored."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_rccl():
    so = os.path.join(HERE, "_build", "libfake_rccl.so")
    src = os.path.join(HERE, "fake_rccl.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-fPIC", "-shared", src, "-o", so, "-lrt", "-lpthread"])
    return so


def _glue(parts, n, m):
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


@pytest.mark.parametrize("world,mode,m,iters", [(2, "gloo", 7, 10), (3, "fakerccl", 5, 9)])
def test_sharded_logdet_and_draws(oracle_built, tmp_path, monkeypatch, world, mode, m, iters):
    import torch
    import lbfgsb_amd as la
    sys.path.insert(0, HERE)
    try:
        import _qn_root_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n = 4099
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", _fake_rccl())
    port = _free_port()
    prefix = str(tmp_path / "qnroot")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_qn_root_mr_worker.py"), str(r), str(world),
                               str(port), mode, str(n), str(m), str(iters), prefix]) for r in range(world)]
    rcs = [p.wait(timeout=300) for p in procs]
    assert rcs == [0] * world, rcs
    parts = [np.load(prefix + ".%d.npz" % r) for r in range(world)]
    assert len({int(p["n_loc"]) for p in parts}) > 1                       # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m and int(parts[0]["head"]) > 1          # a full ring whose head has wrapped
    for key in ("ldb", "ldh", "ld0"):
        assert len({float(p[key]) for p in parts}) == 1, key               # the same bits on every rank
    assert float(parts[0]["ld0"]) == 0.0                                    # no pair, theta = 1

    rng = np.random.default_rng(17)
    mean = torch.from_numpy(rng.standard_normal(n)).cuda()
    V = torch.from_numpy(rng.standard_normal((3, n))).cuda()
    one = la.DeviceSolver(n, m)
    try:
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        g = torch.zeros_like(x)
        nbd = torch.zeros(n, dtype=torch.int32, device="cuda")
        assert one.setulb(x, x.clone(), x.clone(), nbd, g, 0.0, 0.0).startswith("FG_START")
        d0 = one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE).cpu().numpy()
        assert np.array_equal(np.concatenate([p["d0"] for p in parts], axis=1), d0)   # bit-identical at col = 0
        isave = parts[0]["isave"]
        one.import_state(_glue(parts, n, m), np.zeros(3 * n, np.int32), isave)
        one.isave[:] = isave
        ldb, ldh = one.qn_logdet(), one.qn_logdet(inverse=True)
        print("log det B: sharded %.16e, one rank %.16e" % (float(parts[0]["ldb"]), ldb))
        assert abs(float(parts[0]["ldb"]) - ldb) <= 1e-12 * abs(ldb)
        assert abs(float(parts[0]["ldh"]) - ldh) <= 1e-12 * abs(ldh)
        for key, inverse in (("db", False), ("dh", True)):
            ref = one.qn_draw(wk.K, wk.SEED, first=wk.FIRST, mean=mean, scale=wk.SCALE, inverse=inverse).cpu().numpy()
            got = np.concatenate([p[key] for p in parts], axis=1)
            err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            print("%s: |sharded - one rank| / |one rank| = %.3e" % (key, err))
            assert err <= 1e-12
        ref = one.qn_apply(V, sqrt=True, inverse=True).cpu().numpy()
        got = np.concatenate([p["rh"] for p in parts], axis=1)
        assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
    finally:
        one.close()
