"""The stand-in for librccl that the multi-rank tests run on (tests/fake_rccl.cpp) must be able to FAIL
the way RCCL fails, or the 8-rank path's only safety net cannot see a regression:
  * a collective returns BEFORE its data have moved (asynchronous on the caller's stream);
  * ranks that pass different counts are caught: the result is poisoned, the next call is refused.
Two rank processes, one GPU, the stand-in driven directly through ctypes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class UniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def _lib():
    return _lib_at(os.environ["LBFGSB_FAKE_RCCL_SO"])


def _lib_at(so):
    lib = C.CDLL(so)
    lib.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
    lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    lib.ncclAllGather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    lib.ncclCommDestroy.argtypes = [C.c_void_p]
    lib.ncclCommCount.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.ncclCommUserRank.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    return lib


NCCL_DOUBLE = 8   # ncclFloat64 (rccl.h)


def _one_rank(body, rank, uid_hex):
    """run body(rank, comm, lib, stream, torch) as one rank of a 2-rank communicator; (result, rc of destroy)"""
    import torch
    lib = _lib()
    uid = UniqueId.from_buffer_copy(bytes.fromhex(uid_hex))
    torch.cuda.set_device(0)
    comm = C.c_void_p()
    assert lib.ncclCommInitRank(C.byref(comm), 2, uid, rank) == 0
    n, r = C.c_int(), C.c_int()
    assert lib.ncclCommCount(comm, C.byref(n)) == 0 and lib.ncclCommUserRank(comm, C.byref(r)) == 0
    assert (n.value, r.value) == (2, rank)
    stream = torch.cuda.Stream()
    res = body(rank, comm, lib, stream, torch)
    stream.synchronize()
    return res, lib.ncclCommDestroy(comm)


def scenario_async():
    def body(rank, comm, lib, stream, torch):
        k = 1000
        send = torch.full((k,), float(rank + 1), dtype=torch.float64, device="cuda")
        recv = torch.full((2 * k,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            # plenty of work in front of the collective on the same stream (~tens of ms) ...
            a = torch.ones((4096, 4096), device="cuda")
            for _ in range(40):
                a = (a @ a) * 1e-4
            rc = lib.ncclAllGather(send.data_ptr(), recv.data_ptr(), k, NCCL_DOUBLE, comm,
                                   C.c_void_p(stream.cuda_stream))
            # ... so when the call RETURNS the stream has not reached it: nothing has been written yet
            returned_before_done = not stream.query()
        assert rc == 0
        stream.synchronize()
        got = recv.cpu().numpy()
        assert np.all(got[:k] == 1.0) and np.all(got[k:] == 2.0)
        return bool(returned_before_done)
    return body


def scenario_mismatch():
    def body(rank, comm, lib, stream, torch):
        k = 64 + rank    # rank 0 passes 64 elements, rank 1 passes 65
        send = torch.full((65,), float(rank + 1), dtype=torch.float64, device="cuda")
        recv = torch.zeros(130, dtype=torch.float64, device="cuda")
        rc1 = lib.ncclAllGather(send.data_ptr(), recv.data_ptr(), k, NCCL_DOUBLE, comm,
                                C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        poisoned = bool(np.all(np.isnan(recv.cpu().numpy()[:2 * k])))
        rc2 = lib.ncclAllGather(send.data_ptr(), recv.data_ptr(), 64, NCCL_DOUBLE, comm,
                                C.c_void_p(stream.cuda_stream))
        return rc1, poisoned, rc2
    return body


def _child(name):
    """the two ranks are two child processes: each has hardware queues of its own, so a rank's stream-side wait
    never sits in front of the other rank's copies (ranks that are threads of one process can share a queue)"""
    from _sharded import fake_rccl
    so = fake_rccl()
    uid = UniqueId()
    assert _lib_at(so).ncclGetUniqueId(C.byref(uid)) == 0
    env = dict(os.environ, LBFGSB_FAKE_RCCL_SO=so)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), name, str(rank), bytes(uid).hex()],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for rank in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    err = "".join(e for _, e in outs)
    assert [p.returncode for p in procs] == [0, 0], err[-3000:]
    return [json.loads(o.strip().splitlines()[-1]) for o, _ in outs], err


def test_all_gather_is_asynchronous_and_correct():
    out, _ = _child("async")
    assert out[0][0] and out[1][0], "ncclAllGather blocked until its data had moved"
    assert out[0][1] == 0 and out[1][1] == 0


def test_unequal_counts_are_caught():
    out, err = _child("mismatch")
    for (rc1, poisoned, rc2), rc_destroy in out:
        assert rc1 == 0             # (asynchronous: the call itself cannot know yet)
        assert poisoned             # the result of the mismatched collective is NaN, not plausible numbers
        assert rc2 != 0             # ... and the communicator refuses to go on
        assert rc_destroy != 0
    assert "real RCCL would hang or corrupt here" in err


if __name__ == "__main__":
    body = {"async": scenario_async, "mismatch": scenario_mismatch}[sys.argv[1]]()
    print(json.dumps(_one_rank(body, int(sys.argv[2]), sys.argv[3])))
