"""The model over a range of shifts on sharded contexts: 2 and 3 rank processes on one GPU (a gloo host group, or the
library's communicator path with the shared-memory RCCL stand-in of tests/fake_rccl.cpp), n = 1000 split unevenly,
m = 10, under two masks: every third row and a run of 40 rows across every rank boundary pinned, and EVERY row of
rank 1 pinned (that rank contributes exact zeros to every sum).  The pinned count is global; the log det curve, the
norms and the trust scalars are the same bits on every rank; the concatenated solves and the step are within 1e-12
(relative, in the 2-norm: the tolerance of tests/test_gpu_qn_shift_sharded.py) of ONE context's that imported the
concatenated state, the host numbers within 1e-12 relative; pinned rows are exactly +0; and at one shift per mask the
sharded results and the one context's are both inside the bounds of the dense truth of the glued pairs, entry by
entry (tests/_qn_path_truth.py)."""
import os
import sys

import numpy as np
import pytest

import _qn_path_truth as pt
import _qn_synth as qs
import _qn_truth as qt
from _sharded import fake_rccl, import_glued, launch_workers, one_context

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,mode,iters", [(2, "gloo", 14), (3, "fakerccl", 13)])
def test_sharded_path(oracle_built, tmp_path, monkeypatch, world, mode, iters):
    import torch
    sys.path.insert(0, HERE)
    try:
        import _qn_path_mr_worker as wk
    finally:
        sys.path.remove(HERE)
    n, m = 1000, 10
    if mode == "fakerccl":
        monkeypatch.setenv("LBFGSB_RCCL_LIBRARY", fake_rccl())
    parts = launch_workers("_qn_path_mr_worker.py", world, mode, n, m, iters, prefix=str(tmp_path / "qnpath"))
    assert len({int(p["n_loc"]) for p in parts}) == world                # an uneven split
    assert len({(int(p["col"]), int(p["head"])) for p in parts}) == 1
    assert int(parts[0]["col"]) == m
    vh = np.random.default_rng(wk.SEED).standard_normal(n)
    v = torch.from_numpy(vh).cuda()
    with one_context(n, m) as one:
        wa = import_glued(one, parts, n, m)
        S, Y = qs.ring_pairs(wa, n, m, int(parts[0]["col"]), int(parts[0]["head"]))
        truth = qt.Truth(S, Y, g=2)
        for mask in wk.MASKS:
            pin = wk.pins(n, world, mask)
            if mask == "rank1":
                r0, nl = wk.cut(n, world, 1)
                assert pin[r0:r0 + nl].all() and not pin.all()
            for key in ("_pinned", "_logdet", "_info", "_n2", "_vx", "_trust"):
                assert len({p[mask + key].tobytes() for p in parts}) == 1, mask + key   # the same bits on every rank
            p0 = parts[0]
            assert int(p0[mask + "_pinned"]) == int(pin.sum()) and not p0[mask + "_info"].any()
            path = one.qn_path(torch.from_numpy(np.where(pin, 2, 0).astype(np.int8)).cuda())
            assert path.pinned == int(pin.sum())
            ld, info = path.logdet(wk.MUS)
            out, n2, vx = path.solve(v, wk.MUS, norms=True)
            tr = path.trust(v, 0.05 * float(np.sqrt(p0[mask + "_n2"][1])))
            x = np.concatenate([p[mask + "_x"] for p in parts], axis=1)
            step = np.concatenate([p[mask + "_step"] for p in parts])
            ref_x, ref_s = out.cpu().numpy(), tr.step.cpu().numpy()
            ex = np.linalg.norm(x - ref_x, axis=1) / np.linalg.norm(ref_x, axis=1)
            es = np.linalg.norm(step - ref_s) / np.linalg.norm(ref_s)
            rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))  # noqa: E731
            el, en, ev = rel(p0[mask + "_logdet"], ld), rel(p0[mask + "_n2"], n2), rel(p0[mask + "_vx"], vx)
            et = rel(p0[mask + "_trust"][:3], [tr.mu, tr.norm, tr.predicted])
            print("%s: sharded against one rank: solves %.2e, step %.2e, log det %.2e, norms %.2e, v'x %.2e, trust %.2e"
                  % (mask, ex.max(), es, el, en, ev, et))
            assert ex.max() <= 1e-12 and es <= 1e-12 and el <= 1e-12 and en <= 1e-12 and ev <= 1e-12
            assert et <= 1e-9  # (mu is found to rtol = 1e-10 on either side)
            assert p0[mask + "_trust"][3] == 1.0 and tr.on_boundary
            assert qt.pos_zero(x[:, pin]).all() and qt.pos_zero(step[pin]).all()
            assert qt.pos_zero(ref_x[:, pin]).all() and qt.pos_zero(ref_s[pin]).all()
            # ... and both within the bounds of the dense truth of the glued pairs (g = 2: a state from a run), entry by
            # entry, at the shifts TRUTH_AT (a 1000 x 1000 reference in extended precision each)
            for j in wk.TRUTH_AT:
                op = pt.shifted(truth, pin, wk.MUS[j])
                ref = op.apply(vh[None])
                ba = op.bound_apply(vh[None], np.float64, ref)
                qt.check("sharded path solve", x[j:j + 1], ref, ba)
                qt.check("one-context path solve", ref_x[j:j + 1], ref, ba)
                bl = op.bound_logdet(op.sum_abs_log, op.cond_a)
                qt.check("sharded path logdet", p0[mask + "_logdet"][j], op.logdet, bl)
                qt.check("sharded path ||x||^2", p0[mask + "_n2"][j], pt.norm2(op, vh), pt.bound_norm2(op, vh))
                qt.check("sharded path v'x", p0[mask + "_vx"][j], op.quad(vh[None])[0, 0], op.bound_quad(vh[None])[0, 0])
