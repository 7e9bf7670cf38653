"""Eigenvalues and eigenvectors of the curvature model on a sharded context: 2 rank processes on one GPU with a gloo
host group, n = 4099 split unevenly.  The eigenvalues are the same bits on both ranks; the concatenated vectors pass
the single-rank checks of tests/test_gpu_qn_eig.py against ONE context that imported the concatenated state
(orthonormal, A U = U Lambda and A^-1 U = U / Lambda through its qn_apply, within _check_root's bounds), and their
signs agree with that context's own vectors."""
import numpy as np
import pytest

from _sharded import import_glued, launch_workers
from test_gpu_qn_eig import SEP, _orth_bound
from test_gpu_qn_root import _cond_and_norm, _model

pytestmark = pytest.mark.gpu


def test_sharded_spectrum_and_vectors(oracle_built, tmp_path):
    import torch
    import lbfgsb_amd as la
    n, m, iters, world = 4099, 7, 10, 2
    parts = launch_workers("_qn_eig_mr_worker.py", world, n, m, iters, prefix=str(tmp_path / "qneig"))
    assert len({int(p["n_loc"]) for p in parts}) > 1                       # an uneven split
    assert int(parts[0]["col"]) == m and int(parts[0]["head"]) > 1          # a full ring whose head has wrapped
    for key in ("bulk_b", "bulk_h", "lam_b", "lam_h"):
        assert parts[0][key].tobytes() == parts[1][key].tobytes(), key     # the same bits on every rank
    one = la.DeviceSolver(n, m)
    try:
        wa = import_glued(one, parts, n, m)
        one.dsave[0] = float(parts[0]["theta"])  # (what _model reads)
        B, col, theta, W = _model(one, wa)
        cond, nb = _cond_and_norm(B, theta, W)
        for key, inverse in (("b", False), ("h", True)):
            lam = parts[0]["lam_" + key]
            r = len(lam)
            assert 1 <= r <= 2 * m
            bulk1, lam1 = one.qn_eig(inverse=inverse)
            assert len(lam1) == r and np.abs(lam1 - lam).max() <= 1e-12 * np.abs(lam).max()
            U = np.concatenate([p["u_" + key] for p in parts], axis=1)
            assert U.shape == (r, n)
            e_orth = float(np.linalg.norm(U @ U.T - np.eye(r)))
            na = cond / nb if inverse else nb
            assert e_orth <= _orth_bound(cond, na, lam, float(parts[0]["bulk_" + key]), np.linalg.norm(U)), e_orth
            sep = np.abs(lam - float(parts[0]["bulk_" + key])) >= SEP * float(parts[0]["bulk_" + key])
            assert np.linalg.norm(U[sep] @ U[sep].T - np.eye(int(sep.sum()))) <= 1e-10 * cond * np.linalg.norm(U[sep])
            Ut = torch.from_numpy(U).cuda()
            lt = torch.from_numpy(lam).cuda()[:, None]
            for is_h, ref in ((inverse, lt * Ut), (not inverse, Ut / lt)):
                err = float(torch.linalg.norm(one.qn_apply(Ut, inverse=is_h) - ref))
                bound = 1e-10 * cond * float(torch.linalg.norm(ref)) if is_h else 1e-10 * nb * float(np.linalg.norm(U))
                print("%s, apply %s: %.3e (bound %.3e)" % (key, "H" if is_h else "B", err, bound))
                assert err <= bound
            # the signs: a function of the replicated coefficients, not of the sharding
            U1 = one.qn_eigvec(inverse=inverse).cpu().numpy()
            dots = np.einsum("ij,ij->i", U, U1)
            print("%s: u_sharded . u_one in [%.15f, %.15f]" % (key, dots.min(), dots.max()))
            assert np.all(dots > 0.0)
    finally:
        one.close()
