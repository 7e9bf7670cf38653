"""Worker for tests/test_gpu_qn_eig_sharded.py: `world` processes on cuda:0, one block of rows each, reductions
through a gloo host group.  Runs the separable quadratic with all four bound types to iteration `iters`, then calls
the eigen-decomposition of the curvature model collectively (lbfgsb_hip_qn_eig / qn_eigvec, both modes, every
vector) and writes the spectra, this rank's rows of the vectors and its exported state to out_prefix.<rank>.npz.
usage: _qn_eig_mr_worker.py rank world port n m iters out_prefix"""
import sys

from _mr_common import join, leave, quadratic_rows, run_to


def run(rank, world, port, n, m, iters, out_prefix):
    from oracle import pyoracle as po

    sol, row0, n_loc, dev = join(rank, world, port, "gloo", n, m)
    x, g, l, u, nbd = quadratic_rows(po, n, m, row0, n_loc, dev)
    run_to(sol, x, l, u, nbd, g, iters)
    res = dict(theta=float(sol.dsave[0]))
    for key, inverse in (("b", False), ("h", True)):
        bulk, lam = sol.qn_eig(inverse=inverse)
        res.update({"bulk_" + key: bulk, "lam_" + key: lam,
                    "u_" + key: sol.qn_eigvec(inverse=inverse).cpu().numpy()})
    leave(sol, rank, out_prefix, res)


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
