// Test-only C doorway into the eigen-decomposition of the curvature model in host_dense.hpp (qn_eig over
// qn_spectrum, with qn_nmat over qn_coef_b / qn_coef_h), built by tests/test_qn_eig_cpu.py with g++: eigenvalues,
// coefficient columns and the sign rule are checked against numpy without a GPU.
#include <cstdint>
#include <vector>

#include "../include/lbfgsb_hip.h"
#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
double es_cut() { return LBFGSB_QN_EIG_CUT; }
int es_formt(int m, double *wt, const double *sy, const double *ss, int col, double theta) {
  return lbh::formt(m, wt, sy, ss, col, theta);
}
// mode 0: B from (m, sy, wt), mode 1: H from (sty, yty, dg); g = [S, Y]'[S, Y] (2col x 2col), rmax = min(2col, n).
// *r directions, lam[0 .. r) ascending, coef (2col x r, column-major), N into nm.  Returns qn_nmat's info (> 0) or
// qn_eig's (< 0).
int es_eig(int mode, int m, const double *sy, const double *wt, int col, double theta, const double *sty,
           const double *yty, const double *dg, const double *g, int64_t rmax, double *nm, int *r, double *lam,
           double *coef) {
  const int d = 2 * col;
  const int info = lbh::qn_nmat(
      col,
      [&](const double *stv, const double *ytv, double *cs, double *cy) {
        return mode == 0 ? lbh::qn_coef_b(m, sy, wt, col, theta, stv, ytv, cs, cy)
                         : lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
      },
      nm);
  if (info) return info;
  std::vector<double> work((size_t)7 * d * d + 6 * d + 1);
  return lbh::qn_eig(d, mode == 0 ? theta : 1.0 / theta, LBFGSB_QN_EIG_CUT, rmax, g, nm, r, lam, coef, work.data());
}
// qn_eig alone on a caller's symmetric N
int es_eig_n(int d, double alpha, const double *g, const double *nm, int64_t rmax, int *r, double *lam, double *coef) {
  std::vector<double> work((size_t)7 * d * d + 6 * d + 1);
  return lbh::qn_eig(d, alpha, LBFGSB_QN_EIG_CUT, rmax, g, nm, r, lam, coef, work.data());
}
}
