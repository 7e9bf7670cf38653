// Test-only C doorway into the host algebra behind the factor of the model plus a diagonal in host_dense.hpp
// (qn_shift_root on qn_shift_factor's factor; qn_coef_h for the unshifted comparison), built by
// tests/test_qn_shift_root_cpu.py with g++: C and the log-determinant sum are checked against dense numpy without a GPU.
#include <vector>

#include "../include/lbfgsb_hip.h"
#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
// sy: m x m, lower triangle of S'Y; sts: col x col, all of S'S; gw: 2col x 2col weighted Gram (S block first)
int qsr_factor(int col, double theta, const double *sy, int m, const double *sts, const double *gw, double *kf,
               double *logdet) {
  return lbh::qn_shift_factor(col, theta, sy, m, sts, col, gw, kf, logdet);
}
// cm: 2col x 2col, C of L = diag(sqrt w) + diag(w) [S, Y] C [S, Y]' diag(sqrt w); *logsum: sum log1p(delta_i)
int qsr_root(int col, double theta, const double *kf, const double *gw, double *cm, double *logsum) {
  const size_t d = 2 * (size_t)col;
  std::vector<double> work(7 * d * d + d + 1);
  return lbh::qn_shift_root(col, theta, kf, gw, cm, logsum, work.data());
}
int qsr_coef_h(int col, double theta, const double *sty, const double *yty, const double *dg, const double *stv,
               const double *ytv, double *cs, double *cy) {
  return lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
}
}
