// Test-only C doorway into the host algebra of the model plus a diagonal in host_dense.hpp (qn_shift_factor,
// qn_shift_coef; qn_coef_h for the unshifted comparison), built by tests/test_qn_shift_cpu.py with g++: the factor of
// K, the coefficients of a solve and the log-determinant are checked against dense numpy without a GPU.
#include "../include/lbfgsb_hip.h"
#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
// sy: m x m, lower triangle of S'Y; sts: col x col, all of S'S; gw: 2col x 2col weighted Gram (S block first) or NULL
int qs_factor(int col, double theta, const double *sy, int m, const double *sts, const double *gw, double *kf,
              double *logdet) {
  return lbh::qn_shift_factor(col, theta, sy, m, sts, col, gw, kf, logdet);
}
int qs_coef(int col, double theta, const double *kf, const double *stv, const double *ytv, double *cs, double *cy) {
  return lbh::qn_shift_coef(col, theta, kf, stv, ytv, cs, cy);
}
int qs_coef_h(int col, double theta, const double *sty, const double *yty, const double *dg, const double *stv,
              const double *ytv, double *cs, double *cy) {
  return lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
}
}
