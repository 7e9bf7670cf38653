// Test-only C doorway into the host side of lbfgsb_hip_qn_pairs_set / _push: qn_pairs_factor, qn_pairs_append and
// qn_gram_append of host_dense.hpp, built by tests/test_qn_pairs_cpu.py with g++ and checked against the oracle's
// matupd and formt without a GPU.
#include <vector>

#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
// sts, sty, yty: col x col, column-major, logical order.  sy, ss, wt: m x m, column-major.
int qp_factor(int m, int col, const double *sts, const double *sty, const double *yty, double theta_in, double *sy,
              double *ss, double *wt, double *theta) {
  return lbh::qn_pairs_factor(m, col, sts, sty, yty, theta_in, sy, ss, wt, theta);
}
// state: col, head, itail (in / out).  s_old, y_old: s_j's and y_j's over the pairs stored before the call.
int qp_append(int m, int *col, int *head, int *itail, double *sy, double *ss, double *wt, double *theta,
              const double *s_old, const double *y_old, double sts, double sty, double yty, double theta_in) {
  return lbh::qn_pairs_append(m, *col, *head, *itail, sy, ss, wt, *theta, s_old, y_old, sts, sty, yty, theta_in);
}
// g: colold x colold in, the Gram after the step out (at most m x m); returns its order
int qp_gram_append(int m, int colold, double *g, const double *cnew, const double *rnew, double diag) {
  std::vector<double> v(g, g + (size_t)colold * colold);
  lbh::qn_gram_append(m, colold, v, cnew, rnew, diag);
  std::copy(v.begin(), v.end(), g);
  return colold == m ? m : colold + 1;
}
}
