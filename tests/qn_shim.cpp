// Test-only C doorway into the curvature-model algebra of host_dense.hpp (qn_coef_b, qn_coef_h, qn_nmat,
// qn_pack_n), built by tests/test_qn_host_cpu.py with g++: the compact inverse and the matrices of the diagonals
// are checked against numpy without a GPU.
#include <cstdint>

#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
int qs_formt(int m, double *wt, const double *sy, const double *ss, int col, double theta) {
  return lbh::formt(m, wt, sy, ss, col, theta);
}
int qs_coef_b(int m, const double *sy, const double *wt, int col, double theta, const double *stv,
              const double *ytv, double *cs, double *cy) {
  return lbh::qn_coef_b(m, sy, wt, col, theta, stv, ytv, cs, cy);
}
int qs_coef_h(int col, double theta, const double *sty, const double *yty, const double *dg, const double *stv,
              const double *ytv, double *cs, double *cy) {
  return lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
}
// mode 0: N_B from (m, sy, wt); mode 1: N_H from (sty, yty, dg)
int qs_nmat(int mode, int m, const double *sy, const double *wt, int col, double theta, const double *sty,
            const double *yty, const double *dg, double *nm) {
  return lbh::qn_nmat(
      col,
      [&](const double *stv, const double *ytv, double *cs, double *cy) {
        return mode == 0 ? lbh::qn_coef_b(m, sy, wt, col, theta, stv, ytv, cs, cy)
                         : lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
      },
      nm);
}
void qs_pack_n(int col, int mc, const double *nm, double *np) { lbh::qn_pack_n(col, mc, nm, np); }
}
