// Test-only C doorway into the root algebra of host_dense.hpp (jacobi_eig, qn_root, with qn_nmat over qn_coef_b /
// qn_coef_h) and into the generator of philox.hpp, built by tests/test_qn_root_cpu.py with g++: the square root, the
// log-determinant and the Philox known answers are checked against numpy without a GPU.
#include <cstdint>
#include <vector>

#include "../lbfgsb_amd/csrc/host_dense.hpp"
#include "../lbfgsb_amd/csrc/philox.hpp"

extern "C" {
int rs_formt(int m, double *wt, const double *sy, const double *ss, int col, double theta) {
  return lbh::formt(m, wt, sy, ss, col, theta);
}
int rs_jacobi(int d, double *a, double *v, double *w) { return lbh::jacobi_eig(d, a, v, w); }
// mode 0: B from (m, sy, wt), mode 1: H from (sty, yty, dg); g = [S, Y]'[S, Y] (2col x 2col).  C into cm, the
// log-det sum into logsum, N into nm.  Returns qn_nmat's info (> 0) or qn_root's (< 0).
int rs_root(int mode, int m, const double *sy, const double *wt, int col, double theta, const double *sty,
            const double *yty, const double *dg, const double *g, double *nm, double *cm, double *logsum) {
  const int d = 2 * col;
  const int info = lbh::qn_nmat(
      col,
      [&](const double *stv, const double *ytv, double *cs, double *cy) {
        return mode == 0 ? lbh::qn_coef_b(m, sy, wt, col, theta, stv, ytv, cs, cy)
                         : lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
      },
      nm);
  if (info) return info;
  std::vector<double> work((size_t)6 * d * d + d + 1);
  return lbh::qn_root(d, mode == 0 ? theta : 1.0 / theta, g, nm, cm, logsum, work.data());
}
// qn_root alone on a caller's symmetric N
int rs_root_n(int d, double alpha, const double *g, const double *nm, double *cm, double *logsum) {
  std::vector<double> work((size_t)6 * d * d + d + 1);
  return lbh::qn_root(d, alpha, g, nm, cm, logsum, work.data());
}
void rs_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
  lbp::philox4x32_10(c, key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}
void rs_uniforms(uint64_t seed, uint64_t row, uint64_t pair, double *u, double *v) {
  lbp::uniforms(seed, row, pair, *u, *v);
}
}
