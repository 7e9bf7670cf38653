// Test-only C doorway into the host combination of a Gram matrix of the curvature model (host_dense.hpp,
// qn_gram_combine), built by tests/test_qn_gram_cpu.py with g++: G = alpha D'D + P'N P from given sums is checked
// against numpy without a GPU.  The coefficient map c = N p is a dense product with the matrix handed in.
#include <cstdint>

#include "../lbfgsb_amd/csrc/host_dense.hpp"

extern "C" {
// nm: 2col x 2col, column-major; p: 2col x k, column-major; dtd: k x k with the upper triangle set; g: ldg x k
int qgs_combine(int col, int k, double alpha, const double *nm, const double *p, const double *dtd, int ldd,
                double *g, int64_t ldg) {
  const int d = 2 * col;
  return lbh::qn_gram_combine(
      col, k, alpha, p, dtd, ldd,
      [&](const double *stv, const double *ytv, double *cs, double *cy) {
        for (int i = 0; i < d; ++i) {
          double t = 0.0;
          for (int j = 0; j < d; ++j) t = t + nm[i + (size_t)j * d] * (j < col ? stv[j] : ytv[j - col]);
          (i < col ? cs[i] : cy[i - col]) = t;
        }
        return 0;
      },
      g, ldg);
}
// the same with a coefficient map that fails at vector `bad`: g must stay as it was
int qgs_combine_failing(int col, int k, double alpha, const double *p, const double *dtd, int ldd, int bad, double *g,
                        int64_t ldg) {
  int at = 0;
  return lbh::qn_gram_combine(
      col, k, alpha, p, dtd, ldd,
      [&](const double *, const double *, double *cs, double *cy) {
        for (int i = 0; i < col; ++i) cs[i] = cy[i] = 1.0;
        return at++ == bad ? 7 : 0;
      },
      g, ldg);
}
}
