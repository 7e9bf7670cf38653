// Test-only C doorway into the host side of the entries at index lists (lbfgsb_hip_qn_block / qn_cols and the shifted
// twins): qn_entries and qn_shift_entries of host_dense.hpp (with qn_nmat over qn_coef_b / qn_coef_h, and
// qn_shift_factor for the K factor) and the index check and chunk plan of qn_idx.hpp, built by
// tests/test_qn_idx_cpu.py with g++ and checked against dense numpy without a GPU.
#include <cstdint>
#include <vector>

#include "../lbfgsb_amd/csrc/host_dense.hpp"
#include "../lbfgsb_amd/csrc/qn_idx.hpp"

extern "C" {
int qi_formt(int m, double *wt, const double *sy, const double *ss, int col, double theta) {
  return lbh::formt(m, wt, sy, ss, col, theta);
}
// mode 0: B from (m, sy, wt), mode 1: H from (sty, yty, dg).  ra (ka x 2col), rb (kb x 2col): the gathered rows,
// column by column; ib == NULL: ib = ia.  a: ka x kb, leading dimension lda.  Returns qn_nmat's info.
int qi_entries(int mode, int m, const double *sy, const double *wt, int col, double theta, const double *sty,
               const double *yty, const double *dg, const double *ra, int ka, const int64_t *ia, const double *rb,
               int kb, const int64_t *ib, double *a, int64_t lda) {
  const int d = 2 * col;
  std::vector<double> nm((size_t)d * d + 1);
  if (col > 0) {
    const int info = lbh::qn_nmat(
        col,
        [&](const double *stv, const double *ytv, double *cs, double *cy) {
          return mode == 0 ? lbh::qn_coef_b(m, sy, wt, col, theta, stv, ytv, cs, cy)
                           : lbh::qn_coef_h(col, theta, sty, yty, col, dg, stv, ytv, cs, cy);
        },
        nm.data());
    if (info) return info;
  }
  lbh::qn_entries(col, mode == 0 ? theta : 1.0 / theta, nm.data(), ra, ka, ia, rb, kb, ib, ib == nullptr, a, lda);
  return 0;
}
// sy: m x m, lower triangle of S'Y; sts: col x col; gw: the weighted Gram (S block first); wa, wb: the weights at the
// indices.  Returns 100 + qn_shift_factor's code, or qn_shift_entries' info.
int qi_shift_entries(int col, double theta, const double *sy, int m, const double *sts, const double *gw,
                     const double *ra, const double *wa, int ka, const int64_t *ia, const double *rb, const double *wb,
                     int kb, const int64_t *ib, double *a, int64_t lda) {
  const int d = 2 * col;
  std::vector<double> kf((size_t)d * d + 1);
  double logdet = 0.0;
  const int rc = lbh::qn_shift_factor(col, theta, sy, m, sts, col, gw, kf.data(), &logdet);
  if (rc) return 100 + rc;
  return lbh::qn_shift_entries(col, theta, kf.data(), ra, wa, ka, ia, rb, wb, kb, ib, ib == nullptr, a, lda);
}
int64_t qi_bad(int64_t k, const int64_t *idx, int64_t n_global) { return lbk::qn_idx_bad(k, idx, n_global); }
// Walks the chunks of a list of k indices with ncol values each through a buffer of cap doubles.  Returns the number
// of chunks, or -1 when they do not cover 0 .. k - 1 exactly once and in order, -2 when a chunk does not fit the
// buffer, -3 when a chunk is empty.
int qi_walk(int64_t k, int ncol, int64_t cap) {
  const std::vector<lbk::QnIdxChunk> ch = lbk::qn_idx_chunks(k, ncol, cap);
  int64_t next = 0;
  for (const lbk::QnIdxChunk &c : ch) {
    if (c.j0 != next) return -1;
    if (c.kc < 1) return -3;
    if ((int64_t)c.kc * ncol > cap) return -2;
    next += c.kc;
  }
  return next == k ? (int)ch.size() : -1;
}
// qi_walk for every k <= kmax, col <= colmax (2 col values per index, and 2 col + 1 with the weight) and every
// capacity from one index to the whole list and one more -- per index count the smallest and the largest capacity
// that hold exactly that many (the plan depends on cap / ncol alone).  Returns the number of walks that failed or
// whose chunk count is not ceil(k / per); *walks: how many were made.
int64_t qi_walk_all(int kmax, int colmax, int64_t *walks) {
  int64_t bad = 0;
  *walks = 0;
  for (int64_t k = 1; k <= kmax; ++k)
    for (int col = 0; col <= colmax; ++col)
      for (int ncol = std::max(2 * col, 1); ncol <= 2 * col + 1; ++ncol)
        for (int64_t per = 1; per <= k + 1; ++per)
          for (int64_t cap : {per * ncol, per * ncol + ncol - 1}) {
            ++*walks;
            if (qi_walk(k, ncol, cap) != (int)((k + per - 1) / per)) ++bad;
          }
  return bad;
}
int qi_maxk() { return lbk::QN_IDX_MAXK; }
int qi_buf() { return lbk::QN_IDX_BUF; }
}
