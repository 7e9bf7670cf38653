// Walks the plan of the basis pass (qn_plan.hpp: qn_basis_plan, qn_basis_pack) exhaustively on the CPU, for every
// col <= 80 and every k <= QN_BASIS_KMAX: the tiles cover the columns once and in order, only the first stores, the
// coefficient blocks lie back to back inside the buffer the solver allocates, and the launches as the kernel reads
// them -- out_j (+)= sum_c coef[off + j 2mc + c] W(:, tile column c) -- add up to every coefficient exactly once.
// Built and run by tests/test_qn_eig_cpu.py; prints "ok <plans>" and returns 0, or the first violation and 1.
#include <cstdio>
#include <vector>

#include "../lbfgsb_amd/csrc/qn_plan.hpp"

#define REQUIRE(c)                                                                        \
  do {                                                                                    \
    if (!(c)) {                                                                           \
      std::printf("col %d k %d: %s (line %d)\n", col, k, #c, __LINE__);                   \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

int main() {
  using namespace lbk;
  long plans = 0;
  for (int col = 0; col <= 80; ++col)
    for (int k = 1; k <= QN_BASIS_KMAX; ++k) {
      const QnBasisPlan pl = qn_basis_plan(col, k);
      REQUIRE(pl.col == col && pl.k == k);
      REQUIRE((int)pl.tiles.size() == (col + QN_TILE - 1) / QN_TILE);
      int next = 0, off = 0;
      for (const QnBasisTile &t : pl.tiles) {
        REQUIRE(t.c0 == next && t.off == off);
        REQUIRE(t.acc == (t.c0 > 0));
        const int ncols = std::min(QN_TILE, col - t.c0);
        REQUIRE(ncols >= 1 && t.mc == qn_mc(ncols) && t.mc >= ncols);
        REQUIRE(t.mc == 5 || t.mc == 10 || t.mc == QN_TILE);
        next += ncols, off += 2 * t.mc * k;
      }
      REQUIRE(next == col && off == pl.total);
      if (col <= 64) REQUIRE(pl.total <= qn_basis_coefs(64));
      // cf[j * 2 col + i] = a tag of (j, i); the kernel's sums, with W(:, logical column) as a unit vector
      std::vector<double> cf((size_t)2 * col * k), coef((size_t)pl.total + 1, -7.0), got((size_t)2 * col * k, 0.0);
      for (size_t e = 0; e < cf.size(); ++e) cf[e] = 1.0 + (double)e;
      qn_basis_pack(pl, cf.data(), coef.data());
      REQUIRE(coef[(size_t)pl.total] == -7.0);
      for (const QnBasisTile &t : pl.tiles)
        for (int j = 0; j < k; ++j)
          for (int c = 0; c < 2 * t.mc; ++c) {
            const double v = coef[(size_t)t.off + (size_t)j * 2 * t.mc + c];
            const int lc = t.c0 + (c < t.mc ? c : c - t.mc);  // the logical column the kernel's slot c reads
            if (lc >= col || (c < t.mc ? c : c - t.mc) >= std::min(QN_TILE, col - t.c0)) {
              REQUIRE(v == 0.0);  // (a slot beyond the tile's pairs reads the zero line or a live column: no share)
              continue;
            }
            got[(size_t)j * 2 * col + (c < t.mc ? lc : col + lc)] += v;
          }
      for (size_t e = 0; e < cf.size(); ++e) REQUIRE(got[e] == cf[e]);
      ++plans;
    }
  std::printf("ok %ld\n", plans);
  return 0;
}
