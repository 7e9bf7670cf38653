// qn_plan.hpp -- the tiling plan of the curvature-model operators (solver_qn.inl, k_qn.hip, k_qn_draw.hip; DESIGN.md
// section 10): which launches a pass over W = [S, Y] is made of and where each of their sums lands.  Host-only integer
// bookkeeping, no HIP and nothing of Solver: tests/qn_plan_check.cpp walks it exhaustively on the CPU.
//
// The rule, stated here and nowhere else: the columns of W go in tiles of at most QN_TILE pairs from column 0, a tile
// of ncols pairs has the capacity qn_mc(ncols) = 5 / 10 / 16, and the (at most QN_KMAX) vectors of a block go through
// a tile in pieces of 4 / 2 / 1 (qn_piece_k: 3 = 2 + 1, at most 2 on a tile of 16).  One piece is one launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lbk {

constexpr int QN_TILE = 16;
constexpr int QN_KMAX = 4;
// column capacity of a tile of ncols <= QN_TILE pairs
constexpr int qn_mc(int ncols) { return ncols <= 5 ? 5 : (ncols <= 10 ? 10 : QN_TILE); }
// the widest block of vectors a launch on a tile of capacity mc takes
constexpr int qn_kmax(int mc) { return mc <= 10 ? 4 : 2; }
// the vectors that the next launch takes of `left` remaining ones
constexpr int qn_piece_k(int left, int mc) {
  const int k = left < qn_kmax(mc) ? left : qn_kmax(mc);
  return k == 3 ? 2 : k;
}
// a block that a launch accepts: what qn_piece_k can return
constexpr bool qn_block_ok(int mc, int k) { return k >= 1 && qn_piece_k(k, mc) == k; }
// The k vectors of an operator call go through its two passes in blocks of at most QN_KMAX: the width of the block
// that starts at vector k0.  s0: for the draws the sample the block starts at (first + k0) -- a block of more than one
// sample is whole pairs of the generator, so an odd first sample goes alone and every later block starts at an even
// one; 0 for vectors that are loaded.
constexpr int qn_block_kc(int64_t k0, int64_t k, int64_t s0 = 0) {
  return (s0 & 1) ? 1 : (int)(k - k0 < QN_KMAX ? k - k0 : QN_KMAX);
}

// what the launches of the first tile carry behind their W'V sums: nothing, the k squared norms of the piece's
// vectors (quadratic forms, draw densities), or the k (k + 1) / 2 sums d_a'd_b, a <= b, row by row (Gram matrices)
enum class QnCarry { None, Norms, Gram };
constexpr int qn_carried(QnCarry c, int k) {
  return c == QnCarry::Gram ? k * (k + 1) / 2 : c == QnCarry::Norms ? k : 0;
}

struct QnPiece {  // one launch: the vectors k0 .. k0 + k - 1 on the column tile at c0, its sums from slot off on
  int c0, mc, k0, k, off;
  QnCarry carry;  // (None on every tile but the first)
  constexpr int slots() const { return 2 * mc * k + qn_carried(carry, k); }
};
struct QnPlan {
  int col, kc;
  std::vector<QnPiece> pieces;  // tile by tile, within a tile by vector
  int total;                    // slots of all pieces
};
// the slots a plan can need: 2 (col + QN_TILE) kc sums and the widest carry, for col <= max_m and kc <= QN_KMAX
constexpr int qn_res(int max_m) { return 2 * (max_m + QN_TILE) * QN_KMAX + qn_carried(QnCarry::Gram, QN_KMAX); }

// The pieces of one pass over the col stored pairs for a block of kc <= QN_KMAX vectors.  With no pair there is no
// tile, unless something is carried or the pass writes an output (expand: the second pass of qn_apply and the draws):
// then one empty tile, whose launches read the zero line and nothing of W.
inline QnPlan qn_plan(int col, int kc, QnCarry carry, bool expand = false) {
  QnPlan pl{col, kc, {}, 0};
  for (int c0 = 0; c0 < std::max(col, carry != QnCarry::None || expand ? 1 : 0); c0 += QN_TILE) {
    const int mc = qn_mc(std::max(1, std::min(QN_TILE, col - c0)));
    for (int k0 = 0; k0 < kc;) {
      const QnPiece p{c0, mc, k0, qn_piece_k(kc - k0, mc), pl.total, c0 == 0 ? carry : QnCarry::None};
      pl.pieces.push_back(p);
      pl.total += p.slots();
      k0 += p.k;
    }
  }
  return pl;
}

// res (the fetched slots) -> out[k * 2 col + i] = S(:, i)'v_k for i < col, Y(:, i - col)'v_k beyond
inline void qn_scatter_sums(const QnPlan &pl, const double *res, double *out) {
  for (const QnPiece &p : pl.pieces)
    for (int kk = 0; kk < p.k; ++kk) {
      double *o = out + (size_t)(p.k0 + kk) * 2 * pl.col;
      const double *r = res + (size_t)p.off + kk * 2 * p.mc;
      for (int j = 0; j < p.mc && p.c0 + j < pl.col; ++j) o[p.c0 + j] = r[j], o[pl.col + p.c0 + j] = r[p.mc + j];
    }
}
// the carried slots -> dst[k] (Norms), or dst[a + b QN_KMAX] for a <= b of one piece (Gram: entries across two pieces
// are left as they are)
inline void qn_scatter_carry(const QnPlan &pl, const double *res, double *dst) {
  for (const QnPiece &p : pl.pieces) {
    const double *r = res + (size_t)p.off + 2 * p.mc * p.k;
    if (p.carry == QnCarry::Norms)
      for (int kk = 0; kk < p.k; ++kk) dst[p.k0 + kk] = r[kk];
    if (p.carry == QnCarry::Gram)
      for (int a = 0; a < p.k; ++a)
        for (int b = a; b < p.k; ++b) dst[(p.k0 + a) + (size_t)(p.k0 + b) * QN_KMAX] = *r++;
  }
}
// the other way, for an expansion: cf[k * 2 col + i] -> the 2 mc k coefficients of one piece's launch,
// coef[kk * 2 mc + j] for S(:, c0 + j) and coef[kk * 2 mc + mc + j] for Y(:, c0 + j), zero for the columns >= col
inline void qn_pack_coef(const QnPiece &p, int col, const double *cf, double *coef) {
  std::fill(coef, coef + 2 * p.mc * p.k, 0.0);
  for (int kk = 0; kk < p.k; ++kk) {
    const double *c = cf + (size_t)(p.k0 + kk) * 2 * col;
    double *o = coef + (size_t)kk * 2 * p.mc;
    for (int j = 0; j < p.mc && p.c0 + j < col; ++j) o[j] = c[p.c0 + j], o[p.mc + j] = c[col + p.c0 + j];
  }
}

// ---- the sums of a pushed pair (lbfgsb_hip_qn_pairs_push) ----
// One W'V pass of the block (s, y) with its Gram carried: qn_plan(col, 2, QnCarry::Gram).  What qn_scatter_sums and
// qn_scatter_carry make of it, by name: the 4 col sums against the stored pairs (logical order) and the three of the
// pair itself.
struct QnPushSums {
  int col;
  const double *w;  // qn_scatter_sums' out: 2 vectors x 2 col
  const double *g;  // qn_scatter_carry's dst (Gram): entries a + b QN_KMAX, a <= b
  double Ss(int j) const { return w[j]; }            // s_j's
  double Ys(int j) const { return w[col + j]; }      // y_j's
  double Sy(int j) const { return w[2 * col + j]; }  // s_j'y
  double Yy(int j) const { return w[3 * col + j]; }  // y_j'y
  double ss() const { return g[0]; }
  double sy() const { return g[QN_KMAX]; }
  double yy() const { return g[1 + QN_KMAX]; }
  static constexpr int count(int col) { return 4 * col + 3; }
};

// ---- the basis pass (k_qn_eig.hip, lbfgsb_hip_qn_eigvec): OUT(n x k) = W(n x 2col) C(2col x k) ----
// One launch per column tile writes ALL k <= QN_BASIS_KMAX outputs: the tiles are qn_plan's (from column 0, at most
// QN_TILE pairs, capacity qn_mc), the first one stores its sums, every later one adds them to what is there (acc).
// The coefficients of all tiles lie in one buffer, tile after tile: those of output j on a tile from off + j * 2 mc,
// S(:, c0 + i) at + i and Y(:, c0 + i) at + mc + i, zero for the columns >= col (qn_pack_coef on a piece of k vectors).
constexpr int QN_BASIS_KMAX = 128;
struct QnBasisTile {
  int c0, mc;
  bool acc;
  int off;  // of the tile's 2 mc k coefficients in the plan's buffer
  constexpr QnPiece piece(int k) const { return QnPiece{c0, mc, 0, k, 0, QnCarry::None}; }
};
struct QnBasisPlan {
  int col, k;
  std::vector<QnBasisTile> tiles;
  int total;  // coefficients of all tiles
};
// the coefficients a plan can need, for col <= max_col
constexpr int qn_basis_coefs(int max_col) { return 2 * (max_col + QN_TILE) * QN_BASIS_KMAX; }
inline QnBasisPlan qn_basis_plan(int col, int k) {
  QnBasisPlan pl{col, k, {}, 0};
  for (int c0 = 0; c0 < col; c0 += QN_TILE) {
    const QnBasisTile t{c0, qn_mc(std::min(QN_TILE, col - c0)), c0 > 0, pl.total};
    pl.tiles.push_back(t);
    pl.total += 2 * t.mc * k;
  }
  return pl;
}
// cf[j * 2 col + i] (S part, then Y part) of the k outputs -> the plan's buffer
inline void qn_basis_pack(const QnBasisPlan &pl, const double *cf, double *coef) {
  for (const QnBasisTile &t : pl.tiles) qn_pack_coef(t.piece(pl.k), pl.col, cf, coef + t.off);
}

}  // namespace lbk
