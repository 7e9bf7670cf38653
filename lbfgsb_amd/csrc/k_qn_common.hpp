// k_qn_common.hpp -- what the kernel files of the curvature-model operator share (k_qn.hip, k_qn_draw.hip,
// k_qn_shift.hip, k_qn_shift_draw.hip, k_qn_eig.hip, k_qn_idx.hip): the slot of a row in the layout W is in, the
// normal deviates of the draws, the pieces of a trip over a column tile of W (the tile view and its loads, the W'v
// accumulation, the expansion sum, the packed quadratic form, the trip head of the tall-skinny passes), the checks a
// launch makes on its block and its pointers, and the dispatch of a launch over the column capacity MC of a tile, the
// block of K vectors, the layout (CW), the rows per lane (V) and the cache policy of the loads (NT).
#pragma once
#include "kernels_common.hpp"
#include "philox.hpp"

namespace lbk {

template <bool CW>
__device__ __forceinline__ int64_t qn_slot(const uint64_t *__restrict__ lmask, int64_t i) {
  if constexpr (CW) return wrow(lmask, i);
  else return i;
}

// z[kk] = the deviate of (seed, row, s0 + kk), kk < K.  K >= 2: s0 is even.
template <int K>
__device__ __forceinline__ void qn_gauss(uint64_t seed, uint64_t row, uint64_t s0, double (&z)[K]) {
#pragma unroll
  for (int pp = 0; pp < (K + 1) / 2; ++pp) {
    double u, v, sn, cs;
    lbp::uniforms(seed, row, (s0 >> 1) + (uint64_t)pp, u, v);
    const double r = sqrt(-2.0 * log(u));
    sincospi(2.0 * v, &sn, &cs);
    if constexpr (K == 1) {
      z[0] = (s0 & 1) ? r * sn : r * cs;
    } else {
      z[2 * pp] = r * cs;
      z[2 * pp + 1] = r * sn;
    }
  }
}

// ---- the trip over a column tile of W: written here once, for every pass of the six files ----
// The column tile a launch works on.  Every entry point keeps these as flat arguments, in this order (the struct as a
// by-value kernel argument moved registers in 29 of k_qn_draw.hip's 228 instantiations and cost a qn_wtzz one of its
// four waves per SIMD) and builds the view in its body.
template <typename T>
struct QnTile {
  const T *ws, *wy, *zero;
  int64_t ldw;
  int m, head, col, c0;
  const uint64_t *lmask;
};
#define QN_TILE_PARAMS(T)                                                                                           \
  const T *__restrict__ ws, const T *__restrict__ wy, const T *__restrict__ zero, int64_t ldw, int m, int head, \
      int col, int c0, const uint64_t *__restrict__ lmask
#define QN_TILE_VIEW(T) \
  QnTile<T> { ws, wy, zero, ldw, m, head, col, c0, lmask }
// ... and what a launch passes for them
#define QN_TILE_ARGS(w, head, col, c0) (w).ws, (w).wy, (w).zero, (w).ld, (w).m, head, col, c0, (w).lmask

// a[j], b[j] = the W rows from slot s on of S(:, c0 + j), Y(:, c0 + j), j < MC; a column >= col, and every column of
// a lane that is not live, reads the zero line: every load unconditional, none out of bounds
template <typename T, int MC, int W, bool NT>
__device__ __forceinline__ void qn_ld_tile(const QnTile<T> &t, int64_t s, double (*a)[W], double (*b)[W],
                                           bool live = true) {
#pragma unroll
  for (int j = 0; j < MC; ++j) {
    const int64_t off = col_off(t.c0 + j, t.col, t.head, t.m, t.ldw) + s;
    ld_col<T, W, NT>(live && t.c0 + j < t.col, t.ws + off, t.zero, a[j]);
    ld_col<T, W, NT>(live && t.c0 + j < t.col, t.wy + off, t.zero, b[j]);
  }
}
// acc[j] += a[j] x, acc[MC + j] += b[j] x: one vector's 2 MC sums of a W'v pass.  For entry w of the row group (the
// draws, whose x is generated entry by entry) ...
template <int MC, int W>
__device__ __forceinline__ void qn_dot_acc(double *acc, const double (&a)[MC][W], const double (&b)[MC][W], int w,
                                           double x) {
#pragma unroll
  for (int j = 0; j < MC; ++j) {
    acc[j] += a[j][w] * x;
    acc[MC + j] += b[j][w] * x;
  }
}
// ... and for the whole row group of a loaded vector, column by column.  (Not the form above called per entry: every
// sum adds the same terms in the same order either way, but the statement order decides the schedule, and entry by
// entry the natural-order K = 4 and the 16-column K = 2 passes took 30 to 60 registers more and a dozen instantiations
// lost a wave per SIMD.)
template <int MC, int W>
__device__ __forceinline__ void qn_dot_acc(double *acc, const double (&a)[MC][W], const double (&b)[MC][W],
                                           const double (&x)[W]) {
#pragma unroll
  for (int j = 0; j < MC; ++j)
#pragma unroll
    for (int w = 0; w < W; ++w) {
      acc[j] += a[j][w] * x[w];
      acc[MC + j] += b[j][w] * x[w];
    }
}
// e0 + c[0] a[0] + c[MC] b[0] + c[1] a[1] + ... in that order, c = cf.c[kk]: entry w of output kk of an expansion; e0
// is the kernel's own start (alpha x, x, 0 or the selection of a pinned row), which decides the order of its
// additions.  The draws use it; qn_expand_kernel and qn_shift_expand_kernel keep their sums written out (a REAL32
// instantiation of each lost a wave per SIMD through it: the notes there).
template <int MC, int W, int K>
__device__ __forceinline__ double qn_comb(double e0, const QnCoef<MC, K> &cf, int kk, const double (&a)[MC][W],
                                          const double (&b)[MC][W], int w) {
  double e = e0;
#pragma unroll
  for (int j = 0; j < MC; ++j) {
    e += cf.c[kk][j] * a[j][w];
    e += cf.c[kk][MC + j] * b[j][w];
  }
  return e;
}
// r' N r for the row r = (S(i, 0..MC), Y(i, 0..MC)), N packed in LDS (upper triangle row-major over a <= b, the
// off-diagonal entries doubled)
template <int MC>
__device__ __forceinline__ double qn_rnr(const double *sn, const double (&r)[2 * MC][1]) {
  constexpr int D = 2 * MC;
  double acc = 0.0;
  int e = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = a; b < D; ++b) t += sn[e++] * r[b][0];
    acc += r[a][0] * t;
  }
  return acc;
}
// The trip head of the tall-skinny passes (qn_basis_kernel, qn_cols_kernel): a wave owns 64 R consecutive rows per
// trip, lane l the rows base + l + 64 r; w[j][r], w[MC + j][r] = the tile's entries of row r.  A lane past the last
// row is not live and reads the zero line.
template <typename T, int MC, bool CW, bool NT, int R>
__device__ __forceinline__ void qn_ld_rows(const QnTile<T> &t, int64_t n, int64_t base, int lane, int64_t (&row)[R],
                                           bool (&live)[R], double (&w)[2 * MC][R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    row[r] = base + lane + 64 * r;
    live[r] = row[r] < n;
    const int64_t s = live[r] ? qn_slot<CW>(t.lmask, row[r]) : 0;
    double a[MC][1], b[MC][1];
    qn_ld_tile<T, MC, 1, NT>(t, s, a, b, live[r]);
#pragma unroll
    for (int j = 0; j < MC; ++j) w[j][r] = a[j][0], w[MC + j][r] = b[j][0];
  }
}

namespace {
template <typename T>
bool aligned_for(const T *p, int v) {
  return ((uintptr_t)p % ((uintptr_t)v * sizeof(T))) == 0;
}
// every one of k pointers is aligned for v elements per load (the pointer part of a launch's rows-per-lane decision)
template <typename T>
bool all_aligned_for(T *const *p, int k, int v) {
  for (int kk = 0; kk < k; ++kk)
    if (!aligned_for((const T *)p[kk], v)) return false;
  return true;
}
// blocks of 1, 2 or 4 samples of a draw; a block of more than one sample is whole pairs
inline bool draw_block_ok(int mc, int k, int64_t s0) {
  return qn_block_ok(mc, k) && s0 >= 0 && (k == 1 || (s0 & 1) == 0);
}
}  // namespace

// the kernel argument of an expansion from the flat coefficients of its launch (qn_pack_coef: coef[kk * 2 MC + j])
template <int MC, int K>
QnCoef<MC, K> qn_coef_args(const double *coef, double alpha) {
  QnCoef<MC, K> cf{};
  cf.alpha = alpha;
  for (int kk = 0; kk < K; ++kk)
    for (int j = 0; j < 2 * MC; ++j) cf.c[kk][j] = coef[(size_t)kk * 2 * MC + j];
  return cf;
}

#define QN_DISPATCH_MC(mc, ...)   \
  do {                            \
    if ((mc) == 5) {              \
      constexpr int MC = 5;       \
      __VA_ARGS__;                \
    } else if ((mc) == 10) {      \
      constexpr int MC = 10;      \
      __VA_ARGS__;                \
    } else {                      \
      constexpr int MC = QN_TILE; \
      __VA_ARGS__;                \
    }                             \
  } while (0)
#define QN_DISPATCH_K(k, ...)                 \
  do {                                        \
    if ((k) == 1) {                           \
      constexpr int K = 1;                    \
      __VA_ARGS__;                            \
    } else if ((k) == 2) {                    \
      constexpr int K = 2;                    \
      __VA_ARGS__;                            \
    } else if constexpr (qn_kmax(MC) >= 4) {  \
      constexpr int K = 4;                    \
      __VA_ARGS__;                            \
    }                                         \
  } while (0)
#define QN_DISPATCH_BOOL(c, NAME, ...) \
  do {                                 \
    if (c) {                           \
      constexpr bool NAME = true;      \
      __VA_ARGS__;                     \
    } else {                           \
      constexpr bool NAME = false;     \
      __VA_ARGS__;                     \
    }                                  \
  } while (0)
// the tile-local layout exists for fp64 and m <= 10 only (Solver::cw_eligible): no other CW instantiation.  A layout
// handed to any other combination launches nothing (the caller reports hipErrorInvalidValue): never natural-order
// reads of a permuted W
#define QN_DISPATCH_CW(lm, ...)                                 \
  do {                                                          \
    if constexpr (sizeof(T) == 8 && MC <= 10) {                 \
      if (lm) {                                                 \
        constexpr bool CW = true;                               \
        constexpr int V = 1;                                    \
        __VA_ARGS__;                                            \
        break;                                                  \
      }                                                         \
    }                                                           \
    if (lm) break;                                              \
    constexpr bool CW = false;                                  \
    if (vec2) {                                                 \
      constexpr int V = 2;                                      \
      __VA_ARGS__;                                              \
    } else {                                                    \
      constexpr int V = 1;                                      \
      __VA_ARGS__;                                              \
    }                                                           \
  } while (0)

}  // namespace lbk
