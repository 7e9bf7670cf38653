// k_qn_common.hpp -- what the kernel files of the curvature-model operator share (k_qn.hip, k_qn_draw.hip,
// k_qn_shift.hip, k_qn_shift_draw.hip): the slot of a row in the layout W is in, the normal deviates of the draws,
// and the dispatch of a launch over the column capacity MC of a tile, the block of K vectors, the layout (CW), the
// rows per lane (V) and the cache policy of the loads (NT).
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

namespace {
template <typename T>
bool aligned_for(const T *p, int v) {
  return ((uintptr_t)p % ((uintptr_t)v * sizeof(T))) == 0;
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
