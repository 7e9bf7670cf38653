// k_qn_draw.hip -- draws x + sigma A^(1/2) z, z ~ N(0, I), of the curvature model (lbfgsb_hip_qn_draw, solver_qn.inl;
// DESIGN.md section 10).  (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// A^(1/2) = sqrt(alpha) I + [S, Y] C [S, Y]' (host_dense.hpp, qn_root).  The two passes are k_qn.hip's qn_wtv and
// qn_expand with the loads of the vectors replaced by the generator: the Gaussian vectors never exist in memory.
//   qn_wtz   [S'z_k; Y'z_k] for the K samples s0 .. s0 + K - 1 (every W entry read once per block of K samples);
//   qn_wtzz  the same with z_k'z_k carried along (the log-density of a draw, lbfgsb_hip_qn_draw_logpdf);
//   qn_draw  out_k = mean + (scale sqrt(alpha)) z_k + S cs_k + Y cy_k on the first column tile (z generated again),
//            out_k += S cs_k + Y cy_k on the later ones (scale is folded into the coefficients by the host).
// z_k[i] is a function of (seed, row0 + i, s0 + k) alone (philox.hpp): Philox4x32-10 on the counter (row, pair =
// sample >> 1) under the key seed, Box-Muller on its two uniforms; the two samples of a pair share one Philox call
// and one log / sqrt / sincospi.  A block of K >= 2 samples starts at an even sample (the host splits an odd first
// sample off), so a block is K / 2 whole pairs.  REAL32: z and all arithmetic in fp64, rounded on store.
// W is read as it lies (natural order or the tile-local layout through lmask); out and mean are in natural row order.
#include "k_qn_common.hpp"

namespace lbk {

// sums: slot kk * 2MC + j = S(:, c0 + j)' z_kk, slot kk * 2MC + MC + j = Y(:, c0 + j)' z_kk (qn_wtv_kernel's slots)
// ZZ: K more sums z_kk'z_kk in the slots 2MC K + kk (lbfgsb_hip_qn_draw_logpdf, the first column tile's launch).  The
// W'z sums are the plain pass's bit for bit: the same rows per lane, the same operations on every accumulator and
// the same reduction of every slot (block_reduce_store's order within a slot does not depend on the slot count,
// and 2MC K and 2MC K + K are on the same side of its scatter threshold for every MC, K here), on the same grid
// (launch_qn_wtz sizes it from the plain kernel for both).
template <typename T, int MC, int K, int V, bool CW, bool NT, bool ZZ>
__device__ __forceinline__ void qn_wtz_body(int64_t n, const QnTile<T> &t, uint64_t seed, int64_t row0, int64_t s0,
                                            double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  constexpr int NW = 2 * MC * K, NACC = NW + (ZZ ? K : 0);
  static_assert((NW >= 16) == (NACC >= 16), "block_reduce_store reduces the W'z slots as the plain pass does");
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(t.lmask, i);
    double a[MC][W], b[MC][W];
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      double z[K];
      qn_gauss<K>(seed, (uint64_t)(row0 + i + w), (uint64_t)s0, z);
#pragma unroll
      for (int kk = 0; kk < K; ++kk) qn_dot_acc<MC, W>(acc + kk * 2 * MC, a, b, w, z[kk]);
      if constexpr (ZZ) {
#pragma unroll
        for (int kk = 0; kk < K; ++kk) acc[NW + kk] += z[kk] * z[kk];
      }
    }
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_wtz_kernel(int64_t n, QN_TILE_PARAMS(T), uint64_t seed,
                                                       int64_t row0, int64_t s0, double *part) {
  qn_wtz_body<T, MC, K, V, CW, NT, false>(n, QN_TILE_VIEW(T), seed, row0, s0, part);
}

template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_wtzz_kernel(int64_t n, QN_TILE_PARAMS(T), uint64_t seed,
                                                        int64_t row0, int64_t s0, double *part) {
  qn_wtz_body<T, MC, K, V, CW, NT, true>(n, QN_TILE_VIEW(T), seed, row0, s0, part);
}

// first (tile c0 = 0): out_kk[i] =mean[i] + cf.alpha z_kk[i] + sum_j cf.c[kk][j] S(i, j) + cf.c[kk][MC + j] Y(i, j)
// with mean[i] = 0 for a NULL mean; later tiles: out_kk[i] += sum_j ... over the columns c0 + j
template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_draw_kernel(int64_t n, QN_TILE_PARAMS(T), QnCoef<MC, K> cf,
                                                        uint64_t seed, int64_t row0, int64_t s0, int first,
                                                        const T *__restrict__ mean, QnOuts<T> out) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  const QnTile<T> t = QN_TILE_VIEW(T);
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double x[K][W], a[MC][W], b[MC][W];
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
    if (first) {
      double mu[W];
#pragma unroll
      for (int w = 0; w < W; ++w) mu[w] = 0.0;
      if (mean) ldx<W, false>(mean + i, mu);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double z[K];
        qn_gauss<K>(seed, (uint64_t)(row0 + i + w), (uint64_t)s0, z);
#pragma unroll
        for (int kk = 0; kk < K; ++kk) x[kk][w] = mu[w] + cf.alpha * z[kk];
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < K; ++kk) ldx<W, false>(out.p[kk] + i, x[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      double o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) o[w] = qn_comb<MC, W>(x[kk][w], cf, kk, a, b, w);
      stnt<W>(out.p[kk] + i, o);
    }
  });
}

// ---------------------------------------------------------------- launches (dispatch: k_qn_common.hpp)
template <typename T>
hipError_t launch_qn_wtz(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                         uint64_t seed, int64_t row0, int64_t s0, bool zz, double *part, double *res) {
  if (!draw_block_ok(mc, k, s0)) return hipErrorInvalidValue;
  // (two rows per lane only where operands + accumulators leave room for them, as qn_wtv; the same with z'z, whose
  //  K sums add 2 K <= 4 registers there: the W'z sums of the two kernels must agree bit for bit)
  const bool vec2 = 2 * mc * k <= 20;
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    auto kern = zz ? qn_wtzz_kernel<T, MC, K, V, CW, NT> : qn_wtz_kernel<T, MC, K, V, CW, NT>;
    // (the grid of the PLAIN kernel for both: the grid decides every workgroup's rows, hence the partial sums, and
    //  the two code objects need not be resident in the same numbers)
    g = grid_for_w(q, n, V, (const void *)qn_wtz_kernel<T, MC, K, V, CW, NT>);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), seed, row0, s0,
                       part);
  }))));
  return launch_qn_finalize(q, part, g, 2 * mc * k + (zz ? k : 0), res);
}

template <typename T>
hipError_t launch_qn_draw(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                          const double *coef, double alpha, uint64_t seed, int64_t row0, int64_t s0, bool first,
                          const T *mean, QnOuts<T> out) {
  if (!draw_block_ok(mc, k, s0)) return hipErrorInvalidValue;
  // (out / mean that are not 16-byte aligned: one row per lane)
  const bool vec2 = 2 * mc * k <= 20 && (!mean || aligned_for(mean, 2)) && all_aligned_for(out.p, k, 2);
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    const QnCoef<MC, K> cf = qn_coef_args<MC, K>(coef, alpha);
    auto kern = qn_draw_kernel<T, MC, K, V, CW, NT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), cf, seed, row0, s0,
                       first ? 1 : 0, first ? mean : (const T *)nullptr, out);
    done = true;
  }))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

#define QN_DRAW_INST(T)                                                                                           \
  template hipError_t launch_qn_wtz<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int, uint64_t,     \
                                       int64_t, int64_t, bool, double *, double *);                              \
  template hipError_t launch_qn_draw<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,              \
                                        const double *, double, uint64_t, int64_t, int64_t, bool, const T *,    \
                                        QnOuts<T>);
QN_DRAW_INST(double)
QN_DRAW_INST(float)
#undef QN_DRAW_INST

}  // namespace lbk
