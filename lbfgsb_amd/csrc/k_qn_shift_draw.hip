// k_qn_shift_draw.hip -- draws and densities of the curvature model plus a diagonal (lbfgsb_hip_qn_shift_draw /
// _draw_logpdf / _quad / _logpdf, solver_qn.inl).  (part of the gfx950 kernel set;
// kernels_common.hpp has the overview)
//
// With w = 1 / Delta (0 on a pinned row) and C of host_dense.hpp's qn_shift_root,
//   L = diag(sqrt w) + diag(w) W C W' diag(sqrt w),   L L' = (B + mu I + D)^-1 on the free rows, W = [S, Y].
// The passes are k_qn_draw.hip's and k_qn.hip's qn_wtd with the weights of k_qn_shift.hip:
//   qn_shift_wtz   [S'(sqrt w o z_k); Y'(sqrt w o z_k)] for the K samples s0 .. s0 + K - 1, z from the generator;
//   qn_shift_wtzz  the same with the sum of z_k^2 over the FREE rows carried along (the log-density of a draw);
//   qn_shift_draw  out_k = mean + scale sqrt(w) o z_k + w o (S cs_k + Y cy_k) on the first column tile (z generated
//                  again), out_k += w o (S cs_k + Y cy_k) on the later ones; a pinned row is its mean (+0 without one);
//   qn_shift_wtd   [S'(f o q_k); Y'(f o q_k)] for q_k = v_k - center, f = (w != 0), nothing written; on the first tile
//                  the sums of q_k^2 / w over the free rows along (the Delta-weighted squared norm of a quadratic
//                  form).
// z_k[i] is qn_gauss's function of (seed, row0 + i, s0 + k): a pinned row draws its z and discards it, so the free
// rows' z depends neither on which rows are pinned nor on the sharding.  A block of K >= 2 samples starts at an even
// sample.  The weights are fp64 in both real kinds, in natural row order as out, mean, v and center; W is read as it
// lies (lmask).  A pinned row contributes +0 and receives its value by selection, never by multiplication.
#include "k_qn_common.hpp"

namespace lbk {

// sums: qn_wtz_body's slots; ZZ: K more in the slots 2MC K + kk, the sums of z_kk[i]^2 over the rows with w_i != 0.
// The W'z sums of the two kernels agree bit for bit (see qn_wtz_body: the same grid, the same side of
// block_reduce_store's scatter threshold).
template <typename T, int MC, int K, int V, bool CW, bool NT, bool ZZ>
__device__ __forceinline__ void qn_shift_wtz_body(int64_t n, const QnTile<T> &t, uint64_t seed, int64_t row0,
                                                  int64_t s0, const double *__restrict__ wgt, double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  constexpr int NW = 2 * MC * K, NACC = NW + (ZZ ? K : 0);
  static_assert((NW >= 16) == (NACC >= 16), "block_reduce_store reduces the W'z slots as the plain pass does");
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(t.lmask, i);
    double a[MC][W], b[MC][W], wg[W];
    ldx<W, NT>(wgt + i, wg);
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      double z[K];
      qn_gauss<K>(seed, (uint64_t)(row0 + i + w), (uint64_t)s0, z);
      const bool fr = wg[w] != 0.0;
      const double rw = sqrt(wg[w]);
#pragma unroll
      for (int kk = 0; kk < K; ++kk) {
        const double zw = fr ? rw * z[kk] : 0.0;
        // (written out, not qn_dot_acc: through it qn_shift_wtz_kernel<float, 5, 4, 2> went from 161 to 217 registers)
#pragma unroll
        for (int j = 0; j < MC; ++j) {
          acc[kk * 2 * MC + j] += a[j][w] * zw;
          acc[kk * 2 * MC + MC + j] += b[j][w] * zw;
        }
        if constexpr (ZZ) acc[NW + kk] += fr ? z[kk] * z[kk] : 0.0;
      }
    }
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_shift_wtz_kernel(int64_t n, QN_TILE_PARAMS(T), uint64_t seed,
                                                             int64_t row0, int64_t s0, const double *__restrict__ wgt,
                                                             double *part) {
  qn_shift_wtz_body<T, MC, K, V, CW, NT, false>(n, QN_TILE_VIEW(T), seed, row0, s0, wgt, part);
}

template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_shift_wtzz_kernel(int64_t n, QN_TILE_PARAMS(T), uint64_t seed,
                                                              int64_t row0, int64_t s0, const double *__restrict__ wgt,
                                                              double *part) {
  qn_shift_wtz_body<T, MC, K, V, CW, NT, true>(n, QN_TILE_VIEW(T), seed, row0, s0, wgt, part);
}

// first (tile c0 = 0): out_kk[i] = mean[i] + (cf.alpha sqrt(w_i) z_kk[i] + w_i sum_j (cf.c[kk][j] S(i, j) +
// cf.c[kk][MC + j] Y(i, j))) with mean[i] = 0 for a NULL mean, and mean[i] itself where w_i = 0; later tiles:
// out_kk[i] += w_i (the sum over the columns c0 + j), nothing where w_i = 0
template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_shift_draw_kernel(int64_t n, QN_TILE_PARAMS(T), QnCoef<MC, K> cf,
                                                              uint64_t seed, int64_t row0, int64_t s0, int first,
                                                              const T *__restrict__ mean,
                                                              const double *__restrict__ wgt, QnOuts<T> out) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  const QnTile<T> t = QN_TILE_VIEW(T);
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double x[K][W], a[MC][W], b[MC][W], wg[W];
    ldx<W, NT>(wgt + i, wg);
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
    double zs[K][W];  // first: cf.alpha sqrt(w) z; later tiles: not used
    if (first) {
      double mu[W];
#pragma unroll
      for (int w = 0; w < W; ++w) mu[w] = 0.0;
      if (mean) ldx<W, false>(mean + i, mu);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double z[K];
        qn_gauss<K>(seed, (uint64_t)(row0 + i + w), (uint64_t)s0, z);
        const double rw = cf.alpha * sqrt(wg[w]);
#pragma unroll
        for (int kk = 0; kk < K; ++kk) x[kk][w] = mu[w], zs[kk][w] = rw * z[kk];
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < K; ++kk) {
        ldx<W, false>(out.p[kk] + i, x[kk]);
#pragma unroll
        for (int w = 0; w < W; ++w) zs[kk][w] = 0.0;
      }
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      double o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const double e = qn_comb<MC, W>(0.0, cf, kk, a, b, w);
        o[w] = wg[w] == 0.0 ? x[kk][w] : x[kk][w] + (zs[kk][w] + wg[w] * e);
      }
      stnt<W>(out.p[kk] + i, o);
    }
  });
}

// sums: slot kk * 2MC + j = S(:, c0 + j)'(f o q_kk), slot kk * 2MC + MC + j = Y(:, c0 + j)'(f o q_kk), q_kk = v_kk -
// center (CEN) and f = (w != 0); DD: K more sums, of q_kk[i]^2 / w_i over the rows with w_i != 0, in the slots
// 2MC K + kk.  Whatever v or the center hold on a pinned row (a NaN too) contributes +0.
template <typename T, int MC, int K, int V, bool CW, bool NT, bool CEN, bool DD>
__global__ __launch_bounds__(BLOCK) void qn_shift_wtd_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                             const T *__restrict__ center,
                                                             const double *__restrict__ wgt, double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  const QnTile<T> t = QN_TILE_VIEW(T);
  constexpr int NW = 2 * MC * K, NACC = NW + (DD ? K : 0);
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double vv[K][W], a[MC][W], b[MC][W], wg[W];
    ldx<W, NT>(wgt + i, wg);
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, NT>(v.p[kk] + i, vv[kk]);
    double cc[CEN ? W : 1];
    if constexpr (CEN) ldx<W, NT>(center + i, cc);
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double qd = vv[kk][w];
        if constexpr (CEN) qd -= cc[w];
        vv[kk][w] = wg[w] == 0.0 ? 0.0 : qd;
      }
    // (written out, not qn_dot_acc: through it the REAL32 K = 1 instantiations with the norms along lost a wave per
    //  SIMD -- <float, 10, 1, 2, ..., DD> 126 -> 142 registers, <float, 5, 1, 2, ..., DD> 78 -> 82)
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
#pragma unroll
      for (int j = 0; j < MC; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w) {
          acc[kk * 2 * MC + j] += a[j][w] * vv[kk][w];
          acc[kk * 2 * MC + MC + j] += b[j][w] * vv[kk][w];
        }
    if constexpr (DD) {
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[NW + kk] += wg[w] == 0.0 ? 0.0 : vv[kk][w] * vv[kk][w] / wg[w];
    }
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

// ---------------------------------------------------------------- launches (dispatch: k_qn_common.hpp)
template <typename T>
hipError_t launch_qn_shift_wtz(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               uint64_t seed, int64_t row0, int64_t s0, bool zz, const double *wgt, double *part,
                               double *res) {
  if (!draw_block_ok(mc, k, s0)) return hipErrorInvalidValue;
  // (two rows per lane where qn_wtz has them and the weights are 16-byte aligned: they add 2 V registers)
  const bool vec2 = 2 * mc * k <= 20 && aligned_for(wgt, 2);
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    auto kern = zz ? qn_shift_wtzz_kernel<T, MC, K, V, CW, NT> : qn_shift_wtz_kernel<T, MC, K, V, CW, NT>;
    // (the grid of the PLAIN kernel for both, as launch_qn_wtz: the grid decides every workgroup's rows)
    g = grid_for_w(q, n, V, (const void *)qn_shift_wtz_kernel<T, MC, K, V, CW, NT>);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), seed, row0, s0, wgt,
                       part);
  }))));
  return launch_qn_finalize(q, part, g, 2 * mc * k + (zz ? k : 0), res);
}

template <typename T>
hipError_t launch_qn_shift_draw(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                                const double *coef, double alpha, uint64_t seed, int64_t row0, int64_t s0,
                                bool first, const T *mean, const double *wgt, QnOuts<T> out) {
  if (!draw_block_ok(mc, k, s0)) return hipErrorInvalidValue;
  // (out / mean that are not 16-byte aligned: one row per lane)
  const bool vec2 =
      2 * mc * k <= 20 && aligned_for(wgt, 2) && (!mean || aligned_for(mean, 2)) && all_aligned_for(out.p, k, 2);
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    const QnCoef<MC, K> cf = qn_coef_args<MC, K>(coef, alpha);
    auto kern = qn_shift_draw_kernel<T, MC, K, V, CW, NT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), cf, seed, row0, s0,
                       first ? 1 : 0, first ? mean : (const T *)nullptr, wgt, out);
    done = true;
  }))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T>
hipError_t launch_qn_shift_wtd(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               QnVecs<T> v, const T *center, bool dd, const double *wgt, double *part, double *res) {
  if (!qn_block_ok(mc, k)) return hipErrorInvalidValue;
  // (two rows per lane as launch_qn_wtv's centred pass, the weights 2 V registers more)
  const bool vec2 =
      2 * mc * k <= 20 && aligned_for(wgt, 2) && (!center || aligned_for(center, 2)) && all_aligned_for(v.p, k, 2);
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT,
      QN_DISPATCH_BOOL(center != nullptr, CEN, QN_DISPATCH_BOOL(dd, DD, {
    auto kern = qn_shift_wtd_kernel<T, MC, K, V, CW, NT, CEN, DD>;
    g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), v, center, wgt,
                       part);
  }))))));
  return launch_qn_finalize(q, part, g, 2 * mc * k + (dd ? k : 0), res);
}

#define QN_SHIFT_DRAW_INST(T)                                                                                      \
  template hipError_t launch_qn_shift_wtz<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int, uint64_t, \
                                             int64_t, int64_t, bool, const double *, double *, double *);         \
  template hipError_t launch_qn_shift_draw<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,          \
                                              const double *, double, uint64_t, int64_t, int64_t, bool,           \
                                              const T *, const double *, QnOuts<T>);                              \
  template hipError_t launch_qn_shift_wtd<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,           \
                                             QnVecs<T>, const T *, bool, const double *, double *, double *);
QN_SHIFT_DRAW_INST(double)
QN_SHIFT_DRAW_INST(float)
#undef QN_SHIFT_DRAW_INST

}  // namespace lbk
