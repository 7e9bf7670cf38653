// k_qn_shift.hip -- the curvature model plus a diagonal (lbfgsb_hip_qn_shift_set / _solve / _logdet / _diag,
// solver_qn.inl).  (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// With Delta = (theta + mu) I + D, w = 1 / Delta (0 on a pinned row, d_i = +inf) and W = [Y, theta S]:
//   (B + mu I + D)^-1 = diag(w) + diag(w) W K^-1 W' diag(w),   K = M^-1 - W' diag(w) W
// with the 2col x 2col K factorised on the host (host_dense.hpp, qn_shift_factor / qn_shift_coef).  The passes are
// the row-weighted twins of k_qn.hip's:
//   qn_shift_w       w_i from d_i, with sum log Delta_i over the free rows, the pinned count and the count of rows
//                    with Delta_i <= 0 or NaN carried along (16 B per row in fp64);
//   qn_shift_wtv     [S'(w o v); Y'(w o v)] for K vectors at once (VSLOT: the vectors are columns of W: the weighted
//                    Gram): qn_wtv's bytes per row plus 8 for w;
//   qn_shift_expand  out_j = w o (v_j + S cs_j + Y cy_j), coefficients as kernel arguments, nontemporal stores;
//   qn_shift_diag    out_i = w_i + w_i^2 r_i' N r_i, N packed in LDS as qn_diag packs it.
// ROOT (a template switch of qn_shift_wtv and qn_shift_expand): the two passes of L v, L = diag(sqrt w) + diag(w) W C
// W' diag(sqrt w) with L L' = (B + mu I + D)^-1 (lbfgsb_hip_qn_shift_sqrt; section 10g): the sums take the weight
// sqrt(w_i), and the first tile writes sqrt(w) o v + w o (S cs + Y cy).
// w is fp64 in both real kinds and, as d, v and out, in natural row order.  W is read in the layout it is in (lmask);
// none of the kernels writes it.  Reductions: per-lane fp64 accumulators -> block_reduce_store -> qn_finalize.
// A pinned row's output is +0 by selection, not by multiplication: whatever v holds there, and whatever sign the
// bracket has.
#include "k_qn_common.hpp"

namespace lbk {

// slots: 0 sum of log Delta_i over the rows with 0 < Delta_i < inf, 1 the rows with d_i = +inf, 2 the rows with
// Delta_i <= 0 or NaN (a -inf among them); w_i = 0 on the rows of slots 1 and 2
template <typename T, int V, bool NT, bool HAVE_D>
__global__ __launch_bounds__(BLOCK) void qn_shift_w_kernel(int64_t n, const T *__restrict__ d, double shift,
                                                           double *__restrict__ wgt, double *part) {
  double acc[QN_SHIFT_SUMS];
#pragma unroll
  for (int k = 0; k < QN_SHIFT_SUMS; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    double dd[W], o[W];
    if constexpr (HAVE_D) {
      ldx<W, NT>(d + i, dd);
    } else {
#pragma unroll
      for (int w = 0; w < W; ++w) dd[w] = 0.0;
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const double delta = shift + dd[w];
      const bool pin = dd[w] == LB_INF, bad = !(delta > 0.0);
      const bool fr = !pin && !bad;
      o[w] = fr ? 1.0 / delta : 0.0;
      acc[0] += fr ? log(delta) : 0.0;
      acc[1] += pin ? 1.0 : 0.0;
      acc[2] += bad ? 1.0 : 0.0;
    }
    stnt<W>(wgt + i, o);
  });
  block_reduce_store<QN_SHIFT_SUMS>(acc, QN_SHIFT_SUMS, 0, 0, part, MAX_BLOCKS);
}

// w o v of a row group: exactly +0 where w = 0
template <int W>
__device__ __forceinline__ void qn_weigh(const double (&wg)[W], double (&x)[W]) {
#pragma unroll
  for (int w = 0; w < W; ++w) x[w] = wg[w] == 0.0 ? 0.0 : wg[w] * x[w];
}

// sums: slot kk * 2MC + j = S(:, c0 + j)'(w o v_kk), slot kk * 2MC + MC + j = Y(:, c0 + j)'(w o v_kk); VSLOT as in
// qn_wtv_body (the weights stay in natural order).  ROOT: sqrt(w) in place of w
template <typename T, int MC, int K, int V, bool CW, bool VSLOT, bool NT, bool ROOT>
__global__ __launch_bounds__(BLOCK) void qn_shift_wtv_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                             const double *__restrict__ wgt, double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  const QnTile<T> t = QN_TILE_VIEW(T);
  constexpr int NACC = 2 * MC * K;
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double vv[K][W], a[MC][W], b[MC][W], wg[W];
    ldx<W, NT>(wgt + i, wg);
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, NT>(v.p[kk] + (VSLOT ? s : i), vv[kk]);
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
    if constexpr (ROOT) {
#pragma unroll
      for (int w = 0; w < W; ++w) wg[w] = sqrt(wg[w]);
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) qn_weigh<W>(wg, vv[kk]);
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
      qn_dot_acc<MC, W>(acc + kk * 2 * MC, a, b, vv[kk]);
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

// first: out_kk[i] = w_i (src_kk[i] + sum_j cf.c[kk][j] S(i, c0 + j) + cf.c[kk][MC + j] Y(i, c0 + j));
// else (a later column tile, src = out): out_kk[i] = src_kk[i] + w_i (the sum)
// ROOT, first: out_kk[i] = sqrt(w_i) src_kk[i] + w_i (the sum), +0 where w_i = 0; the later tiles as above
template <typename T, int MC, int K, int V, bool CW, bool NT, bool ROOT>
__global__ __launch_bounds__(BLOCK) void qn_shift_expand_kernel(int64_t n, QN_TILE_PARAMS(T), QnCoef<MC, K> cf,
                                                                QnVecs<T> src, const double *__restrict__ wgt,
                                                                int first, QnOuts<T> out) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double x[K][W], a[MC][W], b[MC][W], wg[W];
    ldx<W, NT>(wgt + i, wg);
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, false>(src.p[kk] + i, x[kk]);
    // (loads and sum written out, as in qn_expand_kernel: with qn_ld_tile and qn_comb the REAL32 ROOT instantiation
    //  <float, 10, 4, 2> went from 128 to 130 registers, which is 4 waves per SIMD to 3)
#pragma unroll
    for (int j = 0; j < MC; ++j) {
      const int64_t off = col_off(c0 + j, col, head, m, ldw) + s;
      ld_col<T, W, NT>(c0 + j < col, ws + off, zero, a[j]);
      ld_col<T, W, NT>(c0 + j < col, wy + off, zero, b[j]);
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      double o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double e = first && !ROOT ? x[kk][w] : 0.0;
#pragma unroll
        for (int j = 0; j < MC; ++j) {
          e += cf.c[kk][j] * a[j][w];
          e += cf.c[kk][MC + j] * b[j][w];
        }
        o[w] = e;
      }
      qn_weigh<W>(wg, o);
      if (!first) {
#pragma unroll
        for (int w = 0; w < W; ++w) o[w] += x[kk][w];
      } else if constexpr (ROOT) {
#pragma unroll
        for (int w = 0; w < W; ++w) o[w] = wg[w] == 0.0 ? 0.0 : sqrt(wg[w]) * x[kk][w] + o[w];
      }
      stnt<W>(out.p[kk] + i, o);
    }
  });
}

// out[i] = w_i + w_i^2 r' N r, r = (S(i, 0..MC), Y(i, 0..MC)); np as qn_diag_kernel reads it
template <typename T, int MC, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_shift_diag_kernel(int64_t n, const T *__restrict__ ws,
                                                              const T *__restrict__ wy, const T *__restrict__ zero,
                                                              int64_t ldw, int m, int head, int col,
                                                              const uint64_t *__restrict__ lmask,
                                                              const double *__restrict__ np,
                                                              const double *__restrict__ wgt, T *__restrict__ out) {
  constexpr int D = 2 * MC, NP = D * (D + 1) / 2;
  __shared__ double sn[NP];
  for (int e = threadIdx.x; e < NP; e += BLOCK) sn[e] = np[e];
  __syncthreads();
  const QnTile<T> t{ws, wy, zero, ldw, m, head, col, 0, lmask};
  for_rows<T, 1>(n, [&](int64_t i, auto) {
    // (N stays in LDS: see qn_diag_kernel)
    asm volatile("" ::: "memory");
    const int64_t s = qn_slot<CW>(lmask, i);
    double r[D][1], wg[1];
    ldx<1, NT>(wgt + i, wg);
    qn_ld_tile<T, MC, 1, NT>(t, s, r, r + MC);
    const double acc = qn_rnr<MC>(sn, r);
    const double o[1] = {wg[0] == 0.0 ? 0.0 : wg[0] + wg[0] * wg[0] * acc};
    stnt<1>(out + i, o);
  });
}

// ---------------------------------------------------------------- launches (dispatch: k_qn_common.hpp)
template <typename T>
hipError_t launch_qn_shift_w(const Queue &q, int64_t n, const T *d, double shift, double *wgt, double *part,
                             double *res) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = (!d || aligned_for(d, V)) && aligned_for(wgt, V);
  int g = 0;
  QN_DISPATCH_BOOL(vec, VEC, QN_DISPATCH_BOOL(q.nt, NT, QN_DISPATCH_BOOL(d != nullptr, HAVE_D, {
    auto kern = qn_shift_w_kernel<T, VEC ? V : 1, NT, HAVE_D>;
    g = grid_for_w(q, n, VEC ? V : 1, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, d, shift, wgt, part);
  })));
  return launch_qn_finalize(q, part, g, QN_SHIFT_SUMS, res);
}

template <typename T>
hipError_t launch_qn_shift_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               QnVecs<T> v, bool vslot, bool root, const double *wgt, double *part, double *res) {
  if (!qn_block_ok(mc, k) || (vslot && root)) return hipErrorInvalidValue;
  // (two rows per lane where qn_wtv has them; the weights add 2 V registers to its operands)
  const bool vec2 = !vslot && 2 * mc * k <= 20 && aligned_for(wgt, 2) && all_aligned_for(v.p, k, 2);
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT,
      QN_DISPATCH_BOOL(vslot, VS, QN_DISPATCH_BOOL(root, ROOT, {
    if constexpr ((!VS || V == 1) && !(VS && ROOT)) {
      auto kern = qn_shift_wtv_kernel<T, MC, K, V, CW, VS, NT, ROOT>;
      g = grid_for_w(q, n, V, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), v, wgt, part);
    }
  }))))));
  return launch_qn_finalize(q, part, g, 2 * mc * k, res);
}

template <typename T>
hipError_t launch_qn_shift_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                                  const double *coef, QnVecs<T> src, const double *wgt, bool first, bool root,
                                  QnOuts<T> out) {
  if (!qn_block_ok(mc, k)) return hipErrorInvalidValue;
  const bool vec2 =
      2 * mc * k <= 20 && aligned_for(wgt, 2) && all_aligned_for(src.p, k, 2) && all_aligned_for(out.p, k, 2);
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, QN_DISPATCH_BOOL(root, ROOT, {
    const QnCoef<MC, K> cf = qn_coef_args<MC, K>(coef, 1.0);
    auto kern = qn_shift_expand_kernel<T, MC, K, V, CW, NT, ROOT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), cf, src, wgt,
                       first ? 1 : 0, out);
    done = true;
  })))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T>
hipError_t launch_qn_shift_diag(const Queue &q, int64_t n, WStore<T> w, int head, int col, const double *np,
                                const double *wgt, T *out) {
  const bool vec2 = false;
  bool done = false;
  DISPATCH_MAXC(col, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    if constexpr (V == 1) {
      auto kern = qn_shift_diag_kernel<T, MC, CW, NT>;
      const int g = grid_for_w(q, n, 1, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, w.ws, w.wy, w.zero, w.ld, w.m, head, col,
                         w.lmask, np, wgt, out);
      done = true;
    }
  })));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

#define QN_SHIFT_INST(T)                                                                                            \
  template hipError_t launch_qn_shift_w<T>(const Queue &, int64_t, const T *, double, double *, double *,         \
                                           double *);                                                             \
  template hipError_t launch_qn_shift_wtv<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,          \
                                             QnVecs<T>, bool, bool, const double *, double *, double *);          \
  template hipError_t launch_qn_shift_expand<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,       \
                                                const double *, QnVecs<T>, const double *, bool, bool,            \
                                                QnOuts<T>);                                                       \
  template hipError_t launch_qn_shift_diag<T>(const Queue &, int64_t, WStore<T>, int, int, const double *,        \
                                              const double *, T *);
QN_SHIFT_INST(double)
QN_SHIFT_INST(float)
#undef QN_SHIFT_INST

}  // namespace lbk
