// k_qn_path.hip -- the curvature model along a path of shifts (lbfgsb_hip_qn_path_set / _logdet / _solve / _trust,
// solver_qn_path.inl).  (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// With the diagonal "pins plus a scalar" every free row has the weight w = 1 / (theta + mu), so a shift is a scalar
// on the host and the device keeps one byte per row (1 = free) in place of k_qn_shift.hip's 8-byte weight:
//   (B_FF + mu I)^-1 v_F = w 1_F o (v + [S, Y] c(mu)),   c(mu) from p = [S, Y]_F'v and G_F = [S, Y]_F'[S, Y]_F.
// The passes:
//   qn_path_pin     status byte + code mask -> the free byte of every row, the pinned rows counted;
//   qn_path_wtv     [S'(f o v); Y'(f o v)] for K vectors (VSLOT: columns of W -- the masked Gram G_F), with the sum of
//                   v_i^2 over the free rows carried on the first tile (DD): qn_shift_wtv's pass, 7 bytes per row less;
//   qn_path_expand  out_j[i] (+)= f_i ? a_j (first ? v_i : 0) + a_j sum_c coef[j][c] W(i, c0 + c) : +0 for ALL k <= 64
//                   shifts in one launch per column tile: qn_cols_kernel's trip (a wave owns 64 R consecutive rows,
//                   the tile's 2 MC entries of a row, v and the free byte read once into registers), coef (k x 2 MC)
//                   and a (k) uniform over the wave, nontemporal stores.
// W is read in the layout it is in (lmask) and never written; v, out and the free bytes are in natural row order.
// A pinned row's sums take +0 and its outputs are +0 by selection, whatever v holds there.
// Reductions: per-lane fp64 accumulators -> block_reduce_store -> qn_finalize, into the operator's own buffers.
//
// Registers of qn_path_expand_kernel at R = 2: vector registers (waves per SIMD) from the compile's resource remarks
// (-Rpass-analysis=kernel-resource-usage), first tile / later tile (ACC), next to qn_cols_kernel with the row weight
// and without it, of the same T, MC, CW (profiles/qn_kernel_resources.csv); NT changes none of them, nothing spills,
// no scratch, no LDS:
//                      qn_path_expand          qn_cols              qn_cols (WGT)
//   fp64  MC  5         56 / 53   (8)           58 / 54   (8)        62 / 58   (8)
//   fp64  MC  5  CW     62 / 59   (8)           66 / 62   (7 / 8)    70 / 66   (7)
//   fp64  MC 10         97 / 93   (4 / 5)       99 / 95   (4 / 5)   103 / 99   (4)
//   fp64  MC 10  CW    103 / 101  (4)          107 / 103  (4)       111 / 107  (4)
//   fp64  MC 16        146 / 143  (3)          148 / 143  (3)       152 / 148  (3)
//   fp32  MC  5         56 / 52   (8)           58 / 54   (8)        62 / 58   (8)
//   fp32  MC 10         97 / 93   (4 / 5)       99 / 95   (4 / 5)   110 / 99   (4)
//   fp32  MC 16        146 / 142  (3)          148 / 143  (3)       163 / 168  (3)
// (at or under the columns pass even without its weight: the byte and v take the place of the diagonal term, the
//  index compare and, against WGT, the 8-byte weight)
#include "k_qn_common.hpp"

namespace lbk {

// free[i] = 1 unless bit (status[i] + 1) of code_mask is set (codes -1 .. 3, as lbfgsb_hip_kkt_list selects them; any
// other value pins nothing); slot 0: the pinned rows.  HAVE: false = no status, every row free
template <bool HAVE>
__global__ __launch_bounds__(BLOCK) void qn_path_pin_kernel(int64_t n, const int8_t *__restrict__ status, int code_mask,
                                                            uint8_t *__restrict__ fre, double *part) {
  double acc[1] = {0.0};
  for_rows<double, 1>(n, [&](int64_t i, auto) {
    bool pin = false;
    if constexpr (HAVE) {
      const int c = (int)status[i];
      pin = c >= -1 && c <= 3 && ((code_mask >> (c + 1)) & 1);
    }
    fre[i] = pin ? (uint8_t)0 : (uint8_t)1;
    acc[0] += pin ? 1.0 : 0.0;
  });
  block_reduce_store<1>(acc, 1, 0, 0, part, MAX_BLOCKS);
}

// sums: slot kk * 2MC + j = S(:, c0 + j)'(f o v_kk), slot kk * 2MC + MC + j = Y(:, c0 + j)'(f o v_kk); VSLOT as in
// qn_wtv_body (the free bytes stay in natural order); DD: K more sums (f o v_kk)'(f o v_kk) from slot 2MC K on
template <typename T, int MC, int K, int V, bool CW, bool VSLOT, bool NT, bool DD>
__global__ __launch_bounds__(BLOCK) void qn_path_wtv_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                            const uint8_t *__restrict__ fre, double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  static_assert(!(VSLOT && DD), "the squared norm belongs to a vector in natural order");
  const QnTile<T> t = QN_TILE_VIEW(T);
  constexpr int NW = 2 * MC * K, NACC = NW + (DD ? K : 0);
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double vv[K][W], a[MC][W], b[MC][W];
    uint8_t fr[W];
#pragma unroll
    for (int w = 0; w < W; ++w) fr[w] = fre[i + w];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, NT>(v.p[kk] + (VSLOT ? s : i), vv[kk]);
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
#pragma unroll
      for (int w = 0; w < W; ++w) vv[kk][w] = fr[w] ? vv[kk][w] : 0.0;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) qn_dot_acc<MC, W>(acc + kk * 2 * MC, a, b, vv[kk]);
    if constexpr (DD) {
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[NW + kk] += vv[kk][w] * vv[kk][w];
    }
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

// A wave owns 64 R consecutive rows per trip, lane l the rows base + l + 64 r, as in qn_cols_kernel.  coef (k x 2 MC)
// and a (k) are uniform over the wave: scalar loads.  first: the tile that stores a_j v + a_j (the sum); ACC: a later
// tile, which adds a_j (the sum) to what is there.  A pinned row stores +0 either way.
template <typename T, int MC, bool CW, bool NT, bool ACC, int R>
__global__ __launch_bounds__(BLOCK) void qn_path_expand_kernel(int64_t n, QN_TILE_PARAMS(T),
                                                               const double *__restrict__ coef,
                                                               const double *__restrict__ a,
                                                               const T *__restrict__ v,
                                                               const uint8_t *__restrict__ fre, int k,
                                                               T *__restrict__ out, int64_t ldo) {
  constexpr int D = 2 * MC;
  const QnTile<T> t = QN_TILE_VIEW(T);
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t step = ((int64_t)gridDim.x * BLOCK >> 6) * (64 * R);
  for (int64_t base = wave * (64 * R); base < n; base += step) {
    int64_t row[R];
    bool live[R], fr[R];
    double w[D][R], x[R];
    qn_ld_rows<T, MC, CW, NT, R>(t, n, base, lane, row, live, w);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = live[r] ? row[r] : 0;
      fr[r] = fre[i] != 0;
      x[r] = 0.0;
      if constexpr (!ACC) {
        double xv[1];
        ldx<1, NT>(v + i, xv);
        x[r] = xv[0];
      }
    }
    for (int j = 0; j < k; ++j) {
      double acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.0;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double cf = coef[j * D + c];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = __builtin_fma(cf, w[c][r], acc[r]);
      }
      const double aj = a[j];
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (live[r]) {
          double o = aj * acc[r];
          if constexpr (ACC) o = (double)out[j * ldo + row[r]] + o;
          else o = aj * x[r] + o;
          const double ov[1] = {fr[r] ? o : 0.0};
          stnt<1>(out + (j * ldo + row[r]), ov);
        }
    }
  }
}

constexpr int QN_PATH_ROWS = 2;  // rows per lane, as the columns pass (QN_COLS_ROWS)

// ---------------------------------------------------------------- launches (dispatch: k_qn_common.hpp)
hipError_t launch_qn_path_pin(const Queue &q, int64_t n, const int8_t *status, int code_mask, uint8_t *fre,
                              double *part, double *res) {
  int g = 0;
  QN_DISPATCH_BOOL(status != nullptr, HAVE, {
    auto kern = qn_path_pin_kernel<HAVE>;
    g = grid_for_w(q, n, 1, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, status, code_mask, fre, part);
  });
  return launch_qn_finalize(q, part, g, 1, res);
}

template <typename T>
hipError_t launch_qn_path_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                              QnVecs<T> v, bool vslot, bool dd, const uint8_t *fre, double *part, double *res) {
  // (the masked Gram takes blocks of 1, 2 or 4 columns; a vector goes alone)
  if (!qn_block_ok(mc, k) || (vslot && dd) || (!vslot && k != 1)) return hipErrorInvalidValue;
  const bool vec2 = !vslot && all_aligned_for(v.p, k, 2);
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT,
      QN_DISPATCH_BOOL(vslot, VS, QN_DISPATCH_BOOL(dd, DD, {
    if constexpr ((VS && V == 1 && !DD) || (!VS && K == 1)) {
      auto kern = qn_path_wtv_kernel<T, MC, K, V, CW, VS, NT, DD>;
      g = grid_for_w(q, n, V, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), v, fre, part);
    }
  }))))));
  if (g == 0) return hipErrorInvalidValue;
  return launch_qn_finalize(q, part, g, 2 * mc * k + (dd ? k : 0), res);
}

template <typename T>
hipError_t launch_qn_path_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, bool acc,
                                 const double *coef, const double *a, const T *v, const uint8_t *fre, int k, T *out,
                                 int64_t ldo) {
  if (k < 1 || k > QN_PATH_MAXK || (mc != 5 && mc != 10 && mc != QN_TILE) || (!acc && !v))
    return hipErrorInvalidValue;
  const bool vec2 = false;  // (QN_DISPATCH_CW's rows per load: this kernel's rows are R waves apart)
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, QN_DISPATCH_BOOL(acc, ACC, {
    if constexpr (V == 1) {
      constexpr int R = QN_PATH_ROWS;
      auto kern = qn_path_expand_kernel<T, MC, CW, NT, ACC, R>;
      const int g = grid_for_w(q, (n + R - 1) / R, 1, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), coef, a, v, fre,
                         k, out, ldo);
      done = true;
    }
  }))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

#define INST(T)                                                                                                      \
  template hipError_t launch_qn_path_wtv<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int, QnVecs<T>,   \
                                            bool, bool, const uint8_t *, double *, double *);                       \
  template hipError_t launch_qn_path_expand<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, bool,          \
                                               const double *, const double *, const T *, const uint8_t *, int, T *, \
                                               int64_t);
INST(double)
INST(float)
#undef INST

}  // namespace lbk
