// k_qn_idx.hip -- entries of the curvature model at index lists (lbfgsb_hip_qn_rows / qn_block / qn_cols and the
// shifted twins, solver_qn_idx.inl).  (part of the gfx950 kernel set; kernels_common.hpp has
// the overview)
//
//   qn_rows_kernel   the gather: entry idx_j of every logical column of [S, Y] (and of the weights), widened to
//                    double, k x (2 col [+ 1]) values into a buffer of the caller's own.  A row of another rank
//                    stores 0.0.  The indices have been checked on the host: 0 <= idx < n_global.
//   qn_cols_kernel   qn_basis_kernel's pass with the row weight and the diagonal term fused:
//                      out_j[i] (+)= f_i sum_c coef[j][c] W(i, c0 + c)  (+ dterm_j on the row idx_j, first tile),
//                    f_i = 1 or wgt_i.  One launch per column tile writes all k <= 128 outputs.
// W is read in the layout it is in and never written; the weights and the outputs are in natural row order.  No
// reduction, no partial sums: nothing of the Queue's buffers is touched.
#include "k_qn_common.hpp"

namespace lbk {

// one thread per element e = j + c kc of the chunk: index j, logical column c (c < col: S, c < 2 col: Y, else the
// weight)
template <typename T>
__global__ __launch_bounds__(BLOCK) void qn_rows_kernel(int64_t n, int64_t row0, const T *__restrict__ ws,
                                                        const T *__restrict__ wy, int64_t ldw, int m, int head,
                                                        int col, const uint64_t *__restrict__ lmask,
                                                        const int64_t *__restrict__ idx, int kc,
                                                        const double *__restrict__ wgt, double *__restrict__ out) {
  const int ncol = 2 * col + (wgt ? 1 : 0);
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= (int64_t)kc * ncol) return;
  const int j = (int)(e % kc), c = (int)(e / kc);
  const int64_t loc = idx[j] - row0;
  double v = 0.0;
  if (loc >= 0 && loc < n) {  // this rank owns the row
    if (c < 2 * col) {
      const int64_t s = wrow(lmask, loc);
      const int64_t off = (int64_t)((head - 1 + (c < col ? c : c - col)) % m) * ldw + s;
      v = (double)(c < col ? ws : wy)[off];
    } else {
      v = wgt[loc];
    }
  }
  out[e] = v;
}

template <typename T>
hipError_t launch_qn_rows(const Queue &q, int64_t n, int64_t row0, WStore<T> w, int head, int col,
                          const int64_t *idx, int kc, const double *wgt, double *out) {
  const int64_t total = (int64_t)kc * (2 * col + (wgt ? 1 : 0));
  if (kc < 1 || total < 1 || total > QN_IDX_BUF) return hipErrorInvalidValue;
  const int g = (int)((total + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(qn_rows_kernel<T>, dim3(g), dim3(BLOCK), 0, q.stream, n, row0, w.ws, w.wy, w.ld, w.m, head, col,
                     w.lmask, idx, kc, wgt, out);
  return hipGetLastError();
}

// A wave owns 64 R consecutive rows per trip, lane l the rows base + l + 64 r, as in qn_basis_kernel: the tile's 2 MC
// entries of a row are read once into registers, every store writes 64 consecutive rows of one output.  coef (k x 2 MC),
// dterm (k) and idx (k global rows) are uniform over the wave: scalar loads.  WGT: the sums are weighed by wgt, and a
// row with wgt = 0 stores +0 on the first tile (and keeps it on the later ones: +0 + 0).
template <typename T, int MC, bool CW, bool WGT, bool NT, bool ACC, int R>
__global__ __launch_bounds__(BLOCK) void qn_cols_kernel(int64_t n, int64_t row0, QN_TILE_PARAMS(T),
                                                        const double *__restrict__ coef,
                                                        const double *__restrict__ dterm,
                                                        const int64_t *__restrict__ idx,
                                                        const double *__restrict__ wgt, int k, T *__restrict__ out,
                                                        int64_t ldo) {
  constexpr int D = 2 * MC;
  const QnTile<T> t = QN_TILE_VIEW(T);
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t step = ((int64_t)gridDim.x * BLOCK >> 6) * (64 * R);
  for (int64_t base = wave * (64 * R); base < n; base += step) {
    int64_t row[R];
    bool live[R];
    double w[D][R], f[R];
    qn_ld_rows<T, MC, CW, NT, R>(t, n, base, lane, row, live, w);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      f[r] = 1.0;
      if constexpr (WGT) f[r] = wgt[live[r] ? row[r] : 0];
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
      const int64_t own = idx[j] - row0;  // the local row of the diagonal term (outside 0 .. n - 1: another rank's)
      const double dt = dterm[j];
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (live[r]) {
          double o = acc[r];
          if constexpr (WGT) o = f[r] == 0.0 ? 0.0 : f[r] * o;
          if constexpr (ACC) o = (double)out[j * ldo + row[r]] + o;
          else if (row[r] == own) o = o + dt;
          const double ov[1] = {o};
          stnt<1>(out + (j * ldo + row[r]), ov);
        }
    }
  }
}

constexpr int QN_COLS_ROWS = 2;  // rows per lane, as the basis pass (QN_BASIS_ROWS)

template <typename T>
hipError_t launch_qn_cols(const Queue &q, int64_t n, int64_t row0, WStore<T> w, int head, int col, int c0, int mc,
                          bool acc, const double *coef, const double *dterm, const int64_t *idx, const double *wgt,
                          int k, T *out, int64_t ldo) {
  if (k < 1 || k > QN_BASIS_KMAX || (mc != 5 && mc != 10 && mc != QN_TILE)) return hipErrorInvalidValue;
  const bool vec2 = false;  // (QN_DISPATCH_CW's rows per load: this kernel's rows are R waves apart)
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(wgt != nullptr, WGT,
                 QN_DISPATCH_BOOL(q.nt, NT, QN_DISPATCH_BOOL(acc, ACC, {
    if constexpr (V == 1) {
      constexpr int R = QN_COLS_ROWS;
      auto kern = qn_cols_kernel<T, MC, CW, WGT, NT, ACC, R>;
      const int g = grid_for_w(q, (n + R - 1) / R, 1, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, row0, QN_TILE_ARGS(w, head, col, c0), coef, dterm,
                         idx, wgt, k, out, ldo);
      done = true;
    }
  })))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

#define INST(T)                                                                                                      \
  template hipError_t launch_qn_rows<T>(const Queue &, int64_t, int64_t, WStore<T>, int, int, const int64_t *, int,   \
                                        const double *, double *);                                                   \
  template hipError_t launch_qn_cols<T>(const Queue &, int64_t, int64_t, WStore<T>, int, int, int, int, bool,         \
                                        const double *, const double *, const int64_t *, const double *, int, T *,   \
                                        int64_t);
INST(double)
INST(float)
#undef INST

}  // namespace lbk
