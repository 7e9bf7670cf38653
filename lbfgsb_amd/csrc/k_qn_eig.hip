// k_qn_eig.hip -- the basis pass of the curvature model's eigenvectors (lbfgsb_hip_qn_eigvec, solver_qn.inl;
// DESIGN.md section 10e).  (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// OUT(n x k) = W(n x 2col) C(2col x k), tall and skinny: one launch per column tile of at most 16 pairs (qn_plan.hpp,
// qn_basis_plan) reads the tile's 2 MC entries of a row ONCE into registers and writes all k <= 128 outputs,
//   out_j[i] (+)= sum_c coef[j][c] W(i, c0 + c),
// against qn_expand_kernel's pass over W per 4 vectors.  W is read in the layout it is in and never written; the
// outputs are in natural row order.  No reduction, no partial sums: nothing of the Queue's buffers is touched.
//
// A wave owns 64 R consecutive rows per trip, lane l the rows base + l + 64 r: every store instruction writes 64
// consecutive rows of one output (512 B in fp64), and each coefficient, which is uniform over the wave, is read once
// for R rows per lane.  The coefficients come straight from the kernel argument's buffer, whose uniform indices the
// compiler turns into scalar loads (measured against a copy staged in LDS: DESIGN.md section 10e).
#include "k_qn_common.hpp"

namespace lbk {

template <typename T, int MC, bool CW, bool NT, bool ACC, int R>
__global__ __launch_bounds__(BLOCK) void qn_basis_kernel(int64_t n, QN_TILE_PARAMS(T),
                                                         const double *__restrict__ coef, int k, T *__restrict__ out,
                                                         int64_t ldo) {
  constexpr int D = 2 * MC;
  const QnTile<T> t = QN_TILE_VIEW(T);
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t step = ((int64_t)gridDim.x * BLOCK >> 6) * (64 * R);
  for (int64_t base = wave * (64 * R); base < n; base += step) {
    int64_t row[R];
    bool live[R];
    double w[D][R];
    qn_ld_rows<T, MC, CW, NT, R>(t, n, base, lane, row, live, w);
    for (int j = 0; j < k; ++j) {
      double acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r] = 0.0;
        if constexpr (ACC)
          if (live[r]) acc[r] = (double)out[j * ldo + row[r]];
      }
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double cf = coef[j * D + c];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = __builtin_fma(cf, w[c][r], acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (live[r]) {
          const double o[1] = {acc[r]};
          stnt<1>(out + (j * ldo + row[r]), o);
        }
    }
  }
}

// rows per lane: two at every capacity -- 4 MC doubles of operands, 128 registers at 16 pairs, three waves per SIMD
constexpr int QN_BASIS_ROWS = 2;

template <typename T>
hipError_t launch_qn_basis(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, bool acc,
                           const double *coef, int k, T *out, int64_t ldo) {
  if (k < 1 || k > QN_BASIS_KMAX || (mc != 5 && mc != 10 && mc != QN_TILE)) return hipErrorInvalidValue;
  const bool vec2 = false;  // (QN_DISPATCH_CW's rows per load: this kernel's rows are R waves apart)
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, QN_DISPATCH_BOOL(acc, ACC, {
    if constexpr (V == 1) {
      constexpr int R = QN_BASIS_ROWS;
      auto kern = qn_basis_kernel<T, MC, CW, NT, ACC, R>;
      const int g = grid_for_w(q, (n + R - 1) / R, 1, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), coef, k, out,
                         ldo);
      done = true;
    }
  }))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

template hipError_t launch_qn_basis<double>(const Queue &, int64_t, WStore<double>, int, int, int, int, bool,
                                            const double *, int, double *, int64_t);
template hipError_t launch_qn_basis<float>(const Queue &, int64_t, WStore<float>, int, int, int, int, bool,
                                           const double *, int, float *, int64_t);

}  // namespace lbk
