// k_qn_pairs.hip -- the stored pairs of the curvature model out of W and into it (lbfgsb_hip_qn_pairs_get / _set /
// _push, solver_qn_pairs.inl).  (part of the gfx950 kernel set; kernels_common.hpp has the
// overview)
//
//   qn_pairs_get_kernel   the pairs c0 .. c0 + MC - 1 of a column tile, row by row out of W in the layout it is in,
//                         into the caller's columns S + c lds, Y + c ldy (natural row order, oldest pair first);
//   qn_pairs_load_kernel  k of the caller's columns into the ring slots slot0, slot0 + 1, ... of W in natural row
//                         order (the caller sets the layout mask: launch_lmask_ones): 16 bytes per lane and access
//                         where both sides allow it, else element by element.
// Every value is touched once: nontemporal loads where the context streams W (q.nt), nontemporal stores to the
// caller's columns; the stores into W are plain when W fits the cache (the Gram pass that follows a load reads them
// back).  No reduction: nothing of the Queue's buffers is touched.  The sums of a push are the Gram-carrying W'V pass
// of k_qn.hip (launch_qn_wtv, two vectors): no kernel of its own.
#include "k_qn_common.hpp"

namespace lbk {

// qn_expand_kernel's trip with the stores turned round: the tile's 2 MC entries of V rows per lane are read once,
// every store writes V consecutive rows of one of the caller's columns.  Columns >= col read the zero line and store
// nothing.
template <typename T, int MC, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_pairs_get_kernel(int64_t n, QN_TILE_PARAMS(T), T *__restrict__ s_out,
                                                             int64_t lds, T *__restrict__ y_out, int64_t ldy) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  const QnTile<T> t = QN_TILE_VIEW(T);
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double a[MC][W], b[MC][W];
    qn_ld_tile<T, MC, W, NT>(t, s, a, b);
#pragma unroll
    for (int j = 0; j < MC; ++j)
      if (c0 + j < col) {  // (uniform over the grid)
        stnt<W>(s_out + ((int64_t)(c0 + j) * lds + i), a[j]);
        stnt<W>(y_out + ((int64_t)(c0 + j) * ldy + i), b[j]);
      }
  });
}

template <typename T>
hipError_t launch_qn_pairs_get(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, T *s_out,
                               int64_t lds, T *y_out, int64_t ldy) {
  if (c0 < 0 || c0 >= col || (mc != 5 && mc != 10 && mc != QN_TILE) || lds < n || ldy < n)
    return hipErrorInvalidValue;
  // (two rows per lane where the caller's columns take 2-element stores and the tile's 4 mc operands leave room)
  const bool vec2 = mc <= 10 && aligned_for(s_out, 2) && aligned_for(y_out, 2) && lds % 2 == 0 && ldy % 2 == 0;
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    auto kern = qn_pairs_get_kernel<T, MC, V, CW, NT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), s_out, lds, y_out,
                       ldy);
    done = true;
  })));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

// ws(:, (slot0 + j) % m) = S(:, j), wy(...) = Y(:, j), j < k, natural row order.  V rows per lane and access: 16 bytes
// (launch_qn_pairs_load decides), or 1.  NT: nontemporal loads of the caller's columns and stores into W.
template <typename T, int V, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_pairs_load_kernel(int64_t n, T *__restrict__ ws, T *__restrict__ wy,
                                                              int64_t ldw, int m, int slot0, int k,
                                                              const T *__restrict__ s_in, int64_t lds,
                                                              const T *__restrict__ y_in, int64_t ldy) {
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    for (int j = 0; j < k; ++j) {
      const int64_t off = (int64_t)((slot0 + j) % m) * ldw + i;
      double a[W], b[W];
      ldx<W, NT>(s_in + ((int64_t)j * lds + i), a);
      ldx<W, NT>(y_in + ((int64_t)j * ldy + i), b);
      if constexpr (NT) {
        stnt<W>(ws + off, a);
        stnt<W>(wy + off, b);
      } else {
        st<W>(ws + off, a);
        st<W>(wy + off, b);
      }
    }
  });
}

template <typename T>
hipError_t launch_qn_pairs_load(const Queue &q, int64_t n, WStore<T> w, int slot0, int k, const T *s_in, int64_t lds,
                                const T *y_in, int64_t ldy) {
  if (k < 1 || k > w.m || slot0 < 0 || slot0 >= w.m || lds < n || ldy < n || w.lmask) return hipErrorInvalidValue;
  constexpr int VW = 16 / (int)sizeof(T);
  // (W's columns start on 256-byte boundaries: the caller's side decides)
  const bool wide = aligned_for(s_in, VW) && aligned_for(y_in, VW) && lds % VW == 0 && ldy % VW == 0;
  QN_DISPATCH_BOOL(wide, WIDE, QN_DISPATCH_BOOL(q.nt, NT, {
    constexpr int V = WIDE ? VW : 1;
    auto kern = qn_pairs_load_kernel<T, V, NT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, w.ws, w.wy, w.ld, w.m, slot0, k, s_in, lds, y_in,
                       ldy);
  }));
  return hipGetLastError();
}

#define INST(T)                                                                                                      \
  template hipError_t launch_qn_pairs_get<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, T *, int64_t,    \
                                             T *, int64_t);                                                          \
  template hipError_t launch_qn_pairs_load<T>(const Queue &, int64_t, WStore<T>, int, int, const T *, int64_t,       \
                                              const T *, int64_t);
INST(double)
INST(float)
#undef INST

}  // namespace lbk
