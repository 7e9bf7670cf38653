// k_bounds.hip -- bounds that the caller edits during a run (LBFGSB_F_FOLLOW_BOUNDS)
// (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// The reference re-reads l, u and nbd on every call (projgr src/lbfgsb.f90:582, :781, cauchy :617, subsm
// :2789-2816, lnsrlb :731); the passes over W read the context's snapshot of them instead: constants for arrays
// that hold one value, table entries selected by the packed nbd byte for arrays with a few values, the packed
// byte itself, and -- in a context created with the flag -- device copies l_snap / u_snap of the arrays that are
// streamed.  This pass compares the caller's three arrays with that snapshot bit for bit, once per call.  It
// stores nothing: a difference sends the host to the full rebuild (the same analysis START runs), which also
// decides whether the new arrays are uniform, few-valued or plain.
#include "kernels_common.hpp"

namespace lbk {

// ub bits as in the passes over W.  res: sum [0] rows whose l, u or nbd differ from the snapshot,
// [1] rows whose nbd lies outside 0..3 (the packed byte cannot hold such a value)
template <typename T>
__global__ __launch_bounds__(BLOCK) void bounds_follow_kernel(int64_t n, const T *__restrict__ l,
                                                              const T *__restrict__ u,
                                                              const int32_t *__restrict__ nbd,
                                                              const T *__restrict__ l_snap,
                                                              const T *__restrict__ u_snap,
                                                              const nb_t *__restrict__ code, int ub, BoundTables tb,
                                                              int force, double *part) {
  // (force: a change this rank knows of without looking -- other pointers, an announcement -- counted once, so
  //  that the sum over the ranks sends every rank to the rebuild at the same entry)
  double acc[2] = {(blockIdx.x == 0 && threadIdx.x == 0) ? (double)force : 0.0, 0.0};
  const bool dict = (ub & UB_DICT) != 0;
  for_rows<T>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    double lv[W], uv[W], ls[W], us[W];
    int nb[W], cd[W];
    ld<W>(l + i, lv);
    ld<W>(u + i, uv);
    ldi<W>(nbd + i, nb);
    // (what l, u are compared with outside the dictionary: the constant, or the copy)
    if (!dict && !(ub & 1)) {
      ld<W>(l_snap + i, ls);
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k) ls[k] = tb.l[0];
    }
    if (!dict && !(ub & 2)) {
      ld<W>(u_snap + i, us);
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k) us[k] = tb.u[0];
    }
    if (ub & 4) {
#pragma unroll
      for (int k = 0; k < W; ++k) cd[k] = 0;
    } else {
      ldi<W>(code + i, cd);
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const unsigned c = (unsigned)cd[k] & 0xffu;
      const long long lb = __double_as_longlong(lv[k]), ubits = __double_as_longlong(uv[k]);
      bool bad;
      if (dict) {
        bad = nb[k] != (int)(c & 3u) || lb != __double_as_longlong(tb.l[(c >> 2) & 7u]) ||
              ubits != __double_as_longlong(tb.u[c >> 5]);
      } else {
        bad = (ub & 4) ? nb[k] != tb.nb0 : nb[k] != cd[k];
        bad = bad || lb != __double_as_longlong(ls[k]) || ubits != __double_as_longlong(us[k]);
      }
      if (bad) acc[0] += 1.0;
      if (nb[k] < 0 || nb[k] > 3) acc[1] += 1.0;
    }
  });
  block_reduce_store<2>(acc, 2, 0, 0, part, MAX_BLOCKS);
}
template <typename T>
void launch_bounds_follow(Queue &q, int64_t n, const T *l, const T *u, const int32_t *nbd, const T *l_snap,
                          const T *u_snap, const nb_t *code, int ub, const BoundTables &tb, int force) {
  const int g = grid_for(n, VecOf<T>::V);
  hipLaunchKernelGGL(bounds_follow_kernel<T>, dim3(g), dim3(BLOCK), 0, q.stream, n, l, u, nbd, l_snap, u_snap, code,
                     ub, tb, force, q.part());
  LB_LAUNCHED(q);
  launch_finalize(q, g, 2, 0, 0);
}

#define INSTANTIATE(T)                                                                                              \
  template void launch_bounds_follow<T>(Queue &, int64_t, const T *, const T *, const int32_t *, const T *, const T *, \
                                        const nb_t *, int, const BoundTables &, int);
INSTANTIATE(double)
INSTANTIATE(float)
#undef INSTANTIATE

}  // namespace lbk
