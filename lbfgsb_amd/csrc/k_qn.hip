// k_qn.hip -- the limited-memory curvature model as a device operator (lbfgsb_hip_qn_apply / lbfgsb_hip_qn_diag,
// solver_qn.inl).  (part of the gfx950 kernel set; kernels_common.hpp has the overview)
//
// B = theta I + [S, Y] N_B [S, Y]'   and   H = B^-1 = theta^-1 I + [S, Y] N_H [S, Y]'
// with the 2col x 2col matrices N formed on the host (host_dense.hpp, qn_coef_b / qn_coef_h).  The passes:
//   qn_wtv     [S'v; Y'v] for K vectors at once (every W entry read once per block of K vectors);
//   qn_wtd     the same for d = v - center with d'd carried along: the one pass of a quadratic form d'A d;
//   qn_wtg     qn_wtd with the block's whole Gram d_a'd_b, a <= b, carried along (lbfgsb_hip_qn_gram, section 10d);
//   qn_dtd     d_a'd_b for a in one block of vectors and b in another: vectors only, nothing of W;
//   qn_expand  out_j = alpha src_j + S cs_j + Y cy_j (coefficients as kernel arguments);
//   qn_diag    out_i = alpha + r_i' N r_i,  r_i = row i of [S, Y], N in LDS (upper triangle, off-diagonal doubled).
// None of them writes W: they read it in the layout it is in (natural order, or the tile-local layout of k_layout.hip
// through the lmask bits), and v / out are always in natural row order.  Columns are processed in tiles of at most
// 16 (qn_wtv, qn_expand: any number of pairs) or all at once up to 32 (qn_diag).  Reductions: per-lane fp64
// accumulators -> block_reduce_store -> one partial per workgroup -> qn_finalize in a fixed order, into buffers of
// the operator's own (never the iteration's q.d_part / q.d_res).  Nothing here touches the Queue's counters.
#include "k_qn_common.hpp"

namespace lbk {

// sums: slot kk * 2MC + j = S(:, c0 + j)' v_kk, slot kk * 2MC + MC + j = Y(:, c0 + j)' v_kk (j >= col - c0: zero).
// VSLOT: vector row i is read at the SLOT of row i (the vectors are columns of W themselves: the Gram).
// CEN: the vectors are d_kk = v_kk - center, formed in fp64 in registers (no center: neither a load nor an address).
// DD: K more sums d_kk'd_kk in the slots 2MC K + kk (the first column tile's launch of a quadratic form carries them).
// GG: instead of them the K (K + 1) / 2 sums d_a'd_b, a <= b, row by row of the upper triangle from slot 2MC K on
// (at K = 1 that is DD itself: launch_qn_wtv hands it to qn_wtd_kernel).
// The plain pass (qn_wtv_kernel) is the body with all three off.
template <typename T, int MC, int K, int V, bool CW, bool VSLOT, bool NT, bool CEN, bool DD, bool GG = false>
__device__ __forceinline__ void qn_wtv_body(int64_t n, QN_TILE_PARAMS(T), const QnVecs<T> &v,
                                            const T *__restrict__ center, double *part) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  static_assert(!VSLOT || !(CEN || DD || GG), "a center and the squared norm belong to vectors in natural order");
  static_assert(!(DD && GG), "the Gram holds the squared norms");
  constexpr int NW = 2 * MC * K, NACC = NW + (GG ? K * (K + 1) / 2 : DD ? K : 0);
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double vv[K][W], a[MC][W], b[MC][W];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, NT>(v.p[kk] + (VSLOT ? s : i), vv[kk]);
    double cc[CEN ? W : 1];
    if constexpr (CEN) ldx<W, NT>(center + i, cc);
    // (the tile's loads stay written out here, on the flat arguments, instead of qn_ld_tile on a view: through the
    //  helper qn_wtd_kernel<float, 5, 1, 2> and <float, 5, 2, 2> took 16 and 12 registers more and lost a wave per SIMD)
#pragma unroll
    for (int j = 0; j < MC; ++j) {
      const int64_t off = col_off(c0 + j, col, head, m, ldw) + s;
      ld_col<T, W, NT>(c0 + j < col, ws + off, zero, a[j]);
      ld_col<T, W, NT>(c0 + j < col, wy + off, zero, b[j]);
    }
    // (the differences after every load of the trip is issued, behind a fence for the scheduler: left free, it puts
    //  them between the loads and waits for every column on its own in the natural-order K = 4 kernel)
    if constexpr (CEN) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
#pragma unroll
        for (int w = 0; w < W; ++w) vv[kk][w] -= cc[w];
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
      qn_dot_acc<MC, W>(acc + kk * 2 * MC, a, b, vv[kk]);
    if constexpr (DD) {
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[NW + kk] += vv[kk][w] * vv[kk][w];
    }
    if constexpr (GG) {
      int e = NW;
#pragma unroll
      for (int ka = 0; ka < K; ++ka)
#pragma unroll
        for (int kb = ka; kb < K; ++kb, ++e)
#pragma unroll
          for (int w = 0; w < W; ++w) acc[e] += vv[ka][w] * vv[kb][w];
    }
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

template <typename T, int MC, int K, int V, bool CW, bool VSLOT, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_wtv_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                       double *part) {
  qn_wtv_body<T, MC, K, V, CW, VSLOT, NT, false, false>(n, ws, wy, zero, ldw, m, head, col, c0, lmask, v, nullptr, part);
}

// the W'V pass of a quadratic form (lbfgsb_hip_qn_quad / qn_logpdf): the vectors centred, d'd on the first tile
template <typename T, int MC, int K, int V, bool CW, bool NT, bool CEN, bool DD>
__global__ __launch_bounds__(BLOCK) void qn_wtd_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                       const T *__restrict__ center, double *part) {
  qn_wtv_body<T, MC, K, V, CW, false, NT, CEN, DD>(n, ws, wy, zero, ldw, m, head, col, c0, lmask, v, center, part);
}

// the W'V pass of a Gram matrix (lbfgsb_hip_qn_gram): the first tile's launch, the block's d_a'd_b along (K >= 2)
template <typename T, int MC, int K, int V, bool CW, bool NT, bool CEN>
__global__ __launch_bounds__(BLOCK) void qn_wtg_kernel(int64_t n, QN_TILE_PARAMS(T), QnVecs<T> v,
                                                       const T *__restrict__ center, double *part) {
  qn_wtv_body<T, MC, K, V, CW, false, NT, CEN, false, true>(n, ws, wy, zero, ldw, m, head, col, c0, lmask, v, center, part);
}

// sums: slot ia * KB + ib = d_ia'd_ib, d_ia = a_ia - center of one block of vectors, d_ib = b_ib - center of another:
// the entries of D'D that no W'd launch holds.  (KA + KB + 1) reals per row, natural row order, nothing written.
template <typename T, int KA, int KB, int V, bool NT, bool CEN>
__global__ __launch_bounds__(BLOCK) void qn_dtd_kernel(int64_t n, QnVecs<T> a, QnVecs<T> b,
                                                       const T *__restrict__ center, double *part) {
  constexpr int NACC = KA * KB;
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    double x[KA][W], y[KB][W];
#pragma unroll
    for (int ia = 0; ia < KA; ++ia) ldx<W, NT>(a.p[ia] + i, x[ia]);
#pragma unroll
    for (int ib = 0; ib < KB; ++ib) ldx<W, NT>(b.p[ib] + i, y[ib]);
    double cc[CEN ? W : 1];
    if constexpr (CEN) {
      ldx<W, NT>(center + i, cc);
      __builtin_amdgcn_sched_barrier(0);  // (the differences behind every load of the trip, as in qn_wtv_body)
#pragma unroll
      for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int ia = 0; ia < KA; ++ia) x[ia][w] -= cc[w];
#pragma unroll
        for (int ib = 0; ib < KB; ++ib) y[ib][w] -= cc[w];
      }
    }
#pragma unroll
    for (int ia = 0; ia < KA; ++ia)
#pragma unroll
      for (int ib = 0; ib < KB; ++ib)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[ia * KB + ib] += x[ia][w] * y[ib][w];
  });
  block_reduce_store<NACC>(acc, NACC, 0, 0, part, MAX_BLOCKS);
}

// res[k] = sum over the workgroups' partials of slot k, in a fixed order (one workgroup per slot)
__global__ __launch_bounds__(BLOCK) void qn_finalize_kernel(const double *__restrict__ part, int nblocks,
                                                            double *__restrict__ res) {
  __shared__ double sm[BLOCK];
  const int k = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += BLOCK) v += part[(size_t)k * MAX_BLOCKS + b];
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) res[k] = sm[0];
}

// out_kk[i] = alpha src_kk[i] + sum_j cf.c[kk][j] S(i, c0 + j) + cf.c[kk][MC + j] Y(i, c0 + j)
template <typename T, int MC, int K, int V, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_expand_kernel(int64_t n, QN_TILE_PARAMS(T), QnCoef<MC, K> cf,
                                                          QnVecs<T> src, QnOuts<T> out) {
  static_assert(!CW || V == 1, "the layout is read one row per lane");
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    const int64_t s = qn_slot<CW>(lmask, i);
    double x[K][W], a[MC][W], b[MC][W];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ldx<W, false>(src.p[kk] + i, x[kk]);
    // (loads and sum written out, not qn_ld_tile and qn_comb: with the helpers qn_expand_kernel<float, 16, 1, 1> went
    //  from 130 to 169 registers, 3 waves per SIMD to 2)
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
        double e = cf.alpha * x[kk][w];
#pragma unroll
        for (int j = 0; j < MC; ++j) {
          e += cf.c[kk][j] * a[j][w];
          e += cf.c[kk][MC + j] * b[j][w];
        }
        o[w] = e;
      }
      stnt<W>(out.p[kk] + i, o);
    }
  });
}

// out[i] = alpha + r' N r, r = (S(i, 0..MC), Y(i, 0..MC)); np = the packed upper triangle of N (row-major over
// a <= b, off-diagonal entries doubled), (2MC)(2MC + 1)/2 doubles, staged in LDS once per workgroup
template <typename T, int MC, bool CW, bool NT>
__global__ __launch_bounds__(BLOCK) void qn_diag_kernel(int64_t n, const T *__restrict__ ws, const T *__restrict__ wy,
                                                        const T *__restrict__ zero, int64_t ldw, int m, int head,
                                                        int col, const uint64_t *__restrict__ lmask,
                                                        const double *__restrict__ np, double alpha,
                                                        T *__restrict__ out) {
  constexpr int D = 2 * MC, NP = D * (D + 1) / 2;
  __shared__ double sn[NP];
  for (int e = threadIdx.x; e < NP; e += BLOCK) sn[e] = np[e];
  __syncthreads();
  const QnTile<T> t{ws, wy, zero, ldw, m, head, col, 0, lmask};
  for_rows<T, 1>(n, [&](int64_t i, auto) {
    // (N is re-read from LDS for every row: hoisted out of the row loop, its 2080 entries at 32 pairs would live
    //  in registers and spill to scratch -- the memory clobber keeps the reads here)
    asm volatile("" ::: "memory");
    const int64_t s = qn_slot<CW>(lmask, i);
    double r[D][1];
    qn_ld_tile<T, MC, 1, NT>(t, s, r, r + MC);
    const double o[1] = {alpha + qn_rnr<MC>(sn, r)};
    stnt<1>(out + i, o);
  });
}

// ---------------------------------------------------------------- launches (dispatch: k_qn_common.hpp)
hipError_t launch_qn_finalize(const Queue &q, const double *part, int nblocks, int nslots, double *res) {
  if (nblocks == 0) return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(qn_finalize_kernel, dim3(nslots), dim3(BLOCK), 0, q.stream, part, nblocks, res);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_qn_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                         QnVecs<T> v, bool vslot, const T *center, QnCarry carry, double *part, double *res) {
  if (!qn_block_ok(mc, k) || (vslot && (center || carry != QnCarry::None))) return hipErrorInvalidValue;
  // (one vector: its Gram is its squared norm -- qn_wtd's kernel, no second instantiation of it)
  const bool gg = carry == QnCarry::Gram && k >= 2, dd = carry != QnCarry::None && !gg;
  // (two rows per lane only where operands + accumulators leave room for them: 2 mc k <= 20 sums.  At those shapes
  //  the K squared norms and the center's V entries add 2 (K + V) <= 8 registers to the plain pass's operands and sums
  //  -- 140 against 136 at the largest, mc = 10, k = 1: three waves per SIMD still; a Gram has them at 5 columns and
  //  K = 2 only)
  const bool vec2 = !vslot && 2 * mc * k <= 20 && (!center || aligned_for(center, 2)) && all_aligned_for(v.p, k, 2);
  int g = 0;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    auto go = [&](auto kern, auto... cen) {
      g = grid_for_w(q, n, V, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), v, cen...,
                         part);
    };
    if (!center && carry == QnCarry::None) {  // (the later column tiles of an uncentred form too: the plain pass)
      QN_DISPATCH_BOOL(vslot, VS, go(qn_wtv_kernel<T, MC, K, V, CW, VS, NT>));
    } else if (gg) {
      if constexpr (K >= 2)
        QN_DISPATCH_BOOL(center != nullptr, CEN, go(qn_wtg_kernel<T, MC, K, V, CW, NT, CEN>, center));
    } else {
      QN_DISPATCH_BOOL(center != nullptr, CEN, QN_DISPATCH_BOOL(dd, DD, {
        if constexpr (CEN || DD) go(qn_wtd_kernel<T, MC, K, V, CW, NT, CEN, DD>, center);
      }));
    }
  }))));
  return launch_qn_finalize(q, part, g, 2 * mc * k + qn_carried(carry, k), res);
}

#define QN_DISPATCH_KAB(k, NAME, ...) \
  do {                                \
    if ((k) == 1) {                   \
      constexpr int NAME = 1;         \
      __VA_ARGS__;                    \
    } else if ((k) == 2) {            \
      constexpr int NAME = 2;         \
      __VA_ARGS__;                    \
    } else {                          \
      constexpr int NAME = 4;         \
      __VA_ARGS__;                    \
    }                                 \
  } while (0)

template <typename T>
hipError_t launch_qn_dtd(const Queue &q, int64_t n, QnVecs<T> a, int ka, QnVecs<T> b, int kb, const T *center,
                         double *part, double *res) {
  if ((ka != 1 && ka != 2 && ka != 4) || (kb != 1 && kb != 2 && kb != 4)) return hipErrorInvalidValue;
  const bool vec2 = (!center || aligned_for(center, 2)) && all_aligned_for(a.p, ka, 2) && all_aligned_for(b.p, kb, 2);
  int g = 0;
  QN_DISPATCH_KAB(ka, KA, QN_DISPATCH_KAB(kb, KB, QN_DISPATCH_BOOL(vec2, V2, QN_DISPATCH_BOOL(q.nt, NT,
      QN_DISPATCH_BOOL(center != nullptr, CEN, {
    auto kern = qn_dtd_kernel<T, KA, KB, V2 ? 2 : 1, NT, CEN>;
    g = grid_for_w(q, n, V2 ? 2 : 1, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, a, b, center, part);
  })))));
  return launch_qn_finalize(q, part, g, ka * kb, res);
}
#undef QN_DISPATCH_KAB

template <typename T>
hipError_t launch_qn_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                            const double *coef, double alpha, QnVecs<T> src, QnOuts<T> out) {
  if (!qn_block_ok(mc, k)) return hipErrorInvalidValue;
  const bool vec2 = 2 * mc * k <= 20 && all_aligned_for(src.p, k, 2) && all_aligned_for(out.p, k, 2);
  bool done = false;
  QN_DISPATCH_MC(mc, QN_DISPATCH_K(k, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    const QnCoef<MC, K> cf = qn_coef_args<MC, K>(coef, alpha);
    auto kern = qn_expand_kernel<T, MC, K, V, CW, NT>;
    const int g = grid_for_w(q, n, V, (const void *)kern);
    hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, QN_TILE_ARGS(w, head, col, c0), cf, src, out);
    done = true;
  }))));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T>
hipError_t launch_qn_diag(const Queue &q, int64_t n, WStore<T> w, int head, int col, const double *np, double alpha,
                          T *out) {
  const bool vec2 = false;
  bool done = false;
  DISPATCH_MAXC(col, QN_DISPATCH_CW(w.lmask, QN_DISPATCH_BOOL(q.nt, NT, {
    if constexpr (V == 1) {
      auto kern = qn_diag_kernel<T, MC, CW, NT>;
      const int g = grid_for_w(q, n, 1, (const void *)kern);
      hipLaunchKernelGGL(kern, dim3(g), dim3(BLOCK), 0, q.stream, n, w.ws, w.wy, w.zero, w.ld, w.m, head, col,
                         w.lmask, np, alpha, out);
      done = true;
    }
  })));
  if (!done) return hipErrorInvalidValue;
  return hipGetLastError();
}

#define QN_INST(T)                                                                                                  \
  template hipError_t launch_qn_wtv<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int, QnVecs<T>,   \
                                       bool, const T *, QnCarry, double *, double *);                             \
  template hipError_t launch_qn_dtd<T>(const Queue &, int64_t, QnVecs<T>, int, QnVecs<T>, int, const T *,       \
                                       double *, double *);                                                       \
  template hipError_t launch_qn_expand<T>(const Queue &, int64_t, WStore<T>, int, int, int, int, int,          \
                                          const double *, double, QnVecs<T>, QnOuts<T>);                         \
  template hipError_t launch_qn_diag<T>(const Queue &, int64_t, WStore<T>, int, int, const double *, double, T *);
QN_INST(double)
QN_INST(float)
#undef QN_INST

}  // namespace lbk
