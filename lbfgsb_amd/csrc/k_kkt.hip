// k_kkt.hip -- the active set, the bound multipliers and the projected gradient of an iterate as device data
// (lbfgsb_hip_kkt / lbfgsb_hip_kkt_list, solver_kkt.inl).  (part of the gfx950 kernel set;
// kernels_common.hpp has the overview)
//
//   kkt_kernel   one pass over the caller's x, l, u, nbd, g (36 B per row in fp64): per row the status in the
//                reference's iwhere codes (the precedence of `active`, src/lbfgsb.f90:994-1028), the signed projected
//                gradient (proj_g_signed: projgr's own row formula) and the signed multiplier, into whichever of the
//                three outputs the instantiation has; nine counts and four maxima per lane -> block_reduce_store ->
//                kkt_finalize_kernel in a fixed order.
//   kkt_list_*   the rows of selected status, ascending, as 64-bit global indices: count per chunk, scan of the chunk
//                totals, write with the position inside a wave from ballot and mbcnt -- a stable compaction, no
//                atomic hands out a position.
// Partials, results and the scan space are the report's own buffers (never the iteration's q.d_part / q.d_res), and
// nothing here touches the Queue's counters: a run computes the same bits whether or not these are launched.
#include "kernels_common.hpp"

namespace lbk {

// PG / MU / ST: the instantiation stores pg / mult / status; an output that is absent costs neither a store nor its
// address.  V rows per lane (16 B per array and lane, or 1 where an array is not aligned for that).
template <typename T, int V, bool PG, bool MU, bool ST>
__global__ __launch_bounds__(BLOCK) void kkt_kernel(int64_t n, const T *__restrict__ x, const T *__restrict__ l,
                                                    const T *__restrict__ u, const int32_t *__restrict__ nbd,
                                                    const T *__restrict__ g, double tol, T *__restrict__ pg,
                                                    T *__restrict__ mult, int8_t *__restrict__ status,
                                                    double *part) {
  constexpr KktSlots S{};
  constexpr int NSUM = KktSlots::nsum(), NMAX = KktSlots::NVAL, K = KktSlots::size();
  unsigned cnt[NSUM];  // (per lane: at most its share of the rows -- exact, and cheaper than fp64 adds)
  double mx[NMAX];     // (maxima of magnitudes: 0 is the identity, as in projgr_kernel)
#pragma unroll
  for (int k = 0; k < NSUM; ++k) cnt[k] = 0u;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) mx[k] = 0.0;
  for_rows<T, V>(n, [&](int64_t i, auto wt) {
    constexpr int W = decltype(wt)::value;
    double xv[W], lv[W], uv[W], gv[W];
    int nb[W];
    ld<W>(x + i, xv);
    ld<W>(l + i, lv);
    ld<W>(u + i, uv);
    ld<W>(g + i, gv);
    ldi<W>(nbd + i, nb);
    double pv[W], mv[W];
    int sv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int b = nb[k];
      const double xk = xv[k], lk = lv[k], uk = uv[k], gk = gv[k];
      // (a bound that nbd says does not exist is never compared: NaN there changes nothing)
      const bool hasl = b == 1 || b == 2, hasu = b == 2 || b == 3;
      const bool atl = hasl && xk <= lk, atu = hasu && xk >= uk;
      const int s = b == 0 ? -1 : ((b == 2 && uk - lk <= 0.0) ? 3 : (atl ? 1 : (atu ? 2 : 0)));
      const bool s1 = s == 1, s2 = s == 2;
      const bool bind = (s1 && gk > 0.0) || (s2 && gk < 0.0);
      const double p = proj_g_signed(xk, lk, uk, b, gk);
      const double mk = (s == 3 || bind) ? gk : 0.0;
      const double ag = fabs(gk);
      const bool out = (hasl && xk < lk) || (hasu && xk > uk);
      const double dist = fmax(hasl ? lk - xk : 0.0, hasu ? xk - uk : 0.0);
      pv[k] = p, mv[k] = mk, sv[k] = s;
      // (selects, not an index: a status-indexed accumulator array would live in scratch memory)
#pragma unroll
      for (int c = -1; c <= 3; ++c) cnt[S.status(c)] += s == c ? 1u : 0u;
      cnt[S.binding()] += bind ? 1u : 0u;
      cnt[S.weak()] += ((s1 || s2) && ag <= tol) ? 1u : 0u;
      cnt[S.leaving()] += ((s1 && gk < -tol) || (s2 && gk > tol)) ? 1u : 0u;
      cnt[S.outside()] += out ? 1u : 0u;
      mx[S.pg_max() - NSUM] = fmax(mx[S.pg_max() - NSUM], fabs(p));
      mx[S.mult_max() - NSUM] = fmax(mx[S.mult_max() - NSUM], fabs(mk));
      mx[S.out_max() - NSUM] = fmax(mx[S.out_max() - NSUM], out ? dist : 0.0);
      mx[S.gfree_max() - NSUM] = fmax(mx[S.gfree_max() - NSUM], s <= 0 ? ag : 0.0);
    }
    if constexpr (PG) stnt<W>(pg + i, pv);
    if constexpr (MU) stnt<W>(mult + i, mv);
    if constexpr (ST) sti<W>(status + i, sv);
  });
  double acc[K];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) acc[k] = (double)cnt[k];
#pragma unroll
  for (int k = 0; k < NMAX; ++k) acc[NSUM + k] = mx[k];
  block_reduce_store<K>(acc, NSUM, 0, NMAX, part, MAX_BLOCKS);
}

// res[k] = the workgroups' partials of slot k added (k < nsum) or maximised, in a fixed order: one workgroup per slot
__global__ __launch_bounds__(BLOCK) void kkt_finalize_kernel(const double *__restrict__ part, int nblocks, int nsum,
                                                             double *__restrict__ res) {
  __shared__ double sm[BLOCK];
  const int k = blockIdx.x;
  const bool sum = k < nsum;
  double v = 0.0;  // (the maxima are of magnitudes)
  for (int b = threadIdx.x; b < nblocks; b += BLOCK) {
    const double p = part[(size_t)k * MAX_BLOCKS + b];
    v = sum ? v + p : fmax(v, p);
  }
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double a = sm[threadIdx.x], b = sm[threadIdx.x + s];
      sm[threadIdx.x] = sum ? a + b : fmax(a, b);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) res[k] = sm[0];
}

namespace {
template <typename E>
bool kkt_aligned(const E *p, int v) {
  return ((uintptr_t)p % ((uintptr_t)v * sizeof(E))) == 0;
}
}  // namespace

#define KKT_DISPATCH_BOOL(c, NAME, ...) \
  do {                                  \
    if (c) {                            \
      constexpr bool NAME = true;       \
      __VA_ARGS__;                      \
    } else {                            \
      constexpr bool NAME = false;      \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

template <typename T>
hipError_t launch_kkt(const Queue &q, int64_t n, const T *x, const T *l, const T *u, const int32_t *nbd, const T *g,
                      double tol, T *pg, T *mult, int8_t *status, double *part, double *res) {
  constexpr int VV = VecOf<T>::V;
  const bool vec = kkt_aligned(x, VV) && kkt_aligned(l, VV) && kkt_aligned(u, VV) && kkt_aligned(g, VV) &&
                   kkt_aligned(nbd, VV) && (!pg || kkt_aligned(pg, VV)) && (!mult || kkt_aligned(mult, VV)) &&
                   (!status || kkt_aligned(status, VV));
  int gr = 0;
  KKT_DISPATCH_BOOL(vec, VEC, KKT_DISPATCH_BOOL(pg != nullptr, PG, KKT_DISPATCH_BOOL(mult != nullptr, MU,
                    KKT_DISPATCH_BOOL(status != nullptr, ST, {
    constexpr int V = VEC ? VV : 1;
    gr = grid_for(n, V);
    hipLaunchKernelGGL((kkt_kernel<T, V, PG, MU, ST>), dim3(gr), dim3(BLOCK), 0, q.stream, n, x, l, u, nbd, g, tol,
                       pg, mult, status, part);
  }))));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kkt_finalize_kernel, dim3(KktSlots::size()), dim3(BLOCK), 0, q.stream, (const double *)part, gr,
                     KktSlots::nsum(), res);
  return hipGetLastError();
}

// ---- the ordered index list ----
// A workgroup takes one chunk of KKT_LIST_CHUNK rows, a wave KKT_LIST_STEPS runs of 64 consecutive rows of it: row
// chunk * CHUNK + (wave * STEPS + step) * 64 + lane.  One ballot per run gives the run's selected rows as a mask, whose
// population is the run's count and whose bits below a lane (mbcnt) are that lane's position inside the run.
__device__ __forceinline__ bool kkt_selected(int code, int mask) {  // bytes outside -1 .. 3 select nothing
  return code >= -1 && code <= 3 && ((mask >> (code + 1)) & 1) != 0;
}
// the masks of this wave's runs (wave-uniform); rows beyond n are read at n - 1 and select nothing, so that the
// loads of all runs are unconditional and in flight together
__device__ __forceinline__ void kkt_list_masks(int64_t n, const int8_t *__restrict__ status, int mask,
                                               int64_t wave_row0, uint64_t (&b)[KKT_LIST_STEPS]) {
  const int lane = threadIdx.x & 63;
  int code[KKT_LIST_STEPS];
#pragma unroll
  for (int s = 0; s < KKT_LIST_STEPS; ++s) {
    const int64_t i = wave_row0 + s * 64 + lane;
    code[s] = status[i < n ? i : n - 1];
  }
#pragma unroll
  for (int s = 0; s < KKT_LIST_STEPS; ++s) {
    const int64_t i = wave_row0 + s * 64 + lane;
    b[s] = __builtin_amdgcn_ballot_w64(i < n && kkt_selected(code[s], mask));
  }
}
__global__ __launch_bounds__(BLOCK) void kkt_list_count_kernel(int64_t n, const int8_t *__restrict__ status, int mask,
                                                               int64_t *__restrict__ tmp) {
  __shared__ int sw[BLOCK / 64];
  const int w = threadIdx.x >> 6;
  uint64_t b[KKT_LIST_STEPS];
  kkt_list_masks(n, status, mask, (int64_t)blockIdx.x * KKT_LIST_CHUNK + (int64_t)w * KKT_LIST_STEPS * 64, b);
  int c = 0;
#pragma unroll
  for (int s = 0; s < KKT_LIST_STEPS; ++s) c += __popcll(b[s]);
  if ((threadIdx.x & 63) == 0) sw[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int k = 0; k < BLOCK / 64; ++k) t += sw[k];
    tmp[blockIdx.x] = t;
  }
}
// exclusive scan of the chunk counts in place (a single workgroup: thread t takes a contiguous run of chunks, the
// runs' totals are scanned by one thread); the full count goes to tmp[nch]
__global__ __launch_bounds__(BLOCK) void kkt_list_scan_kernel(int64_t nch, int64_t *tmp) {
  __shared__ int64_t tot[BLOCK];
  const int64_t per = (nch + BLOCK - 1) / BLOCK;
  const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nch ? b0 + per : nch;
  int64_t c = 0;
  for (int64_t b = b0; b < b1; ++b) c += tmp[b];
  tot[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < BLOCK; ++t) {
      const int64_t v = tot[t];
      tot[t] = run;
      run += v;
    }
    tmp[nch] = run;
  }
  __syncthreads();
  int64_t run = tot[threadIdx.x];
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v = tmp[b];
    tmp[b] = run;
    run += v;
  }
}
__global__ __launch_bounds__(BLOCK) void kkt_list_write_kernel(int64_t n, int64_t row0,
                                                               const int8_t *__restrict__ status, int mask,
                                                               const int64_t *__restrict__ tmp,
                                                               int64_t *__restrict__ idx, int64_t cap) {
  __shared__ int sw[BLOCK / 64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t wr0 = (int64_t)blockIdx.x * KKT_LIST_CHUNK + (int64_t)w * KKT_LIST_STEPS * 64;
  uint64_t b[KKT_LIST_STEPS];
  kkt_list_masks(n, status, mask, wr0, b);
  int c = 0;
#pragma unroll
  for (int s = 0; s < KKT_LIST_STEPS; ++s) c += __popcll(b[s]);
  if (lane == 0) sw[w] = c;
  __syncthreads();
  int64_t pos = tmp[blockIdx.x];  // selected rows in front of this chunk ...
  for (int k = 0; k < w; ++k) pos += sw[k];  // ... of this wave ...
#pragma unroll
  for (int s = 0; s < KKT_LIST_STEPS; ++s) {
    const uint64_t m = b[s];
    // ... of this lane inside the run
    const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int64_t p = pos + before;
    if (((m >> lane) & 1ull) && p < cap) idx[p] = row0 + wr0 + s * 64 + lane;
    pos += __popcll(m);
  }
}

hipError_t launch_kkt_list(const Queue &q, int64_t n, int64_t row0, const int8_t *status, int code_mask, int64_t *idx,
                           int64_t cap, int64_t *tmp) {
  const int64_t nch = kkt_list_chunks(n);
  if (nch < 1 || nch > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kkt_list_count_kernel, dim3((unsigned)nch), dim3(BLOCK), 0, q.stream, n, status, code_mask, tmp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kkt_list_scan_kernel, dim3(1), dim3(BLOCK), 0, q.stream, nch, tmp);
  e = hipGetLastError();
  if (e != hipSuccess || !idx || cap <= 0) return e;
  hipLaunchKernelGGL(kkt_list_write_kernel, dim3((unsigned)nch), dim3(BLOCK), 0, q.stream, n, row0, status, code_mask,
                     (const int64_t *)tmp, idx, cap);
  return hipGetLastError();
}

#define KKT_INST(T)                                                                                              \
  template hipError_t launch_kkt<T>(const Queue &, int64_t, const T *, const T *, const T *, const int32_t *, \
                                    const T *, double, T *, T *, int8_t *, double *, double *);
KKT_INST(double)
KKT_INST(float)
#undef KKT_INST

}  // namespace lbk
