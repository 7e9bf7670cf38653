// kernels.hpp -- launch interface of the gfx950 kernels (k_*.hip).
//
// Every function enqueues work on `q.stream` and returns immediately; results
// of reductions land in q.d_res (device) after the finalize kernel and are
// fetched by the solver (solver.hip) in one D2H copy per phase.  No function
// here synchronises, allocates or frees (graph-capturable, cdna guide G9).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qn_idx.hpp"      // QN_IDX_MAXK, QN_IDX_BUF: index lists of the curvature-model operators and their chunks
#include "qn_plan.hpp"     // QN_TILE, QN_KMAX, qn_mc, qn_kmax, QnCarry: the tiling of the curvature-model operators
#include "res_layout.hpp"  // the slot layouts of the results, MAXM, maxc_for, RES_MAX, the split pass's sizes

namespace lbk {

constexpr int BLOCK = 256;        // 4 wave64 per workgroup
constexpr int MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond that
constexpr int GRAM_BLOCKS = 1024;

// per-context launch options (lbfgsb_hip_set_option; nothing is read from the environment)
struct Tune {
  int wgrid = 0;    // workgroups of the passes over W: 0 = what is resident for the kernel launched
                    // (grid_for_w asks the runtime: 256 ... 768), > 0 = this many
  int pipe = -1;    // two trips in flight per wave: -1 / 1 default rule (pipe_on), 0 off
  int pair = 2;     // MC = 20 update pass with new-row sums: lane pairs share the per-column
                    // accumulators; 0 off, 1 one trip in flight, 2 two trips
  int split_from = 20;  // update pass with the new-row sums: split over the columns beyond this many old pairs ...
  int split_cols = 16;  // ... into parts of at most this many (experiment: 10 / 10 = two MC = 10 launches at m = 20)
  int gram_rows = 0;  // formk from scratch: 1 = the LDS-slab kernel instead of the quad kernel
  int pair_cw = 1;    // compact W, MC = 10 update pass with the new-row sums: lane pairs share the column accumulators
};

// one reduction waiting to be finalized: `nblocks` partials per slot in part[slot * pstride + block],
// results to d_res[off + slot] (nsum sums, then nmin minima, then nmax maxima)
struct FinJob {
  const double *part;
  int pstride, nblocks, off, nsum, nmin, nmax;
};

// launch queue + reduction scratch owned by the context
struct Queue {
  hipStream_t stream;
  double *d_part;   // [rows][MAX_BLOCKS] block partials (row = output slot)
  // two small partial-sum matrices (ALT_SLOTS slots) for kernels whose finalize is parked (k_misc.hip,
  // finalize): part_sel = 1 / 2 makes the next launch write there, hold_fin parks its job
  static constexpr int ALT_SLOTS = 8;
  double *d_part_alt[2] = {nullptr, nullptr};
  int part_sel = 0;
  bool hold_fin = false;
  FinJob held[2];
  int nheld = 0;
  double *part() const { return part_sel == 0 ? d_part : d_part_alt[part_sel - 1]; }
  // finalize as publisher (single-rank contexts): device views of the host mirror of d_res and of the
  // sequence word, the workgroup counter, the number of the last publishing launch
  bool fin_publish = false;
  double *hd_pub = nullptr;
  unsigned long long *hd_fin_flag = nullptr;
  unsigned int *d_fin_count = nullptr;
  unsigned long long fin_seq = 0;
  int64_t launches_at_fin = -1;  // q.launches right after the last publishing finalize launch
  double *d_res;    // [RES_MAX or gram size] finalized results, device
  double *d_gpart;  // gram partials [E][GRAM_BLOCKS]
  int64_t launches;
  int res_off = 0;  // finalize writes d_res[res_off + slot] (lets two phases share one fetch)
  // m > 32: the parts of a split update pass never start below this offset of d_res (behind the LONGEST merged
  // layout the context can have + the deferred line-search sums, whatever the current number of pairs)
  int split_base_min = 0;
  bool nt = false;  // nontemporal loads in the W-pass kernels (W much larger than the Infinity Cache)
  bool cw_dense = true;  // option "cw_dense": the layout's passes fetch a tile's run of a column by 16-byte loads
  int64_t n_dense_subsm = 0, n_dense_update = 0;  // launches of the two dense kernels (lbfgsb_hip_dense_launches)
  // option "cw_ub": under uniform_bounds_mask = 7 the steady-state dense update kernel reads l, u, nbd once per
  // workgroup
  bool cw_ub = true;
  int64_t n_ub_update = 0;  // launches of that form, counted in n_dense_update too (lbfgsb_hip_ub_launches)
  Tune tune{};
  // first kernel launch that failed since the last check (hipGetLastError right behind the launch,
  // so that the error is reported with the kernel's name and not at the next stream sync)
  const char *launch_err_where = nullptr;
  hipError_t launch_err = hipSuccess;
  void launched(const char *where) {
    launches++;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && launch_err == hipSuccess) launch_err = e, launch_err_where = where;
  }
};
#define LB_LAUNCHED(q) (q).launched(__func__)

// the circular correction-pair store: Ws, Wy column-major n x m, leading
// dimension ld (multiple of 32 rows).  head is 1-based like the reference.
template <typename T>
struct WStore {
  T *ws;
  T *wy;
  int64_t ld;
  int m;
  const T *zero;  // >= 64 bytes of zeros: what the unroll slots beyond the stored pairs read
  // Tile-local free-row layout ("compact W"): nullptr = every column holds its rows in
  // natural order.  Else one bit per row: inside each aligned tile of CW_TILE rows a column stores the rows whose
  // bit is set first (ascending: the order of the reference's Index(1:nfree), src/lbfgsb.f90:2044-2054), the others
  // behind them.  Only the kernels that take the layout into account may be handed a WStore with lmask set
  // (update_scan, subsm_update, the record gathers and formk's patch); the solver's W() hands out natural order.
  const uint64_t *lmask = nullptr;
};
constexpr int CW_TILE = 128;  // rows per layout tile = what one wave64 covers per trip with two rows per lane

// iwhere (cauchy's per-variable status, -3..3) is kept as one byte per row on the device; the
// reference's int32 layout exists only in export_state / import_state
using iw_t = int8_t;
// nbd as the hot passes read it: one byte per row, a private copy of the caller's int32 array
// (values 0..3; made by nbd_pack_kernel) -- 3 bytes per row less in each pass over W
using nb_t = int8_t;

// small coefficient vectors travel as kernel arguments (scalar loads)
struct Coef {
  double a[2 * MAXM];
};

// A pair that matupd has accepted but that is not stored in W yet (see "pending pair" in
// kernels_common.hpp): logical column col-1 is  y = T(g - r), s = T(stp * d)  until it is committed.
struct Pend {
  int on;      // 0: every column is in W
  double stp;  // step length of the accepted trial
  int impl;    // 1: d itself is not stored either -- the unit first trial step was accepted, so
               //    d = x - t (x the accepted point, t the previous iterate); the `pd` argument of
               //    the kernels then points at t and s = T(x - t)
};

int grid_for(int64_t n, int vec);
// the same for the passes over W: as many workgroups as are resident for `kernel` (1-3 per CU)
int grid_for_w(const Queue &q, int64_t n, int vec, const void *kernel = nullptr);

// ---- one-off (START) ----------------------------------------------------
// active (ref :965-1040): clip x, init iwhere.  res: [0]=#projected (sum),
// [1]=#(nbd!=0) (sum), [2]=#(nbd!=2) (sum), [3]=nbdd (sum)
template <typename T>
void launch_active(Queue &q, int64_t n, T *x, const T *l, const T *u, const int32_t *nbd,
                   iw_t *iwhere, int8_t *wasfree);
// errclb (ref :1601-1643): res max-slots: [0]=largest 1-based global index with invalid nbd
// (0 if none), [1]=largest index with l>u and nbd==2; [2], [3], [4] = 1 if some l_i / u_i / nbd_i
// differs from the first one of this rank's rows (uniform-bounds detection, see `ub` below).
template <typename T>
void launch_errclb(Queue &q, int64_t n, int64_t row0, const T *l, const T *u,
                   const int32_t *nbd);

// ---- projgr (ref :2594-2622): res max-slot [0] = sbgnrm -------------------
template <typename T>
void launch_projgr(Queue &q, int64_t n, const T *x, const T *l, const T *u,
                   const int32_t *nbd, const T *g);
// level-1 doors (k_misc.hip): out = a - b; v = alpha v; sum slot 0 = a'b
template <typename T>
void launch_vec_sub(Queue &q, int64_t n, const T *a, const T *b, T *out);
template <typename T>
void launch_vec_scale(Queue &q, int64_t n, double alpha, T *v);
template <typename T>
void launch_dot(Queue &q, int64_t n, const T *a, const T *b);

// ---- W'v (the WS/WY correction-pair matvec) -------------------------------
// res: WtvSlots{maxc_for(col)} (logical column order)
template <typename T>
void launch_wtv(Queue &q, int64_t n, WStore<T> w, int head, int col, const T *v);
template <typename T>
void launch_wtv_nofinalize(Queue &q, int64_t n, WStore<T> w, int head, int col, const T *v);

// ---- cauchy (ref :1157-1532) ----------------------------------------------
// scan (:1270-1330): updates iwhere, writes tbrk (breakpoint t_i > 0; +inf = moves
// without bound; -1 = does not move).  res: CauchyScanSlots::of(col)
template <typename T>
void launch_cauchy_scan(Queue &q, int64_t n, const T *x, const T *l, const T *u,
                        const int32_t *nbd, const T *g, iw_t *iwhere, T *tbrk,
                        WStore<T> w, int head, int col);
// candidates with (lo_t, lo_i) < (t, gidx) and t <= hi_t, appended (unordered)
// to keys/idx (capacity cap); *d_count receives the total number found.
template <typename T>
void launch_cauchy_window(Queue &q, int64_t n, int64_t row0, const T *tbrk, double lo_t,
                          int64_t lo_i, double hi_t, uint64_t *keys, uint32_t *idx,
                          uint32_t cap, uint32_t *d_count);
// keys for a full sort of the remaining breakpoints (non candidates -> UINT64_MAX)
template <typename T>
void launch_cauchy_allkeys(Queue &q, int64_t n, int64_t row0, const T *tbrk, double lo_t,
                           int64_t lo_i, uint64_t *keys, uint32_t *idx);
// stable LSD radix sort of (key, idx) pairs, count elements; temp storage query
// when d_temp == nullptr.  Uses both halves of the double buffers; the sorted
// result is left in keys_out/idx_out.
size_t sort_pairs_temp_bytes(size_t count);
void launch_sort_pairs(Queue &q, void *d_temp, size_t temp_bytes, const uint64_t *keys_in,
                       uint64_t *keys_out, const uint32_t *idx_in, uint32_t *idx_out,
                       size_t count);
// ascending order for a list of row numbers (freev's changed rows, <= 2^18): in place for short lists
// (one-workgroup bitonic network), through `scratch` otherwise; returns where the sorted list is
uint32_t *launch_sort_u32(Queue &q, void *d_temp, size_t temp_bytes, uint32_t *keys, uint32_t *scratch,
                          uint32_t count);
// several ranks: merge the all-gathered record chunks (nranks sorted runs, blocks of `stride` doubles:
// count, more, records[chunk][recl]) into ONE (t, global index)-ordered run on the device.
// out = { 4 doubles per rank: count, more, t and index of its last record | the merged records |
// one byte per merged record: the rank it came from }
void launch_merge_chunks(Queue &q, int nranks, uint32_t chunk, int recl, size_t stride, const double *all,
                         uint64_t *keys0, uint64_t *keys1, uint32_t *vals0, uint32_t *vals1, void *d_temp,
                         size_t temp_bytes, double *out);
// stable sort of the same pairs by idx (first pass of a (t, idx) lexicographic order)
void launch_sort_by_idx(Queue &q, void *d_temp, size_t temp_bytes, const uint32_t *idx_in,
                        uint32_t *idx_out, const uint64_t *keys_in, uint64_t *keys_out,
                        size_t count);
// records for `cnt` breakpoints listed in idx (local rows): rec[k*(2col+4)+..] =
// { t, global index, d_i (= -g_i), zibp (= bound - x_i), Wy(i,0..col), Ws(i,0..col) }
// (t comes from keys[k]: the sort key is the bit pattern of the breakpoint time)
template <typename T>
void launch_cauchy_gather(Queue &q, const uint32_t *idx, const uint64_t *keys, uint32_t cnt,
                          int64_t row0, const T *x, const T *l, const T *u, const T *g, WStore<T> w,
                          int head, int col, const T *pr, const T *pd, Pend pe, double *rec);
// one-sync fast path: msg = { *d_count, 0, records of the first min(*d_count, cap) candidates }
template <typename T>
void launch_cauchy_gather_dyn(Queue &q, const uint32_t *idx, const uint64_t *keys,
                              const uint32_t *d_count, uint32_t cap, int64_t row0, const T *x,
                              const T *l, const T *u, const T *g, WStore<T> w, int head, int col,
                              const T *pr, const T *pd, Pend pe, double *msg);
// the window compaction with the breakpoint times recomputed per row (no stored tbrk)
template <typename T>
void launch_cauchy_window_fly(Queue &q, int64_t n, int64_t row0, const T *x, const T *l, const T *u,
                              const nb_t *nbd, const T *g, const iw_t *iwhere, double lo_t,
                              int64_t lo_i, double hi_t, uint64_t *keys, uint32_t *idx, uint32_t cap,
                              uint32_t *d_count, int ub = 0);
// cauchy's iwhere update (:1284-1291) alone
template <typename T>
void launch_iwhere_update(Queue &q, int64_t n, const T *x, const T *l, const T *u,
                          const int32_t *nbd, const T *g, iw_t *iwhere);
// the Cauchy point as a vector from (x, g, l, u, iwhere-after-the-walk, tsum)
template <typename T>
void launch_xcp_fill(Queue &q, int64_t n, const T *x, const T *g, const T *l, const T *u,
                     const iw_t *iwhere, double tsum, T *dst);
// ---- parallel GCP search for col > 0 (LBFGSB_F_PARALLEL_GCP; see k_cauchy.hip) ----
size_t scan_temp_bytes(size_t count);
void launch_scan(Queue &q, void *d_temp, size_t temp_bytes, const double *in, double *out,
                 size_t count, int exclusive);
template <typename T>
void launch_pgcp_gather(Queue &q, const uint32_t *idx, const uint64_t *keys, int64_t nb, int64_t nbp,
                        const T *x, const T *l, const T *u, const T *g, WStore<T> w, int head, int col,
                        double theta, const T *pr, const T *pd, Pend pe, double *tt, double *dd,
                        double *a0, double *wb, double *uu, double *gi, int64_t row0);
void launch_pgcp_mergekeys(Queue &q, int nranks, int64_t nbp, int narr, const double *counts,
                           const double *G, uint64_t *keys, uint32_t *vals);
void launch_pgcp_permute(Queue &q, int64_t NB, int64_t NBp, int64_t nbp, int narr, const uint32_t *vals,
                         const double *G, double *out, const int *map);
size_t f2scan_temp_bytes(size_t count);
void launch_pgcp_f2(Queue &q, void *d_temp, size_t temp_bytes, int64_t nb, double f2_0, double cl,
                    const double *df2, double *maps, double *F2);
template <typename T>
void launch_gcp_rest_mass(Queue &q, int64_t n, const T *g, const T *tbrk, double tstar);
void launch_pgcp_last(Queue &q, int64_t nb, int64_t nbp, int col2, const double *uu, double *uu_last);
void launch_pgcp_dtp(Queue &q, int64_t nb, int64_t nbp, int col2, const double *tt, const double *pp,
                     double *qq);
void launch_pgcp_terms(Queue &q, int64_t nb, int64_t nbp, int col2, double theta, const double *mm,
                       const double *p0, const double *tt, const double *dd, const double *a0,
                       const double *wb, const double *pp, const double *sq, double *df2, double *a1);
void launch_pgcp_f1(Queue &q, int64_t nb, double f2_0, const double *tt, const double *sf2,
                    const double *a1, double *df1);
void launch_pgcp_find(Queue &q, int64_t nb, double f1_0, double f2_0, const double *tt,
                      const double *sf1, const double *sf2);  // res min-slot [0] = k* (or +inf)
void launch_pgcp_pick(Queue &q, int64_t ks, int64_t nb, int64_t nbp, int col2, double f1_0, double f2_0,
                      const double *tt, const double *sf1, const double *sf2, const double *pp,
                      const double *uu_last, const double *sq, const uint32_t *idx, const double *gi,
                      double *out);
// tbrk as a vector from (x, l, u, nbd, g, iwhere-after-the-scan, BEFORE the walk fixes rows)
template <typename T>
void launch_tbrk_fill(Queue &q, int64_t n, const T *x, const T *l, const T *u, const int32_t *nbd,
                      const T *g, const iw_t *iwhere, T *tbrk);
// finish (:1425-1433, :1515): fix every processed breakpoint variable at its bound,
// move the others by tsum*d.  processed = (t, gidx) <= (last_t, last_i).
// count != 0: res[0] = number of rows fixed (finalize launched).
template <typename T>
void launch_cauchy_finish(Queue &q, int64_t n, int64_t row0, const T *x, const T *l, const T *u,
                          const T *g, const T *tbrk, iw_t *iwhere, T *xcp, double tsum,
                          double last_t, int64_t last_i, int count = 0);

// rows fixed by a short walk (list entry = global row * 2 + upper?): iwhere = 1 / 2
void launch_cauchy_fix(Queue &q, const int64_t *list, int count, int64_t row0, int64_t n,
                       iw_t *iwhere);

// ---- freev (ref :1980-2059) -------------------------------------------------
// res sum-slots: [0]=nfree, [1]=nenter, [2]=nleave, [3]=rows whose status changed; updates wasfree.
// chg (optional): rows whose free/active status changed are appended (unordered) as
// row | 0x80000000 if it LEFT the free set ([3] may exceed chg_cap: the list is then truncated).
// cnt2: two zero-initialised position counters, parity = which one this launch uses (it zeroes the other)
// write = 0: counts and list only (speculative pass); launch_freev_apply then updates wasfree from the list
void launch_freev_count(Queue &q, int64_t n, const iw_t *iwhere, int8_t *wasfree,
                        uint32_t *chg, uint32_t chg_cap, uint32_t *cnt2, int parity, int write = 1);
void launch_freev_apply(Queue &q, const uint32_t *chg, const uint32_t *cnt_ptr, uint32_t cap, int8_t *wasfree);
// mirror of Index / Indx2 (1-based global numbers, reference ordering).  prev = wasfree
// BEFORE launch_freev_count of this iteration (copy kept by the solver).
void launch_freev_lists(Queue &q, int64_t n, const iw_t *iwhere, const int8_t *prevfree,
                        int do_enterleave, int32_t *index, int32_t *indx2, int32_t *scan_tmp);

// ---- formk inner products (ref :1756-1851, from scratch) --------------------
// res (in d_res, E = 2col^2+col entries):
//   [ (i*(i+1)/2 + j) ]             i>=j : sum_free Wy_i Wy_j
//   [ T + (i*(i+1)/2 + j) ]         i>=j : sum_act  Ws_i Ws_j       (T = col(col+1)/2)
//   [ 2T + i*col + j ]              all  : sum_{i>j ? act : free} Ws_i Wy_j
template <typename T>
void launch_formk_gram(Queue &q, int64_t n, WStore<T> w, int head, int col,
                       const iw_t *iwhere);

// cmprlb + the first matvec of subsm (W'r, :2742-2754) in one pass over W.
// res: CmprlbWtvSlots{maxc_for(col), newrow} -- W'r; with newrow also the new row/column of formk's WN1 for the
// pair in logical column col-1 (ref :1756-1793).  r itself is not stored: launch_subsm_update recomputes it.
// The Cauchy point is evaluated per row from (x, g, iwhere, tsum), see xcp_free in kernels_common.hpp.
template <typename T>
void launch_cmprlb_wtv(Queue &q, int64_t n, const T *x, const T *g, double tsum,
                       const iw_t *iwhere, WStore<T> w, int head, int col, double theta,
                       const Coef &a, int newrow, const T *pr, const T *pd, Pend pe);
// formk patches (ref :1801-1851): signed Gram over the listed rows (+ entered, - left the free
// set) for the first upcl logical columns; res layout as launch_formk_gram with col = upcl.
template <typename T>
void launch_formk_patch(Queue &q, const uint32_t *chg, uint32_t cnt, WStore<T> w, int head, int upcl);
// the same queued right behind freev's counting pass, the list's length still on the device (*cnt_ptr): lists of
// up to `cap` rows (<= small_sort_cap(), sorted by launch_sort_u32_small_dev first) are patched, longer ones
// are not; res = the 2 upcl^2 + upcl sums, then one more: 1.0 if the list was too long
template <typename T>
void launch_formk_patch_dev(Queue &q, const uint32_t *chg, const uint32_t *cnt_ptr, uint32_t cap, WStore<T> w,
                            int head, int upcl);
void launch_sort_u32_small_dev(Queue &q, uint32_t *keys, const uint32_t *cnt_ptr);
int small_sort_cap();

// ---- subsm (ref :2676-2885) --------------------------------------------------
// update (cmprlb's r recomputed, :2770-2816, :2824-2827) + the line-search set-up of mainlb
// :720-722 / lnsrlb :2196-2236 in one pass: zout = projected subspace point from the Cauchy
// point (evaluated per row from x, g, l, u, iwhere, tsum), dvec = zout - x, tvec = x, r = g.
// cf = the coefficients the preceding launch_cmprlb_wtv used (all zero, with tsum = 0, for the
// reference's unconstrained shortcut r = -g, cmprlb :1560-1563: the general formula then gives
// exactly -g); wv = K^-1 W'r.
// res (SubsmSlot): sums #bound hits (iword), dd_p (= g'(z-x)), dtd ; min = stpmx candidate.
// xout (= the caller's x, or nullptr): also store the first trial point of the
// line search, x = z, when its step length is known to be 1 (:2265).  pr: the vector a pending
// pair's y is formed from (r of the previous line search); rout / tvec: where r = g and t = x are
// stored -- nullptr with ping-pong iterate buffers, where they are a change of roles, not copies.
template <typename T>
void launch_subsm_update(Queue &q, int64_t n, double tsum, T *zout, const T *pr, T *rout, const T *l,
                         const T *u, const nb_t *nbd, const iw_t *iwhere, const T *xx, const T *gg,
                         WStore<T> w, int head, int col, double theta, const Coef &cf,
                         const Coef &wv, T *dvec, T *tvec, T *xout, int do_stpmx, Pend pe,
                         const T *pd, int ub = 0);
// the Newton direction of the free rows as a vector (0 elsewhere) -- backtracking branch only
template <typename T>
void launch_subsm_dir(Queue &q, int64_t n, const T *xcp, const iw_t *iwhere, const T *xx,
                      const T *gg, WStore<T> w, int head, int col, double theta, const Coef &cf,
                      const Coef &wv, T *ndir);
// backtrack (:2836-2863): res min-slot [0] = alpha; then argmin pass:
// res min-slot [0] = smallest global index attaining alpha (as double)
template <typename T>
void launch_subsm_alpha(Queue &q, int64_t n, const T *xp, const T *r, const T *l, const T *u,
                        const int32_t *nbd, const iw_t *iwhere);
template <typename T>
void launch_subsm_argalpha(Queue &q, int64_t n, int64_t row0, const T *xp, const T *r,
                           const T *l, const T *u, const int32_t *nbd, const iw_t *iwhere,
                           double alpha);
template <typename T>
void launch_subsm_backtrack(Queue &q, int64_t n, int64_t row0, T *z, const T *xp, T *r,
                            const T *l, const T *u, const iw_t *iwhere, double alpha,
                            int64_t ibd);

// ---- lnsrlb (ref :2174-2275) + mainlb d=z-x (:720-722) ------------------------
// begin: d = z - x, t = x, r = g.  res sum [0]=dtd, [1]=gd ; min [2]=stpmx candidate
template <typename T>
void launch_lnsrlb_begin(Queue &q, int64_t n, const T *z, const T *x, const T *g, const T *l,
                         const T *u, const int32_t *nbd, T *d, T *t, T *r, int do_stpmx);
// trial point (:2264-2270): x = z (stp == 1) or stp*d + t
template <typename T>
void launch_lnsrlb_step(Queue &q, int64_t n, T *x, const T *z, const T *d, const T *t,
                        double stp);
// after f,g evaluation: res sum [0] = g.d ; max [1] = |proj g|_inf (speculative projgr)
template <typename T>
void launch_lnsrlb_eval(Queue &q, int64_t n, const T *x, const T *l, const T *u,
                        const int32_t *nbd, const T *g, const T *d);

// ---- mainlb :812-824 + matupd (ref :2291-2346) --------------------------------
// y = g - r, s = stp*d stored into column itail (1-based physical);
// res: UpdatePairsSlots{maxc_for(col-1)} over the col-1 older columns (logical order from head)
template <typename T>
void launch_update_pairs(Queue &q, int64_t n, const T *g, const T *r, const T *d, double stp,
                         WStore<T> w, int head, int col, int itail);

// the two above fused (one pass over the old columns); res: UpdScanSlots{maxc_stride(col-1), newrow}
template <typename T>
void launch_update_scan(Queue &q, int64_t n, const T *x, const T *l, const T *u,
                        const nb_t *nbd, const T *g, const T *r, const T *d, int dimpl,
                        double stp, iw_t *iwhere, T *tbrk, WStore<T> w, int head, int col, int itail,
                        int store_pair, int store_iw, int newrow = 0, double cand_hi = -1.0,
                        uint64_t *ckeys = nullptr, uint32_t *cidx = nullptr, uint32_t ccap = 0,
                        uint32_t *ccount = nullptr, int ub = 0);
// ub (launch_update_scan, launch_subsm_update, launch_cauchy_window_fly): UNIFORM BOUNDS.  bit 0: every
// l_i is one value, bit 1: every u_i, bit 2: every nbd_i -- the corresponding pointer then is a
// 64-byte device buffer filled with that value, which every lane reads from its start (a cache hit
// instead of an HBM stream of 8 / 8 / 1 bytes per row).  Detected at START (errclb's pass).
// bit 3 (UB_DICT, with bits 0 and 1 set, bit 2 clear): FEW-VALUED bounds -- the l / u buffers hold tables of
// <= 8 values each and the nbd byte stream carries nbd | l-index << 2 | u-index << 5 (kernels_common.hpp).
// cand_hi >= 0: rows whose breakpoint t lies in [0, cand_hi] are appended (unordered) to
// ckeys / cidx (capacity ccap), *ccount = how many there are (zeroed by the launch)
// Can ONE call of launch_update_scan hand the candidates over for ALL of its n rows?  (What the host asks before it
// passes cand_hi >= 0: a list that misses rows is taken by the next walk for every breakpoint up to cand_hi.)  No
//   * with the new-row sums at col - 1 > 10: the pair-shared MC = 20 instantiation has no registers for the
//     hand-over, the split pass (col - 1 > Tune::split_from) runs its parts without it;
//   * on the free-row layout (`layout`: the WStore carries lmask) with the new-row sums at 6 <= col - 1 <= 10 under
//     Tune::pair_cw, when n >= CW_TILE is no multiple of CW_TILE: the pair-shared instantiation covers the whole
//     tiles, the rows behind them are a launch of their own on offset pointers, which appends nothing.
inline bool update_scan_hands_over(const Queue &q, int64_t n, int col, int newrow, bool layout) {
  const int nold = col - 1;
  if (newrow && (maxc_for(nold) > 10 || nold > q.tune.split_from)) return false;
  if (layout && newrow && nold > 5 && nold <= 10 && q.tune.pair_cw && n >= CW_TILE && n % CW_TILE != 0) return false;
  return true;
}
// Ws/Wy slot of logical column col-1 <- the pending pair (paths without a subspace pass)
void launch_nbd_pack(Queue &q, int64_t n, const int32_t *nbd, nb_t *out);
// Dictionary-coded bounds (ub bit 3 = UB_DICT, kernels_common.hpp): bound arrays with <= 8 distinct values each.
// The tables travel by value; entry j of l / u beyond nl / nu repeats entry 0.
constexpr int UB_DICT = 8;  // the dictionary bit of `ub`
struct BoundTables {
  double l[8], u[8];  // values of the context's real kind, widened exactly
  int nl, nu, nb0;    // entries in use; nb0: the value of a uniform nbd array
};
// res: sum [0] #l_i outside the table, [1] #u_i outside | min [2] smallest such l_i, [3] smallest such u_i
template <typename T>
void launch_dict_probe(Queue &q, int64_t n, const T *l, const T *u, const BoundTables &tb);
// out[i] = nbd_i | index of l_i << 2 | index of u_i << 5
template <typename T>
void launch_nbd_pack_dict(Queue &q, int64_t n, const int32_t *nbd, const T *l, const T *u, const BoundTables &tb,
                          nb_t *out);
// the caller's l, u, nbd against the snapshot the passes over W read (packed byte / constants / tables), bit for
// bit.  res: sum [0] = rows that differ
template <typename T>
void launch_bounds_verify(Queue &q, int64_t n, const T *l, const T *u, const int32_t *nbd, const nb_t *code,
                          int ub, const BoundTables &tb);
// LBFGSB_F_FOLLOW_BOUNDS (k_bounds.hip): the caller's l, u, nbd against the snapshot, with l_snap / u_snap
// standing in for the arrays the passes stream; force is added once to [0].
// res: sum [0] = rows that differ (+ force), [1] = rows with nbd outside 0..3
template <typename T>
void launch_bounds_follow(Queue &q, int64_t n, const T *l, const T *u, const int32_t *nbd, const T *l_snap,
                          const T *u_snap, const nb_t *code, int ub, const BoundTables &tb, int force);
// two copies of (l, u, nbd) against each other, bit for bit.  res: sum [0] = rows that differ
template <typename T>
void launch_bounds_same(Queue &q, int64_t n, const T *l0, const T *u0, const int32_t *nb0, const T *l1,
                        const T *u1, const int32_t *nb1);
// d = x - t, z = x: the vectors a lean subsm_update_kernel pass left implicit (Pend::impl)
template <typename T>
void launch_dz_materialise(Queue &q, int64_t n, const T *x, const T *t, T *d, T *z, T *xnew = nullptr,
                           double stp = 1.0);
template <typename T>
void launch_pair_commit(Queue &q, int64_t n, const T *g, const T *r, const T *d, Pend pe,
                        WStore<T> w, int head, int col);

// ---- tile-local free-row layout of W (k_layout.hip) ----
// Re-sort every live column (logical 0 .. col-1 from head) of Ws and Wy, tile by tile, from the layout `lmask`
// describes to the one where the rows with iwhere <= 0 come first (iwhere == nullptr: natural order, every bit
// set), and write the new bits.  Tiles whose bits do not change are skipped.  fp64 contexts only use it.
template <typename T>
void launch_w_relayout(Queue &q, int64_t n, const iw_t *iwhere, uint64_t *lmask, WStore<T> w, int head, int col);
// every bit of rows [0, n) set, the rest clear (natural order)
void launch_lmask_ones(Queue &q, int64_t n, uint64_t *lmask);

// ---- m > 32: unfused tile primitives (k_wide.hip) -------------------------------------------------
// out_i (+)= sum_j (Wy(i,j) a_j) / div + Ws(i,j) b_j over the tc <= 32 logical columns from `head`
// (a = cf.a[0..), b = cf.a[MAXM..)); masked: only rows with iwhere <= 0
template <typename T>
void launch_tile_axpy(Queue &q, int64_t n, WStore<T> w, int head, int tc, const Coef &cf, double div,
                      const iw_t *iwhere, int masked, T *out);
// The r pass of an m > 32 iteration (solver_wide.inl, wide_subspace): the same tiles, with what cmprlb and subsm do
// around them folded into the first and the last one.  first: the sum of a row starts from r0 = -theta (xcp - x) - g
// (cmprlb :1565-1574; plain: -g) on the free rows instead of from `out` -- the Cauchy point evaluated per row
// (xcp_row), neither xcp nor r0 exists as a vector.  last: the finished sum is the Newton direction; the projected
// step (:2780-2816), dd_p (:2824-2827), d = z - x, dtd, the stpmx ratios (:2196-2225) and the stores of
// subsm_update_kernel (trial x / z, d, t, r: any of them may be nullptr) follow in the same kernel.
// res (last only): SubsmSlot
template <typename T>
struct WideTail {
  const T *x, *g, *l, *u;
  const int32_t *nbd;
  double tsum, theta;
  int plain, do_stpmx;
  T *zout, *dvec, *tvec, *rout, *xout;
};
template <typename T>
void launch_tile_axpy_fused(Queue &q, int64_t n, WStore<T> w, int head, int tc, const Coef &cf, const iw_t *iwhere,
                            T *out, int first, int last, const WideTail<T> &wt);
// The same pass as ONE launch over all col <= WIDE_MAXC columns (the coefficients are a kernel argument): no partial
// sum of r goes through memory between tiles, and the pair matupd left pending is read from the vectors it was
// formed from and stored into its W slot here, as subsm_update_kernel does for m <= 32 (cwy / cws = that slot;
// pe.on == 0: every column is in W).  wt.l / wt.u / nbd8 with the uniform / dictionary-coded bounds of `ub`.
constexpr int WIDE_MAXC = 96;
struct CoefWide {
  double a[2 * WIDE_MAXC];  // a = [0, WIDE_MAXC), b = [WIDE_MAXC, ...)
};
template <typename T>
void launch_wide_r_pass(Queue &q, int64_t n, WStore<T> w, int head, int col, const CoefWide &cf, const iw_t *iwhere,
                        const nb_t *nbd8, int ub, const WideTail<T> &wt, Pend pe, const T *pr, const T *pd);
// out = src on the free (want_free) / active rows, 0 elsewhere
template <typename T>
void launch_masked_copy(Queue &q, int64_t n, const T *src, const iw_t *iwhere, int want_free, T *out);
template <typename T>
void launch_rows_gather(Queue &q, const uint32_t *chg, uint32_t cnt, WStore<T> w, int head, int upcl, double *out);
// cauchy's d as a vector from tbrk (moving rows: -g, others 0)
template <typename T>
void launch_cauchy_dvec(Queue &q, int64_t n, const T *g, const T *tbrk, T *out);
// cmprlb's r before the W terms (0 on the rows that are not free)
template <typename T>
void launch_cmprlb_init(Queue &q, int64_t n, const T *x, const T *g, const T *z, const iw_t *iwhere,
                        double theta, int plain, T *out);
// subsm's projected step from the Newton direction vector; res sum [0] = iword count, [1] = dd_p
template <typename T>
void launch_subsm_project(Queue &q, int64_t n, T *z, T *dir, const T *x, const T *g, const T *l, const T *u,
                          const int32_t *nbd, const iw_t *iwhere, double rtheta);

// ---- built-in objectives -------------------------------------------------------
// res sum [0] = f contribution of this rank
template <typename T>
void launch_obj_quadratic(Queue &q, int64_t n, int64_t row0, const T *x, T *g);
template <typename T>
void launch_obj_rosenbrock(Queue &q, int64_t n, int64_t row0, int64_t nglob, const T *x, T *g,
                           double xl, double xr);
template <typename T>
void launch_halo_pack(Queue &q, int64_t n, const T *x, double *out);
// res sum [0] = *d_val (this rank's part of an objective value the caller computed on the device)
void launch_scalar_partial(Queue &q, const double *d_val);

// finalize: partials -> d_res (nsum sums, then nmin mins, then nmax maxes); takes parked jobs along
void launch_finalize(Queue &q, int nblocks, int nsum, int nmin, int nmax);
void finalize_flush(Queue &q);  // launch the parked jobs alone (a fetch that no finalize precedes)
// publish: count doubles from src (device) to dst_host (device address of mapped host memory), then
// *flag_host = seq with release semantics at system scope -- what the host polls instead of waiting
// for the stream (solver.hip, fetch)
void launch_publish(Queue &q, const double *src, double *dst_host, int count, unsigned long long seq,
                    unsigned long long *flag_host);

// ---- the curvature model as a device operator (k_qn.hip, solver_qn.inl) ----
// (qn_plan.hpp: the tiles of at most QN_TILE pairs and blocks of K = 1, 2 or 4 vectors that one launch of the W'V and
//  expand passes takes, and where its sums land)
template <typename T>
struct QnVecs {  // the vectors of a block, each of n rows in natural order
  const T *p[QN_KMAX];
};
template <typename T>
struct QnOuts {
  T *p[QN_KMAX];
};
template <int MC, int K>
struct QnCoef {  // out_k = alpha src_k + S c[k][0..MC) + Y c[k][MC..2MC): <= 4 x 2 x 10 doubles of kernel arguments
  double c[K][2 * MC];
  double alpha;
};
// [S'd_k; Y'd_k] of the columns c0 .. c0 + mc - 1 (those >= col give zeros), d_k = v_k - center (center may be NULL:
// the vectors as they are): partials into part ([slot][MAX_BLOCKS]), then a fixed-order finalize into res[k * 2 mc + j]
// (j < mc: S, j >= mc: Y).  carry: behind them, in res[2 mc k ...], the k sums d_k'd_k (Norms: the first tile's launch
// of a quadratic form) or the k (k + 1) / 2 sums d_a'd_b, a <= b, row by row of the upper triangle (Gram: that of a
// Gram matrix).  vslot: the vectors are columns of W (row i read at its slot in the layout; no center, nothing
// carried).  w.lmask may be set: the layout is read as it is.  The kernel: qn_wtv_kernel with no center and nothing
// carried, qn_wtg_kernel for a Gram of k >= 2 vectors, else qn_wtd_kernel (the Gram of one vector is its norm).
template <typename T>
hipError_t launch_qn_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                         QnVecs<T> v, bool vslot, const T *center, QnCarry carry, double *part, double *res);
// res[ia * kb + ib] = (a_ia - center)'(b_ib - center), ka, kb in {1, 2, 4} (center may be NULL): the entries of D'D
// across two blocks of vectors, from the vectors alone
template <typename T>
hipError_t launch_qn_dtd(const Queue &q, int64_t n, QnVecs<T> a, int ka, QnVecs<T> b, int kb, const T *center,
                         double *part, double *res);
// res[k] = the sum of slot k's nblocks partials, k < nslots, in a fixed order: how launch_qn_wtv / wtz / dtd end, with
// the grid of the pass they launched (0: the dispatch found no kernel) and after asking for its launch error
hipError_t launch_qn_finalize(const Queue &q, const double *part, int nblocks, int nslots, double *res);
// out_k = alpha src_k + [S, Y](:, tile) coef[k * 2 mc ...] (src_k may be out_k: the second and later tiles)
template <typename T>
hipError_t launch_qn_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                            const double *coef, double alpha, QnVecs<T> src, QnOuts<T> out);
// out_i = alpha + r_i' N r_i (col <= 32; np: packed upper triangle of the maxc_for(col)-padded N, off-diagonal doubled)
template <typename T>
hipError_t launch_qn_diag(const Queue &q, int64_t n, WStore<T> w, int head, int col, const double *np, double alpha,
                          T *out);

// The model plus a diagonal (k_qn_shift.hip, lbfgsb_hip_qn_shift_*): the row-weighted twins of the passes above.  The
// weights wgt (n doubles in both real kinds, natural row order) are w_i = 1 / (shift + d_i), 0 on a pinned row.
// wgt[i] = 1 / (shift + d[i]) (d may be NULL: all zero; d[i] = +inf pins the row: 0); res[0] = the sum of
// log(shift + d[i]) over the free rows, res[1] = the pinned rows, res[2] = the rows with shift + d[i] <= 0 or NaN
constexpr int QN_SHIFT_SUMS = 3;
template <typename T>
hipError_t launch_qn_shift_w(const Queue &q, int64_t n, const T *d, double shift, double *wgt, double *part,
                             double *res);
// launch_qn_wtv's plain pass on wgt o v_k (vslot: the vectors are columns of W, the weights still natural); root: on
// sqrt(wgt) o v_k (not with vslot)
template <typename T>
hipError_t launch_qn_shift_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               QnVecs<T> v, bool vslot, bool root, const double *wgt, double *part, double *res);
// first: out_k = wgt o (src_k + [S, Y](:, tile) coef[k * 2 mc ...]); else out_k = src_k + wgt o ([S, Y] coef) (src_k
// is out_k: the second and later tiles).  Rows with wgt = 0 of a first tile are +0 whatever src holds there.  root: a
// first tile writes sqrt(wgt) o src_k + wgt o ([S, Y] coef)
template <typename T>
hipError_t launch_qn_shift_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                                  const double *coef, QnVecs<T> src, const double *wgt, bool first, bool root,
                                  QnOuts<T> out);
// out_i = wgt_i + wgt_i^2 r_i' N r_i (col <= 32; np as launch_qn_diag takes it)
template <typename T>
hipError_t launch_qn_shift_diag(const Queue &q, int64_t n, WStore<T> w, int head, int col, const double *np,
                                const double *wgt, T *out);
// Draws and densities of the model plus a diagonal (k_qn_shift_draw.hip): launch_qn_wtz / _draw / _wtv's centred pass
// with the weights.  wtz: the sums of sqrt(wgt) o z_k; zz: k more, z_k'z_k over the rows with wgt != 0
template <typename T>
hipError_t launch_qn_shift_wtz(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               uint64_t seed, int64_t row0, int64_t s0, bool zz, const double *wgt, double *part,
                               double *res);
// first: out_k = mean + alpha sqrt(wgt) o z_k + wgt o ([S, Y](:, tile) coef[k * 2 mc ...]) (mean may be NULL), the
// mean itself (+0 without one) where wgt = 0; else out_k += wgt o ([S, Y] coef)
template <typename T>
hipError_t launch_qn_shift_draw(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                                const double *coef, double alpha, uint64_t seed, int64_t row0, int64_t s0,
                                bool first, const T *mean, const double *wgt, QnOuts<T> out);
// the sums of f o (v_k - center), f = (wgt != 0) (center may be NULL); dd: k more in res[2 mc k + kk], the sums of
// (v_k - center)^2 / wgt over the rows with wgt != 0
template <typename T>
hipError_t launch_qn_shift_wtd(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                               QnVecs<T> v, const T *center, bool dd, const double *wgt, double *part, double *res);

// The basis pass (k_qn_eig.hip): out_j (+)= [S, Y](:, tile) coef[j * 2 mc ...] for ALL j < k <= QN_BASIS_KMAX in one
// launch, output j at out + j * ldo; the tile's columns are read once per row.  acc: add to what out holds (the tiles
// after the first).  coef: DEVICE memory, 2 mc k doubles as qn_basis_pack lays them out, read through uniform (scalar)
// loads.
template <typename T>
hipError_t launch_qn_basis(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, bool acc,
                           const double *coef, int k, T *out, int64_t ldo);

// Entries at index lists (k_qn_idx.hip, lbfgsb_hip_qn_rows / qn_block / qn_cols and the shifted twins).
// The gather: out[j + c kc] = entry idx[j] of logical column c of [S, Y] (c < col: S, else Y), widened to double, and
// with wgt != NULL one more column out[j + 2 col kc] = wgt[idx[j] - row0]; 0.0 for a row outside row0 .. row0 + n - 1.
// idx: DEVICE memory, kc global rows that the host has checked; kc (2 col [+ 1]) <= QN_IDX_BUF doubles of out, a buffer
// of the caller's own.  w.lmask may be set: the layout is read as it is.
template <typename T>
hipError_t launch_qn_rows(const Queue &q, int64_t n, int64_t row0, WStore<T> w, int head, int col,
                          const int64_t *idx, int kc, const double *wgt, double *out);
// launch_qn_basis with the row weight and the diagonal term fused: out_j[i] (+)= f_i ([S, Y](i, tile) coef[j * 2 mc
// ...]) for all j < k, f_i = wgt[i] (wgt == NULL: 1; a row with wgt = 0 stores +0), and the first tile (acc = false)
// adds dterm[j] on the row idx[j] - row0 where this rank owns it.  coef, dterm, idx: DEVICE memory.
template <typename T>
hipError_t launch_qn_cols(const Queue &q, int64_t n, int64_t row0, WStore<T> w, int head, int col, int c0, int mc,
                          bool acc, const double *coef, const double *dterm, const int64_t *idx, const double *wgt,
                          int k, T *out, int64_t ldo);

// The model along a path of shifts (k_qn_path.hip, lbfgsb_hip_qn_path_*): one byte per row (1 = free) in place of the
// weights of the passes above, the shifts being scalars of the host.
constexpr int QN_PATH_MAXK = 64;  // LBFGSB_QN_PATH_MAXK
// fre[i] = 0 where bit (status[i] + 1) of code_mask is set (status == NULL: every row free); res[0] = the pinned rows
hipError_t launch_qn_path_pin(const Queue &q, int64_t n, const int8_t *status, int code_mask, uint8_t *fre,
                              double *part, double *res);
// launch_qn_wtv's plain pass on fre o v: k = 1 vector in natural order, with dd its squared norm over the free rows in
// res[2 mc]; or vslot, k = 1, 2, 4 columns of W read at their slots (the masked Gram)
template <typename T>
hipError_t launch_qn_path_wtv(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                              QnVecs<T> v, bool vslot, bool dd, const uint8_t *fre, double *part, double *res);
// out_j[i] (+)= fre_i ? a[j] (acc ? 0 : v_i) + a[j] ([S, Y](i, tile) coef[j * 2 mc ...]) : +0 for all j < k <=
// QN_PATH_MAXK in one launch; coef (qn_basis_pack's layout) and a: DEVICE memory, read through uniform loads
template <typename T>
hipError_t launch_qn_path_expand(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, bool acc,
                                 const double *coef, const double *a, const T *v, const uint8_t *fre, int k, T *out,
                                 int64_t ldo);

// Draws of the model (k_qn_draw.hip): the two passes above with the vectors generated, never loaded -- z_k[i] is the
// N(0, 1) deviate of (seed, row0 + i, s0 + k) (philox.hpp).  k = 1, 2 or 4 (qn_kmax) samples from s0; s0 even
// unless k = 1.
// [S'z_k; Y'z_k] of the tile's columns, as launch_qn_wtv lays them out; zz: k more sums z_k'z_k in res[2 mc k + kk],
// the other sums bit for bit what zz = false gives
template <typename T>
hipError_t launch_qn_wtz(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                         uint64_t seed, int64_t row0, int64_t s0, bool zz, double *part, double *res);
// first: out_k = mean + alpha z_k + [S, Y](:, tile) coef[k * 2 mc ...] (mean may be NULL); else out_k += [S, Y] coef
template <typename T>
hipError_t launch_qn_draw(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, int k,
                          const double *coef, double alpha, uint64_t seed, int64_t row0, int64_t s0, bool first,
                          const T *mean, QnOuts<T> out);

// The stored pairs out of W and into it (k_qn_pairs.hip, lbfgsb_hip_qn_pairs_get / _set / _push).
// The pairs c0 .. min(c0 + mc, col) - 1 (logical order, oldest first) -> s_out + c lds, y_out + c ldy, n rows each in
// natural row order; lds, ldy >= n.  w.lmask may be set: the layout is read as it is.
template <typename T>
hipError_t launch_qn_pairs_get(const Queue &q, int64_t n, WStore<T> w, int head, int col, int c0, int mc, T *s_out,
                               int64_t lds, T *y_out, int64_t ldy);
// The caller's columns s_in + j lds, y_in + j ldy, j < k <= m, -> the physical columns (slot0 + j) % m of W (natural
// order: w.lmask must be NULL, the layout mask all ones), by 16-byte accesses where the caller's side is aligned for
// them.
template <typename T>
hipError_t launch_qn_pairs_load(const Queue &q, int64_t n, WStore<T> w, int slot0, int k, const T *s_in, int64_t lds,
                                const T *y_in, int64_t ldy);

// ---- the active-set report (k_kkt.hip, solver_kkt.inl) ----
// One pass over the caller's x, l, u, nbd, g: per row the status (iwhere codes), the signed projected gradient and the
// bound multiplier into whichever of status / pg / mult is not NULL, and the KktSlots sums and maxima: partials into
// part ([slot][MAX_BLOCKS]), then a fixed-order finalize into res[0 .. KktSlots::size()).  Buffers of the caller's
// own; the Queue is read for its stream only.
template <typename T>
hipError_t launch_kkt(const Queue &q, int64_t n, const T *x, const T *l, const T *u, const int32_t *nbd, const T *g,
                      double tol, T *pg, T *mult, int8_t *status, double *part, double *res);
// The rows whose status byte is selected by code_mask (bit code + 1, codes -1 .. 3), ascending, as row0 + i into
// idx[0 .. min(count, cap)): count per chunk of KKT_LIST_CHUNK rows, scan of the chunk totals, write.  tmp holds
// kkt_list_chunks(n) + 1 counts; tmp[kkt_list_chunks(n)] is the full count afterwards.  idx == nullptr or cap == 0:
// the count alone.
constexpr int KKT_LIST_STEPS = 16;                          // rows per lane
constexpr int KKT_LIST_CHUNK = BLOCK * KKT_LIST_STEPS;      // rows per workgroup
inline int64_t kkt_list_chunks(int64_t n) { return (n + KKT_LIST_CHUNK - 1) / KKT_LIST_CHUNK; }
hipError_t launch_kkt_list(const Queue &q, int64_t n, int64_t row0, const int8_t *status, int code_mask, int64_t *idx,
                           int64_t cap, int64_t *tmp);

}  // namespace lbk
