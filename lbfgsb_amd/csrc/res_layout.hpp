// res_layout.hpp -- the reduction-slot layouts kernels and host share.
// Every pass over the rows hands its sums, then its minima, then its maxima to the host as one flat run of doubles
// (block_reduce_store -> launch_finalize -> d_res -> Solver::fetch).  Which double is what is said HERE only: one
// struct per layout, built from the column capacity the kernel is unrolled to, whose methods are the slot names.
// Kernels index their accumulators with them (constants after unrolling), the host decodes with the same calls.
// In a kernel a count handed to block_reduce_store goes through a constexpr int (NSUM): as a call it is folded too
// late for the reduction's tail, which then compiles to other instructions than with the literal.
// Plain C++17 without HIP: tests/cpu_walk compiles the host code with g++.
#pragma once
#include <algorithm>
#include <cstddef>

namespace lbk {

constexpr int MAXM = 32;  // pairs the fused kernels are unrolled for; more: the split pass, solver_wide.inl
// compile-time column capacity the kernels are unrolled to for `col` pairs: the stride of the layouts
constexpr int maxc_for(int col) { return col <= 5 ? 5 : (col <= 10 ? 10 : (col <= 20 ? 20 : 32)); }
// ... of the update pass: beyond 32 columns, where it is split into sub-launches and merged, the next multiple of 32
constexpr int maxc_stride(int col) { return col <= MAXM ? maxc_for(col) : (col + 31) / 32 * 32; }

struct WtvSlots {  // W'v (wtv_kernel); mc = maxc_for(col)
  int mc;
  constexpr int wy(int j) const { return j; }       // Wy_j'v
  constexpr int ws(int j) const { return mc + j; }  // Ws_j'v
  constexpr int size() const { return ws(mc); }     // (all sums)
  // out[j] = Wy_j'v, out[col + j] = scale Ws_j'v: wa(1:2col) as the reference holds it
  void decode(const double *res, int col, double *out, double scale = 1.0) const {
    for (int j = 0; j < col; ++j) out[j] = res[wy(j)], out[col + j] = scale * res[ws(j)];
  }
};
// cmprlb + W'r (cmprlb_wtv_kernel): `groups()` vectors of mc sums -- W'r and, newrow, the new row/column of formk's
// WN1 (ref :1756-1793): k = 0 sum_free Wy_new Wy_j, 1 sum_act Ws_new Ws_j, 2 sum_act Ws_new Wy_j, 3 sum_free Ws_j Wy_new
struct CmprlbWtvSlots {  // mc = maxc_for(col)
  int mc;
  bool newrow;
  constexpr int group(int g, int j) const { return g * mc + j; }
  constexpr int groups() const { return newrow ? 6 : 2; }
  constexpr int wy(int j) const { return group(0, j); }  // Wy_j'r
  constexpr int ws(int j) const { return group(1, j); }  // Ws_j'r
  constexpr int nr(int k, int j) const { return group(2 + k, j); }
  constexpr int size() const { return group(groups(), 0); }
  constexpr WtvSlots wtv() const { return {mc}; }  // (groups 0 and 1)
};
struct UpdatePairsSlots {  // matupd's sums over the col - 1 older columns (update_pairs_kernel); mc = maxc_for(col - 1)
  int mc;
  constexpr int sy(int j) const { return j; }       // s'Wy_j
  constexpr int ss(int j) const { return mc + j; }  // Ws_j's
  constexpr int yy() const { return ss(mc); }       // y'y
  constexpr int size() const { return yy() + 1; }
};
struct CauchyScanSlots {  // cauchy's n-loop (cauchy_scan_kernel)
  int mc;
  static constexpr CauchyScanSlots of(int col) { return {col ? maxc_for(col) : 0}; }
  constexpr int p_wy(int j) const { return j; }       // Wy_j'd
  constexpr int p_ws(int j) const { return mc + j; }  // Ws_j'd
  constexpr int f1() const { return p_ws(mc); }
  constexpr int nbreak() const { return f1() + 1; }
  constexpr int nunb() const { return f1() + 2; }    // rows that move without a breakpoint
  constexpr int nunbnz() const { return f1() + 3; }  // ... of those with g != 0
  constexpr int nsum() const { return f1() + 4; }
  constexpr int bkmin() const { return nsum(); }  // the min slot (+inf if none)
  constexpr int size() const { return nsum() + 1; }
};
// The fused update pass (update_scan_kernel): matupd's sums, cauchy's n-loop with the new pair as column col - 1, the
// line search's sums at the trial point and, newrow, formk's new row/column with the PRE-walk free set: vectors k = 0
// sum_free y Wy_j, 1 sum_act s Ws_j, 2 sum_act s Wy_j, 3 sum_free Ws_j y; scalars y y (free), s s, s y (act), s y (free)
struct UpdScanSlots {  // mc = maxc_stride(col - 1)
  int mc;
  bool newrow;
  constexpr int sy(int j) const { return j; }               // s'Wy_j
  constexpr int ss(int j) const { return sy(mc) + j; }      // Ws_j's
  constexpr int yy() const { return ss(mc); }               // y'y
  constexpr int p_wy(int j) const { return yy() + 1 + j; }  // Wy_j'd
  constexpr int yd() const { return p_wy(mc); }             // new Wy column . d
  constexpr int p_ws(int j) const { return yd() + 1 + j; }  // Ws_j'd
  constexpr int sd() const { return p_ws(mc); }             // new Ws column . d
  constexpr int f1() const { return sd() + 1; }
  constexpr int nbreak() const { return sd() + 2; }
  constexpr int nunb() const { return sd() + 3; }
  constexpr int nunbnz() const { return sd() + 4; }
  constexpr int gd() const { return sd() + 5; }          // g'd, d unscaled
  constexpr int iw_changed() const { return sd() + 6; }  // rows whose iwhere changed
  constexpr int nr_vec(int k, int j) const { return iw_changed() + 1 + k * mc + j; }
  constexpr int nr_scalar(int k) const { return nr_vec(4, 0) + k; }
  constexpr int nsum() const { return newrow ? nr_scalar(4) : nr_vec(0, 0); }
  constexpr int bkmin() const { return nsum(); }       // the min slot
  constexpr int pgnorm() const { return nsum() + 1; }  // the max slot: |proj g|
  constexpr int size() const { return nsum() + 2; }
};
// the storing pass (subsm_update_kernel, the last tile of the m > 32 r pass): three sums and a minimum
enum SubsmSlot { SUBSM_IWORD = 0, SUBSM_DDP = 1, SUBSM_DTD = 2, SUBSM_STPMX = 3, SUBSM_NSUM = 3, SUBSM_SIZE = 4 };

// the active-set report (kkt_kernel, lbfgsb_hip_kkt): nine counts, then four maxima, in the order of the header's
// LBFGSB_KKT_* indices (cnt(k) is h_cnt[k], val(k) is h_val[k])
struct KktSlots {
  static constexpr int NCNT = 9, NVAL = 4;
  static constexpr int status(int code) { return code + 1; }  // rows of status -1 .. 3
  static constexpr int binding() { return 5; }
  static constexpr int weak() { return 6; }
  static constexpr int leaving() { return 7; }
  static constexpr int outside() { return 8; }
  static constexpr int cnt(int k) { return k; }
  static constexpr int nsum() { return NCNT; }
  static constexpr int pg_max() { return nsum() + 0; }     // max |proj g|: projgr's slot
  static constexpr int mult_max() { return nsum() + 1; }   // max |multiplier|
  static constexpr int out_max() { return nsum() + 2; }    // largest distance outside the box
  static constexpr int gfree_max() { return nsum() + 3; }  // max |g| over the rows of status -1 and 0
  static constexpr int val(int k) { return nsum() + k; }
  static constexpr int size() { return nsum() + NVAL; }
};

constexpr int RES_MAX = 8 * MAXM + 16;  // rows of the partial-sum matrix, doubles of d_res for one phase
static_assert(RES_MAX >= UpdScanSlots{MAXM, true}.size() && RES_MAX >= CmprlbWtvSlots{MAXM, true}.size(), "RES_MAX");
// update pass with formk's new-row sums at col - 1 > 20 (k_update.hip, "the split pass"): several launches of the
// MC <= 20 kernels over <= SPLIT_COLS columns each; their results land behind the merged layout in d_res
// (split_base), SPLIT_SLOTS doubles apart, and are merged into the one-launch layout
constexpr int SPLIT_SLOTS = 8 * 20 + 16, SPLIT_COLS = 16, SPLIT_MAXPARTS = 64;
static_assert(SPLIT_SLOTS >= UpdScanSlots{20, true}.size(), "SPLIT_SLOTS");
// m > 32, behind the longest merged layout: DEFER_PAD doubles on the deferred line-search sums (solver.hip,
// DEFER_OFF), SPLIT_PAD doubles on the parts
constexpr int DEFER_PAD = 9, SPLIT_PAD = DEFER_PAD + 8;
inline int split_base(int nold, int dst) {
  return std::max(RES_MAX + 16, dst + UpdScanSlots{maxc_stride(nold), true}.size() + SPLIT_PAD);
}
inline int split_parts(int nold, int cols = SPLIT_COLS) { return (nold + cols - 1) / cols; }
// d_res doubles a context with m pairs needs for a split update pass (parts of >= 5 columns)
inline size_t split_res_len(int m) {
  return m <= 5 ? 0 : (size_t)split_base(m, 1) + (size_t)split_parts(m, 5) * SPLIT_SLOTS + 8;
}

}  // namespace lbk
