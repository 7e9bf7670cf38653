// qn_plan_check.cpp -- the tiling plan of the curvature-model operators (lbfgsb_amd/csrc/qn_plan.hpp) against a naive
// restatement of its rule, for every col in 0 .. 70 and 1024, every block of 1 .. QN_KMAX vectors, the three carries
// and the expansion variant; and the split of a call's k = 1 .. 9 vectors or samples into blocks (qn_block_kc), from
// an even and from an odd first sample.  Built and run under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_qn_plan_cpu.py; every buffer a scatter or a pack touches is a heap block of exactly its size.
//
// The restatement does not use qn_mc / qn_kmax / qn_piece_k: it walks (column, vector) pairs and says in which slot
// each sum lies, from a table of the pieces a block of vectors splits into.
#include <cstdio>
#include <vector>

#include "../lbfgsb_amd/csrc/qn_plan.hpp"

using namespace lbk;

static int failures = 0;
static int g_col, g_kc, g_carry, g_expand;  // the case under test, for the report
#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    if (!(cond) && ++failures <= 20)                                                                  \
      std::printf("FAILED %s (line %d): col %d kc %d carry %d expand %d\n", #cond, __LINE__, g_col,   \
                  g_kc, g_carry, g_expand);                                                           \
  } while (0)

static const int MAX_M = 1024;  // LBFGSB_MAX_M
static const double SENTINEL = -7.0;

// the widths of the pieces of kc vectors: on a tile of 16 columns at most 2 per piece, else 4 / 2 / 1, 3 = 2 + 1
static const int SPLIT_NARROW[5][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {2, 1, 0}, {4, 0, 0}};
static const int SPLIT_WIDE[5][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {2, 1, 0}, {2, 2, 0}};

struct Naive {
  std::vector<int> out;  // slot of out[k * 2 col + i]
  int sq[4];             // slot of the squared norm of vector k (Norms), -1: none
  int gr[16];            // slot of gr[a + 4 b] (Gram), -1: none
  int total = 0, npieces = 0;
};

static Naive naive(int col, int kc, int carry, bool expand) {
  Naive nv;
  nv.out.assign((size_t)kc * 2 * col, -1);
  for (int k = 0; k < 4; ++k) nv.sq[k] = -1;
  for (int e = 0; e < 16; ++e) nv.gr[e] = -1;
  int ntiles = (col + 15) / 16;
  if (col == 0 && (carry != 0 || expand)) ntiles = 1;
  int base = 0;
  for (int t = 0; t < ntiles; ++t) {
    int ncols = col - 16 * t;
    if (ncols > 16) ncols = 16;
    const int cap = ncols <= 5 ? 5 : ncols <= 10 ? 10 : 16;
    const int *widths = cap == 16 ? SPLIT_WIDE[kc] : SPLIT_NARROW[kc];
    int first = 0;
    for (int pi = 0; pi < 3 && widths[pi] > 0; ++pi) {
      const int kw = widths[pi];
      for (int kk = 0; kk < kw; ++kk)
        for (int j = 0; j < ncols; ++j) {
          nv.out[(size_t)(first + kk) * 2 * col + 16 * t + j] = base + kk * 2 * cap + j;
          nv.out[(size_t)(first + kk) * 2 * col + col + 16 * t + j] = base + kk * 2 * cap + cap + j;
        }
      base += 2 * cap * kw;
      if (t == 0 && carry == 1)
        for (int kk = 0; kk < kw; ++kk) nv.sq[first + kk] = base++;
      if (t == 0 && carry == 2)
        for (int a = 0; a < kw; ++a)
          for (int b = a; b < kw; ++b) nv.gr[(first + a) + 4 * (first + b)] = base++;
      first += kw;
      nv.npieces++;
    }
  }
  nv.total = base;
  return nv;
}

static void check_one(int col, int kc, QnCarry carry, bool expand) {
  g_col = col, g_kc = kc, g_carry = (int)carry, g_expand = expand;
  const QnPlan pl = qn_plan(col, kc, carry, expand);
  const Naive nv = naive(col, kc, (int)carry, expand);
  CHECK(pl.col == col && pl.kc == kc);
  CHECK((int)pl.pieces.size() == nv.npieces);
  CHECK(pl.total == nv.total);
  CHECK(pl.total <= qn_res(MAX_M));

  // the pieces themselves: shapes a launch takes, offsets contiguous from 0, every (column, vector) once
  std::vector<int> cover((size_t)col * kc, 0);
  int off = 0;
  for (const QnPiece &p : pl.pieces) {
    CHECK(p.k == 1 || p.k == 2 || p.k == 4);
    CHECK(p.k <= qn_kmax(p.mc) && qn_block_ok(p.mc, p.k));
    CHECK(p.mc == 5 || p.mc == 10 || p.mc == 16);
    CHECK(p.c0 >= 0 && p.c0 % QN_TILE == 0 && p.c0 < (col > 0 ? col : 1));
    CHECK(p.mc >= (col - p.c0 < 16 ? col - p.c0 : 16));
    CHECK(p.k0 >= 0 && p.k0 + p.k <= kc);
    CHECK(p.off == off);
    CHECK(p.carry == (p.c0 == 0 ? carry : QnCarry::None));
    const int ncarried = p.carry == QnCarry::Norms ? p.k : p.carry == QnCarry::Gram ? p.k * (p.k + 1) / 2 : 0;
    CHECK(p.slots() == 2 * p.mc * p.k + ncarried);
    off += p.slots();
    for (int kk = 0; kk < p.k; ++kk)
      for (int j = 0; j < p.mc && p.c0 + j < col; ++j) cover[(size_t)(p.c0 + j) * kc + p.k0 + kk]++;
  }
  CHECK(off == pl.total);
  for (int c : cover) CHECK(c == 1);
  if (col == 0) {  // nothing to sum: no piece, or the pieces of one empty tile of the smallest capacity
    const bool tile = carry != QnCarry::None || expand;
    CHECK(pl.pieces.empty() == !tile);
    for (const QnPiece &p : pl.pieces) CHECK(p.c0 == 0 && p.mc == 5);
  }

  // the scatters: slot index + 0.5 arrives where the restatement says, nothing else is written
  std::vector<double> res((size_t)pl.total);
  for (int i = 0; i < pl.total; ++i) res[i] = i + 0.5;
  std::vector<double> out((size_t)kc * 2 * col, SENTINEL);
  qn_scatter_sums(pl, res.data(), out.data());
  for (size_t e = 0; e < out.size(); ++e) CHECK(nv.out[e] >= 0 && out[e] == nv.out[e] + 0.5);
  if (carry == QnCarry::None) {
    qn_scatter_carry(pl, res.data(), nullptr);  // (as the callers without a carry do)
  } else if (carry == QnCarry::Norms) {
    std::vector<double> sq((size_t)kc, SENTINEL);
    qn_scatter_carry(pl, res.data(), sq.data());
    for (int k = 0; k < kc; ++k) CHECK(nv.sq[k] >= 0 && sq[k] == nv.sq[k] + 0.5);
  } else {
    std::vector<double> gr((size_t)QN_KMAX * QN_KMAX, SENTINEL);
    qn_scatter_carry(pl, res.data(), gr.data());
    for (int e = 0; e < QN_KMAX * QN_KMAX; ++e) CHECK(gr[e] == (nv.gr[e] >= 0 ? nv.gr[e] + 0.5 : SENTINEL));
    for (int k = 0; k < kc; ++k) CHECK(nv.gr[k + QN_KMAX * k] >= 0);  // (the squared norms are among them)
  }

  // the pack: the inverse map of the W'V scatter, zeros in the columns >= col
  std::vector<double> cf((size_t)kc * 2 * col);
  for (size_t e = 0; e < cf.size(); ++e) cf[e] = 1.0 + (double)e;
  std::vector<int> used(cf.size(), 0);
  for (const QnPiece &p : pl.pieces) {
    std::vector<double> coef((size_t)2 * p.mc * p.k, SENTINEL);
    qn_pack_coef(p, col, cf.data(), coef.data());
    for (int kk = 0; kk < p.k; ++kk)
      for (int j = 0; j < p.mc; ++j) {
        const double s = coef[(size_t)kk * 2 * p.mc + j], y = coef[(size_t)kk * 2 * p.mc + p.mc + j];
        if (p.c0 + j < col) {
          const size_t es = (size_t)(p.k0 + kk) * 2 * col + p.c0 + j, ey = es + col;
          CHECK(s == cf[es] && y == cf[ey]);
          CHECK(nv.out[es] == p.off + kk * 2 * p.mc + j && nv.out[ey] == p.off + kk * 2 * p.mc + p.mc + j);
          used[es]++, used[ey]++;
        } else {
          CHECK(s == 0.0 && y == 0.0);
        }
      }
  }
  for (int u : used) CHECK(u == 1);
}

// The blocks of a call on k vectors (qn_block_kc) against the rule said naively: loaded vectors go four at a time, the
// rest last; samples from `first` go as an odd first sample alone, then four at a time from an even one, the rest last.
// Returns the number of blocks walked.
static int check_blocks(int k, int first, bool samples) {
  g_col = -1, g_kc = k, g_carry = first, g_expand = samples;  // (the report's fields, reused)
  std::vector<int> want;                                       // the widths, naively
  int left = k;
  if (samples && first % 2 != 0) want.push_back(1), left -= 1;
  for (; left >= 4; left -= 4) want.push_back(4);
  if (left > 0) want.push_back(left);
  size_t nb = 0;
  std::vector<int> seen((size_t)k, 0);
  for (int64_t k0 = 0; k0 < k; ++nb) {
    const int64_t s0 = samples ? first + k0 : 0;
    const int kc = qn_block_kc(k0, k, s0);
    CHECK(nb < want.size() && kc == want[nb < want.size() ? nb : 0]);
    CHECK(kc >= 1 && kc <= QN_KMAX && k0 + kc <= k);
    CHECK(kc == 1 || s0 % 2 == 0);  // (a block of more than one sample: whole pairs)
    if (kc < 1) break;
    for (int kk = 0; kk < kc && k0 + kk < k; ++kk) seen[(size_t)(k0 + kk)]++;
    k0 += kc;
  }
  CHECK(nb == want.size());
  for (int c : seen) CHECK(c == 1);
  return (int)nb;
}

int main() {
  static_assert(qn_mc(1) == 5 && qn_mc(5) == 5 && qn_mc(6) == 10 && qn_mc(10) == 10 && qn_mc(11) == 16, "capacities");
  static_assert(qn_res(MAX_M) == 2 * (MAX_M + 16) * 4 + 10, "the result buffer");
  int cases = 0;
  for (int ci = 0; ci <= 71; ++ci) {
    const int col = ci <= 70 ? ci : MAX_M;
    for (int kc = 1; kc <= QN_KMAX; ++kc) {
      for (QnCarry carry : {QnCarry::None, QnCarry::Norms, QnCarry::Gram}) check_one(col, kc, carry, false), ++cases;
      check_one(col, kc, QnCarry::None, true), ++cases;
    }
  }
  // the blocks of a call: k = 1 .. 9 loaded vectors, and k = 1 .. 9 samples from an even and from an odd first sample
  int blocks = 0;
  for (int k = 1; k <= 9; ++k) {
    blocks += check_blocks(k, 0, false);
    for (int first : {0, 6, 1, 7}) blocks += check_blocks(k, first, true);
  }
  std::printf("qn_plan_check: %d blocks of vectors walked\n", blocks);
  std::printf("qn_plan_check: %d cases, %d failed\n", cases, failures);
  return failures ? 1 : 0;
}
