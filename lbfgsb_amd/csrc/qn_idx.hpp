// qn_idx.hpp -- index lists of the curvature-model operators (lbfgsb_hip_qn_rows / qn_block / qn_cols and their
// shifted twins; solver_qn_idx.inl, k_qn_idx.hip): the check of a caller's list and the chunks
// in which a list goes through the gather buffer.  Host-only integer bookkeeping, no HIP and nothing of Solver:
// tests/qn_idx_shim.cpp walks it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lbk {

constexpr int QN_IDX_MAXK = 4096;    // the longest list of a call (LBFGSB_QN_IDX_MAXK)
constexpr int QN_IDX_BUF = 1 << 16;  // doubles of the gather buffer: what one launch of the gather may write

// the position of the first index outside 0 .. n_global - 1, or -1: every index is a row of the problem
inline int64_t qn_idx_bad(int64_t k, const int64_t *idx, int64_t n_global) {
  for (int64_t j = 0; j < k; ++j)
    if (idx[j] < 0 || idx[j] >= n_global) return j;
  return -1;
}

// One launch of the gather: the indices j0 .. j0 + kc - 1 of the list, kc ncol doubles of the buffer (ncol values per
// index: the 2 col entries of [S, Y], one more with the weight)
struct QnIdxChunk {
  int64_t j0;
  int kc;
};
// the indices per launch that a buffer of cap doubles holds (0: not even one)
inline int64_t qn_idx_chunk_rows(int64_t cap, int ncol) { return cap / std::max(ncol, 1); }
// the chunks of a list of k indices, in order; empty when the buffer does not hold one index
inline std::vector<QnIdxChunk> qn_idx_chunks(int64_t k, int ncol, int64_t cap) {
  std::vector<QnIdxChunk> ch;
  const int64_t per = qn_idx_chunk_rows(cap, ncol);
  if (per < 1) return ch;
  for (int64_t j0 = 0; j0 < k; j0 += per) ch.push_back(QnIdxChunk{j0, (int)std::min(per, k - j0)});
  return ch;
}

}  // namespace lbk
