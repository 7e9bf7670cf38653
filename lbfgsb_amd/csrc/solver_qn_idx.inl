// solver_qn_idx.inl -- member functions of Solver<T> (included inside the class body in solver.hip, behind
// solver_qn.inl): entries, sub-blocks and columns of the curvature model and of the model plus a diagonal at index
// lists (lbfgsb_hip_qn_rows / qn_block / qn_cols / qn_shift_block / qn_shift_cols; k_qn_idx.hip has the kernels,
// host_dense.hpp the algebra, qn_idx.hpp the check and the chunks of a list).
//
// A[ia, ib] = alpha [ia == ib] + R_a N R_b' depends on the rows R of [S, Y] at the indices alone: one gather of
// k 2col reals, no vector of length n.  The indices are global rows, given on the host and checked there before
// anything is launched; every rank passes the same list, contributes the rows it owns and zeros elsewhere, and the
// contributions are added as qn_reduce adds its sums -- one rank per row, so the stored value survives exactly.
// As in solver_qn.inl, W is read in the layout it is in (Wc()), the gather goes through buffers of its own and the
// Queue's counters stay as they are: the run does not notice the calls.
  struct QnIdx {
    int64_t *d_idx = nullptr, *h_idx = nullptr;  // the list of a call (QN_IDX_MAXK) and its pinned staging
    double *d_buf = nullptr;                     // the gather buffer (QN_IDX_BUF doubles)
    double *d_all = nullptr;                     // ... of every rank (the communicator's all-gather)
    int all_ranks = 0;                           // ranks d_all was sized for
    std::vector<double> h_buf, h_all;
    double *d_coef = nullptr, *h_coef = nullptr;  // the columns pass: the coefficients of all tiles, then k diagonal
    size_t coef_cap = 0;                          // terms; their pinned staging; doubles of each
  } qi;

  int qn_idx_alloc() {
    if (!qi.h_idx) {  // (the last of the three: a call that failed part-way starts over)
      HIPCHK(own.device(&qi.d_idx, (size_t)lbk::QN_IDX_MAXK * sizeof(int64_t)));
      HIPCHK(own.device(&qi.d_buf, (size_t)lbk::QN_IDX_BUF * sizeof(double)));
      qi.h_buf.assign((size_t)lbk::QN_IDX_BUF, 0.0);
      HIPCHK(own.pinned(&qi.h_idx, (size_t)lbk::QN_IDX_MAXK * sizeof(int64_t)));
    }
    if (comm && qi.all_ranks != nranks) {
      qi.all_ranks = 0;
      HIPCHK(own.device(&qi.d_all, (size_t)lbk::QN_IDX_BUF * nranks * sizeof(double)));
      qi.all_ranks = nranks;
    }
    if (comm && qi.h_all.size() < (size_t)lbk::QN_IDX_BUF * nranks) qi.h_all.assign((size_t)lbk::QN_IDX_BUF * nranks, 0.0);
    return 0;
  }
  // the list -> the device (the staging buffer may still feed an earlier copy: wait first, as qn_diag does)
  int qn_idx_stage(int64_t k, const int64_t *idx) {
    HIPCHK(hipStreamSynchronize(stream));
    std::copy_n(idx, k, qi.h_idx);
    HIPCHK(hipMemcpyAsync(qi.d_idx, qi.h_idx, (size_t)k * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    return 0;
  }
  int qn_idx_check(const char *who, int64_t k, const int64_t *idx) {
    if (lbk::qn_idx_bad(k, idx, nglob) >= 0)
      return fail(LBFGSB_E_ARG, std::string(who) + ": an index outside 0 .. n_global - 1");
    return 0;
  }
  // every rank's `cnt` values of qi.d_buf -> qi.h_buf, added over the ranks in rank order (qn_reduce's rule with the
  // gather's own buffers): the same bits on every rank
  int qn_idx_reduce(int cnt) {
    if (comm) {
      if (g_rccl.AllGather(qi.d_buf, qi.d_all, (size_t)cnt, ncclDouble, comm, stream) != ncclSuccess)
        return fail(LBFGSB_E_COMM, "qn: ncclAllGather of the gathered rows failed");
      HIPCHK(hipMemcpyAsync(qi.h_all.data(), qi.d_all, (size_t)cnt * nranks * sizeof(double), hipMemcpyDeviceToHost,
                            stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int j = 0; j < cnt; ++j) {
        double v = qi.h_all[j];
        for (int rk = 1; rk < nranks; ++rk) v = v + qi.h_all[(size_t)rk * cnt + j];
        qi.h_buf[j] = v;
      }
      return 0;
    }
    HIPCHK(hipMemcpyAsync(qi.h_buf.data(), qi.d_buf, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (nranks > 1) {
      if (!cb_ar) return fail(LBFGSB_E_COMM, "qn: multi-rank context without a reducer");
      if (cb_ar(cb_user, qi.h_buf.data(), cnt, 0, 0) != 0) return fail(LBFGSB_E_COMM, "qn: host all-reduce failed");
    }
    return 0;
  }
  // rows[j + c k] = entry idx_j of logical column c of [S, Y] (c < col: S, else Y) over all ranks, and with wgt the
  // weights at the indices -> wv[j].  The list is already on the device (qn_idx_stage); chunk by chunk through the
  // gather buffer, each chunk fetched (and waited for) before the next launch writes there.
  int qn_idx_gather(int64_t k, const double *wgt, double *rows, double *wv) {
    const int col = qn.col, ncol = 2 * col + (wgt ? 1 : 0);
    if (ncol == 0) return 0;
    const lbk::WStore<T> w = Wc();
    const std::vector<lbk::QnIdxChunk> chunks = lbk::qn_idx_chunks(k, ncol, lbk::QN_IDX_BUF);
    if (chunks.empty()) return fail(LBFGSB_E_STATE, "qn: the gather buffer does not hold one row");
    for (const lbk::QnIdxChunk &ch : chunks) {
      CHK(qn_launched(lbk::launch_qn_rows<T>(q, n, row0, w, qn.head, col, qi.d_idx + ch.j0, ch.kc, wgt, qi.d_buf),
                      "qn_rows"));
      CHK(qn_idx_reduce(ch.kc * ncol));
      for (int c = 0; c < 2 * col; ++c)
        std::copy_n(qi.h_buf.data() + (size_t)c * ch.kc, ch.kc, rows + ch.j0 + (size_t)c * k);
      if (wgt) std::copy_n(qi.h_buf.data() + (size_t)2 * col * ch.kc, ch.kc, wv + ch.j0);
    }
    return 0;
  }
  // N of the mode, 2col x 2col, as qn_diag forms it
  int qn_idx_nmat(bool inv, std::vector<double> &nm) {
    const int col = qn.col;
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    nm.assign((size_t)4 * col * col + 1, 0.0);
    if (col > 0) {
      const int info = lbh::qn_nmat(col, qn_coef_map(inv), nm.data());
      if (info) return info;
    }
    return 0;
  }

  int qn_rows(int64_t k, const int64_t *h_idx, double *h_rows, int64_t ldr) override {
    CHK(qn_idx_check("qn_rows", k, h_idx));
    CHK(qn_ready());
    CHK(qn_idx_alloc());
    const int col = qn.col;
    if (col == 0) return 0;
    std::vector<double> rows((size_t)k * 2 * col);
    CHK(qn_idx_stage(k, h_idx));
    CHK(qn_idx_gather(k, nullptr, rows.data(), nullptr));
    for (int c = 0; c < 2 * col; ++c) std::copy_n(rows.data() + (size_t)c * k, k, h_rows + c * ldr);
    return 0;
  }
  // the rows of one or two lists (h_ib == NULL: one), with the weights when wgt is given
  int qn_idx_lists(int64_t ka, const int64_t *h_ia, int64_t kb, const int64_t *h_ib, const double *wgt,
                   std::vector<double> &ra, std::vector<double> &wa, std::vector<double> &rb, std::vector<double> &wb) {
    const int d = 2 * qn.col;
    ra.assign((size_t)ka * d + 1, 0.0), wa.assign((size_t)ka, 0.0);
    CHK(qn_idx_stage(ka, h_ia));
    CHK(qn_idx_gather(ka, wgt, ra.data(), wa.data()));
    if (!h_ib) return 0;
    rb.assign((size_t)kb * d + 1, 0.0), wb.assign((size_t)kb, 0.0);
    CHK(qn_idx_stage(kb, h_ib));
    return qn_idx_gather(kb, wgt, rb.data(), wb.data());
  }
  int qn_block(int mode, int64_t ka, const int64_t *h_ia, int64_t kb, const int64_t *h_ib, double *h_a,
               int64_t lda) override {
    CHK(qn_idx_check("qn_block", ka, h_ia));
    if (h_ib) CHK(qn_idx_check("qn_block", kb, h_ib));
    CHK(qn_ready());
    CHK(qn_idx_alloc());
    const bool inv = mode == LBFGSB_QN_H;
    std::vector<double> nm, ra, wa, rb, wb;
    CHK(qn_idx_nmat(inv, nm));
    CHK(qn_idx_lists(ka, h_ia, kb, h_ib, nullptr, ra, wa, rb, wb));
    lbh::qn_entries(qn.col, qn_alpha(inv), nm.data(), ra.data(), (int)ka, h_ia, rb.data(), (int)kb, h_ib, !h_ib, h_a,
                    lda);
    return 0;
  }
  int qn_shift_block(int64_t ka, const int64_t *h_ia, int64_t kb, const int64_t *h_ib, double *h_a,
                     int64_t lda) override {
    CHK(qn_idx_check("qn_shift_block", ka, h_ia));
    if (h_ib) CHK(qn_idx_check("qn_shift_block", kb, h_ib));
    CHK(qn_ready());
    CHK(qn_shift_live());
    CHK(qn_idx_alloc());
    std::vector<double> ra, wa, rb, wb;
    CHK(qn_idx_lists(ka, h_ia, kb, h_ib, qsh.d_w[qsh.cur], ra, wa, rb, wb));
    if (lbh::qn_shift_entries(qn.col, qn.theta, qsh.kf.data(), ra.data(), wa.data(), (int)ka, h_ia, rb.data(),
                              wb.data(), (int)kb, h_ib, !h_ib, h_a, lda))
      return fail(LBFGSB_E_STATE, "qn_shift_block: a zero pivot in the factor of K");
    return 0;
  }
  // out_j = column idx_j of the mode (shift: of Sigma): the gather, c_j on the host, then one launch of the columns
  // pass per column tile for all k outputs (qn_plan.hpp, qn_basis_plan; with no pair one empty tile, which writes the
  // diagonal term alone)
  int qn_cols_by(bool shift, bool inv, int64_t k_, const int64_t *h_idx, void *out_, int64_t ldo) {
    const int col = qn.col, d = 2 * col, k = (int)k_;
    const double *wgt = shift ? qsh.d_w[qsh.cur] : nullptr;
    std::vector<double> nm, r((size_t)k * d + 1), wv((size_t)k, 0.0), cf((size_t)k * d + 1), dterm((size_t)k);
    if (!shift) CHK(qn_idx_nmat(inv, nm));
    CHK(qn_idx_stage(k, h_idx));
    CHK(qn_idx_gather(k, wgt, r.data(), wv.data()));
    if (!shift) lbh::qn_rows_times_n(col, nm.data(), r.data(), k, k, cf.data());
    else if (lbh::qn_shift_rows_coef(col, qn.theta, qsh.kf.data(), r.data(), wv.data(), k, k, cf.data()))
      return fail(LBFGSB_E_STATE, "qn_shift_cols: a zero pivot in the factor of K");
    for (int j = 0; j < k; ++j) dterm[(size_t)j] = shift ? wv[(size_t)j] : qn_alpha(inv);
    lbk::QnBasisPlan pl = lbk::qn_basis_plan(col, k);
    if (pl.tiles.empty()) pl.tiles.push_back(lbk::QnBasisTile{0, lbk::qn_mc(1), false, 0}), pl.total = 2 * lbk::qn_mc(1) * k;
    const size_t need = (size_t)pl.total + k;
    if (qi.coef_cap < need) {
      const size_t cap = (size_t)lbk::qn_basis_coefs(std::max(m, col)) + lbk::QN_BASIS_KMAX;
      if (cap < need) return fail(LBFGSB_E_STATE, "qn: more coefficients than the buffer holds");
      qi.coef_cap = 0;
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(own.device(&qi.d_coef, cap * sizeof(double)));
      HIPCHK(own.pinned(&qi.h_coef, cap * sizeof(double)));
      qi.coef_cap = cap;
    }
    HIPCHK(hipStreamSynchronize(stream));  // (the staging buffer may still feed an earlier copy)
    std::fill(qi.h_coef, qi.h_coef + pl.total, 0.0);
    if (col > 0) lbk::qn_basis_pack(pl, cf.data(), qi.h_coef);
    std::copy_n(dterm.data(), k, qi.h_coef + pl.total);
    HIPCHK(hipMemcpyAsync(qi.d_coef, qi.h_coef, need * sizeof(double), hipMemcpyHostToDevice, stream));
    const lbk::WStore<T> w = Wc();
    for (const lbk::QnBasisTile &t : pl.tiles)
      CHK(qn_launched(lbk::launch_qn_cols<T>(q, n, row0, w, qn.head, col, t.c0, t.mc, t.acc, qi.d_coef + t.off,
                                             qi.d_coef + pl.total, qi.d_idx, wgt, k, (T *)out_, ldo),
                      "qn_cols"));
    return qn_finish();
  }
  int qn_cols(int mode, int64_t k, const int64_t *h_idx, void *out, int64_t ldo) override {
    CHK(qn_idx_check("qn_cols", k, h_idx));
    CHK(qn_ready());
    CHK(qn_idx_alloc());
    return qn_cols_by(false, mode == LBFGSB_QN_H, k, h_idx, out, ldo);
  }
  int qn_shift_cols(int64_t k, const int64_t *h_idx, void *out, int64_t ldo) override {
    CHK(qn_idx_check("qn_shift_cols", k, h_idx));
    CHK(qn_ready());
    CHK(qn_shift_live());
    CHK(qn_idx_alloc());
    return qn_cols_by(true, false, k, h_idx, out, ldo);
  }
