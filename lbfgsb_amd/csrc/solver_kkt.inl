// solver_kkt.inl -- member functions of Solver<T> (included inside the class body in solver.hip): the active set, the
// bound multipliers and the projected gradient of the caller's arrays as device data (lbfgsb_hip_kkt,
// lbfgsb_hip_kkt_list; k_kkt.hip has the kernels, res_layout.hpp's KktSlots the summary's layout, DESIGN.md
// section 12).
//
// The entries read the CALLER's x, l, u, nbd, g (not the context's bound snapshot) and need no run: of the context
// they use the stream, the real kind, the communicator and row0.  The contract is qn_apply's (solver_qn.inl): partials,
// results and scan space are buffers of their own (never q.d_part / q.d_res, which may hold the sums of a deferred or
// speculative phase across a return), the Queue's launch counters stay as they are, and every later return of a run is
// bit-identical whether the entries were called or not.
  struct KktState {
    double *d_part = nullptr, *d_res = nullptr, *d_res_all = nullptr;
    int64_t *d_tmp = nullptr;   // the list's chunk counts and their total
    int all_ranks = 0;          // ranks d_res_all / h_all were sized for
    double *h_res = nullptr;    // pinned: this rank's summary, then (a communicator) every rank's, rank-major
    int64_t *h_count = nullptr;  // pinned: the list's full count
  } kk;
  static constexpr int KKT_RES = lbk::KktSlots::size();
  // (the header's indices are the layout's)
  static_assert(LBFGSB_KKT_NCNT == lbk::KktSlots::NCNT && LBFGSB_KKT_NVAL == lbk::KktSlots::NVAL &&
                    LBFGSB_KKT_N_UNBOUNDED == lbk::KktSlots::status(-1) &&
                    LBFGSB_KKT_N_FIXED == lbk::KktSlots::status(3) &&
                    LBFGSB_KKT_N_BINDING == lbk::KktSlots::binding() && LBFGSB_KKT_N_WEAK == lbk::KktSlots::weak() &&
                    LBFGSB_KKT_N_LEAVING == lbk::KktSlots::leaving() &&
                    LBFGSB_KKT_N_OUTSIDE == lbk::KktSlots::outside() &&
                    LBFGSB_KKT_PG_MAX == lbk::KktSlots::pg_max() - lbk::KktSlots::nsum() &&
                    LBFGSB_KKT_GFREE_MAX == lbk::KktSlots::gfree_max() - lbk::KktSlots::nsum(),
                "LBFGSB_KKT_* and KktSlots disagree");

  // the refusals of both entries (nothing has been touched when they return), then the buffers
  int kkt_ready(const char *who) {
    if (defer_live)
      return fail(LBFGSB_E_STATE, std::string(who) + ": the line-search set-up of this 'FG_LNSRCH' return is still "
                                                     "deferred (LBFGSB_F_DEFER_LNSRCH): call at a NEW_X return");
    if (f_pending)
      return fail(LBFGSB_E_STATE, std::string(who) + ": a built-in objective's value is still on the device: call "
                                                     "after the next setulb call has collected it");
    HIPCHK(hipSetDevice(device));
    if (!kk.h_count) {  // (the last of the four: a call that failed part-way starts over)
      HIPCHK(own.device(&kk.d_part, (size_t)KKT_RES * lbk::MAX_BLOCKS * sizeof(double)));
      HIPCHK(own.device(&kk.d_res, (size_t)KKT_RES * sizeof(double)));
      HIPCHK(own.device(&kk.d_tmp, (size_t)(lbk::kkt_list_chunks(n) + 1) * sizeof(int64_t)));
      HIPCHK(own.pinned(&kk.h_count, sizeof(int64_t)));
    }
    // the gather space follows the communicator of THIS call (one may be attached after an earlier call)
    const int want = comm ? nranks : 1;
    if (kk.all_ranks != want) {
      kk.all_ranks = 0;
      own.drop(&kk.d_res_all);
      if (comm) HIPCHK(own.device(&kk.d_res_all, (size_t)KKT_RES * nranks * sizeof(double)));
      HIPCHK(own.pinned(&kk.h_res, (size_t)KKT_RES * (want + 1) * sizeof(double)));
      kk.all_ranks = want;
    }
    return 0;
  }
  // every rank's summary -> kk.h_res[0 .. KKT_RES): the counts added and the maxima taken over the ranks in rank order
  // (the communicator) or by the host reducer -- the same bits on every rank.  Waits for the stream.
  int kkt_reduce() {
    constexpr int NS = lbk::KktSlots::nsum();
    if (comm) {
      if (g_rccl.AllGather(kk.d_res, kk.d_res_all, (size_t)KKT_RES, ncclDouble, comm, stream) != ncclSuccess)
        return fail(LBFGSB_E_COMM, "kkt: ncclAllGather of the summaries failed");
      double *all = kk.h_res + KKT_RES;
      HIPCHK(hipMemcpyAsync(all, kk.d_res_all, (size_t)KKT_RES * nranks * sizeof(double), hipMemcpyDeviceToHost,
                            stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int j = 0; j < KKT_RES; ++j) {
        double v = all[j];
        for (int rk = 1; rk < nranks; ++rk) {
          const double p = all[(size_t)rk * KKT_RES + j];
          v = j < NS ? v + p : std::fmax(v, p);
        }
        kk.h_res[j] = v;
      }
      return 0;
    }
    HIPCHK(hipMemcpyAsync(kk.h_res, kk.d_res, (size_t)KKT_RES * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (nranks > 1) {
      if (!cb_ar) return fail(LBFGSB_E_COMM, "kkt: multi-rank context without a reducer");
      if (cb_ar(cb_user, kk.h_res, NS, 0, lbk::KktSlots::NVAL) != 0)
        return fail(LBFGSB_E_COMM, "kkt: host all-reduce failed");
    }
    return 0;
  }

  int kkt(const void *x, const void *l, const void *u, const int32_t *nbd, const void *g, double tol, void *pg_out,
          void *mult_out, int8_t *status_out, int64_t *h_cnt, double *h_val) override {
    CHK(kkt_ready("kkt"));
    const hipError_t e = lbk::launch_kkt<T>(q, n, (const T *)x, (const T *)l, (const T *)u, nbd, (const T *)g, tol,
                                            (T *)pg_out, (T *)mult_out, status_out, kk.d_part, kk.d_res);
    if (e != hipSuccess)
      return fail(LBFGSB_E_NOGPU, std::string("kkt: launch of kkt_kernel failed: ") + hipGetErrorString(e));
    CHK(kkt_reduce());  // (the summary is host data: the stream has been waited for, the outputs are complete)
    constexpr lbk::KktSlots S{};
    for (int k = 0; k < LBFGSB_KKT_NCNT; ++k) h_cnt[k] = (int64_t)kk.h_res[S.cnt(k)];
    for (int k = 0; k < LBFGSB_KKT_NVAL; ++k) h_val[k] = kk.h_res[S.val(k)];
    return 0;
  }

  int kkt_list(const int8_t *status, int code_mask, int64_t *idx_out, int64_t cap, int64_t *h_count) override {
    CHK(kkt_ready("kkt_list"));
    const hipError_t e = lbk::launch_kkt_list(q, n, row0, status, code_mask, idx_out, cap, kk.d_tmp);
    if (e != hipSuccess)
      return fail(LBFGSB_E_NOGPU, std::string("kkt_list: launch failed: ") + hipGetErrorString(e));
    HIPCHK(hipMemcpyAsync(kk.h_count, kk.d_tmp + lbk::kkt_list_chunks(n), sizeof(int64_t), hipMemcpyDeviceToHost,
                          stream));
    HIPCHK(hipStreamSynchronize(stream));  // (the count is host data: idx_out is complete too)
    *h_count = *kk.h_count;
    return 0;
  }
