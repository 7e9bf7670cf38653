// solver_qn_pairs.inl -- member functions of Solver<T> (included inside the class body in solver.hip, behind
// solver_qn_idx.inl): the stored pairs of the curvature model as device data (lbfgsb_hip_qn_pairs_get / _set / _push;
// k_qn_pairs.hip has the two copy kernels, host_dense.hpp the algebra -- qn_pairs_factor, qn_pairs_append --, DESIGN.md
// section 10i).
//
// get reads the pairs of the last return as every qn entry does: W in the layout it is in (Wc()), nothing of the
// iteration's state touched.  set ENDS whatever run the context holds and makes it the keeper of a model of the
// caller's own ("model mode"): the columns go to the ring slots 1 .. k in natural row order, the host matrices the
// operators read (sy, ss, wt) and their Gram cache come from one Gram pass over the loaded columns (qn_gram_by), and
// every operator of solver_qn.inl / solver_qn_idx.inl then works as after a return.  push appends one pair to such a
// model the way matupd does, from the 4 col + 3 sums of one W'V pass (the block (s, y) with its Gram carried: qn_plan's
// QnPushSums) -- no Gram pass over W afterwards.  A run never continues from a model: setulb refuses every task but
// START (model_refuses), START and import_state leave the mode.
  int model = 0;  // 0: a run, or nothing; 1: model mode; 2: a refused qn_pairs_set left neither a model nor a run

  // the one refusal of the run path: before anything else of a setulb call happens
  int model_refuses(const char *task) {
    if (lbh::str60_eq(task, "START")) {
      model = 0;
      return 0;
    }
    if (model == 1) return fail(LBFGSB_E_STATE, "setulb: the context holds a caller's model: START a new run");
    if (model == 2) return fail(LBFGSB_E_STATE, "setulb: a refused qn_pairs_set ended the run: START a new run");
    return 0;
  }

  int qn_pairs_get(int32_t cap, int32_t *h_col, double *h_theta, void *s_out, int64_t lds, void *y_out,
                   int64_t ldy) override {
    CHK(qn_ready());
    const int col = qn.col;
    if (col > 0 && qn.theta_gram) CHK(qn_gram());  // (after import_state: theta comes from the Gram)
    *h_col = col, *h_theta = qn.theta;
    if (cap == 0) return 0;
    if (cap < col) return fail(LBFGSB_E_ARG, "qn_pairs_get: cap < the stored pairs (*h_col)");
    const lbk::WStore<T> w = Wc();
    for (int c0 = 0; c0 < col; c0 += lbk::QN_TILE)
      CHK(qn_launched(lbk::launch_qn_pairs_get<T>(q, n, w, qn.head, col, c0, lbk::qn_mc(std::min(lbk::QN_TILE, col - c0)),
                                                  (T *)s_out, lds, (T *)y_out, ldy),
                      "qn_pairs_get"));
    return qn_finish();
  }

  // what import_state resets of a run, without its arrays: nothing deferred, speculative or pending survives
  void model_end_run() {
    cw_packed = false, cw_stale = 0, cw_hold = 0, cw_settled = 0;
    spec.valid = false, pend.on = 0, pend.impl = 0, d_impl = z_in_x = false, tbrk_valid = false, scan.ready = false;
    ls.deferred = false, defer_live = false, wl.pending = false;
    sfv.valid = false, sfv_hot = false, eager.valid = false, spec_live_len = 0;
    spcand.valid = false, snap_valid = false, z_valid = false, index_valid = false;
    if (f_pending) q.nheld = 0, f_pending = false;  // (the parked finalize of an objective value nobody will collect)
    t = t_own, r = r_own, entry_mode = 0, ub_mask = 0, nbd8_src = nullptr, iw_dirty = 1.0;
  }
  // the model is gone (a refused set, a push whose formt failed): no pair, theta as given
  void model_clear(double theta) {
    qn.gen++;
    qn.col = 0, qn.head = 1, qn.theta = theta, qn.theta_gram = false, qn.iupdat = -1, qn.nref = nrefresh;
    qn.sty.clear(), qn.yty.clear(), qn.sts.clear();
    qn.gram_gen = qn.sts_gen = qn.gen;
    live_head = 1, live_col = 0;
  }

  int qn_pairs_set(int32_t k, const void *s_in, int64_t lds, const void *y_in, int64_t ldy, double theta_in) override {
    HIPCHK(hipSetDevice(device));
    CHK(qn_alloc());
    model_end_run();
    model_clear(1.0);
    qn.have = false, model = 2;  // (until the model stands: a failure below leaves neither a model nor a run)
    lbk::launch_lmask_ones(q, n, lmask);  // (the loaded columns are in natural row order)
    if (k > 0)
      CHK(qn_launched(lbk::launch_qn_pairs_load<T>(q, n, Wraw(), 0, k, (const T *)s_in, lds, (const T *)y_in, ldy),
                      "qn_pairs_load"));
    qn.col = k, live_col = k;
    // S'S, S'Y and Y'Y over all rows: every loaded column through the W'V pass of the Gram
    std::vector<double> sts((size_t)k * k), sty((size_t)k * k), yty((size_t)k * k);
    CHK(qn_gram_cols(0, 2 * k, [&](int j, const double *sums) {
      if (j < k) {
        std::copy_n(sums, k, sts.data() + (size_t)j * k);
      } else {
        std::copy_n(sums, k, sty.data() + (size_t)(j - k) * k);
        std::copy_n(sums + k, k, yty.data() + (size_t)(j - k) * k);
      }
    }));
    double theta = 1.0;
    const int info =
        lbh::qn_pairs_factor(m, k, sts.data(), sty.data(), yty.data(), theta_in, sy.data(), ss.data(), wt.data(), &theta);
    if (info) {
      model_clear(1.0);
      if (info > 0)
        return fail(LBFGSB_E_ARG, "qn_pairs_set: s'y of pair " + std::to_string(info - 1) +
                                      " (0-based, oldest first) is not finite or not positive");
      if (info == -1) return fail(LBFGSB_E_ARG, "qn_pairs_set: theta = 0 (from the newest pair) needs k >= 1");
      return fail(LBFGSB_E_ARG, "qn_pairs_set: the pairs do not give a positive definite model (formt)");
    }
    qn.sty.swap(sty), qn.yty.swap(yty), qn.sts.swap(sts);
    qn.theta = theta;
    qn.have = true, model = 1;
    return 0;
  }

  int qn_pairs_push(const void *s_, const void *y_, double theta_in, int32_t *h_stored) override {
    if (model != 1)
      return fail(LBFGSB_E_STATE, "qn_pairs_push: the pairs of a run belong to the run (lbfgsb_hip_qn_pairs_set first)");
    CHK(qn_ready());
    const int col = qn.col;
    const T *vp[2] = {(const T *)s_, (const T *)y_};
    std::vector<double> w((size_t)4 * std::max(col, 1));
    double gr[lbk::QN_KMAX * lbk::QN_KMAX] = {};
    CHK(qn_sums(lbk::qn_plan(col, 2, QnCarry::Gram), vp, false, nullptr, w.data(), gr));
    const lbk::QnPushSums P{col, w.data(), gr};
    const double eps = sizeof(T) == 4 ? (double)std::numeric_limits<float>::epsilon()
                                      : std::numeric_limits<double>::epsilon();
    const double dr = P.sy();
    *h_stored = 0;
    if (!(std::isfinite(dr) && dr > eps * std::sqrt(P.ss() * P.yy()))) return 0;
    int c = col, h = qn.head, it = col > 0 ? (qn.head + col - 2) % m + 1 : 0;
    double theta = qn.theta;
    const int info = lbh::qn_pairs_append(m, c, h, it, sy.data(), ss.data(), wt.data(), theta, &P.w[0], &P.w[col],
                                          P.ss(), dr, P.yy(), theta_in);
    const int64_t ld1 = (n + 3) / 4 * 4;  // (one column each: any leading dimension that keeps 16-byte accesses)
    CHK(qn_launched(lbk::launch_qn_pairs_load<T>(q, n, Wraw(), it - 1, 1, vp[0], ld1, vp[1], ld1), "qn_pairs_load"));
    if (info) {  // (as the reference refreshes after a failed formt, :849-857: no pair, theta = 1)
      model_clear(1.0);
      *h_stored = -1;
      return qn_finish();
    }
    lbh::qn_gram_append(m, col, qn.sts, &P.w[0], &P.w[0], P.ss());
    lbh::qn_gram_append(m, col, qn.sty, &P.w[2 * col], &P.w[col], dr);
    lbh::qn_gram_append(m, col, qn.yty, &P.w[3 * col], &P.w[3 * col], P.yy());
    qn.gen++;
    qn.col = c, qn.head = h, qn.theta = theta;
    qn.gram_gen = qn.sts_gen = qn.gen;
    live_head = h, live_col = c;
    *h_stored = 1;
    return qn_finish();
  }
