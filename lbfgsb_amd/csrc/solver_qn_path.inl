// solver_qn_path.inl -- member functions of Solver<T> (included inside the class body in solver.hip, behind
// solver_qn_idx.inl): the curvature model along a path of shifts (lbfgsb_hip_qn_path_set / _logdet / _solve / _trust;
// k_qn_path.hip has the kernels, host_dense.hpp the algebra -- qn_path_factor / _eval / _secular --, DESIGN.md section
// 10j).
//
// With the diagonal "pins plus a scalar", w = 1 / (theta + mu) is one number, the weighted Gram of qn_shift_set is
// w G_F with G_F = [S, Y]_F'[S, Y]_F, and p = [S, Y]_F'v does not depend on mu.  qn_path_set makes the free bytes, the
// pinned count and G_F (the pairs' cached Gram when nothing is pinned); after it a shift costs the host a 2col x 2col
// factorisation and nothing on the device.  One read pass gives p and sum_F v^2 for a vector, one write pass per
// column tile stores the solutions of all requested shifts.
// As in solver_qn.inl, W is read in the layout it is in (Wc()), the sums go through qn.d_part / qn.d_res and the
// Queue's counters stay as they are: the run does not notice the calls.  The state is independent of qsh.
  struct QnPath {
    bool have = false;
    int64_t gen = -1;          // the pair generation the bytes and the Gram were made at
    int64_t pinned = 0;        // pinned rows, all ranks
    std::vector<double> gf;    // G_F, 2col x 2col, the S block first, symmetric
    std::vector<double> sts, syl;  // M^-1's blocks (qn_shift_minv)
    double ldm = 0.0;          // log |det M^-1|
    uint8_t *d_free = nullptr;  // one byte per row, 1 = free (natural order)
    int64_t free_cap = 0;       // rows d_free was sized for
    double *d_coef = nullptr, *h_coef = nullptr;  // the expansion's coefficients of all tiles, then k weights; staging
    // of one evaluation
    std::vector<double> kf, work;
  } qp;
  static constexpr int QN_PATH_COEFS =
      2 * (LBFGSB_QN_ROOT_MAXCOL + lbk::QN_TILE) * lbk::QN_PATH_MAXK + lbk::QN_PATH_MAXK;

  int qn_path_live() {
    if (!qp.have || qp.gen != qn.gen)
      return fail(LBFGSB_E_STATE, qp.have ? "qn_path: the pairs have changed since lbfgsb_hip_qn_path_set: call "
                                            "qn_path_set again"
                                          : "qn_path: no path is set: call qn_path_set again");
    return 0;
  }
  double qn_path_free() const { return (double)(nglob - qp.pinned); }

  int qn_path_set(const int8_t *status, int code_mask, int64_t *h_pinned) override {
    CHK(qn_ready());
    const int col = qn.col, d = 2 * col;
    if (col > LBFGSB_QN_ROOT_MAXCOL) return fail(LBFGSB_E_ARG, "qn_path_set: more than 64 stored pairs");
    if (col > 0 && qn.theta_gram) CHK(qn_gram());  // (theta of an imported state)
    qp.have = false;
    if (!qp.d_free || qp.free_cap < n) {
      qp.free_cap = 0;
      HIPCHK(own.device(&qp.d_free, (size_t)std::max<int64_t>(n, 1)));
      qp.free_cap = std::max<int64_t>(n, 1);
    }
    CHK(qn_launched(lbk::launch_qn_path_pin(q, n, status, code_mask, qp.d_free, qn.d_part, qn.d_res), "qn_path_pin"));
    CHK(qn_reduce(1));
    const int64_t pinned = (int64_t)qn.h_res[0];
    std::vector<double> gf((size_t)d * d + 1, 0.0), sts, syl, km((size_t)d * d + 1);
    double ldm = 0.0;
    if (col > 0) {
      CHK(qn_shift_minv(sts, syl));
      if (pinned == 0) {  // G_F = G: the pairs' cached Gram, no pass over W beyond the one that fills the cache
        CHK(qn_gram());
        for (int j = 0; j < col; ++j)
          for (int i = 0; i < col; ++i) {
            gf[i + (size_t)j * d] = sts[i + (size_t)j * col];
            gf[i + (size_t)(col + j) * d] = gf[(col + j) + (size_t)i * d] = qn.sty[i + (size_t)j * col];
            gf[(col + i) + (size_t)(col + j) * d] = qn.yty[i + (size_t)j * col];
          }
        qn_symmetrise(d, gf.data());
      } else if (pinned < nglob) {
        const uint8_t *fre = qp.d_free;
        CHK(qn_gram_by(0, d, [&](const QnPiece &p, QnVecs vv) {
          return qn_go_sums("qn_path_wtv", lbk::launch_qn_path_wtv<T>, p, vv, true, false, fre);
        }, [&](int j, const double *sums) { std::copy_n(sums, d, gf.data() + (size_t)j * d); }));
        qn_symmetrise(d, gf.data());
      }
      if (lbh::qn_shift_factor(col, qn.theta, syl.data(), col, sts.data(), col, nullptr, km.data(), &ldm))
        return fail(LBFGSB_E_STATE, "qn_path_set: the middle matrix is not factorisable (s'y <= 0 or S'S singular)");
    }
    qp.gf.swap(gf), qp.sts.swap(sts), qp.syl.swap(syl);
    qp.ldm = ldm, qp.pinned = pinned, qp.gen = qn.gen, qp.have = true;
    qp.kf.assign((size_t)d * d + 1, 0.0), qp.work.assign((size_t)d * d + 6 * (size_t)col + 1, 0.0);
    if (h_pinned) *h_pinned = pinned;
    return 0;
  }

  // the factor of K(mu) into qp.kf and log det (B_FF + mu I): 0, 1 (theta + mu <= 0 or mu not finite) or 2 (the
  // shifted model is not positive definite on the free rows)
  int qn_path_factor_at(double mu, double *w, double *logdet) {
    return lbh::qn_path_shift(qn.col, qn.theta, mu, qp.syl.data(), qp.sts.data(), qp.gf.data(), qn_path_free(), qp.ldm,
                              qp.kf.data(), w, logdet, qp.work.data());
  }
  int qn_path_logdet(int64_t k, const double *h_mu, double *h_logdet, int32_t *h_info) override {
    CHK(qn_ready());
    CHK(qn_path_live());
    for (int64_t j = 0; j < k; ++j) {
      double w = 0.0, ld = 0.0;
      const int info = qn_path_factor_at(h_mu[j], &w, &ld);
      h_info[j] = info;
      if (!info) h_logdet[j] = ld;
    }
    return 0;
  }

  // p = [S, Y]_F'v (2col, S part first) and vv = sum_F v^2 over all ranks: the read pass
  int qn_path_read(const T *v, double *p, double *vv) {
    const uint8_t *fre = qp.d_free;
    const T *vp[1] = {v};
    return qn_sums_by(lbk::qn_plan(qn.col, 1, QnCarry::Norms), p, vv, [&](const QnPiece &pc) {
      QnVecs x{};
      x.p[0] = vp[0];
      return qn_go_sums("qn_path_wtv", lbk::launch_qn_path_wtv<T>, pc, x, false, pc.carry == QnCarry::Norms, fre);
    });
  }
  // out_j = a_j 1_F o (v + [S, Y] c_j), j < k: cf[j * 2col ...] and a[j] go to the device, then one launch per column
  // tile (qn_basis_plan; with no pair one empty tile, which writes a_j v)
  int qn_path_write(const T *v, int k, const double *cf, const double *a, T *out, int64_t ldo) {
    const int col = qn.col;
    lbk::QnBasisPlan pl = lbk::qn_basis_plan(col, k);
    if (pl.tiles.empty()) pl.tiles.push_back(lbk::QnBasisTile{0, lbk::qn_mc(1), false, 0}), pl.total = 2 * lbk::qn_mc(1) * k;
    const size_t need = (size_t)pl.total + k;
    if (need > (size_t)QN_PATH_COEFS) return fail(LBFGSB_E_STATE, "qn_path: more coefficients than the buffer holds");
    if (!qp.h_coef) {
      HIPCHK(own.device(&qp.d_coef, (size_t)QN_PATH_COEFS * sizeof(double)));
      HIPCHK(own.pinned(&qp.h_coef, (size_t)QN_PATH_COEFS * sizeof(double)));
    }
    HIPCHK(hipStreamSynchronize(stream));  // (the staging buffer may still feed an earlier copy)
    std::fill(qp.h_coef, qp.h_coef + pl.total, 0.0);
    if (col > 0) lbk::qn_basis_pack(pl, cf, qp.h_coef);
    std::copy_n(a, k, qp.h_coef + pl.total);
    HIPCHK(hipMemcpyAsync(qp.d_coef, qp.h_coef, need * sizeof(double), hipMemcpyHostToDevice, stream));
    const lbk::WStore<T> w = Wc();
    for (const lbk::QnBasisTile &t : pl.tiles)
      CHK(qn_launched(lbk::launch_qn_path_expand<T>(q, n, w, qn.head, col, t.c0, t.mc, t.acc, qp.d_coef + t.off,
                                                    qp.d_coef + pl.total, v, qp.d_free, k, out, ldo),
                      "qn_path_expand"));
    return 0;
  }
  // one evaluation at mu from p and vv: c (2col), ||x||^2, v'x, x'(B_FF + mu I)^-1 x; the info of qn_path_factor_at
  int qn_path_eval_at(double mu, const double *p, double vv, double *c, double *w, double *norm2, double *vx,
                      double *xbx) {
    double ld = 0.0;
    const int info = qn_path_factor_at(mu, w, &ld);
    if (info) return info;
    if (qn.col == 0) {
      *norm2 = *w * *w * vv, *vx = *w * vv, *xbx = *w * *norm2;
      return 0;
    }
    return lbh::qn_path_eval(qn.col, qn.theta, qp.kf.data(), *w, p, vv, qp.gf.data(), c, norm2, vx, xbx,
                             qp.work.data())
               ? 2
               : 0;
  }

  int qn_path_solve(const void *v_, int64_t k_, const double *h_mu, void *out_, int64_t ldo, double *h_norm2,
                    double *h_vx) override {
    CHK(qn_ready());
    CHK(qn_path_live());
    const int col = qn.col, d = 2 * col, k = (int)k_;
    for (int j = 0; j < k; ++j) {  // every shift is judged before anything is launched
      double w = 0.0, ld = 0.0;
      const int info = qn_path_factor_at(h_mu[j], &w, &ld);
      if (info == 1)
        return fail(LBFGSB_E_ARG, "qn_path_solve: theta + mu <= 0 or mu not finite at j = " + std::to_string(j));
      if (info)
        return fail(LBFGSB_E_STATE, "qn_path_solve: the shifted model is not positive definite on the free rows at "
                                    "j = " + std::to_string(j));
    }
    std::vector<double> p((size_t)std::max(d, 1)), cf((size_t)std::max(d, 1) * k), a((size_t)k);
    std::vector<double> n2((size_t)k), vx((size_t)k);
    double vv = 0.0;
    CHK(qn_path_read((const T *)v_, p.data(), &vv));
    for (int j = 0; j < k; ++j) {
      double xbx = 0.0;
      if (qn_path_eval_at(h_mu[j], p.data(), vv, cf.data() + (size_t)j * d, &a[(size_t)j], &n2[(size_t)j],
                          &vx[(size_t)j], &xbx))
        return fail(LBFGSB_E_STATE, "qn_path_solve: a zero pivot in the factor of K at j = " + std::to_string(j));
    }
    if (out_) CHK(qn_path_write((const T *)v_, k, cf.data(), a.data(), (T *)out_, ldo));
    if (h_norm2) std::copy_n(n2.data(), k, h_norm2);
    if (h_vx) std::copy_n(vx.data(), k, h_vx);
    return qn_finish();
  }

  int qn_path_trust(const void *g_, double delta, double rtol, int max_it, void *step_, double *h_res,
                    int32_t *h_iters) override {
    CHK(qn_ready());
    CHK(qn_path_live());
    const int col = qn.col, d = 2 * col;
    if (rtol == 0.0) rtol = 1e-10;
    if (max_it == 0) max_it = 100;
    std::vector<double> p((size_t)std::max(d, 1)), c((size_t)std::max(d, 1));
    double vv = 0.0;
    CHK(qn_path_read((const T *)g_, p.data(), &vv));
    if (!(vv > 0.0) || qn_path_free() == 0.0) {  // g_F = 0 or nothing free: the zero step
      if (vv != vv) return fail(LBFGSB_E_ARG, "qn_path_trust: g holds a NaN on a free row");
      h_res[0] = h_res[1] = h_res[2] = h_res[3] = 0.0;
      *h_iters = 0;
      if (step_ && n > 0) HIPCHK(hipMemsetAsync(step_, 0, (size_t)n * sizeof(T), stream));
      return qn_finish();
    }
    double w = 0.0, mu = 0.0, n2 = 0.0, vx = 0.0, xbx = 0.0;
    int iters = 0;
    const int rc = lbh::qn_path_secular(
        delta, rtol, max_it,
        [&](double m, double *norm2, double *xb) { return qn_path_eval_at(m, p.data(), vv, c.data(), &w, norm2, &vx, xb); },
        &mu, &n2, &xbx, &iters);
    if (rc < 0) return fail(LBFGSB_E_STATE, "qn_path_trust: the model is not positive definite on the free rows");
    // (never a step outside the region: with no upper end of the bracket after max_it evaluations there is none)
    if (rc == 4)
      return fail(LBFGSB_E_STATE, "qn_path_trust: no shift with ||step|| <= delta within max_it = " +
                                      std::to_string(max_it) + " evaluations (the last at mu = " + std::to_string(mu) +
                                      "): nothing written");
    // (c, w and v'x of the accepted shift: the last evaluation may have been at another one)
    if (qn_path_eval_at(mu, p.data(), vv, c.data(), &w, &n2, &vx, &xbx))
      return fail(LBFGSB_E_STATE, "qn_path_trust: the shifted model is not positive definite on the free rows");
    const double a = -w;
    if (step_) CHK(qn_path_write((const T *)g_, 1, c.data(), &a, (T *)step_, n));
    *h_iters = iters;
    h_res[0] = mu, h_res[1] = std::sqrt(n2), h_res[2] = 0.5 * vx + 0.5 * mu * n2, h_res[3] = mu > 0.0 ? 1.0 : 0.0;
    return qn_finish();
  }
