// solver_qn.inl -- member functions of Solver<T> (included inside the class body in solver.hip): the
// limited-memory curvature model B and its inverse H = B^-1 as device operators (lbfgsb_hip_qn_apply,
// lbfgsb_hip_qn_diag; k_qn.hip has the kernels, host_dense.hpp the 2col x 2col algebra).
//
// The entries read the pairs of the last return (or import) and nothing else of the iteration's state changes:
// W is read in the layout it is in (Wc(), never W()), the sums go through buffers of their own (never q.d_part /
// q.d_res, which may hold the sums of a deferred or speculative phase across a return), and the Queue's launch
// counters stay as they are.  Every later return of the run is bit-identical whether the entries were called or not.
  struct QnState {
    bool have = false;          // a return (save_locals) or an import has recorded the model below
    int col = 0, head = 1;      // the pairs of that return
    double theta = 1.0;
    bool theta_gram = false;    // after import_state: theta = y'y / s'y of the newest pair, from the Gram
    int iupdat = -1;            // (what identifies the pairs of a return: a new pair counts iupdat up,
    int64_t nref = -1;          //  a refresh counts nrefresh up)
    int64_t gen = 0;            // pair generation: bumped by everything that changes W or col / head
    int64_t gram_gen = -1;      // generation of the Gram below
    std::vector<double> sty, yty;  // S'Y, Y'Y over all rows (col x col, logical order)
    int64_t n_gen[2] = {-1, -1};   // generation of the packed N of each mode (device copy in d_n[mode])
    double *d_part = nullptr, *d_res = nullptr, *d_res_all = nullptr, *d_n[2] = {nullptr, nullptr};
    int all_ranks = 0;          // ranks d_res_all was sized for
    double *h_n = nullptr;      // pinned staging of a packed N
    std::vector<double> h_res, h_all;
  } qn;
  static constexpr int QN_RES = 2 * (LBFGSB_MAX_M + lbk::QN_TILE) * lbk::QN_KMAX;  // sums of one vector block
  static constexpr int QN_NP = 64 * 65 / 2;                                         // packed N at 32 pairs

  // save_locals: what the entries will read until the next return
  void qn_record(int col, int head, double theta, int iupdat) {
    if (!qn.have || iupdat != qn.iupdat || nrefresh != qn.nref || col != qn.col || head != qn.head) qn.gen++;
    qn.have = true, qn.col = col, qn.head = head, qn.theta = theta, qn.theta_gram = false;
    qn.iupdat = iupdat, qn.nref = nrefresh;
  }
  void qn_release() {
    auto F = [](double *&p) {
      if (p) (void)hipFree(p);
      p = nullptr;
    };
    F(qn.d_part), F(qn.d_res), F(qn.d_res_all), F(qn.d_n[0]), F(qn.d_n[1]);
    qn.all_ranks = 0;
    if (qn.h_n) (void)hipHostFree(qn.h_n);
    qn.h_n = nullptr;
  }
  int qn_alloc() {
    if (!qn.d_part) {
      HIPCHK(hipMalloc(&qn.d_part, (size_t)2 * lbk::QN_TILE * lbk::QN_KMAX * lbk::MAX_BLOCKS * sizeof(double)));
      HIPCHK(hipMalloc(&qn.d_res, (size_t)QN_RES * sizeof(double)));
      HIPCHK(hipMalloc(&qn.d_n[0], (size_t)QN_NP * sizeof(double)));
      HIPCHK(hipMalloc(&qn.d_n[1], (size_t)QN_NP * sizeof(double)));
      HIPCHK(hipHostMalloc(&qn.h_n, (size_t)QN_NP * sizeof(double), hipHostMallocDefault));
      qn.h_res.assign(QN_RES, 0.0);
    }
    // the gather space follows the communicator of THIS call (one may be attached after an earlier call)
    if (comm && qn.all_ranks != nranks) {
      if (qn.d_res_all) HIPCHK(hipFree(qn.d_res_all));
      qn.d_res_all = nullptr, qn.all_ranks = 0;
      HIPCHK(hipMalloc(&qn.d_res_all, (size_t)QN_RES * nranks * sizeof(double)));
      qn.all_ranks = nranks;
    }
    if (qn.h_all.size() < (size_t)QN_RES * nranks) qn.h_all.assign((size_t)QN_RES * nranks, 0.0);
    return 0;
  }
  int qn_ready() {
    if (!qn.have) return fail(LBFGSB_E_STATE, "qn: the context has no run (no return, no import_state)");
    if (defer_live)
      return fail(LBFGSB_E_STATE, "qn: the line-search set-up of this 'FG_LNSRCH' return is still deferred "
                                  "(LBFGSB_F_DEFER_LNSRCH): call at a NEW_X return");
    if (f_pending)
      return fail(LBFGSB_E_STATE, "qn: a built-in objective's value is still on the device: call after the "
                                  "next setulb call has collected it");
    if (pend.on) return fail(LBFGSB_E_STATE, "qn: a pair is accepted but not stored yet");
    HIPCHK(hipSetDevice(device));
    return qn_alloc();
  }
  // every rank's `cnt` sums of qn.d_res -> qn.h_res, added over the ranks in rank order (the communicator) or by
  // the host reducer: the same bits on every rank
  int qn_reduce(int cnt) {
    if (comm) {
      if (g_rccl.AllGather(qn.d_res, qn.d_res_all, (size_t)cnt, ncclDouble, comm, stream) != ncclSuccess)
        return fail(LBFGSB_E_COMM, "qn: ncclAllGather of the partial sums failed");
      HIPCHK(hipMemcpyAsync(qn.h_all.data(), qn.d_res_all, (size_t)cnt * nranks * sizeof(double),
                            hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int j = 0; j < cnt; ++j) {
        double v = qn.h_all[j];
        for (int rk = 1; rk < nranks; ++rk) v = v + qn.h_all[(size_t)rk * cnt + j];
        qn.h_res[j] = v;
      }
      return 0;
    }
    HIPCHK(hipMemcpyAsync(qn.h_res.data(), qn.d_res, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (nranks > 1) {
      if (!cb_ar) return fail(LBFGSB_E_COMM, "qn: multi-rank context without a reducer");
      if (cb_ar(cb_user, qn.h_res.data(), cnt, 0, 0) != 0) return fail(LBFGSB_E_COMM, "qn: host all-reduce failed");
    }
    return 0;
  }
  static int qn_launched(hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    return fail(LBFGSB_E_NOGPU, std::string("qn: launch of ") + what + " failed: " + hipGetErrorString(e));
  }
  // [S'v_k; Y'v_k] for kc <= QN_KMAX vectors -> out[k * 2 col + i] (i < col: S, else Y), all ranks reduced
  int qn_sums(const T *const *v, int kc, bool vslot, double *out) {
    const int col = qn.col;
    const lbk::WStore<T> w = Wc();
    struct Piece {
      int c0, mc, k0, k, off;
    };
    std::vector<Piece> pieces;
    int off = 0;
    for (int c0 = 0; c0 < col; c0 += lbk::QN_TILE) {
      const int mc = lbk::qn_mc(std::min(lbk::QN_TILE, col - c0));
      for (int k0 = 0; k0 < kc;) {  // blocks of 4 / 2 / 1 vectors the tile's kernels take
        int k = std::min(kc - k0, lbk::qn_kmax(mc));
        if (k == 3) k = 2;
        pieces.push_back(Piece{c0, mc, k0, k, off});
        off += 2 * mc * k;
        k0 += k;
      }
    }
    // (<= 2 (col + QN_TILE) kc <= QN_RES for every col <= LBFGSB_MAX_M; checked before anything is written)
    if (off > QN_RES) return fail(LBFGSB_E_STATE, "qn: more sums than the buffer holds");
    for (const Piece &p : pieces) {
      lbk::QnVecs<T> vv{};
      for (int kk = 0; kk < p.k; ++kk) vv.p[kk] = v[p.k0 + kk];
      CHK(qn_launched(lbk::launch_qn_wtv<T>(q, n, w, qn.head, col, p.c0, p.mc, p.k, vv, vslot, qn.d_part,
                                            qn.d_res + p.off),
                      "qn_wtv"));
    }
    CHK(qn_reduce(off));
    for (const Piece &p : pieces)
      for (int kk = 0; kk < p.k; ++kk)
        for (int j = 0; j < p.mc && p.c0 + j < col; ++j) {
          double *o = out + (size_t)(p.k0 + kk) * 2 * col;
          o[p.c0 + j] = qn.h_res[(size_t)p.off + kk * 2 * p.mc + j];
          o[col + p.c0 + j] = qn.h_res[(size_t)p.off + kk * 2 * p.mc + p.mc + j];
        }
    return 0;
  }
  // S'Y and Y'Y over all rows, once per pair generation (the vectors of the W'V pass are the columns of Y)
  int qn_gram() {
    if (qn.gram_gen == qn.gen) return 0;
    const int col = qn.col;
    qn.sty.assign((size_t)col * col, 0.0), qn.yty.assign((size_t)col * col, 0.0);
    std::vector<double> sums((size_t)2 * col * lbk::QN_KMAX);
    for (int k0 = 0; k0 < col; k0 += lbk::QN_KMAX) {
      const int kc = std::min(lbk::QN_KMAX, col - k0);
      const T *v[lbk::QN_KMAX];
      for (int kk = 0; kk < kc; ++kk) v[kk] = wy + (int64_t)((qn.head - 1 + k0 + kk) % m) * ld;
      CHK(qn_sums(v, kc, true, sums.data()));
      for (int kk = 0; kk < kc; ++kk)
        for (int i = 0; i < col; ++i) {
          qn.sty[i + (size_t)(k0 + kk) * col] = sums[(size_t)kk * 2 * col + i];
          qn.yty[i + (size_t)(k0 + kk) * col] = sums[(size_t)kk * 2 * col + col + i];
        }
    }
    qn.gram_gen = qn.gen;
    if (qn.theta_gram && col > 0)  // matupd's theta = y'y / s'y of the newest pair (:2318)
      qn.theta = qn.yty[(size_t)(col - 1) * (col + 1)] / sy[(size_t)(col - 1) * (m + 1)];
    return 0;
  }
  std::vector<double> qn_dg() const {
    std::vector<double> dg((size_t)qn.col);
    for (int i = 0; i < qn.col; ++i) dg[(size_t)i] = sy[(size_t)i * (m + 1)];
    return dg;
  }
  // (cs; cy) of one vector from (S'v; Y'v)
  int qn_coef(bool inv, const double *dg, const double *stv, const double *ytv, double *cs, double *cy) {
    const int col = qn.col;
    if (inv) {
      const int info = lbh::qn_coef_h(col, qn.theta, qn.sty.data(), qn.yty.data(), col, dg, stv, ytv, cs, cy);
      return info ? fail(LBFGSB_E_STATE, "qn: s'y <= 0 in a stored pair") : 0;
    }
    const int info = lbh::qn_coef_b(m, sy.data(), wt.data(), col, qn.theta, stv, ytv, cs, cy);
    return info ? fail(LBFGSB_E_STATE, "qn: the middle matrix is singular (wt)") : 0;
  }

  int qn_apply(int mode, int64_t k, const void *v_, int64_t ldv, void *out_, int64_t ldo) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    const int col = qn.col;
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const double alpha = inv ? 1.0 / qn.theta : qn.theta;
    const std::vector<double> dg = qn_dg();
    const lbk::WStore<T> w = Wc();
    const T *v = (const T *)v_;
    T *out = (T *)out_;
    std::vector<double> sums((size_t)2 * std::max(col, 1) * lbk::QN_KMAX), cf((size_t)2 * std::max(col, 1) * lbk::QN_KMAX);
    for (int64_t k0 = 0; k0 < k; k0 += lbk::QN_KMAX) {
      const int kc = (int)std::min<int64_t>(lbk::QN_KMAX, k - k0);
      const T *vp[lbk::QN_KMAX];
      for (int kk = 0; kk < kc; ++kk) vp[kk] = v + (k0 + kk) * ldv;
      if (col > 0) {
        CHK(qn_sums(vp, kc, false, sums.data()));
        for (int kk = 0; kk < kc; ++kk) {
          const double *sv = sums.data() + (size_t)kk * 2 * col;
          double *c = cf.data() + (size_t)kk * 2 * col;
          CHK(qn_coef(inv, dg.data(), sv, sv + col, c, c + col));
        }
      }
      // out = alpha v + [S, Y] (cs; cy), one launch per column tile and block of vectors (col = 0: alpha v)
      for (int c0 = 0; c0 < std::max(col, 1); c0 += lbk::QN_TILE) {
        const int mc = lbk::qn_mc(std::max(1, std::min(lbk::QN_TILE, col - c0)));
        for (int j0 = 0; j0 < kc;) {
          int kb = std::min(kc - j0, lbk::qn_kmax(mc));
          if (kb == 3) kb = 2;
          double coef[2 * lbk::QN_TILE * lbk::QN_KMAX] = {};
          lbk::QnVecs<T> src{};
          lbk::QnOuts<T> dst{};
          for (int kk = 0; kk < kb; ++kk) {
            const double *c = cf.data() + (size_t)(j0 + kk) * 2 * col;
            for (int j = 0; j < mc && c0 + j < col; ++j) {
              coef[(size_t)kk * 2 * mc + j] = c[c0 + j];
              coef[(size_t)kk * 2 * mc + mc + j] = c[col + c0 + j];
            }
            dst.p[kk] = out + (k0 + j0 + kk) * ldo;
            src.p[kk] = c0 == 0 ? vp[j0 + kk] : dst.p[kk];
          }
          CHK(qn_launched(lbk::launch_qn_expand<T>(q, n, w, qn.head, col, c0, mc, kb, coef, c0 == 0 ? alpha : 1.0,
                                                   src, dst),
                          "qn_expand"));
          j0 += kb;
        }
      }
    }
    return qn_finish();
  }

  int qn_diag(int mode, void *out_) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    const int col = qn.col;
    if (col > lbk::MAXM) return fail(LBFGSB_E_ARG, "qn_diag: more than 32 stored pairs");
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const double alpha = inv ? 1.0 / qn.theta : qn.theta;
    const int md = inv ? 1 : 0;
    if (qn.n_gen[md] != qn.gen || col == 0) {
      std::vector<double> nm((size_t)4 * col * col + 1);
      if (col > 0) {
        const std::vector<double> dg = qn_dg();
        const int info = lbh::qn_nmat(
            col, [&](const double *stv, const double *ytv, double *cs, double *cy) {
              return qn_coef(inv, dg.data(), stv, ytv, cs, cy);
            },
            nm.data());
        if (info) return info;
      }
      HIPCHK(hipStreamSynchronize(stream));  // (the staging buffer may still feed an earlier copy)
      lbh::qn_pack_n(col, lbk::maxc_for(std::max(col, 1)), nm.data(), qn.h_n);
      HIPCHK(hipMemcpyAsync(qn.d_n[md], qn.h_n, (size_t)QN_NP * sizeof(double), hipMemcpyHostToDevice, stream));
      qn.n_gen[md] = qn.gen;
    }
    CHK(qn_launched(lbk::launch_qn_diag<T>(q, n, Wc(), qn.head, col, qn.d_n[md], alpha, (T *)out_), "qn_diag"));
    return qn_finish();
  }
  int qn_finish() {
    if (!(flags & LBFGSB_F_NO_RETURN_SYNC)) {
      HIPCHK(hipStreamSynchronize(stream));
    }
    return 0;
  }
