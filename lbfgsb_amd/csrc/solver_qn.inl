// solver_qn.inl -- member functions of Solver<T> (included inside the class body in solver.hip): the
// limited-memory curvature model B and its inverse H = B^-1 as device operators (lbfgsb_hip_qn_apply,
// lbfgsb_hip_qn_diag; k_qn.hip has the kernels, host_dense.hpp the 2col x 2col algebra), their
// symmetric square roots, log-determinants and draws (lbfgsb_hip_qn_logdet, lbfgsb_hip_qn_draw; k_qn_draw.hip), and
// quadratic forms and Gaussian log-densities (lbfgsb_hip_qn_quad, qn_logpdf, qn_draw_logpdf),
// and Gram matrices on blocks of vectors (lbfgsb_hip_qn_gram; section 10d), and solves, log-determinants and diagonals
// of the model plus a diagonal (lbfgsb_hip_qn_shift_*; k_qn_shift.hip, section 10f), and its square roots, draws and
// log-densities (lbfgsb_hip_qn_shift_sqrt / _draw / _quad / _logpdf; k_qn_shift_draw.hip, section 10g).
// Which launches a pass over W is made of and where their sums land is decided in one place, qn_plan.hpp (host-only,
// walked on the CPU by tests/qn_plan_check.cpp): every W'V pass here goes through qn_sums_by on a plan, every
// expansion through qn_expand_by, and the loops around them exist once: qn_blocks_by (the two passes of an operator,
// block by block: apply, solve, the roots and the draws), qn_gram_by (the columns of W as the vectors: the three
// Grams), qn_quad_sums (the quadratic forms) and qn_upload_n (the packed N of the diagonals).  A new operator hooks in
// with its launches and its coefficient map.
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
    int64_t sts_gen = -1;          // generation of S'S below (qn_gram_ss: REAL32 contexts, the spectrum only)
    std::vector<double> sts;       // S'S over all rows from the stored pairs
    int64_t n_gen[2] = {-1, -1};   // generation of the packed N of each mode (device copy in d_n[mode])
    int64_t root_gen[2] = {-1, -1};  // generation of the root of each mode below (qn_root_coef)
    std::vector<double> root_c[2];   // C of A^(1/2) = sqrt(alpha) I + [S, Y] C [S, Y]' (2col x 2col, column-major)
    double root_logsum[2] = {0.0, 0.0};  // sum_i log1p(delta_i / alpha): log det A - n log alpha
    int64_t eig_gen[2] = {-1, -1};   // generation of the spectrum of each mode below (qn_eig_coef)
    int eig_r[2] = {0, 0};           // directions off the bulk eigenvalue alpha
    std::vector<double> eig_lam[2];  // their eigenvalues alpha + delta_i, ascending
    std::vector<double> eig_c[2];    // their coefficient columns in the [S, Y] basis (2col x r, column-major)
    bool basis = true;               // option "qn_basis": qn_eigvec by the basis pass (0: by qn_expand, 4 at a time)
    std::vector<int64_t> coef_key;   // what d_coef holds: (generation, mode, k, the indices); empty: nothing
    double *d_coef = nullptr, *h_coef = nullptr;  // the basis pass's coefficients and their pinned staging
    double *d_part = nullptr, *d_res = nullptr, *d_res_all = nullptr, *d_n[2] = {nullptr, nullptr};
    int all_ranks = 0;          // ranks d_res_all was sized for
    double *h_n = nullptr;      // pinned staging of a packed N
    std::vector<double> h_res, h_all;
  } qn;
  static constexpr int QN_RES = lbk::qn_res(LBFGSB_MAX_M);                          // the sums of one vector block
  static constexpr int QN_NP = 64 * 65 / 2;                                         // packed N at 32 pairs
  static constexpr int QN_COEFS = lbk::qn_basis_coefs(LBFGSB_QN_ROOT_MAXCOL);       // the basis pass's coefficients

  // save_locals: what the entries will read until the next return
  void qn_record(int col, int head, double theta, int iupdat) {
    if (!qn.have || iupdat != qn.iupdat || nrefresh != qn.nref || col != qn.col || head != qn.head) qn.gen++;
    qn.have = true, qn.col = col, qn.head = head, qn.theta = theta, qn.theta_gram = false;
    qn.iupdat = iupdat, qn.nref = nrefresh;
  }
  int qn_alloc() {
    if (!qn.h_n) {  // (the last of the five: a call that failed part-way starts over)
      HIPCHK(own.device(&qn.d_part, (size_t)2 * lbk::QN_TILE * lbk::QN_KMAX * lbk::MAX_BLOCKS * sizeof(double)));
      HIPCHK(own.device(&qn.d_res, (size_t)QN_RES * sizeof(double)));
      HIPCHK(own.device(&qn.d_n[0], (size_t)QN_NP * sizeof(double)));
      HIPCHK(own.device(&qn.d_n[1], (size_t)QN_NP * sizeof(double)));
      HIPCHK(own.pinned(&qn.h_n, (size_t)QN_NP * sizeof(double)));
      qn.h_res.assign(QN_RES, 0.0);
    }
    // the gather space follows the communicator of THIS call (one may be attached after an earlier call)
    if (comm && qn.all_ranks != nranks) {
      qn.all_ranks = 0;
      HIPCHK(own.device(&qn.d_res_all, (size_t)QN_RES * nranks * sizeof(double)));
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
  using QnCarry = lbk::QnCarry;
  using QnPiece = lbk::QnPiece;
  using QnVecs = lbk::QnVecs<T>;
  using QnOuts = lbk::QnOuts<T>;
  // one launch on a piece, a failure reported under its name: launch_fn(q, n, W, head, col, c0, mc, k, args...)
  template <typename F, typename... A>
  int qn_go(const char *what, F launch_fn, const QnPiece &p, A... args) {
    return qn_launched(launch_fn(q, n, Wc(), qn.head, qn.col, p.c0, p.mc, p.k, args...), what);
  }
  // ... of a W'V pass: its partials and the piece's slots of the result buffer come last
  template <typename F, typename... A>
  int qn_go_sums(const char *what, F launch_fn, const QnPiece &p, A... args) {
    return qn_go(what, launch_fn, p, args..., qn.d_part, qn.d_res + p.off);
  }
  double qn_alpha(bool inv) const { return inv ? 1.0 / qn.theta : qn.theta; }
  // One W'V pass by a plan of qn.col pairs (qn_plan.hpp): a launch per piece, one fetch of all their sums (all ranks
  // reduced), then [S'v_k; Y'v_k] -> out[k * 2 col + i] (i < col: S, else Y) and what the first tile's launches
  // carried -> carried (qn_scatter_carry; NULL with QnCarry::None).  With no stored pair a carry goes by launches on
  // an empty tile, which read the zero line and nothing of W.
  template <typename L>
  int qn_sums_by(const lbk::QnPlan &pl, double *out, double *carried, L &&launch) {
    // (<= qn_res(LBFGSB_MAX_M) for every col <= LBFGSB_MAX_M; checked before anything is written)
    if (pl.total > QN_RES) return fail(LBFGSB_E_STATE, "qn: more sums than the buffer holds");
    for (const QnPiece &p : pl.pieces) CHK(launch(p));
    CHK(qn_reduce(pl.total));
    lbk::qn_scatter_sums(pl, qn.h_res.data(), out);
    lbk::qn_scatter_carry(pl, qn.h_res.data(), carried);
    return 0;
  }
  // the pass for d_k = v_k - center (center may be NULL: the vectors as they are).  vslot: the vectors are columns of
  // W, read at their slots in its layout (no center, nothing carried)
  int qn_sums(const lbk::QnPlan &pl, const T *const *v, bool vslot, const T *center, double *out, double *carried) {
    return qn_sums_by(pl, out, carried, [&](const QnPiece &p) {
      QnVecs vv{};
      for (int kk = 0; kk < p.k; ++kk) vv.p[kk] = v[p.k0 + kk];
      return qn_go_sums("qn_wtv", lbk::launch_qn_wtv<T>, p, vv, vslot, center, p.carry);
    });
  }
  // The second pass of qn_apply and the draws: out_k (+)= [S, Y] cf_k tile by tile (with no pair one empty tile, which
  // writes alpha v or the plain draw).  launch(piece, coef): one launch with the piece's 2 mc k packed coefficients
  template <typename L>
  int qn_expand_by(int kc, const double *cf, L &&launch) {
    const lbk::QnPlan pl = lbk::qn_plan(qn.col, kc, QnCarry::None, true);
    for (const QnPiece &p : pl.pieces) {
      double coef[2 * lbk::QN_TILE * lbk::QN_KMAX];
      lbk::qn_pack_coef(p, qn.col, cf, coef);
      CHK(launch(p, coef));
    }
    return 0;
  }
  // the vectors of one piece of the block that starts at vector k0: columns of v, ldv apart
  QnVecs qn_vecs(const QnPiece &p, const T *v, int64_t ldv, int64_t k0) const {
    QnVecs vv{};
    for (int kk = 0; kk < p.k; ++kk) vv.p[kk] = v + (k0 + p.k0 + kk) * ldv;
    return vv;
  }
  // qn_expand_by for the block that starts at vector k0, into the columns of out (ldo apart): the first tile reads
  // column j of v (ldv apart; ldv = 0: one vector for all; v NULL: nothing, the draws generate), a later tile reads
  // what the earlier ones wrote.  launch(piece, coef, src, dst)
  template <typename L>
  int qn_expand_block(int64_t k0, int kc, const double *cf, const T *v, int64_t ldv, T *out, int64_t ldo, L &&launch) {
    return qn_expand_by(kc, cf, [&](const QnPiece &p, const double *coef) {
      QnVecs src{};
      QnOuts dst{};
      for (int kk = 0; kk < p.k; ++kk) {
        dst.p[kk] = out + (k0 + p.k0 + kk) * ldo;
        src.p[kk] = p.c0 > 0 ? dst.p[kk] : v ? v + (k0 + p.k0 + kk) * ldv : nullptr;
      }
      return launch(p, coef, src, dst);
    });
  }
  // The two passes of an operator on k vectors, block by block (qn_plan.hpp, qn_block_kc; first: the first sample of
  // a draw, 0 for vectors that are loaded): sums(k0, piece) launches one piece of the W'V pass of the block at k0
  // -- with no pair it runs only for what it carries --, coef(j, sums, carried, c) maps [S'v; Y'v] of vector j and
  // what was carried for it to its (cs; cy) on the host, and expand(k0, piece, coef, src, dst) launches one piece of
  // the expansion (qn_expand_block).
  template <typename S, typename C, typename E>
  int qn_blocks_by(int64_t k, int64_t first, QnCarry carry, const T *v, int64_t ldv, T *out, int64_t ldo, S &&sums,
                   C &&coef, E &&expand) {
    const int col = qn.col;
    std::vector<double> sm((size_t)2 * std::max(col, 1) * lbk::QN_KMAX), cf(sm.size());
    double carried[lbk::QN_KMAX] = {};
    for (int64_t k0 = 0; k0 < k;) {
      const int kc = lbk::qn_block_kc(k0, k, first + k0);
      if (col > 0 || carry != QnCarry::None) {
        CHK(qn_sums_by(lbk::qn_plan(col, kc, carry), sm.data(), carried,
                       [&](const QnPiece &p) { return sums(k0, p); }));
        for (int kk = 0; kk < kc; ++kk)
          CHK(coef(k0 + kk, sm.data() + (size_t)kk * 2 * col, carried[kk], cf.data() + (size_t)kk * 2 * col));
      }
      CHK(qn_expand_block(k0, kc, cf.data(), v, ldv, out, ldo,
                          [&](const QnPiece &p, const double *coef, QnVecs src, QnOuts dst) {
                            return expand(k0, p, coef, src, dst);
                          }));
      k0 += kc;
    }
    return qn_finish();
  }
  // The columns j0 .. j1 - 1 of [S, Y] (j < col: S, else Y) as the vectors of a W'V pass, QN_KMAX at a time and read
  // at their slots in W's layout: launch(piece, vectors) is one launch, put(j, sums) takes [S'w_j; Y'w_j] of column j
  template <typename L, typename P>
  int qn_gram_by(int j0, int j1, L &&launch, P &&put) {
    const int col = qn.col;
    std::vector<double> sums((size_t)2 * col * lbk::QN_KMAX);
    for (int k0 = j0; k0 < j1; k0 += lbk::QN_KMAX) {
      const int kc = std::min(lbk::QN_KMAX, j1 - k0);
      CHK(qn_sums_by(lbk::qn_plan(col, kc, QnCarry::None), sums.data(), nullptr, [&](const QnPiece &p) {
        QnVecs vv{};
        for (int kk = 0; kk < p.k; ++kk) {
          const int j = k0 + p.k0 + kk;
          vv.p[kk] = (j < col ? ws : wy) + (int64_t)((qn.head - 1 + (j < col ? j : j - col)) % m) * ld;
        }
        return launch(p, vv);
      }));
      for (int kk = 0; kk < kc; ++kk) put(k0 + kk, sums.data() + (size_t)kk * 2 * col);
    }
    return 0;
  }
  // ... of the plain model: the pass of qn_sums on them
  template <typename P>
  int qn_gram_cols(int j0, int j1, P &&put) {
    return qn_gram_by(j0, j1, [&](const QnPiece &p, QnVecs vv) {
      return qn_go_sums("qn_wtv", lbk::launch_qn_wtv<T>, p, vv, true, nullptr, p.carry);
    }, put);
  }
  // S'Y and Y'Y over all rows, once per pair generation (the vectors of the W'V pass are the columns of Y)
  int qn_gram() {
    if (qn.gram_gen == qn.gen) return 0;
    const int col = qn.col;
    qn.sty.assign((size_t)col * col, 0.0), qn.yty.assign((size_t)col * col, 0.0);
    CHK(qn_gram_cols(col, 2 * col, [&](int j, const double *sums) {
      std::copy_n(sums, col, qn.sty.data() + (size_t)(j - col) * col);
      std::copy_n(sums + col, col, qn.yty.data() + (size_t)(j - col) * col);
    }));
    qn.gram_gen = qn.gen;
    if (qn.theta_gram && col > 0)  // matupd's theta = y'y / s'y of the newest pair (:2318)
      qn.theta = qn.yty[(size_t)(col - 1) * (col + 1)] / sy[(size_t)(col - 1) * (m + 1)];
    return 0;
  }
  // S'S over all rows from the stored pairs, once per pair generation, for the spectrum of a REAL32 context: the Ss
  // the iteration keeps is summed from the steps before they are rounded into W, so it agrees with the stored fp32
  // pairs to fp32 rounding only -- enough for B v, not for G = [S, Y]'[S, Y], whose error the coefficients of an
  // eigenvector multiply by their square (unit vectors came out 2e-3 short).  fp64 contexts keep using Ss.
  int qn_gram_ss() {
    if (qn.sts_gen == qn.gen) return 0;
    const int col = qn.col;
    qn.sts.assign((size_t)col * col, 0.0);
    CHK(qn_gram_cols(0, col,
                     [&](int j, const double *sums) { std::copy_n(sums, col, qn.sts.data() + (size_t)j * col); }));
    qn.sts_gen = qn.gen;
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
  // that as the map (S'v, Y'v, cs, cy) which lbh::qn_nmat and lbh::qn_gram_combine take
  auto qn_coef_map(bool inv) {
    return [this, inv, dg = qn_dg()](const double *stv, const double *ytv, double *cs, double *cy) {
      return qn_coef(inv, dg.data(), stv, ytv, cs, cy);
    };
  }

  // g (d x d, column-major) <- (g + g') / 2
  static void qn_symmetrise(int d, double *g) {
    for (int j = 0; j < d; ++j)
      for (int i = 0; i < j; ++i)
        g[i + (size_t)j * d] = g[j + (size_t)i * d] = 0.5 * (g[i + (size_t)j * d] + g[j + (size_t)i * d]);
  }
  // N of the mode (as qn_diag forms it) and G = [S, Y]'[S, Y] from ss and the Gram (after qn_gram()), both 2col x 2col
  // (sts: S'S from qn_gram_ss in place of Ss)
  int qn_model_mats(bool inv, double *nm, double *g, const double *sts = nullptr) {
    const int col = qn.col, d = 2 * col;
    const int info = lbh::qn_nmat(col, qn_coef_map(inv), nm);
    if (info) return info;
    for (int j = 0; j < col; ++j)
      for (int i = 0; i < col; ++i) {
        g[i + (size_t)j * d] = sts ? sts[i + (size_t)j * col] : ss[(size_t)std::min(i, j) + (size_t)std::max(i, j) * m];
        g[i + (size_t)(col + j) * d] = g[(col + j) + (size_t)i * d] = qn.sty[i + (size_t)j * col];
        g[(col + i) + (size_t)(col + j) * d] = qn.yty[i + (size_t)j * col];
      }
    qn_symmetrise(d, g);  // (Y'Y as the Gram pass summed it: symmetric up to rounding)
    return 0;
  }
  // C of A^(1/2) = sqrt(alpha) I + [S, Y] C [S, Y]' and the log-det sum of B (inv = false) or H, once per pair
  // generation (host_dense.hpp, qn_root): G = [S, Y]'[S, Y] from ss and the Gram, N as qn_diag forms it
  int qn_root_coef(bool inv) {
    const int col = qn.col, md = inv ? 1 : 0, d = 2 * col;
    if (col > LBFGSB_QN_ROOT_MAXCOL) return fail(LBFGSB_E_ARG, "qn: a root of more than 64 stored pairs");
    if (col == 0) return 0;
    CHK(qn_gram());
    if (qn.root_gen[md] == qn.gen) return 0;
    std::vector<double> nm((size_t)d * d), g((size_t)d * d), work((size_t)6 * d * d + d);
    const int info = qn_model_mats(inv, nm.data(), g.data());
    if (info) return info;
    qn.root_c[md].assign((size_t)d * d, 0.0);
    qn.root_gen[md] = -1;
    const int rc =
        lbh::qn_root(d, qn_alpha(inv), g.data(), nm.data(), qn.root_c[md].data(), &qn.root_logsum[md], work.data());
    if (rc == -2) return fail(LBFGSB_E_STATE, "qn: the model is not positive definite");
    if (rc) return fail(LBFGSB_E_STATE, "qn: the eigensolver of the root did not converge");
    qn.root_gen[md] = qn.gen;
    return 0;
  }
  // c = f C sums for one vector: C (2col x 2col, column-major) of a root -- qn.root_c[mode], qsh.root_c -- and
  // sums = [S'v; Y'v] as that root's W'V pass weighs them
  void qn_root_map(const std::vector<double> &cm, double f, const double *sums, double *c) const {
    const int d = 2 * qn.col;
    for (int i = 0; i < d; ++i) {
      double t = 0.0;
      for (int j = 0; j < d; ++j) t = t + cm[i + (size_t)j * d] * sums[j];
      c[i] = f * t;
    }
  }

  // log det A over all rows (after qn_root_coef(inv))
  double qn_logdet_of(bool inv) const {
    return (double)nglob * std::log(qn_alpha(inv)) + (qn.col > 0 ? qn.root_logsum[inv ? 1 : 0] : 0.0);
  }
  int qn_logdet(int mode, double *h_logdet) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    CHK(qn_root_coef(inv));
    *h_logdet = qn_logdet_of(inv);
    return 0;
  }

  // out_j = mean + scale A^(1/2) z_(first + j): per block of samples the W'z sums, c = scale C sums on the host, then
  // the expansion with z generated again (k_qn_draw.hip).  A block of more than one sample starts at an even sample.
  int qn_draw(int mode, int64_t k, uint64_t seed, int64_t first, const void *mean_, double scale, void *out_,
              int64_t ldo) override {
    return qn_draw_by(mode, k, seed, first, mean_, scale, out_, ldo, nullptr);
  }
  // h_logp (k values) or NULL: the log-density of every draw under N(mean, scale^2 A), from z'z of the W'z pass
  int qn_draw_logpdf(int mode, int64_t k, uint64_t seed, int64_t first, const void *mean_, double scale, void *out_,
                     int64_t ldo, double *h_logp) override {
    return qn_draw_by(mode, k, seed, first, mean_, scale, out_, ldo, h_logp);
  }
  int qn_draw_by(int mode, int64_t k, uint64_t seed, int64_t first, const void *mean_, double scale, void *out_,
                 int64_t ldo, double *h_logp) {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    CHK(qn_root_coef(inv));
    const double lconst = h_logp ? qn_log_norm(inv, scale) : 0.0;
    const double ra = std::sqrt(qn_alpha(inv));
    const T *mean = (const T *)mean_;
    return qn_blocks_by(
        k, first, h_logp ? QnCarry::Norms : QnCarry::None, nullptr, 0, (T *)out_, ldo,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_wtz", lbk::launch_qn_wtz<T>, p, seed, row0, first + k0 + p.k0,
                            p.carry == QnCarry::Norms);
        },
        [&](int64_t j, const double *sums, double zz, double *c) {
          qn_root_map(qn.root_c[inv ? 1 : 0], scale, sums, c);
          if (h_logp) h_logp[j] = -0.5 * (lconst + zz);
          return 0;
        },
        [&](int64_t k0, const QnPiece &p, const double *coef, QnVecs, QnOuts dst) {
          return qn_go("qn_draw", lbk::launch_qn_draw<T>, p, coef, scale * ra, seed, row0, first + k0 + p.k0,
                       p.c0 == 0, mean, dst);
        });
  }

  // n_global log 2 pi + 2 n_global log |scale| + log det A (after qn_root_coef(inv))
  double qn_log_norm(bool inv, double scale) const {
    return (double)nglob * std::log(6.283185307179586476925) + 2.0 * (double)nglob * std::log(std::fabs(scale)) +
           qn_logdet_of(inv);
  }
  // q_j = norm(dd_j) + p_j'N p_j, p_j = [S, Y]'d_j, N of the mode, for the k vectors d_j = v_j - center: the W'd pass
  // alone, nothing written.  launch(k0, piece): one piece of that pass for the block that starts at vector k0, with
  // what the norm term is made of (dd_j) carried along; norm is asked after the Gram, which may set theta
  template <typename L, typename F>
  int qn_quad_sums(bool inv, int64_t k, double *h_q, L &&launch, F &&norm) {
    const int col = qn.col;
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const std::vector<double> dg = qn_dg();
    std::vector<double> sums((size_t)2 * std::max(col, 1) * lbk::QN_KMAX), c((size_t)2 * std::max(col, 1));
    double dd[lbk::QN_KMAX];
    for (int64_t k0 = 0; k0 < k; k0 += lbk::QN_KMAX) {
      const int kc = lbk::qn_block_kc(k0, k);
      CHK(qn_sums_by(lbk::qn_plan(col, kc, QnCarry::Norms), sums.data(), dd,
                     [&](const QnPiece &p) { return launch(k0, p); }));
      for (int kk = 0; kk < kc; ++kk) {
        const double *sv = sums.data() + (size_t)kk * 2 * col;
        double t = 0.0;  // p'(N p), S part then Y part, ascending
        if (col > 0) {
          CHK(qn_coef(inv, dg.data(), sv, sv + col, c.data(), c.data() + col));
          for (int i = 0; i < 2 * col; ++i) t = t + sv[i] * c[(size_t)i];
        }
        h_q[k0 + kk] = norm(dd[kk]) + t;
      }
    }
    return 0;
  }
  // (v_j - center)' A (v_j - center) = alpha d'd + p'N p with d'd carried along
  int qn_quad_by(bool inv, int64_t k, const T *v, int64_t ldv, const T *center, double *h_q) {
    return qn_quad_sums(
        inv, k, h_q,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_wtv", lbk::launch_qn_wtv<T>, p, qn_vecs(p, v, ldv, k0), false, center, p.carry);
        },
        [&](double dd) { return qn_alpha(inv) * dd; });
  }
  // d_a'd_b for every a of one piece and b of a later one: one vectors-only launch per pair of pieces, all of them
  // back to back and fetched with one wait (fewer than k^2 / 2 <= 2048 sums: they fit the result buffer together).
  // pc: (first vector, width) of the pieces; dtd[a + b ldd], a < b
  int qn_sums_dd(const T *v, int64_t ldv, const T *center, const std::vector<std::pair<int, int>> &pc, double *dtd,
                 int ldd) {
    struct Job {
      int a0, ka, b0, kb, off;
    };
    std::vector<Job> jobs;
    int off = 0;
    for (size_t ia = 0; ia < pc.size(); ++ia)
      for (size_t ib = ia + 1; ib < pc.size(); ++ib) {
        jobs.push_back(Job{pc[ia].first, pc[ia].second, pc[ib].first, pc[ib].second, off});
        off += pc[ia].second * pc[ib].second;
      }
    if (jobs.empty()) return 0;
    if (off > QN_RES) return fail(LBFGSB_E_STATE, "qn: more sums than the buffer holds");  // (before any launch)
    for (const Job &j : jobs) {
      QnVecs va{}, vb{};
      for (int kk = 0; kk < j.ka; ++kk) va.p[kk] = v + (int64_t)(j.a0 + kk) * ldv;
      for (int kk = 0; kk < j.kb; ++kk) vb.p[kk] = v + (int64_t)(j.b0 + kk) * ldv;
      CHK(qn_launched(lbk::launch_qn_dtd<T>(q, n, va, j.ka, vb, j.kb, center, qn.d_part, qn.d_res + j.off),
                      "qn_dtd"));
    }
    CHK(qn_reduce(off));
    for (const Job &j : jobs)
      for (int ia = 0; ia < j.ka; ++ia)
        for (int ib = 0; ib < j.kb; ++ib)
          dtd[(j.a0 + ia) + (size_t)(j.b0 + ib) * ldd] = qn.h_res[(size_t)j.off + ia * j.kb + ib];
    return 0;
  }
  // G = (V - c)' A (V - c): per block of QN_KMAX vectors the W'd pass with the Gram of each piece along (p_a and the
  // d_a'd_b inside a piece), across pieces the vectors-only pass, then g_ab = alpha d_a'd_b + p_a'(N p_b) on the host
  int qn_vgram(int mode, int64_t k_, const void *v_, int64_t ldv, const void *center_, double *h_g,
               int64_t ldg) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    const int col = qn.col, k = (int)k_, d = 2 * col;
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const T *v = (const T *)v_, *center = (const T *)center_;
    std::vector<double> p((size_t)std::max(d, 1) * k), dtd((size_t)k * k, 0.0);
    std::vector<std::pair<int, int>> pc;
    for (int k0 = 0; k0 < k; k0 += lbk::QN_KMAX) {
      const lbk::QnPlan pl = lbk::qn_plan(col, std::min(lbk::QN_KMAX, k - k0), QnCarry::Gram);
      const T *vp[lbk::QN_KMAX];
      for (int kk = 0; kk < pl.kc; ++kk) vp[kk] = v + (int64_t)(k0 + kk) * ldv;
      double gr[lbk::QN_KMAX * lbk::QN_KMAX] = {};
      CHK(qn_sums(pl, vp, false, center, p.data() + (size_t)k0 * d, gr));
      for (const QnPiece &pp : pl.pieces) {  // the pieces of the first tile: they carried their Grams
        if (pp.carry != QnCarry::Gram) continue;
        pc.emplace_back(k0 + pp.k0, pp.k);
        for (int a = pp.k0; a < pp.k0 + pp.k; ++a)
          for (int b = a; b < pp.k0 + pp.k; ++b)
            dtd[(k0 + a) + (size_t)(k0 + b) * k] = gr[a + (size_t)b * lbk::QN_KMAX];
      }
    }
    CHK(qn_sums_dd(v, ldv, center, pc, dtd.data(), k));
    return lbh::qn_gram_combine(col, k, qn_alpha(inv), p.data(), dtd.data(), k, qn_coef_map(inv), h_g, ldg);
  }
  int qn_quad(int mode, int64_t k, const void *v, int64_t ldv, const void *center, double *h_q) override {
    CHK(qn_ready());
    return qn_quad_by(mode == LBFGSB_QN_H, k, (const T *)v, ldv, (const T *)center, h_q);
  }
  // log N(x_j; mean, scale^2 A): the quadratic form of the OTHER mode (A^-1) at x_j - mean, log det A of the root
  int qn_logpdf(int mode, int64_t k, const void *x, int64_t ldx, const void *mean, double scale,
                double *h_logp) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    CHK(qn_root_coef(inv));
    const double lconst = qn_log_norm(inv, scale);
    CHK(qn_quad_by(!inv, k, (const T *)x, ldx, (const T *)mean, h_logp));
    for (int64_t j = 0; j < k; ++j) h_logp[j] = -0.5 * (lconst + h_logp[j] / (scale * scale));
    return 0;
  }

  int qn_apply(int mode, int64_t k, const void *v_, int64_t ldv, void *out_, int64_t ldo) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H || mode == LBFGSB_QN_H_SQRT;
    const bool root = mode == LBFGSB_QN_B_SQRT || mode == LBFGSB_QN_H_SQRT;
    const int col = qn.col;
    if (root) CHK(qn_root_coef(inv));
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const double alpha = root ? std::sqrt(qn_alpha(inv)) : qn_alpha(inv);
    const std::vector<double> dg = qn_dg();
    const T *v = (const T *)v_;
    // out = alpha v + [S, Y] (cs; cy), one launch per column tile and block of vectors (col = 0: alpha v)
    return qn_blocks_by(
        k, 0, QnCarry::None, v, ldv, (T *)out_, ldo,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_wtv", lbk::launch_qn_wtv<T>, p, qn_vecs(p, v, ldv, k0), false, nullptr, p.carry);
        },
        [&](int64_t, const double *sums, double, double *c) {
          if (!root) return qn_coef(inv, dg.data(), sums, sums + col, c, c + col);
          qn_root_map(qn.root_c[inv ? 1 : 0], 1.0, sums, c);
          return 0;
        },
        [&](int64_t, const QnPiece &p, const double *coef, QnVecs src, QnOuts dst) {
          return qn_go("qn_expand", lbk::launch_qn_expand<T>, p, coef, p.c0 == 0 ? alpha : 1.0, src, dst);
        });
  }

  // N of a coefficient map (lbh::qn_nmat; with no pair nothing of it), packed as the diagonal kernels read it, into
  // d_n: the wait for the staging buffer, which may still feed an earlier copy, then the upload
  template <typename M>
  int qn_upload_n(M &&map, double *d_n) {
    const int col = qn.col;
    std::vector<double> nm((size_t)4 * col * col + 1);
    if (col > 0) {
      const int info = lbh::qn_nmat(col, map, nm.data());
      if (info) return info;
    }
    HIPCHK(hipStreamSynchronize(stream));
    lbh::qn_pack_n(col, lbk::maxc_for(std::max(col, 1)), nm.data(), qn.h_n);
    HIPCHK(hipMemcpyAsync(d_n, qn.h_n, (size_t)QN_NP * sizeof(double), hipMemcpyHostToDevice, stream));
    return 0;
  }
  int qn_diag(int mode, void *out_) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    const int col = qn.col;
    if (col > lbk::MAXM) return fail(LBFGSB_E_ARG, "qn_diag: more than 32 stored pairs");
    if (col > 0 && (inv || qn.theta_gram)) CHK(qn_gram());
    const int md = inv ? 1 : 0;
    if (qn.n_gen[md] != qn.gen || col == 0) {
      CHK(qn_upload_n(qn_coef_map(inv), qn.d_n[md]));
      qn.n_gen[md] = qn.gen;
    }
    CHK(qn_launched(lbk::launch_qn_diag<T>(q, n, Wc(), qn.head, col, qn.d_n[md], qn_alpha(inv), (T *)out_),
                    "qn_diag"));
    return qn_finish();
  }
  // The spectrum of B (inv = false) or H off the bulk eigenvalue alpha, once per pair generation (host_dense.hpp,
  // qn_eig): the Gram pass and the host algebra of the root, no other pass over W
  int qn_eig_coef(bool inv) {
    const int col = qn.col, md = inv ? 1 : 0, d = 2 * col;
    if (col > LBFGSB_QN_ROOT_MAXCOL) return fail(LBFGSB_E_ARG, "qn: the spectrum of more than 64 stored pairs");
    if (col == 0) {
      qn.eig_r[md] = 0;
      return 0;
    }
    CHK(qn_gram());
    if (qn.eig_gen[md] == qn.gen) return 0;
    if (sizeof(T) == 4) CHK(qn_gram_ss());
    std::vector<double> nm((size_t)d * d), g((size_t)d * d), work((size_t)7 * d * d + 6 * d);
    const int info = qn_model_mats(inv, nm.data(), g.data(), sizeof(T) == 4 ? qn.sts.data() : nullptr);
    if (info) return info;
    qn.eig_lam[md].assign((size_t)d, 0.0), qn.eig_c[md].assign((size_t)d * d, 0.0);
    qn.eig_gen[md] = -1;
    const int rc = lbh::qn_eig(d, qn_alpha(inv), LBFGSB_QN_EIG_CUT, nglob, g.data(), nm.data(), &qn.eig_r[md],
                               qn.eig_lam[md].data(), qn.eig_c[md].data(), work.data());
    if (rc == -2) return fail(LBFGSB_E_STATE, "qn: the model is not positive definite");
    if (rc) return fail(LBFGSB_E_STATE, "qn: the eigensolver of the spectrum did not converge");
    qn.eig_gen[md] = qn.gen;
    return 0;
  }
  int qn_eig(int mode, int32_t cap, int32_t *h_r, double *h_bulk, double *h_lambda) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    CHK(qn_eig_coef(inv));
    const int r = qn.eig_r[inv ? 1 : 0];
    *h_bulk = qn_alpha(inv), *h_r = r;
    for (int i = 0; i < std::min<int>(r, cap); ++i) h_lambda[i] = qn.eig_lam[inv ? 1 : 0][(size_t)i];
    return 0;
  }
  // out_j = the unit eigenvector number which[j] (NULL: j) of the mode: U = [S, Y] C, by one launch of the basis pass
  // per column tile for all k outputs (qn_plan.hpp, qn_basis_plan), or, with the option "qn_basis" off, by qn_apply's
  // expansion in blocks of QN_KMAX vectors with alpha = 0 (its src: a stored column of S, finite and never used)
  int qn_eigvec(int mode, int64_t k_, const int32_t *which, void *out_, int64_t ldo) override {
    CHK(qn_ready());
    const bool inv = mode == LBFGSB_QN_H;
    CHK(qn_eig_coef(inv));
    const int col = qn.col, md = inv ? 1 : 0, d = 2 * col, k = (int)k_, r = qn.eig_r[md];
    for (int j = 0; j < k; ++j)
      if ((which ? which[j] : j) < 0 || (which ? which[j] : j) >= r)
        return fail(LBFGSB_E_ARG, "qn_eigvec: an index outside 0 .. r - 1 (r of lbfgsb_hip_qn_eig)");
    std::vector<double> cf((size_t)d * k);
    for (int j = 0; j < k; ++j)
      std::copy_n(qn.eig_c[md].data() + (size_t)(which ? which[j] : j) * d, d, cf.data() + (size_t)j * d);
    T *out = (T *)out_;
    if (!qn.basis) {
      const T *any = ws + (int64_t)((qn.head - 1) % m) * ld;
      auto expand = [&](const QnPiece &p, const double *coef, QnVecs src, QnOuts dst) {
        return qn_go("qn_expand", lbk::launch_qn_expand<T>, p, coef, p.c0 == 0 ? 0.0 : 1.0, src, dst);
      };
      for (int k0 = 0; k0 < k; k0 += lbk::QN_KMAX)
        CHK(qn_expand_block(k0, lbk::qn_block_kc(k0, k), cf.data() + (size_t)k0 * d, any, 0, out, ldo, expand));
      return qn_finish();
    }
    const lbk::QnBasisPlan pl = lbk::qn_basis_plan(col, k);
    if (pl.total > QN_COEFS) return fail(LBFGSB_E_STATE, "qn: more coefficients than the buffer holds");
    if (!qn.h_coef) {
      HIPCHK(own.device(&qn.d_coef, (size_t)QN_COEFS * sizeof(double)));
      HIPCHK(own.pinned(&qn.h_coef, (size_t)QN_COEFS * sizeof(double)));
    }
    // (the coefficients stay on the device while the pairs, the mode and the indices do: a repeated call neither
    //  copies nor waits; a new set waits for the launches that may still read the old one, then for nothing)
    std::vector<int64_t> key{qn.gen, (int64_t)md, (int64_t)k};
    for (int j = 0; j < k; ++j) key.push_back(which ? which[j] : j);
    if (key != qn.coef_key) {
      qn.coef_key.clear();
      HIPCHK(hipStreamSynchronize(stream));
      lbk::qn_basis_pack(pl, cf.data(), qn.h_coef);
      HIPCHK(hipMemcpyAsync(qn.d_coef, qn.h_coef, (size_t)pl.total * sizeof(double), hipMemcpyHostToDevice, stream));
      qn.coef_key = key;
    }
    for (const lbk::QnBasisTile &t : pl.tiles)
      CHK(qn_launched(lbk::launch_qn_basis<T>(q, n, Wc(), qn.head, col, t.c0, t.mc, t.acc, qn.d_coef + t.off, k, out,
                                              ldo),
                      "qn_basis"));
    return qn_finish();
  }

  // ---- the model plus a diagonal (lbfgsb_hip_qn_shift_*; k_qn_shift.hip, host_dense.hpp qn_shift_factor / _coef,
  // DESIGN.md section 10f): (B + mu I + D)^-1 = diag(w) + diag(w) W K^-1 W' diag(w) on the rows that are not pinned.
  // qn_shift_set makes the weights and the factor of K for the pairs of this generation; solve, logdet and diag use
  // them while that generation lasts and refuse afterwards.
  struct QnShift {
    bool have = false;
    int64_t gen = -1;            // the pair generation the weights and the factor were made at
    int64_t pinned = 0;          // rows with d_i = +inf, all ranks
    double logdet = 0.0;         // log det of the shifted model on the free rows
    double sumlog = 0.0;         // the sum of log Delta_i over the free rows, all ranks
    std::vector<double> kf;      // qn_shift_factor's factor of K (2col x 2col)
    std::vector<double> gw;      // the weighted Gram [S, Y]' diag(w) [S, Y] the factor was made from
    int64_t root_gen = -1;       // the pair generation of the root below; -1 after every qn_shift_set (made at its
    std::vector<double> root_c;  // first use: host_dense.hpp, qn_shift_root): C of L = w^1/2 + w W C W' w^1/2
    double root_logsum = 0.0;    // sum log Delta - log det of the shifted model, by the root's route
    double *d_w[2] = {nullptr, nullptr};  // the weights (n doubles, natural order); a set that is refused leaves the
    int cur = 0;                          // live ones alone: it writes the other buffer, and success swaps
    double *d_n = nullptr;       // qn_shift_diag's packed N
    bool n_ok = false;           // ... is the one of this factor
  } qsh;
  int qn_shift_live() {
    if (!qsh.have || qsh.gen != qn.gen)
      return fail(LBFGSB_E_STATE, qsh.have ? "qn_shift: the pairs have changed since lbfgsb_hip_qn_shift_set: call "
                                             "qn_shift_set again"
                                           : "qn_shift: no shift is set: call qn_shift_set again");
    return 0;
  }
  // M^-1's blocks (col x col each): S'S, all of it, and S'Y, the lower triangle and the diagonal -- from Ss and Sy.  In
  // a REAL32 context both come from the stored pairs instead (qn_gram_ss, qn_gram): Ss and Sy are summed from the
  // steps before these are rounded into W, and K = M^-1 - W'wW cancels to the weighted part's size (at mu = 0, D = 0
  // its (2, 2) block is rounding noise), where an M^-1 that is 1e-7 off the pairs shows in full
  int qn_shift_minv(std::vector<double> &sts, std::vector<double> &syl) {
    const int col = qn.col;
    if (sizeof(T) == 4) {
      CHK(qn_gram_ss());
      CHK(qn_gram());
    }
    sts.assign((size_t)col * col, 0.0), syl.assign((size_t)col * col, 0.0);
    for (int j = 0; j < col; ++j)
      for (int i = 0; i < col; ++i) {
        sts[i + (size_t)j * col] = sizeof(T) == 4 ? 0.5 * (qn.sts[i + (size_t)j * col] + qn.sts[j + (size_t)i * col])
                                                  : ss[(size_t)std::min(i, j) + (size_t)std::max(i, j) * m];
        if (i >= j) syl[i + (size_t)j * col] = sizeof(T) == 4 ? qn.sty[i + (size_t)j * col] : sy[i + (size_t)j * m];
      }
    return 0;
  }
  // gw = [S, Y]' diag(w) [S, Y] over all rows (2col x 2col, the S block first): the weighted W'V pass with the
  // columns of W as its vectors, 4 at a time, then symmetrised as qn_model_mats does
  int qn_shift_gram(const double *wgt, double *gw) {
    const int d = 2 * qn.col;
    CHK(qn_gram_by(0, d, [&](const QnPiece &p, QnVecs vv) {
      return qn_go_sums("qn_shift_wtv", lbk::launch_qn_shift_wtv<T>, p, vv, true, false, wgt);
    }, [&](int j, const double *sums) { std::copy_n(sums, d, gw + (size_t)j * d); }));
    qn_symmetrise(d, gw);
    return 0;
  }
  int qn_shift_set(const void *d_, double mu, int64_t *h_pinned) override {
    CHK(qn_ready());
    const int col = qn.col, d = 2 * col;
    if (col > LBFGSB_QN_ROOT_MAXCOL) return fail(LBFGSB_E_ARG, "qn_shift_set: more than 64 stored pairs");
    if (col > 0 && qn.theta_gram) CHK(qn_gram());  // (theta of an imported state)
    const double shift = qn.theta + mu;
    if (!d_ && !(shift > 0.0)) return fail(LBFGSB_E_ARG, "qn_shift_set: theta + mu <= 0");
    // the first pass: the weights, sum log Delta over the free rows, the pinned and the refused rows
    const bool live = qsh.have && qsh.gen == qn.gen;
    const int dst = live ? 1 - qsh.cur : qsh.cur;
    if (!qsh.d_w[dst]) HIPCHK(own.device(&qsh.d_w[dst], (size_t)std::max<int64_t>(n, 1) * sizeof(double)));
    double *wgt = qsh.d_w[dst];
    CHK(qn_launched(lbk::launch_qn_shift_w<T>(q, n, (const T *)d_, shift, wgt, qn.d_part, qn.d_res), "qn_shift_w"));
    CHK(qn_reduce(lbk::QN_SHIFT_SUMS));
    const double sumlog = qn.h_res[0], pinned = qn.h_res[1], bad = qn.h_res[2];
    if (bad > 0.0)
      return fail(LBFGSB_E_ARG, "qn_shift_set: theta + mu + d_i <= 0 or NaN on " + std::to_string((long long)bad) +
                                    " rows");
    std::vector<double> kf((size_t)d * d + 1), km((size_t)d * d + 1), gw((size_t)d * d);
    double ldk = 0.0, ldm = 0.0;
    if (col > 0) {
      std::vector<double> sts, syl;
      CHK(qn_shift_minv(sts, syl));
      CHK(qn_shift_gram(wgt, gw.data()));
      if (lbh::qn_shift_factor(col, qn.theta, syl.data(), col, sts.data(), col, nullptr, km.data(), &ldm))
        return fail(LBFGSB_E_STATE, "qn_shift_set: the middle matrix is not factorisable (s'y <= 0 or S'S singular)");
      if (lbh::qn_shift_factor(col, qn.theta, syl.data(), col, sts.data(), col, gw.data(), kf.data(), &ldk))
        return fail(LBFGSB_E_STATE, "qn_shift_set: the shifted model is not positive definite on the free rows");
    }
    qsh.kf.swap(kf), qsh.gw.swap(gw);
    qsh.root_gen = -1, qsh.sumlog = sumlog;
    qsh.logdet = sumlog + (ldk - ldm);
    qsh.pinned = (int64_t)pinned;
    qsh.cur = dst, qsh.gen = qn.gen, qsh.have = true, qsh.n_ok = false;
    if (h_pinned) *h_pinned = qsh.pinned;
    return 0;
  }
  int qn_shift_logdet(double *h_logdet) override {
    CHK(qn_ready());
    CHK(qn_shift_live());
    *h_logdet = qsh.logdet;
    return 0;
  }
  // out_j = w o (v_j + S cs_j + Y cy_j): per block of QN_KMAX vectors the weighted W'V pass, the coefficients from
  // the factor, the weighted expansion
  int qn_shift_solve(int64_t k, const void *v_, int64_t ldv, void *out_, int64_t ldo) override {
    CHK(qn_ready());
    CHK(qn_shift_live());
    return qn_shift_apply(false, k, v_, ldv, out_, ldo);
  }
  // (cs; cy) of one vector from (S'(w o v); Y'(w o v)) by the factor of K: the map of which qn_shift_diag's N is the
  // matrix
  auto qn_shift_coef_map(const char *who) {
    return [this, who](const double *stv, const double *ytv, double *cs, double *cy) {
      if (lbh::qn_shift_coef(qn.col, qn.theta, qsh.kf.data(), stv, ytv, cs, cy))
        return fail(LBFGSB_E_STATE, std::string(who) + ": a zero pivot in the factor of K");
      return 0;
    };
  }
  // root: out_j = L v_j = sqrt(w) o v_j + w o (S cs_j + Y cy_j), (cs; cy) = C [S'(sqrt(w) o v_j); Y'(sqrt(w) o v_j)] --
  // the same two passes with the root's weights
  int qn_shift_apply(bool root, int64_t k, const void *v_, int64_t ldv, void *out_, int64_t ldo) {
    const int col = qn.col;
    const double *wgt = qsh.d_w[qsh.cur];
    const T *v = (const T *)v_;
    return qn_blocks_by(
        k, 0, QnCarry::None, v, ldv, (T *)out_, ldo,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_shift_wtv", lbk::launch_qn_shift_wtv<T>, p, qn_vecs(p, v, ldv, k0), false, root, wgt);
        },
        [&](int64_t, const double *sums, double, double *c) {
          if (!root) return qn_shift_coef_map("qn_shift_solve")(sums, sums + col, c, c + col);
          qn_root_map(qsh.root_c, 1.0, sums, c);
          return 0;
        },
        [&](int64_t, const QnPiece &p, const double *coef, QnVecs src, QnOuts dst) {
          return qn_go("qn_shift_expand", lbk::launch_qn_shift_expand<T>, p, coef, src, wgt, p.c0 == 0, root, dst);
        });
  }
  // out_i = w_i + w_i^2 r_i' N r_i, N = K^-1 in the [S, Y] basis: the matrix of qn_shift_coef's map
  int qn_shift_diag(void *out_) override {
    CHK(qn_ready());
    CHK(qn_shift_live());
    const int col = qn.col;
    if (col > lbk::MAXM) return fail(LBFGSB_E_ARG, "qn_shift_diag: more than 32 stored pairs");
    if (!qsh.d_n) HIPCHK(own.device(&qsh.d_n, (size_t)QN_NP * sizeof(double)));
    if (!qsh.n_ok) {
      CHK(qn_upload_n(qn_shift_coef_map("qn_shift_diag"), qsh.d_n));
      qsh.n_ok = true;
    }
    CHK(qn_launched(lbk::launch_qn_shift_diag<T>(q, n, Wc(), qn.head, col, qsh.d_n, qsh.d_w[qsh.cur], (T *)out_),
                    "qn_shift_diag"));
    return qn_finish();
  }

  // ---- square roots, draws and log-densities of the model plus a diagonal.  With Sigma =
  // (B + mu I + D)^-1 on the free rows: L = diag(sqrt w) + diag(w) W C W' diag(sqrt w), L L' = Sigma, C from
  // qn_shift_root on the weighted Gram that qn_shift_set reduced -- host algebra only, at the first use after a set.
  // (more than 64 pairs: LBFGSB_E_ARG, as every root -- before the shift is asked for, which qn_shift_set refuses
  //  there)
  int qn_shift_root_coef() {
    const int col = qn.col, d = 2 * col;
    if (col > LBFGSB_QN_ROOT_MAXCOL) return fail(LBFGSB_E_ARG, "qn_shift: a root of more than 64 stored pairs");
    CHK(qn_shift_live());
    if (qsh.root_gen == qsh.gen) return 0;
    std::vector<double> cm((size_t)d * d + 1), work((size_t)7 * d * d + d + 1);
    double logsum = 0.0;
    const int rc = lbh::qn_shift_root(col, qn.theta, qsh.kf.data(), qsh.gw.data(), cm.data(), &logsum, work.data());
    if (rc == -2) return fail(LBFGSB_E_STATE, "qn_shift: the shifted model is not positive definite on the free rows");
    if (rc < 0) return fail(LBFGSB_E_STATE, "qn_shift: the eigensolver of the root did not converge");
    if (rc) return fail(LBFGSB_E_STATE, "qn_shift: a zero pivot in the factor of K");
    qsh.root_c.swap(cm);
    qsh.root_logsum = logsum, qsh.root_gen = qsh.gen;
    return 0;
  }
  // the free rows of all ranks, and nf log 2 pi + 2 nf log |scale| - log det (B + mu I + D) by the root's route (after
  // qn_shift_root_coef): -2 x the constant of a log-density under N(mean, scale^2 Sigma)
  double qn_shift_free() const { return (double)(nglob - qsh.pinned); }
  double qn_shift_log_norm(double scale) const {
    const double nf = qn_shift_free();
    return nf * std::log(6.283185307179586476925) + 2.0 * nf * std::log(std::fabs(scale)) -
           (qsh.sumlog - qsh.root_logsum);
  }
  int qn_shift_sqrt(int64_t k, const void *v_, int64_t ldv, void *out_, int64_t ldo) override {
    CHK(qn_ready());
    CHK(qn_shift_root_coef());
    return qn_shift_apply(true, k, v_, ldv, out_, ldo);
  }
  // out_j = mean + scale L z_(first + j): per block of samples the weighted W'z sums, c = scale C sums on the host,
  // then the weighted expansion with z generated again.  h_logp (k values) or NULL: the log-density of every draw under
  // N(mean, scale^2 Sigma) on the free rows, from the z'z over them that the W'z pass carries
  int qn_shift_draw(int64_t k, uint64_t seed, int64_t first, const void *mean_, double scale, void *out_, int64_t ldo,
                    double *h_logp) override {
    CHK(qn_ready());
    CHK(qn_shift_root_coef());
    const double lconst = h_logp ? qn_shift_log_norm(scale) : 0.0;
    const bool none_free = nglob == qsh.pinned;
    const double *wgt = qsh.d_w[qsh.cur];
    const T *mean = (const T *)mean_;
    return qn_blocks_by(
        k, first, h_logp ? QnCarry::Norms : QnCarry::None, nullptr, 0, (T *)out_, ldo,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_shift_wtz", lbk::launch_qn_shift_wtz<T>, p, seed, row0, first + k0 + p.k0,
                            p.carry == QnCarry::Norms, wgt);
        },
        [&](int64_t j, const double *sums, double zz, double *c) {
          qn_root_map(qsh.root_c, scale, sums, c);
          if (h_logp) h_logp[j] = none_free ? 0.0 : -0.5 * (lconst + zz);
          return 0;
        },
        [&](int64_t k0, const QnPiece &p, const double *coef, QnVecs, QnOuts dst) {
          return qn_go("qn_shift_draw", lbk::launch_qn_shift_draw<T>, p, coef, scale, seed, row0, first + k0 + p.k0,
                       p.c0 == 0, mean, wgt, dst);
        });
  }
  // q_j = (v_j - center)'(B + mu I + D)(v_j - center) on the free rows = sum Delta_i q_i^2 + t'N_B t with
  // t = [S, Y]'(f o q): qn_quad's route for B with the Delta-weighted squared norm in place of theta q'q, one pass and
  // nothing written
  int qn_shift_quad_by(int64_t k, const T *v, int64_t ldv, const T *center, double *h_q) {
    const double *wgt = qsh.d_w[qsh.cur];
    return qn_quad_sums(
        false, k, h_q,
        [&](int64_t k0, const QnPiece &p) {
          return qn_go_sums("qn_shift_wtd", lbk::launch_qn_shift_wtd<T>, p, qn_vecs(p, v, ldv, k0), center,
                            p.carry == QnCarry::Norms, wgt);
        },
        [](double dd) { return dd; });
  }
  int qn_shift_quad(int64_t k, const void *v, int64_t ldv, const void *center, double *h_q) override {
    CHK(qn_ready());
    CHK(qn_shift_live());
    return qn_shift_quad_by(k, (const T *)v, ldv, (const T *)center, h_q);
  }
  // log N(x_j; mean, scale^2 Sigma) on the free rows: the quadratic form above, log det by the root's route
  int qn_shift_logpdf(int64_t k, const void *x, int64_t ldx, const void *mean, double scale,
                      double *h_logp) override {
    CHK(qn_ready());
    CHK(qn_shift_root_coef());
    const double lconst = qn_shift_log_norm(scale);
    CHK(qn_shift_quad_by(k, (const T *)x, ldx, (const T *)mean, h_logp));
    for (int64_t j = 0; j < k; ++j)
      h_logp[j] = nglob == qsh.pinned ? 0.0 : -0.5 * (lconst + h_logp[j] / (scale * scale));
    return 0;
  }

  int qn_finish() {
    if (!(flags & LBFGSB_F_NO_RETURN_SYNC)) {
      HIPCHK(hipStreamSynchronize(stream));
    }
    return 0;
  }
