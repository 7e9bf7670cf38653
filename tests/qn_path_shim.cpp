// Test-only C doorway into the host algebra of the model along a path of shifts in host_dense.hpp (qn_path_factor,
// qn_path_eval, qn_path_secular; qn_shift_factor for the bit-for-bit comparison), built by tests/test_qn_path_cpu.py
// with g++: the factor, the four scalars of an evaluation and the secular iteration are checked against dense numpy
// without a GPU.  With -DQN_PATH_MAIN the file is a program of its own that walks the same code on pairs it makes
// itself: what the test builds under -fsanitize=address,undefined and runs.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/lbfgsb_hip.h"
#include "../lbfgsb_amd/csrc/host_dense.hpp"

namespace {
// the evaluation of the secular iteration as solver_qn_path.inl makes it: the factor at mu, then the scalars
struct PathEval {
  int col;
  double theta;
  const double *sy, *sts, *gf, *p;
  double vv;
  std::vector<double> kf, c, work;
  PathEval(int col_, double theta_, const double *sy_, const double *sts_, const double *gf_, const double *p_,
           double vv_)
      : col(col_), theta(theta_), sy(sy_), sts(sts_), gf(gf_), p(p_), vv(vv_), kf((size_t)4 * col_ * col_ + 1),
        c((size_t)2 * col_ + 1), work((size_t)4 * col_ * col_ + 6 * col_ + 1) {}
  int operator()(double mu, double *norm2, double *xbx) {
    double w = 0.0, ld = 0.0, vx = 0.0;
    const int info = lbh::qn_path_shift(col, theta, mu, sy, sts, gf, 1.0, 0.0, kf.data(), &w, &ld, work.data());
    if (info) return info;
    if (col == 0) {
      *norm2 = w * w * vv, *xbx = w * *norm2;
      return 0;
    }
    return lbh::qn_path_eval(col, theta, kf.data(), w, p, vv, gf, c.data(), norm2, &vx, xbx, work.data()) ? 2 : 0;
  }
};
}  // namespace

extern "C" {
// sy: col x col, lower triangle of S'Y; sts: col x col, all of S'S; gf: 2col x 2col Gram on the free rows (S first)
int qp_factor(int col, double theta, const double *sy, const double *sts, const double *gf, double w, double *kf,
              double *logdet) {
  std::vector<double> work((size_t)4 * col * col + 1);
  return lbh::qn_path_factor(col, theta, sy, sts, gf, w, kf, logdet, work.data());
}
int qp_shift_factor(int col, double theta, const double *sy, const double *sts, const double *gw, double *kf,
                    double *logdet) {
  return lbh::qn_shift_factor(col, theta, sy, col, sts, col, gw, kf, logdet);
}
// the info of a shift (0, 1, 2) with w, the factor and log det (B_FF + mu I) for nf free rows
int qp_shift(int col, double theta, double mu, const double *sy, const double *sts, const double *gf, double nf,
             double ldm, double *kf, double *w, double *logdet) {
  std::vector<double> work((size_t)4 * col * col + 1);
  return lbh::qn_path_shift(col, theta, mu, sy, sts, gf, nf, ldm, kf, w, logdet, work.data());
}
// out = {||x||^2, v'x, x'(B_FF + mu I)^-1 x}
int qp_eval(int col, double theta, const double *kf, double w, const double *p, double vv, const double *gf, double *c,
            double *out) {
  std::vector<double> work((size_t)6 * col + 1);
  return lbh::qn_path_eval(col, theta, kf, w, p, vv, gf, c, out, out + 1, out + 2, work.data());
}
// out = {mu, ||x||^2, x'(B_FF + mu I)^-1 x}; returns qn_path_secular's code
int qp_secular(int col, double theta, const double *sy, const double *sts, const double *gf, const double *p,
               double vv, double delta, double rtol, int max_it, double *out, int *iters) {
  PathEval ev(col, theta, sy, sts, gf, p, vv);
  return lbh::qn_path_secular(delta, rtol, max_it, ev, out, out + 1, out + 2, iters);
}
}

#ifdef QN_PATH_MAIN
// pairs of the quadratic with the Hessian diag(1 + i / n): y = A s, so s'y > 0 and B is positive definite
int main() {
  int bad = 0;
  for (int col : {0, 1, 3, 10, 17}) {
    const int n = 60, d = 2 * col;
    std::vector<double> r((size_t)n * std::max(d, 1)), v((size_t)n);
    uint64_t st = 88172645463325252ull + (uint64_t)col;
    auto rnd = [&]() {
      st ^= st << 13, st ^= st >> 7, st ^= st << 17;
      return (double)(st >> 11) / 9007199254740992.0 - 0.5;
    };
    for (int j = 0; j < col; ++j)
      for (int i = 0; i < n; ++i) {
        const double s = rnd();
        r[(size_t)j * n + i] = s, r[(size_t)(col + j) * n + i] = (1.0 + (double)i / n) * s;
      }
    for (int i = 0; i < n; ++i) v[(size_t)i] = rnd();
    auto dot = [&](const double *a, const double *b, int i0) {
      double s = 0.0;
      for (int i = i0; i < n; i += (i0 ? 2 : 1)) s += a[i] * b[i];
      return s;
    };
    for (int pin = 0; pin < 2; ++pin) {  // pin: the even rows are pinned
      std::vector<double> gf((size_t)d * d + 1), sy((size_t)col * col + 1), sts((size_t)col * col + 1), p((size_t)d + 1);
      for (int a = 0; a < d; ++a) {
        for (int b = 0; b < d; ++b) gf[a + (size_t)b * d] = dot(&r[(size_t)a * n], &r[(size_t)b * n], pin);
        p[(size_t)a] = dot(&r[(size_t)a * n], v.data(), pin);
      }
      for (int a = 0; a < col; ++a)
        for (int b = 0; b < col; ++b) {
          sts[a + (size_t)b * col] = dot(&r[(size_t)a * n], &r[(size_t)b * n], 0);
          if (a >= b) sy[a + (size_t)b * col] = dot(&r[(size_t)a * n], &r[(size_t)(col + b) * n], 0);
        }
      const double vv = dot(v.data(), v.data(), pin);
      const double theta = col ? dot(&r[(size_t)(d - 1) * n], &r[(size_t)(d - 1) * n], 0) / sy[(size_t)col * col - 1] : 1.7;
      std::vector<double> kf((size_t)d * d + 1), c((size_t)d + 1);
      double out[3], x0[3], ld = 0.0;
      for (double mu : {0.0, 0.3, 5.0, 1e4 * theta, -2.0 * theta}) {
        const double shift = theta + mu;
        if (!(shift > 0.0)) continue;
        if (qp_factor(col, theta, sy.data(), sts.data(), gf.data(), 1.0 / shift, kf.data(), &ld)) ++bad;
        if (col && qp_eval(col, theta, kf.data(), 1.0 / shift, p.data(), vv, gf.data(), c.data(), out)) ++bad;
      }
      PathEval ev(col, theta, sy.data(), sts.data(), gf.data(), p.data(), vv);
      if (ev(0.0, &x0[0], &x0[2])) ++bad;
      for (double ratio : {2.0, 1.0, 0.9, 0.1, 1e-3, 1e-9})
        for (double rtol : {1e-6, 1e-10, 1e-17}) {
          int iters = 0;
          const double delta = ratio * std::sqrt(x0[0]);
          const int rc = qp_secular(col, theta, sy.data(), sts.data(), gf.data(), p.data(), vv, delta, rtol, 400, out,
                                    &iters);
          const bool ok = ratio >= 1.0 ? rc == 0 && out[0] == 0.0
                                       : (rc == 1 || rc == 2) && std::fabs(std::sqrt(out[1]) - delta) <= 1e-6 * delta;
          if (!ok) {
            std::printf("col %d pin %d ratio %g rtol %g: rc %d mu %g norm %g delta %g iters %d\n", col, pin, ratio, rtol,
                        rc, out[0], std::sqrt(out[1]), delta, iters);
            ++bad;
          }
        }
    }
  }
  std::printf("qn_path host algebra: %d failures\n", bad);
  return bad ? 1 : 0;
}
#endif
