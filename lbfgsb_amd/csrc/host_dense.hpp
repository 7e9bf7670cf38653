// host_dense.hpp -- the 2m x 2m algebra of the L-BFGS-B iteration, on the host.
//
// BASELINE.json north_star: "the 2m x 2m bmv middle-matrix solve and dpofa/dtrsl
// from lbfgsb_linpack_module stay on the host".  Everything here is O(m^2) or
// O(m^3) scalar work on matrices of order <= 2m <= 64; the n-dimensional work is
// in the k_*.hip files.  Arithmetic is fp64 for both REAL64 and REAL32 contexts.
//
// Follows (operation order included, so the CPU oracle can be compared to the
// last bit on identical inputs):
//   dpofa   reference src/lbfgsb_linpack_module.f90:30-67
//   dtrsl   reference src/lbfgsb_linpack_module.f90:87-165
//   bmv     reference src/lbfgsb.f90:1057-1123
//   formt   reference src/lbfgsb.f90:1926-1963
//   dcsrch  reference src/lbfgsb.f90:2942-3198
//   dcstep  reference src/lbfgsb.f90:3227-3415
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace lbh {

// column-major view, 0-based
struct Mat {
  double *p;
  int ld;
  double &operator()(int i, int j) const { return p[i + (size_t)j * ld]; }
};

inline double dot_seq(int n, const double *a, const double *b) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + a[i] * b[i];
  return s;
}

// Cholesky A = R'R in the upper triangle; returns 0 or the order of the
// leading minor that is not positive definite.
inline int dpofa(Mat a, int n) {
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = 0; k < j; ++k) {
      double t = a(k, j) - dot_seq(k, &a(0, k), &a(0, j));
      t = t / a(k, k);
      a(k, j) = t;
      s = s + t * t;
    }
    s = a(j, j) - s;
    if (s <= 0.0) return j + 1;
    a(j, j) = std::sqrt(s);
  }
  return 0;
}

// Triangular solves; job 00: T x = b (T lower), 01: T x = b (T upper),
// 10: T' x = b (T lower), 11: T' x = b (T upper).  Returns 0 or the 1-based
// index of a zero diagonal element.
inline int dtrsl(Mat t, int n, double *b, int job) {
  for (int i = 0; i < n; ++i)
    if (t(i, i) == 0.0) return i + 1;
  int kase = 1;
  if (job % 10 != 0) kase = 2;
  if ((job % 100) / 10 != 0) kase += 2;
  switch (kase) {
    case 1:
      b[0] = b[0] / t(0, 0);
      for (int j = 1; j < n; ++j) {
        double temp = -b[j - 1];
        if (temp != 0.0)
          for (int i = j; i < n; ++i) b[i] = b[i] + temp * t(i, j - 1);
        b[j] = b[j] / t(j, j);
      }
      break;
    case 2:
      b[n - 1] = b[n - 1] / t(n - 1, n - 1);
      for (int j = n - 2; j >= 0; --j) {
        double temp = -b[j + 1];
        if (temp != 0.0)
          for (int i = 0; i <= j; ++i) b[i] = b[i] + temp * t(i, j + 1);
        b[j] = b[j] / t(j, j);
      }
      break;
    case 3:
      b[n - 1] = b[n - 1] / t(n - 1, n - 1);
      for (int j = n - 2; j >= 0; --j) {
        b[j] = b[j] - dot_seq(n - 1 - j, &t(j + 1, j), &b[j + 1]);
        b[j] = b[j] / t(j, j);
      }
      break;
    case 4:
      b[0] = b[0] / t(0, 0);
      for (int j = 1; j < n; ++j) {
        b[j] = b[j] - dot_seq(j, &t(0, j), &b[0]);
        b[j] = b[j] / t(j, j);
      }
      break;
  }
  return 0;
}

// p = M v, M the 2col x 2col middle matrix of the compact L-BFGS formula.
inline int bmv(int m, const double *sy_, const double *wt_, int col, const double *v,
               double *p) {
  if (col == 0) return 0;
  Mat sy{const_cast<double *>(sy_), m}, wt{const_cast<double *>(wt_), m};
  p[col] = v[col];
  for (int i = 1; i < col; ++i) {
    double sum = 0.0;
    for (int k = 0; k < i; ++k) sum = sum + sy(i, k) * v[k] / sy(k, k);
    p[col + i] = v[col + i] + sum;
  }
  int info = dtrsl(wt, col, p + col, 11);
  if (info) return info;
  for (int i = 0; i < col; ++i) p[i] = v[i] / std::sqrt(sy(i, i));
  info = dtrsl(wt, col, p + col, 1);
  if (info) return info;
  for (int i = 0; i < col; ++i) p[i] = -p[i] / std::sqrt(sy(i, i));
  for (int i = 0; i < col; ++i) {
    double sum = 0.0;
    for (int k = i + 1; k < col; ++k) sum = sum + sy(k, i) * p[col + k] / sy(i, i);
    p[i] = p[i] + sum;
  }
  return 0;
}

// T = theta*S'S + L D^-1 L' (upper), then Cholesky.  Returns 0 or -3.
inline int formt(int m, double *wt_, const double *sy_, const double *ss_, int col,
                 double theta) {
  Mat wt{wt_, m}, sy{const_cast<double *>(sy_), m}, ss{const_cast<double *>(ss_), m};
  for (int j = 0; j < col; ++j) wt(0, j) = theta * ss(0, j);
  for (int i = 1; i < col; ++i)
    for (int j = i; j < col; ++j) {
      int k1 = std::min(i, j);
      double ddum = 0.0;
      for (int k = 0; k < k1; ++k) ddum = ddum + sy(i, k) * sy(j, k) / sy(k, k);
      wt(i, j) = ddum + theta * ss(i, j);
    }
  return dpofa(wt, col) ? -3 : 0;
}

// ---- the curvature model as an operator (lbfgsb_hip_qn_apply / qn_diag, solver_qn.inl) ----
// Both matrices are written over [S, Y] (logical column order, oldest pair first):
//   B = theta I + S cs + Y cy,      (cs; cy) = N_B (S'v; Y'v)
//   H = theta^-1 I + S cs + Y cy,   (cs; cy) = N_H (S'v; Y'v)
// B is the matrix bmv's middle matrix defines: B = theta I - [Y, theta S] M [Y, theta S]'.  H = B^-1 in the
// compact form of Byrd, Nocedal and Schnabel (1994, eq. 2.16 with gamma = 1 / theta):
//   H = theta^-1 I + [S, theta^-1 Y] [[R^-T (D + theta^-1 Y'Y) R^-1, -R^-T], [-R^-1, 0]] [S'; theta^-1 Y']
// with R the upper triangle of S'Y (diagonal included) and D its diagonal.

// coefficients of B v: stv = S'v, ytv = Y'v (col each) -> cs, cy.  Returns bmv's info.
inline int qn_coef_b(int m, const double *sy, const double *wt, int col, double theta, const double *stv,
                     const double *ytv, double *cs, double *cy) {
  if (col == 0) return 0;
  double v[2 * 1024], p[2 * 1024];
  for (int i = 0; i < col; ++i) v[i] = ytv[i], v[col + i] = theta * stv[i];
  const int info = bmv(m, sy, wt, col, v, p);
  if (info) return info;
  for (int i = 0; i < col; ++i) cy[i] = -p[i], cs[i] = -(theta * p[col + i]);
  return 0;
}

// coefficients of H v.  sty: S'Y (col x col, leading dimension ldg: sty[i + k ldg] = s_i'y_k), yty: Y'Y (same
// layout), dg: the diagonal s_i'y_i the iteration keeps (sy), which is also R's.  Returns 0, or i + 1 when
// R(i, i) <= 0 (no pair is stored without s'y > 0: reference src/lbfgsb.f90:820-826).
inline int qn_coef_h(int col, double theta, const double *sty, const double *yty, int ldg, const double *dg,
                     const double *stv, const double *ytv, double *cs, double *cy) {
  if (col == 0) return 0;
  for (int i = 0; i < col; ++i)
    if (!(dg[i] > 0.0)) return i + 1;
  const double ti = 1.0 / theta;
  double u[1024], w[1024];
  for (int i = col - 1; i >= 0; --i) {  // u = R^-1 S'v
    double s = stv[i];
    for (int k = i + 1; k < col; ++k) s = s - sty[i + (size_t)k * ldg] * u[k];
    u[i] = s / dg[i];
  }
  for (int i = 0; i < col; ++i) {  // w = (D + theta^-1 Y'Y) u - theta^-1 Y'v
    double s = 0.0;
    for (int k = 0; k < col; ++k) s = s + yty[i + (size_t)k * ldg] * u[k];
    w[i] = dg[i] * u[i] + ti * s - ti * ytv[i];
  }
  for (int i = 0; i < col; ++i) {  // cs = R^-T w
    double s = w[i];
    for (int k = 0; k < i; ++k) s = s - sty[k + (size_t)i * ldg] * cs[k];
    cs[i] = s / dg[i];
  }
  for (int i = 0; i < col; ++i) cy[i] = -(ti * u[i]);
  return 0;
}

// N (2col x 2col, column-major, leading dimension 2col) of a coefficient map coef(stv, ytv, cs, cy): column k is
// the map of the k-th unit vector; then symmetrised, (N + N') / 2 (the exact matrix is symmetric).
template <typename F>
inline int qn_nmat(int col, F &&coef, double *nm) {
  const int d = 2 * col;
  double e[2 * 1024], c[2 * 1024];
  for (int k = 0; k < d; ++k) {
    for (int i = 0; i < d; ++i) e[i] = i == k ? 1.0 : 0.0;
    const int info = coef(e, e + col, c, c + col);
    if (info) return info;
    for (int i = 0; i < d; ++i) nm[i + (size_t)k * d] = c[i];
  }
  for (int k = 0; k < d; ++k)
    for (int i = k + 1; i < d; ++i) {
      const double s = 0.5 * (nm[i + (size_t)k * d] + nm[k + (size_t)i * d]);
      nm[i + (size_t)k * d] = nm[k + (size_t)i * d] = s;
    }
  return 0;
}

// N as the diagonal kernel reads it: rows / columns padded to mc pairs (S block 0..mc, Y block mc..2mc), the upper
// triangle row by row, off-diagonal entries doubled (r'Nr = sum_a r_a (N_aa r_a + sum_{b > a} 2 N_ab r_b)).
inline void qn_pack_n(int col, int mc, const double *nm, double *np) {
  const int d = 2 * col, dp = 2 * mc;
  auto at = [&](int a) { return a < mc ? (a < col ? a : -1) : (a - mc < col ? col + a - mc : -1); };
  int e = 0;
  for (int a = 0; a < dp; ++a)
    for (int b = a; b < dp; ++b) {
      const int ia = at(a), ib = at(b);
      const double v = ia < 0 || ib < 0 ? 0.0 : nm[ia + (size_t)ib * d];
      np[e++] = a == b ? v : 2.0 * v;
    }
}

// The Gram matrix of k vectors d_a under A = alpha I + [S, Y] N [S, Y]' from the device's sums (lbfgsb_hip_qn_gram):
// p holds p_a = [S, Y]'d_a at p[i + a d], d = 2col (S part, then Y part), dtd the upper triangle of D'D at
// dtd[a + b ldd], a <= b, and coef(stv, ytv, cs, cy) maps p_b to c_b = N p_b (qn_coef_b / qn_coef_h).
//   g_ab = alpha d_a'd_b + sum_i p_a,i c_b,i,  i ascending (the S part first),  a <= b,
// and entry (b, a) is a copy of entry (a, b): symmetric bit for bit, and g_aa is the quadratic form's own formula
// (Solver::qn_quad_by).  Rows a >= k of g's columns (ldg > k) are not touched.  Returns 0 or coef's info, g then as
// it was.
template <typename F>
inline int qn_gram_combine(int col, int k, double alpha, const double *p, const double *dtd, int ldd, F &&coef,
                           double *g, int64_t ldg) {
  const int d = 2 * col;
  std::vector<double> c((size_t)std::max(d, 1) * k);
  for (int b = 0; b < k && col > 0; ++b) {
    const double *pb = p + (size_t)b * d;
    const int info = coef(pb, pb + col, c.data() + (size_t)b * d, c.data() + (size_t)b * d + col);
    if (info) return info;
  }
  for (int b = 0; b < k; ++b)
    for (int a = 0; a <= b; ++a) {
      double t = 0.0;
      for (int i = 0; i < d; ++i) t = t + p[i + (size_t)a * d] * c[i + (size_t)b * d];
      g[a + b * ldg] = g[b + a * ldg] = alpha * dtd[a + (size_t)b * ldd] + t;
    }
  return 0;
}

// ---- the model plus a diagonal (lbfgsb_hip_qn_shift_*, solver_qn.inl) ----
// With Delta = (theta + mu) I + D, w = 1 / Delta (0 on a pinned row), W = [Y, theta S] and bmv's middle matrix M,
//   (B + mu I + D)^-1 = diag(w) + diag(w) W K^-1 W' diag(w),   K = M^-1 - W' diag(w) W,
//   M^-1 = [[-D_sy, L'], [L, theta S'S]]  (D_sy, L: the diagonal and the strict lower triangle of S'Y),
// so K = [[-A, Bm'], [Bm, C]] with A = D_sy + Y'wY, Bm = L - theta S'wY, C = theta S'S - theta^2 S'wS.  When the shifted
// model is positive definite on the free rows K has col negative and col positive eigenvalues, and formk's route
// factorises it: A = R1'R1, X = R1^-T Bm', C + X'X = R2'R2 (the Schur complement).
//
// sy: S'Y, lower triangle and diagonal read (sy[i + j ldsy], i >= j); sts: S'S, all of it (sts[i + j ldss]); gw: the
// weighted Gram [S, Y]' diag(w) [S, Y], symmetric, 2col x 2col with the S block first -- NULL stands for zero, K = M^-1.
// kf (2col x 2col, column-major) receives R1 in the upper triangle of its (1, 1) block, X in the (1, 2) block and R2
// in the upper triangle of the (2, 2) block; *logdet = log |det K|.  Returns 0, 1 when A is not positive definite (a
// stored pair with s'y <= 0) or 2 when the Schur complement is not: K does not have the inertia (col, col).
inline int qn_shift_factor(int col, double theta, const double *sy, int ldsy, const double *sts, int ldss,
                           const double *gw, double *kf, double *logdet) {
  const int d = 2 * col;
  *logdet = 0.0;
  if (col == 0) return 0;
  std::fill(kf, kf + (size_t)d * d, 0.0);
  Mat k{kf, d}, r1{kf, d}, r2{kf + col + (size_t)col * d, d};
  auto g = [&](int i, int j) { return gw ? gw[i + (size_t)j * d] : 0.0; };
  for (int j = 0; j < col; ++j)
    for (int i = 0; i <= j; ++i) k(i, j) = (i == j ? sy[i + (size_t)i * ldsy] : 0.0) + g(col + i, col + j);
  if (dpofa(r1, col)) return 1;
  for (int j = 0; j < col; ++j) {  // column j of X: R1' x = row j of Bm
    double *x = &k(0, col + j);
    for (int i = 0; i < col; ++i) x[i] = (j > i ? sy[j + (size_t)i * ldsy] : 0.0) - theta * g(j, col + i);
    dtrsl(r1, col, x, 11);
  }
  for (int j = 0; j < col; ++j)
    for (int i = 0; i <= j; ++i)
      k(col + i, col + j) = (theta * sts[i + (size_t)j * ldss] - theta * theta * g(i, j)) +
                            dot_seq(col, &k(0, col + i), &k(0, col + j));
  if (dpofa(r2, col)) return 2;
  double s = 0.0;
  for (int i = 0; i < d; ++i) s = s + std::log(k(i, i));
  *logdet = 2.0 * s;
  return 0;
}

// (cs; cy) of out = w o (v + S cs + Y cy) from stv = S'(w o v), ytv = Y'(w o v) and qn_shift_factor's kf:
// K (z1; z2) = (ytv; theta stv), cy = z1, cs = theta z2
inline int qn_shift_coef(int col, double theta, const double *kf, const double *stv, const double *ytv, double *cs,
                         double *cy) {
  if (col == 0) return 0;
  const int d = 2 * col;
  double *p = const_cast<double *>(kf);
  Mat k{p, d}, r1{p, d}, r2{p + col + (size_t)col * d, d};
  double t[1024], z[1024];
  for (int i = 0; i < col; ++i) t[i] = ytv[i];
  int info = dtrsl(r1, col, t, 11);  // t = R1^-T b1
  if (info) return info;
  for (int j = 0; j < col; ++j) z[j] = theta * stv[j] + dot_seq(col, &k(0, col + j), t);  // b2 + X't
  info = dtrsl(r2, col, z, 11);
  if (info) return info;
  dtrsl(r2, col, z, 1);  // z2
  for (int i = 0; i < col; ++i) {  // X z2 - t
    double s = -t[i];
    for (int j = 0; j < col; ++j) s = s + k(i, col + j) * z[j];
    cy[i] = s;
  }
  dtrsl(r1, col, cy, 1);  // z1
  for (int i = 0; i < col; ++i) cs[i] = theta * z[i];
  return 0;
}

// ---- the model along a path of shifts (lbfgsb_hip_qn_path_*, solver_qn_path.inl) ----
// When the diagonal is "pins plus a scalar", every free row has the same weight w = 1 / (theta + mu), the weighted Gram
// of qn_shift_factor is w G_F with G_F = R_F'R_F, R = [S, Y] on the free rows F, and p = R_F'v does not depend on mu
// either: from one Gram and one read pass per vector the host answers for any number of shifts.
//
// kf, *logdet = qn_shift_factor's for the weighted Gram w g_f (g_f: 2col x 2col, the S block first; sy, sts: col x col
// as qn_shift_factor reads them, leading dimension col).  work: 4 col^2 doubles.  Returns qn_shift_factor's info.
inline int qn_path_factor(int col, double theta, const double *sy, const double *sts, const double *g_f, double w,
                          double *kf, double *logdet, double *work) {
  const int d = 2 * col;
  for (size_t e = 0; e < (size_t)d * d; ++e) work[e] = w * g_f[e];
  return qn_shift_factor(col, theta, sy, col, sts, col, work, kf, logdet);
}

// The shift mu judged and factorised: returns 1 when theta + mu <= 0 or mu is not finite, 2 when K(mu) does not have
// the inertia (col, col) -- the shifted model is not positive definite on the free rows --, else 0 with *w =
// 1 / (theta + mu), kf and *logdet = log det (B_FF + mu I) = nf log(theta + mu) + log |det K| - ldm (ldm = log |det
// M^-1|, qn_shift_factor without a Gram; nf = 0, no free row: 0).  work: 4 col^2 doubles.
inline int qn_path_shift(int col, double theta, double mu, const double *sy, const double *sts, const double *g_f,
                         double nf, double ldm, double *kf, double *w, double *logdet, double *work) {
  const double shift = theta + mu;
  if (!std::isfinite(mu) || !(shift > 0.0)) return 1;
  *w = 1.0 / shift;
  double ldk = 0.0;
  if (col > 0 && qn_path_factor(col, theta, sy, sts, g_f, *w, kf, &ldk, work)) return 2;
  *logdet = nf == 0.0 ? 0.0 : nf * std::log(shift) + (ldk - ldm);
  return 0;
}

// For x = (B_FF + mu I)^-1 v_F = w 1_F o (v + R c), from p = R_F'v (S part first), vv = sum_F v_i^2, g_f and the factor
// of K(mu): c (2col), *norm2 = x'x = w^2 (vv + 2 c'p + c'G_F c), *vx = v'x = w (vv + p'c) and *xbx =
// x'(B_FF + mu I)^-1 x = w x'x + w t'c2 with t = R_F'x = w (p + G_F c) and c2 the coefficients of the solve on x (the
// map applied, its matrix never formed); d(x'x) / d mu = -2 xbx.  work: 6 col doubles.  Returns qn_shift_coef's info.
inline int qn_path_eval(int col, double theta, const double *kf, double w, const double *p, double vv,
                        const double *g_f, double *c, double *norm2, double *vx, double *xbx, double *work) {
  const int d = 2 * col;
  double *t = work, *wt = work + d, *c2 = work + 2 * d;
  for (int i = 0; i < d; ++i) wt[i] = w * p[i];
  int info = qn_shift_coef(col, theta, kf, wt, wt + col, c, c + col);
  if (info) return info;
  double cp = 0.0, cgc = 0.0;
  for (int i = 0; i < d; ++i) {
    double gc = 0.0;
    for (int j = 0; j < d; ++j) gc = gc + g_f[i + (size_t)j * d] * c[j];
    t[i] = w * (p[i] + gc);
    cp = cp + c[i] * p[i];
    cgc = cgc + c[i] * gc;
  }
  *norm2 = w * w * ((vv + 2.0 * cp) + cgc);
  *vx = w * (vv + cp);
  for (int i = 0; i < d; ++i) wt[i] = w * t[i];
  info = qn_shift_coef(col, theta, kf, wt, wt + col, c2, c2 + col);
  if (info) return info;
  double tc = 0.0;
  for (int i = 0; i < d; ++i) tc = tc + t[i] * c2[i];
  *xbx = w * *norm2 + w * tc;
  return 0;
}

// The shift of a trust-region step: the mu >= 0 with ||x(mu)|| = delta, or 0 when ||x(0)|| <= delta, by Newton on
// phi(mu) = 1 / ||x(mu)|| - 1 / delta (More and Sorensen) from mu = 0 inside a bracket [lo, hi], ||x(lo)|| > delta >=
// ||x(hi)||: a Newton point outside the open bracket is replaced by its middle (by doubling while no upper end is
// known).  eval(mu, &norm2, &xbx) evaluates x'x and x'(B + mu I)^-1 x and returns 0, or nonzero where the shifted
// model is not positive definite (such a mu is a lower end).  Stops when | ||x|| - delta | <= rtol delta, when the
// ends of the bracket are adjacent doubles (then at the upper end), or after max_it evaluations (then at the upper end
// too, if one is known).  *mu, *norm2 and *xbx are those of the evaluation handed out, *iters the evaluations made.
// Returns 0 (mu = 0 is inside), 1 (on the boundary to rtol), 2 (the adjacent-doubles exit), 3 (max_it reached: the
// upper end, ||x|| <= delta but not to rtol), 4 (max_it reached with no upper end known: every evaluation had ||x|| >
// delta, *mu is the last of them and NOT a step inside the region) or -1 (the model is not positive definite at
// mu = 0 and no evaluation succeeded).  So 0 .. 3 always hand out ||x|| <= delta (1 + rtol).
template <typename F>
inline int qn_path_secular(double delta, double rtol, int max_it, F &&eval, double *mu, double *norm2, double *xbx,
                           int *iters) {
  double lo = 0.0, hi = HUGE_VAL, m = 0.0, n2 = 0.0, xb = 0.0;
  double hi_n2 = 0.0, hi_xb = 0.0;
  bool any = false;
  int it = 0, rc = 3;
  *mu = 0.0, *norm2 = 0.0, *xbx = 0.0;
  while (it < max_it) {
    const int info = eval(m, &n2, &xb);
    ++it;
    double next;
    if (info == 0) {
      const double nx = std::sqrt(n2);
      any = true, *mu = m, *norm2 = n2, *xbx = xb;
      if (m == 0.0 && nx <= delta) {
        rc = 0;
        break;
      }
      if (std::fabs(nx - delta) <= rtol * delta) {
        rc = 1;
        break;
      }
      if (nx > delta) lo = m;
      else hi = m, hi_n2 = n2, hi_xb = xb;
      next = m + (nx - delta) / delta * (n2 / xb);
    } else {
      lo = m;
      next = HUGE_VAL;
    }
    if (hi < HUGE_VAL && !(std::nextafter(lo, hi) < hi)) {  // nothing between the ends
      *mu = hi, *norm2 = hi_n2, *xbx = hi_xb;
      rc = 2;
      break;
    }
    if (!(next > lo && next < hi)) next = hi < HUGE_VAL ? lo + 0.5 * (hi - lo) : (lo > 0.0 ? 2.0 * lo : 1.0);
    if (!(next > lo)) next = std::nextafter(lo, hi);
    m = next;
  }
  *iters = it;
  if (!any) return -1;
  if (rc == 3) {  // max_it ran out: the upper end of the bracket where one is known, else nothing to hand out
    if (!(hi < HUGE_VAL)) return 4;
    *mu = hi, *norm2 = hi_n2, *xbx = hi_xb;
  }
  return rc;
}

// ---- entries at index lists (lbfgsb_hip_qn_block / qn_cols and the shifted twins) ----
// The gathered rows of [S, Y] lie column by column: r[j + c ldr] is entry idx_j of logical column c (c < col: S, else
// Y), j < k, as the gather delivers them.
//
// c_j = N r_j for every row of a list: cf[i + j d], d = 2col (what the columns pass expands: A e_idx_j = alpha e + W c_j)
inline void qn_rows_times_n(int col, const double *nm, const double *r, int k, int64_t ldr, double *cf) {
  const int d = 2 * col;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < d; ++i) {
      double t = 0.0;
      for (int c = 0; c < d; ++c) t = t + nm[i + (size_t)c * d] * r[j + c * ldr];
      cf[i + (size_t)j * d] = t;
    }
}
// the gathered rows row by row, rt[c + j d] = r[j + c k]: the dot products of a block then read both operands in order
inline void qn_rows_transposed(int d, const double *r, int k, double *rt) {
  for (int c = 0; c < d; ++c)
    for (int j = 0; j < k; ++j) rt[c + (size_t)j * d] = r[j + (size_t)c * k];
}
// a[ja + jb lda] = A[ia_ja, ib_jb] for A = alpha I + [S, Y] N [S, Y]' (N symmetric, 2col x 2col: qn_nmat):
//   alpha [ia_ja == ib_jb] + sum_i ra_ja,i (N rb_jb)_i,  i ascending (the S part first),
// with N rb_jb formed once per column, kb (2col)^2 operations.  same: ib is ia (rb, ib are not read); the upper
// triangle is computed, each sum as the mean of its two orders (r_a'(N r_b) and r_b'(N r_a)), and entry (b, a) is a
// copy of entry (a, b): symmetric bit for bit, as qn_gram_combine's block, and a repeated index repeats its row.
inline void qn_entries(int col, double alpha, const double *nm, const double *ra, int ka, const int64_t *ia,
                       const double *rb, int kb, const int64_t *ib, bool same, double *a, int64_t lda) {
  const int d = 2 * col;
  if (same) rb = ra, kb = ka, ib = ia;
  std::vector<double> cf((size_t)std::max(d, 1) * kb), rt((size_t)std::max(d, 1) * ka);
  qn_rows_times_n(col, nm, rb, kb, kb, cf.data());
  qn_rows_transposed(d, ra, ka, rt.data());
  for (int jb = 0; jb < kb; ++jb)
    for (int ja = 0; ja < (same ? jb + 1 : ka); ++ja) {
      double t = dot_seq(d, &rt[(size_t)ja * d], &cf[(size_t)jb * d]);
      if (same)  // (both orders: a repeated index then gives a repeated row and column bit for bit)
        t = 0.5 * (t + dot_seq(d, &rt[(size_t)jb * d], &cf[(size_t)ja * d]));
      const double v = (ia[ja] == ib[jb] ? alpha : 0.0) + t;
      a[ja + jb * lda] = v;
      if (same) a[jb + ja * lda] = v;
    }
}
// c_j = K^-1 (w_j r_j) in the [S, Y] basis for every row of a list, by qn_shift_coef on qn_shift_factor's kf:
// cf[i + j d] (what the shifted columns pass expands: Sigma e_idx_j = w_j e + w o (W c_j)).  Returns 0 or
// qn_shift_coef's info.
inline int qn_shift_rows_coef(int col, double theta, const double *kf, const double *r, const double *w, int k,
                              int64_t ldr, double *cf) {
  const int d = 2 * col;
  std::vector<double> t((size_t)std::max(d, 1));
  for (int j = 0; j < k; ++j) {
    for (int c = 0; c < d; ++c) t[(size_t)c] = w[j] * r[j + c * ldr];
    const int info = qn_shift_coef(col, theta, kf, t.data(), t.data() + col, cf + (size_t)j * d, cf + (size_t)j * d + col);
    if (info) return info;
  }
  return 0;
}
// The twin for Sigma = (B + mu I + D)^-1 = diag(w) + diag(w) W K^-1 W' diag(w): wa, wb are the weights at the indices
// (0 on a pinned row),
//   a[ja + jb lda] = wa_ja [ia_ja == ib_jb] + wa_ja sum_i ra_ja,i (K^-1 (wb_jb rb_jb))_i,
// and exactly +0 where either row is pinned.  Returns 0 or qn_shift_coef's info, a then as it was.
inline int qn_shift_entries(int col, double theta, const double *kf, const double *ra, const double *wa, int ka,
                            const int64_t *ia, const double *rb, const double *wb, int kb, const int64_t *ib,
                            bool same, double *a, int64_t lda) {
  const int d = 2 * col;
  if (same) rb = ra, wb = wa, kb = ka, ib = ia;
  std::vector<double> cf((size_t)std::max(d, 1) * kb);
  const int info = qn_shift_rows_coef(col, theta, kf, rb, wb, kb, kb, cf.data());
  if (info) return info;
  std::vector<double> rt((size_t)std::max(d, 1) * ka);
  qn_rows_transposed(d, ra, ka, rt.data());
  for (int jb = 0; jb < kb; ++jb)
    for (int ja = 0; ja < (same ? jb + 1 : ka); ++ja) {
      double t = wa[ja] * dot_seq(d, &rt[(size_t)ja * d], &cf[(size_t)jb * d]);
      if (same) t = 0.5 * (t + wa[jb] * dot_seq(d, &rt[(size_t)jb * d], &cf[(size_t)ja * d]));
      const double v = wa[ja] == 0.0 || wb[jb] == 0.0 ? 0.0 : (ia[ja] == ib[jb] ? wa[ja] : 0.0) + t;
      a[ja + jb * lda] = v;
      if (same) a[jb + ja * lda] = v;
    }
  return 0;
}

// ---- the square root and the log-determinant of the model (lbfgsb_hip_qn_apply's root modes, qn_logdet, qn_draw) ----
// Both models are A = alpha I + W N W' with W = [S, Y] and G = W'W.  With P = G^(1/2) and P N P = V diag(delta) V'
// (delta: the non-zero eigenvalues of W N W'),
//   A^(1/2) = sqrt(alpha) I + W C W',
//   C = N / (2 sqrt(alpha)) - (N P V) diag(1 / (2 sqrt(alpha) (sqrt(alpha) + sqrt(alpha + delta_i))^2)) (N P V)'
//   log det A = n log alpha + sum_i log1p(delta_i / alpha)
// -- symmetric eigenproblems only, and no division by G (nearly parallel pairs cost nothing).  The columns of W are
// scaled to unit length first (W D^-1, D N D, D = diag(G)^(1/2): the same A): the pairs of a converging run shrink
// by many orders of magnitude while N grows as their inverse, and the eigensolver's absolute accuracy would
// otherwise be spent on the largest columns alone.

// Cyclic Jacobi for a symmetric matrix of order d (column-major, leading dimension d; a is destroyed): eigenvalues
// into w, eigenvectors into the columns of v.  Fixed sweep order (p < q, row by row), so the same input gives the
// same bits everywhere.  Returns the number of sweeps, or -1 when 60 sweeps did not converge.
inline int jacobi_eig(int d, double *a, double *v, double *w) {
  for (int j = 0; j < d; ++j)
    for (int i = 0; i < d; ++i) v[i + (size_t)j * d] = i == j ? 1.0 : 0.0;
  double fro = 0.0;
  for (int k = 0; k < d * d; ++k) fro = fro + a[k] * a[k];
  const double tiny = 1e-18 * std::sqrt(fro);  // entries below this no longer move an eigenvalue in fp64
  for (int sweep = 0; sweep < 60; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < d - 1; ++p)
      for (int q = p + 1; q < d; ++q) {
        const double apq = a[p + (size_t)q * d];
        if (std::fabs(apq) <= tiny) {
          a[p + (size_t)q * d] = a[q + (size_t)p * d] = 0.0;
          continue;
        }
        ++rotated;
        const double app = a[p + (size_t)p * d], aqq = a[q + (size_t)q * d];
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < d; ++k) {  // columns p, q of a J
          const double akp = a[k + (size_t)p * d], akq = a[k + (size_t)q * d];
          a[k + (size_t)p * d] = c * akp - s * akq;
          a[k + (size_t)q * d] = s * akp + c * akq;
        }
        for (int k = 0; k < d; ++k) {  // rows p, q of J' (a J)
          const double apk = a[p + (size_t)k * d], aqk = a[q + (size_t)k * d];
          a[p + (size_t)k * d] = c * apk - s * aqk;
          a[q + (size_t)k * d] = s * apk + c * aqk;
        }
        a[p + (size_t)q * d] = a[q + (size_t)p * d] = 0.0;
        for (int k = 0; k < d; ++k) {
          const double vkp = v[k + (size_t)p * d], vkq = v[k + (size_t)q * d];
          v[k + (size_t)p * d] = c * vkp - s * vkq;
          v[k + (size_t)q * d] = s * vkp + c * vkq;
        }
      }
    if (!rotated) {
      for (int i = 0; i < d; ++i) w[i] = a[i + (size_t)i * d];
      return sweep;
    }
  }
  return -1;
}

// The spectral part that the root and the eigen-decomposition share: the unit-column scaling ds = diag(G)^(1/2) (d
// doubles), P = (D^-1 G D^-1)^(1/2), P (D N D) P = V diag(delta) V' and N P V of the scaled model.  work: 6 d^2 + d
// doubles; on return delta is at work + 5 d^2, N P V (d x d, column i belongs to delta_i) at work, the scaled N at
// work + 5 d^2 + d, and work + d^2 (V) is free.  clip: eigenvalues of the scaled G below d eps max(w) count as zero
// before the square root (qn_eig's path only: the rank of [S, Y] when it has fewer rows than columns).  keep (d^2 + d
// doubles, or NULL): the eigenvectors of the scaled G and the square roots of its eigenvalues as P was built from
// them (copies: nothing of the arithmetic changes).  Returns 0, or -1 when the eigensolver did not converge.
inline int qn_spectrum(int d, const double *g, const double *n_, double *ds, double *work, bool clip,
                       double *keep = nullptr) {
  const size_t dd = (size_t)d * d;
  double *a = work, *u = work + dd, *p = work + 2 * dd, *t = work + 3 * dd, *x = work + 4 * dd, *w = work + 5 * dd;
  auto at = [d](double *m, int i, int j) -> double & { return m[i + (size_t)j * d]; };
  auto mul = [&](const double *l, const double *r, double *o) {  // o = l r
    for (int j = 0; j < d; ++j)
      for (int i = 0; i < d; ++i) {
        double s = 0.0;
        for (int k = 0; k < d; ++k) s = s + l[i + (size_t)k * d] * r[k + (size_t)j * d];
        o[i + (size_t)j * d] = s;
      }
  };
  // unit columns: G <- D^-1 G D^-1 (in a), N <- D N D (in t, then nn)
  for (int i = 0; i < d; ++i) ds[i] = g[i + (size_t)i * d] > 0.0 ? std::sqrt(g[i + (size_t)i * d]) : 1.0;
  for (int j = 0; j < d; ++j)
    for (int i = 0; i < d; ++i) {
      at(a, i, j) = g[i + (size_t)j * d] / (ds[i] * ds[j]);
      at(t, i, j) = 0.5 * (n_[i + (size_t)j * d] + n_[j + (size_t)i * d]) * (ds[i] * ds[j]);
    }
  // P = U max(Lambda, 0)^(1/2) U'
  if (jacobi_eig(d, a, u, w) < 0) return -1;
  double floor_w = 0.0;
  if (clip) {
    for (int j = 0; j < d; ++j) floor_w = std::max(floor_w, w[j]);
    floor_w = floor_w * ((double)d * 2.220446049250313e-16);
  }
  for (int j = 0; j < d; ++j) {
    const double r = clip && w[j] < floor_w ? 0.0 : std::sqrt(std::max(w[j], 0.0));
    for (int i = 0; i < d; ++i) at(x, i, j) = at(u, i, j) * r;
    if (keep) keep[dd + j] = r;
  }
  if (keep) std::copy(u, u + dd, keep);
  for (int j = 0; j < d; ++j)
    for (int i = 0; i <= j; ++i) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = s + at(x, i, k) * at(u, j, k);
      at(p, i, j) = at(p, j, i) = s;
    }
  // T = P N P, symmetrised = V diag(delta) V'
  double *nn = work + 5 * dd + d;  // the scaled N
  for (size_t k = 0; k < dd; ++k) nn[k] = t[k];
  mul(nn, p, x);  // x = N P
  mul(p, x, t);
  for (int j = 0; j < d; ++j)
    for (int i = 0; i < j; ++i) at(t, i, j) = at(t, j, i) = 0.5 * (at(t, i, j) + at(t, j, i));
  if (jacobi_eig(d, t, u, w) < 0) return -1;  // u = V, w = delta
  mul(x, u, a);                               // a = N P V
  return 0;
}

// C (d x d, d = 2col, column-major, symmetric) and sum_i log1p(delta_i / alpha) from the Gram g = W'W and the
// symmetric n_ of the model (both d x d).  work: 6 d^2 + d doubles.  Returns 0, -1 (the eigensolver did not
// converge) or -2 (alpha + delta_i < -1e-8 alpha: the model is not positive definite).
inline int qn_root(int d, double alpha, const double *g, const double *n_, double *cm, double *logsum, double *work) {
  *logsum = 0.0;
  if (d == 0) return 0;
  const size_t dd = (size_t)d * d;
  double *a = work, *u = work + dd, *w = work + 5 * dd, *nn = work + 5 * dd + d;
  auto at = [d](double *m, int i, int j) -> double & { return m[i + (size_t)j * d]; };
  double *ds = cm;  // (cm is written last: its first d entries hold D until then; C <- D^-1 C D^-1 at the end)
  if (qn_spectrum(d, g, n_, ds, work, false) < 0) return -1;
  const double ra = std::sqrt(alpha);
  for (int i = 0; i < d; ++i) {
    if (alpha + w[i] < -1e-8 * alpha) return -2;
    const double rs = ra + std::sqrt(std::max(alpha + w[i], 0.0));
    *logsum = *logsum + std::log1p(std::max(w[i], -alpha) / alpha);
    w[i] = 1.0 / (2.0 * ra * (rs * rs));
  }
  for (int i = 0; i < d; ++i) u[i] = ds[i];  // (V is used up; cm is written from here on)
  for (int j = 0; j < d; ++j)
    for (int i = 0; i <= j; ++i) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = s + at(a, i, k) * w[k] * at(a, j, k);
      at(cm, i, j) = at(cm, j, i) = (at(nn, i, j) / (2.0 * ra) - s) / (u[i] * u[j]);
    }
  return 0;
}

// ---- a factor of the model plus a diagonal (lbfgsb_hip_qn_shift_sqrt / _draw / _logpdf) ----
// Sigma = (B + mu I + D)^-1 = diag(w) + diag(w) W N W' diag(w) on the free rows, W = [S, Y] and N the matrix of
// qn_shift_coef's map.  With What = diag(w^(1/2)) W: Sigma = w^(1/2) (I + What N What') w^(1/2), and the bracket is
// qn_root's model at alpha = 1 on the weighted Gram gw = What'What = W' diag(w) W.  Its symmetric root I + What C What'
// gives L = diag(w^(1/2)) + diag(w) W C W' diag(w^(1/2)) with L L' = Sigma, and
//   log det (B + mu I + D) on the free rows = sum log Delta_i - *logsum.
// kf: qn_shift_factor's factor; gw: 2col x 2col, the S block first; cm: C (2col x 2col); work: 7 d^2 + d doubles,
// d = 2col.  Returns 0, -1 / -2 as qn_root, or qn_shift_coef's info > 0 (a zero pivot in the factor).
inline int qn_shift_root(int col, double theta, const double *kf, const double *gw, double *cm, double *logsum,
                         double *work) {
  *logsum = 0.0;
  if (col == 0) return 0;
  const int d = 2 * col;
  double *nm = work + 6 * (size_t)d * d + d;
  const int info = qn_nmat(col, [&](const double *stv, const double *ytv, double *cs, double *cy) {
    return qn_shift_coef(col, theta, kf, stv, ytv, cs, cy);
  }, nm);
  if (info) return info;
  return qn_root(d, 1.0, gw, nm, cm, logsum, work);
}

// ---- eigenvalues and eigenvectors of the model (lbfgsb_hip_qn_eig / qn_eigvec) ----
// A = alpha I + W N W' has the eigenvalue alpha + delta_i with the unit eigenvector u_i = W (N P V)_i / delta_i for
// every delta_i != 0 of qn_spectrum (|u_i|^2 = v_i'(P N P)^2 v_i / delta_i^2 = 1, and A u_i = alpha u_i + W N P
// (P N P) v_i / delta_i), and alpha on the complement.  Directions with |delta_i| <= cut alpha belong to the bulk
// eigenvalue alpha and are not returned.  *r directions remain; lam[0 .. r) = alpha + delta_i ascending (equal values
// in the order of i); coef (d x r, column-major): column j holds the coefficients c of u in the unscaled [S, Y]
// basis, its sign such that the entry of largest magnitude is positive (the first of equals).
//
// The coefficients.  (N P V)_i carries an absolute error of eps |N| |P|, so c = (N P V)_i / (delta_i D) loses what
// delta_i is smaller than |N| |P|^2: a direction 1e-7 alpha off the bulk value keeps seven digits.  Since v_i lies in
// the range of P, the same vector is u_i = W P^+ v_i, c = P^+ v_i / D, which costs the condition of P instead -- nothing
// when the pairs are well separated, everything when two of them are nearly parallel, where the first form is exact to
// rounding.  Both are formed, and a direction takes the second only where its own residual is below a quarter of the
// first's (two residuals at the floor of their own rounding: the first form stays) -- the residual |W rho|, |W rho|^2
// = rho'G rho with rho = N G c - delta_i c (A u - lambda u = W rho), plus the defect of the norm |delta_i| |c'G c - 1|,
// measured on the scaled matrices: multiplications by G only, replicated host data, the same choice on every rank.
// Many pairs of one run make the scaled G numerically singular (cond 1e16 at 33 pairs) and N as large as G is small:
// then neither form resolves a direction to 1e-10 even at delta_i = 1e-2 alpha.  So every direction more than 100 cuts
// off the bulk value takes one step of inverse iteration on M = N G, whose eigenvector for delta_i holds the
// coefficients of u_i: delta_i is known to rounding, the step divides what the chosen form has of other directions
// by their distance to delta_i, and it needs G as a matrix only (its absolute error, not its small eigenvalues).
// Closer to the bulk value the step cannot tell the direction from the bulk (M's eigenvalue 0) and only adds its
// own rounding to the norm: those directions stay as chosen.
// W has rank <= rmax (its rows over all ranks): should more directions pass the cut, those of the smallest |delta|
// go to the bulk as well.  lam: d doubles, coef: d^2 doubles, work: 7 d^2 + 6 d doubles.  Returns 0, -1 or -2 as
// qn_root; *r = 0 then.
inline int qn_eig(int d, double alpha, double cut, int64_t rmax, const double *g, const double *n_, int *r,
                  double *lam, double *coef, double *work) {
  *r = 0;
  if (d == 0) return 0;
  const size_t dd = (size_t)d * d;
  const double *a = work, *v = work + dd, *w = work + 5 * dd, *nn = work + 5 * dd + d;
  double *ds = work + 6 * dd + d, *keep = work + 6 * dd + 2 * d, *tmp = work + 7 * dd + 3 * d;
  if (qn_spectrum(d, g, n_, ds, work, true, keep) < 0) return -1;
  for (int i = 0; i < d; ++i)
    if (alpha + w[i] < -1e-8 * alpha) return -2;
  int idx[2 * 1024];
  int cnt = 0;
  for (int i = 0; i < d; ++i)
    if (std::fabs(w[i]) > cut * alpha) idx[cnt++] = i;
  while (cnt > rmax) {
    int lo = 0;
    for (int j = 1; j < cnt; ++j)
      if (std::fabs(w[idx[j]]) < std::fabs(w[idx[lo]])) lo = j;
    for (int j = lo; j + 1 < cnt; ++j) idx[j] = idx[j + 1];
    --cnt;
  }
  std::stable_sort(idx, idx + cnt, [&](int x, int y) { return w[x] < w[y]; });
  const double *ug = keep, *rg = keep + dd;  // the scaled G = ug diag(rg^2) ug'
  double *c1 = tmp, *c2 = tmp + d, *t1 = tmp + 2 * d;
  // the defect of a candidate c (scaled basis) for delta: sqrt(rho'G rho) + |c'G c - 1|, G and N the scaled ones
  auto gmul = [&](const double *x, double *o) {  // o = G x through its factors
    for (int k = 0; k < d; ++k) {
      double s = 0.0;
      for (int i = 0; i < d; ++i) s = s + ug[i + (size_t)k * d] * x[i];
      t1[k] = s * (rg[k] * rg[k]);
    }
    for (int i = 0; i < d; ++i) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = s + ug[i + (size_t)k * d] * t1[k];
      o[i] = s;
    }
  };
  std::vector<double> gc((size_t)d), rho((size_t)d), grho((size_t)d);
  auto defect = [&](const double *c, double delta) {
    gmul(c, gc.data());
    double nrm = 0.0;
    for (int i = 0; i < d; ++i) nrm = nrm + c[i] * gc[(size_t)i];
    for (int i = 0; i < d; ++i) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = s + nn[i + (size_t)k * d] * gc[(size_t)k];
      rho[(size_t)i] = s - delta * c[i];
    }
    gmul(rho.data(), grho.data());
    double q = 0.0;
    for (int i = 0; i < d; ++i) q = q + rho[(size_t)i] * grho[(size_t)i];
    return std::sqrt(std::max(q, 0.0)) + std::fabs(nrm - 1.0) * std::fabs(delta);
  };
  // One step of inverse iteration on M = N G (scaled; M c = delta c for the coefficients of an eigenvector, the bulk
  // at M's eigenvalue 0) from the chosen form x: o = (M - delta I)^-1 x, scaled to o'G o = 1.  G here is the scaled
  // Gram itself, not its clipped factors; LU with partial pivoting.  false, o undefined: a zero pivot or a result
  // that is not finite.  (o may be x)
  std::vector<double> gt(dd), mm(dd), lu(dd);
  for (int q = 0; q < d; ++q)
    for (int p = 0; p < d; ++p) gt[p + (size_t)q * d] = g[p + (size_t)q * d] / (ds[p] * ds[q]);
  for (int q = 0; q < d; ++q)
    for (int p = 0; p < d; ++p) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = s + nn[p + (size_t)k * d] * gt[k + (size_t)q * d];
      mm[p + (size_t)q * d] = s;
    }
  auto refine = [&](const double *x, double delta, double *o) {
    lu = mm;
    for (int p = 0; p < d; ++p) lu[p + (size_t)p * d] -= delta;
    std::vector<double> b(x, x + d);
    for (int k = 0; k < d; ++k) {
      int piv = k;
      for (int p = k + 1; p < d; ++p)
        if (std::fabs(lu[p + (size_t)k * d]) > std::fabs(lu[piv + (size_t)k * d])) piv = p;
      if (lu[piv + (size_t)k * d] == 0.0) return false;
      if (piv != k) {
        for (int q = 0; q < d; ++q) std::swap(lu[k + (size_t)q * d], lu[piv + (size_t)q * d]);
        std::swap(b[(size_t)k], b[(size_t)piv]);
      }
      for (int p = k + 1; p < d; ++p) {
        const double f = lu[p + (size_t)k * d] / lu[k + (size_t)k * d];
        if (f == 0.0) continue;
        for (int q = k + 1; q < d; ++q) lu[p + (size_t)q * d] -= f * lu[k + (size_t)q * d];
        b[(size_t)p] -= f * b[(size_t)k];
      }
    }
    for (int k = d - 1; k >= 0; --k) {
      double s = b[(size_t)k];
      for (int q = k + 1; q < d; ++q) s = s - lu[k + (size_t)q * d] * b[(size_t)q];
      b[(size_t)k] = s / lu[k + (size_t)k * d];
    }
    double big = 0.0;  // (the solution is as long as the shift is close: scale before the norm)
    for (int k = 0; k < d; ++k) big = std::max(big, std::fabs(b[(size_t)k]));
    if (!(big > 0.0) || !std::isfinite(big)) return false;
    for (int k = 0; k < d; ++k) b[(size_t)k] = b[(size_t)k] / big;
    double nrm = 0.0;
    for (int p = 0; p < d; ++p) {
      double s = 0.0;
      for (int q = 0; q < d; ++q) s = s + gt[p + (size_t)q * d] * b[(size_t)q];
      nrm = nrm + b[(size_t)p] * s;
    }
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return false;
    nrm = std::sqrt(nrm);
    for (int k = 0; k < d; ++k) o[k] = b[(size_t)k] / nrm;
    return true;
  };
  for (int j = 0; j < cnt; ++j) {
    const int i = idx[j];
    lam[j] = alpha + w[i];
    for (int k = 0; k < d; ++k) c1[k] = a[k + (size_t)i * d] / w[i];
    for (int k = 0; k < d; ++k) {  // P^+ v_i = ug diag(1 / rg) ug' v_i over the kept directions
      double s = 0.0;
      for (int l = 0; l < d; ++l) s = s + ug[l + (size_t)k * d] * v[l + (size_t)i * d];
      t1[k] = rg[k] > 0.0 ? s / rg[k] : 0.0;
    }
    for (int k = 0; k < d; ++k) {
      double s = 0.0;
      for (int l = 0; l < d; ++l) s = s + ug[k + (size_t)l * d] * t1[l];
      c2[k] = s;
    }
    double *c = coef + (size_t)j * d;
    const double *best = defect(c2, w[i]) < 0.25 * defect(c1, w[i]) ? c2 : c1;
    if (std::fabs(w[i]) > 100.0 * cut * alpha && refine(best, w[i], c1)) best = c1;
    int big = 0;
    for (int k = 0; k < d; ++k) {
      c[k] = best[k] / ds[k];
      if (std::fabs(c[k]) > std::fabs(c[big])) big = k;
    }
    if (c[big] < 0.0)
      for (int k = 0; k < d; ++k) c[k] = -c[k];
  }
  *r = cnt;
  return 0;
}

// ---- a curvature model of the caller's own (lbfgsb_hip_qn_pairs_set / _push, solver_qn_pairs.inl) ----
// The m x m matrices the operators read, from the Grams of col loaded pairs (col x col, column-major, logical order:
// sts[i + j col] = s_i's_j, sty[i + j col] = s_i'y_j, yty likewise): sy = the lower triangle and diagonal of S'Y, ss =
// the upper triangle of S'S as matupd keeps them (reference src/lbfgsb.f90:2311-2340), theta = theta_in when that is
// > 0, else y'y / s'y of the newest pair (:2318; needs col >= 1), then wt by formt (:1926-1963).  Returns 0; j + 1
// when s_j'y_j is not finite or not positive (no pair is stored without s'y > 0, :820-826); -1 for theta_in = 0
// without a pair; -3 when formt fails.  sy, ss and wt are written in every case.
inline int qn_pairs_factor(int m, int col, const double *sts, const double *sty, const double *yty, double theta_in,
                           double *sy_, double *ss_, double *wt_, double *theta) {
  Mat sy{sy_, m}, ss{ss_, m};
  for (int j = 0; j < col; ++j)
    for (int i = 0; i < col; ++i) {
      if (i >= j) sy(i, j) = sty[i + (size_t)j * col];
      if (i <= j) ss(i, j) = sts[i + (size_t)j * col];
    }
  for (int j = 0; j < col; ++j)
    if (!std::isfinite(sy(j, j)) || !(sy(j, j) > 0.0)) return j + 1;
  if (theta_in > 0.0) {
    *theta = theta_in;
  } else {
    if (col < 1) return -1;
    *theta = yty[(size_t)(col - 1) * (col + 1)] / sy(col - 1, col - 1);
  }
  return formt(m, wt_, sy_, ss_, col, *theta);
}

// matupd's host part for one appended pair (s, y) (reference src/lbfgsb.f90:2303-2340), from the sums alone: the
// pointer update (:2303-2309; a full ring drops the oldest pair), the shift of Ss and Sy once the memory is full
// (:2324-2330), Sy's new row s'y_j and Ss's new column s_j's over the pairs that stay, oldest first (:2333-2338),
// the two diagonal entries (:2339-2344), theta = y'y / s'y (:2318) unless theta_in > 0, then formt (:849).  s_old,
// y_old: s_j's and y_j's for the col pairs stored BEFORE the call, oldest first.  Returns formt's info.
inline int qn_pairs_append(int m, int &col, int &head, int &itail, double *sy_, double *ss_, double *wt_,
                           double &theta, const double *s_old, const double *y_old, double sts, double sty, double yty,
                           double theta_in) {
  Mat sy{sy_, m}, ss{ss_, m};
  const bool full = col == m;
  if (!full) {
    col = col + 1;
    itail = (head + col - 2) % m + 1;
  } else {
    itail = itail % m + 1;
    head = head % m + 1;
  }
  theta = theta_in > 0.0 ? theta_in : yty / sty;
  if (full)
    for (int j = 0; j < col - 1; ++j) {
      for (int i = 0; i <= j; ++i) ss(i, j) = ss(i + 1, j + 1);
      for (int i = j; i < col - 1; ++i) sy(i, j) = sy(i + 1, j + 1);
    }
  const int drop = full ? 1 : 0;  // (the sums against the pair that leaves are not used)
  for (int j = 0; j < col - 1; ++j) {
    sy(col - 1, j) = y_old[j + drop];
    ss(j, col - 1) = s_old[j + drop];
  }
  ss(col - 1, col - 1) = sts;
  sy(col - 1, col - 1) = sty;
  return formt(m, wt_, sy_, ss_, col, theta);
}

// The same step on a full Gram g (colold x colold, column-major, logical order) of the operators' cache: the oldest
// pair's row and column leave when the ring was full, then the new pair's column cnew[i] = (pair i)'(new), its row
// rnew[i] = (new)'(pair i) and the diagonal entry, for the colold pairs stored before, oldest first.
inline void qn_gram_append(int m, int colold, std::vector<double> &g, const double *cnew, const double *rnew,
                           double diag) {
  const int drop = colold == m ? 1 : 0, keep = colold - drop, col = keep + 1;
  std::vector<double> o((size_t)col * col, 0.0);
  for (int j = 0; j < keep; ++j)
    for (int i = 0; i < keep; ++i) o[i + (size_t)j * col] = g[(i + drop) + (size_t)(j + drop) * colold];
  for (int i = 0; i < keep; ++i) {
    o[i + (size_t)keep * col] = cnew[i + drop];
    o[keep + (size_t)i * col] = rnew[i + drop];
  }
  o[(size_t)keep * (col + 1)] = diag;
  g.swap(o);
}

// ---- 60-byte blank padded strings (Fortran character(len=60)) ----
inline void str60_set(char *t, const char *s) {
  size_t k = std::strlen(s);
  if (k > 60) k = 60;
  std::memcpy(t, s, k);
  std::memset(t + k, ' ', 60 - k);
}
inline bool str60_pre(const char *t, const char *s) { return std::strncmp(t, s, std::strlen(s)) == 0; }
inline bool str60_eq(const char *t, const char *s) {
  size_t k = std::strlen(s);
  if (std::strncmp(t, s, k) != 0) return false;
  for (size_t i = k; i < 60; ++i)
    if (t[i] != ' ') return false;
  return true;
}

// ---- More'-Thuente line search (MINPACK-2) ----
inline void dcstep(double &stx, double &fx, double &dx, double &sty, double &fy, double &dy,
                   double &stp, double fp, double dp, bool &brackt, double stpmin,
                   double stpmax) {
  const double p66 = 0.66;
  double gamma, p, q, r, s, stpc, stpf, stpq, theta;
  const double sgnd = dp * (dx / std::fabs(dx));
  auto max3 = [](double a, double b, double c) { return std::max(std::max(a, b), c); };
  auto sq = [](double a) { return a * a; };

  if (fp > fx) {
    theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    s = max3(std::fabs(theta), std::fabs(dx), std::fabs(dp));
    gamma = s * std::sqrt(sq(theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    p = (gamma - dx) + theta;
    q = ((gamma - dx) + gamma) + dp;
    r = p / q;
    stpc = stx + r * (stp - stx);
    stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
    stpf = std::fabs(stpc - stx) < std::fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
    brackt = true;
  } else if (sgnd < 0.0) {
    theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    s = max3(std::fabs(theta), std::fabs(dx), std::fabs(dp));
    gamma = s * std::sqrt(sq(theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    p = (gamma - dp) + theta;
    q = ((gamma - dp) + gamma) + dx;
    r = p / q;
    stpc = stp + r * (stx - stp);
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    stpf = std::fabs(stpc - stp) > std::fabs(stpq - stp) ? stpc : stpq;
    brackt = true;
  } else if (std::fabs(dp) < std::fabs(dx)) {
    theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    s = max3(std::fabs(theta), std::fabs(dx), std::fabs(dp));
    gamma = s * std::sqrt(std::max(0.0, sq(theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    p = (gamma - dp) + theta;
    q = (gamma + (dx - dp)) + gamma;
    r = p / q;
    if (r < 0.0 && gamma != 0.0)
      stpc = stp + r * (stx - stp);
    else if (stp > stx)
      stpc = stpmax;
    else
      stpc = stpmin;
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      stpf = std::fabs(stpc - stp) < std::fabs(stpq - stp) ? stpc : stpq;
      if (stp > stx)
        stpf = std::min(stp + p66 * (sty - stp), stpf);
      else
        stpf = std::max(stp + p66 * (sty - stp), stpf);
    } else {
      stpf = std::fabs(stpc - stp) > std::fabs(stpq - stp) ? stpc : stpq;
      stpf = std::min(stpmax, stpf);
      stpf = std::max(stpmin, stpf);
    }
  } else {
    if (brackt) {
      theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
      s = max3(std::fabs(theta), std::fabs(dy), std::fabs(dp));
      gamma = s * std::sqrt(sq(theta / s) - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      p = (gamma - dp) + theta;
      q = ((gamma - dp) + gamma) + dy;
      r = p / q;
      stpc = stp + r * (sty - stp);
      stpf = stpc;
    } else if (stp > stx) {
      stpf = stpmax;
    } else {
      stpf = stpmin;
    }
  }
  if (fp > fx) {
    sty = stp;
    fy = fp;
    dy = dp;
  } else {
    if (sgnd < 0.0) {
      sty = stx;
      fy = fx;
      dy = dx;
    }
    stx = stp;
    fx = fp;
    dx = dp;
  }
  stp = stpf;
}

// State lives in the caller's isave(43:44) / dsave(17:29) exactly as in the
// reference, so a reference-style caller can inspect or checkpoint it.
inline void dcsrch(double f, double g, double &stp, double ftol, double gtol, double xtol,
                   double stpmin, double stpmax, char *task, int32_t *isave, double *dsave) {
  const double p5 = 0.5, p66 = 0.66, xtrapl = 1.1, xtrapu = 4.0;
  bool brackt;
  int stage;
  double finit, ftest, fx, fy, ginit, gtest, gx, gy, stx, sty, stmin, stmax, width, width1;

  auto save = [&]() {
    isave[0] = brackt ? 1 : 0;
    isave[1] = stage;
    dsave[0] = ginit;
    dsave[1] = gtest;
    dsave[2] = gx;
    dsave[3] = gy;
    dsave[4] = finit;
    dsave[5] = fx;
    dsave[6] = fy;
    dsave[7] = stx;
    dsave[8] = sty;
    dsave[9] = stmin;
    dsave[10] = stmax;
    dsave[11] = width;
    dsave[12] = width1;
  };

  if (str60_pre(task, "START")) {
    if (stp < stpmin) str60_set(task, "ERROR: STP < STPMIN");
    if (stp > stpmax) str60_set(task, "ERROR: STP > STPMAX");
    if (g >= 0.0) str60_set(task, "ERROR: INITIAL G >= ZERO");
    if (ftol < 0.0) str60_set(task, "ERROR: FTOL < ZERO");
    if (gtol < 0.0) str60_set(task, "ERROR: GTOL < ZERO");
    if (xtol < 0.0) str60_set(task, "ERROR: XTOL < ZERO");
    if (stpmin < 0.0) str60_set(task, "ERROR: STPMIN < ZERO");
    if (stpmax < stpmin) str60_set(task, "ERROR: STPMAX < STPMIN");
    if (str60_pre(task, "ERROR")) return;
    brackt = false;
    stage = 1;
    finit = f;
    ginit = g;
    gtest = ftol * ginit;
    width = stpmax - stpmin;
    width1 = width / p5;
    stx = 0.0;
    fx = finit;
    gx = ginit;
    sty = 0.0;
    fy = finit;
    gy = ginit;
    stmin = 0.0;
    stmax = stp + xtrapu * stp;
    str60_set(task, "FG");
    save();
    return;
  }
  brackt = isave[0] == 1;
  stage = isave[1];
  ginit = dsave[0];
  gtest = dsave[1];
  gx = dsave[2];
  gy = dsave[3];
  finit = dsave[4];
  fx = dsave[5];
  fy = dsave[6];
  stx = dsave[7];
  sty = dsave[8];
  stmin = dsave[9];
  stmax = dsave[10];
  width = dsave[11];
  width1 = dsave[12];

  ftest = finit + stp * gtest;
  if (stage == 1 && f <= ftest && g >= 0.0) stage = 2;

  if (brackt && (stp <= stmin || stp >= stmax))
    str60_set(task, "WARNING: ROUNDING ERRORS PREVENT PROGRESS");
  if (brackt && stmax - stmin <= xtol * stmax) str60_set(task, "WARNING: XTOL TEST SATISFIED");
  if (stp == stpmax && f <= ftest && g <= gtest) str60_set(task, "WARNING: STP = STPMAX");
  if (stp == stpmin && (f > ftest || g >= gtest)) str60_set(task, "WARNING: STP = STPMIN");
  if (f <= ftest && std::fabs(g) <= gtol * (-ginit)) str60_set(task, "CONVERGENCE");
  if (str60_pre(task, "WARN") || str60_pre(task, "CONV")) {
    save();
    return;
  }

  if (stage == 1 && f <= fx && f > ftest) {
    double fm = f - stp * gtest, fxm = fx - stx * gtest, fym = fy - sty * gtest;
    double gm = g - gtest, gxm = gx - gtest, gym = gy - gtest;
    dcstep(stx, fxm, gxm, sty, fym, gym, stp, fm, gm, brackt, stmin, stmax);
    fx = fxm + stx * gtest;
    fy = fym + sty * gtest;
    gx = gxm + gtest;
    gy = gym + gtest;
  } else {
    dcstep(stx, fx, gx, sty, fy, gy, stp, f, g, brackt, stmin, stmax);
  }
  if (brackt) {
    if (std::fabs(sty - stx) >= p66 * width1) stp = stx + p5 * (sty - stx);
    width1 = width;
    width = std::fabs(sty - stx);
  }
  if (brackt) {
    stmin = std::min(stx, sty);
    stmax = std::max(stx, sty);
  } else {
    stmin = stp + xtrapl * (stp - stx);
    stmax = stp + xtrapu * (stp - stx);
  }
  stp = std::max(stp, stpmin);
  stp = std::min(stp, stpmax);
  if ((brackt && (stp <= stmin || stp >= stmax)) || (brackt && stmax - stmin <= xtol * stmax))
    stp = stx;
  str60_set(task, "FG");
  save();
}

// hpsolb (src/lbfgsb.f90:2079-2157): t(1:n) / iorder(1:n) hold the breakpoints not yet used.
// iheap == 0: first rearrange them into a min-heap by sifting t(2), t(3), ... up; then move the
// least element to t(n) and restore the heap on t(1:n-1).  Used by the replay of the reference's
// pop order among EQUAL breakpoints (a walk that ends inside a tie group, solver.hip exact_init);
// arrays are 0-based here, i and j keep the reference's 1-based meaning.  I = the type of the row
// numbers (uint32_t while n_global < 2^32, int64_t beyond).
template <typename I>
inline void hpsolb(int64_t n, double *t, I *iorder, int iheap) {
  if (iheap == 0) {
    for (int64_t k = 2; k <= n; ++k) {
      const double ddum = t[k - 1];
      const I indxin = iorder[k - 1];
      int64_t i = k;
      while (i > 1) {
        const int64_t j = i / 2;
        if (!(ddum < t[j - 1])) break;
        t[i - 1] = t[j - 1];
        iorder[i - 1] = iorder[j - 1];
        i = j;
      }
      t[i - 1] = ddum;
      iorder[i - 1] = indxin;
    }
  }
  if (n > 1) {
    int64_t i = 1;
    const double out = t[0];
    const I indxou = iorder[0];
    const double ddum = t[n - 1];
    const I indxin = iorder[n - 1];
    for (;;) {
      int64_t j = i + i;
      if (j > n - 1) break;
      if (t[j] < t[j - 1]) j = j + 1;  // t(j+1) < t(j)
      if (!(t[j - 1] < ddum)) break;
      t[i - 1] = t[j - 1];
      iorder[i - 1] = iorder[j - 1];
      i = j;
    }
    t[i - 1] = ddum;
    iorder[i - 1] = indxin;
    t[n - 1] = out;
    iorder[n - 1] = indxou;
  }
}

}  // namespace lbh
