// lbfgs.hpp -- unconstrained limited-memory BFGS (m = 10) with a strong-Wolfe line search, the
// role scipy.optimize.fmin_l_bfgs_b (no bounds) plays under GPy's `m.optimize()`
// (core_navigation/script/gp_slip_node.py:36; paramz 'lbfgsb': factr 1e7, pgtol 1e-5, maxfun 1000).
// Written as an ask/tell stepper so that many independent problems can share one batched objective
// evaluation per round; lbfgs_minimize drives a single stepper, lbfgs_minimize_logexp_batch a batch of
// them over positive parameters (cgp_optimize_batch, cgp_optimize_multi_batch, cgp_window_optimize).
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <memory>
#include <cstddef>
#include <vector>

#include "lbfgs_core.hpp"

namespace corenav {

struct LbfgsResult {
  double f = 0.0;
  int evals = 0, iters = 0;
  int status = 0;  // 0 converged (gradient), 1 converged (function decrease), 2 max evals, 3 line search failed
};

// vector-facing wrapper of LbfgsCore (lbfgs_core.hpp: the state machine itself, shared with the device optimiser)
constexpr int LB_NBIG = 4112;   // parameters of a problem with free coordinates: CGP_MAX_THETA + 512 inducing inputs x 8 dimensions
class LbfgsStepper {
 public:
  LbfgsStepper(const std::vector<double> &x0, int max_evals, double pgtol, double factr) : xn_(x0), x_(x0) {
    if ((int)x0.size() > LB_N) {
      big_.reset(new LbfgsCoreT<LB_NBIG>());
      big_->init(x0.data(), (int)x0.size(), max_evals, pgtol, factr);
    } else {
      c_.init(x0.data(), (int)x0.size(), max_evals, pgtol, factr);
    }
  }

  bool done() const { return big_ ? big_->done() : c_.done(); }
  const std::vector<double> &trial() const { return xn_; }  // the point to evaluate next
  const std::vector<double> &best() const { return x_; }
  LbfgsResult result() const { return big_ ? result_of(*big_) : result_of(c_); }

  // Feed f(trial()) and its gradient.  Non-finite f marks an infeasible point.
  void tell(double fv, const std::vector<double> &gv) {
    if (big_) tell_to(*big_, fv, gv);
    else tell_to(c_, fv, gv);
  }

 private:
  template <class C> static LbfgsResult result_of(const C &c) {
    LbfgsResult r;
    r.f = c.f;
    r.evals = c.evals;
    r.iters = c.iters;
    r.status = c.status;
    return r;
  }
  template <class C> void tell_to(C &c, double fv, const std::vector<double> &gv) {
    c.tell(fv, gv.data());
    std::copy(c.xn, c.xn + c.n, xn_.begin());
    std::copy(c.x, c.x + c.n, x_.begin());
  }
  LbfgsCore c_;
  std::unique_ptr<LbfgsCoreT<LB_NBIG>> big_;   // more than LB_N parameters
  std::vector<double> xn_, x_;
};

// fg(x, grad) -> f.  Returns non-finite f to signal an infeasible point (treated as +inf).
inline LbfgsResult lbfgs_minimize(const std::function<double(const std::vector<double> &, std::vector<double> &)> &fg,
                                  std::vector<double> &x, int max_evals = 1000, double pgtol = 1e-5,
                                  double factr = 1e7) {
  LbfgsStepper st(x, max_evals, pgtol, factr);
  std::vector<double> g(x.size());
  while (!st.done()) {
    const double f = fg(st.trial(), g);
    st.tell(f, g);
  }
  x = st.best();
  return st.result();
}

// Logexp transform of a positive parameter (GPy paramz.transformations.Logexp): theta = log(1 + exp(x)), its inverse,
// and dtheta/dx = 1 - exp(-theta)
inline double logexp_theta(double x) { return x > 35.0 ? x : std::log1p(std::exp(x)); }
inline double logexp_x(double th) { return th > 35.0 ? th : std::log(std::expm1(th)); }
inline double logexp_dtheta_dx(double x, double th) { return x > 35.0 ? 1.0 : -std::expm1(-th); }
// the theta an objective is evaluated at: never exactly zero
inline double logexp_theta_eval(double x) { return std::max(logexp_theta(x), 1e-300); }

struct LbfgsBatchResult {
  std::vector<double> theta;        // [n][nth] logexp_theta(best point) of a selected problem, theta0 of an unselected one
  std::vector<double> f;            // [n] the objective there
  std::vector<int> evals, status;   // [n] (LbfgsResult)
  std::vector<char> last_is_best;   // [n] the last point the problem was evaluated at is its best point
  int rounds = 0;                   // calls of the evaluation
};

// One evaluation of the whole batch: theta [n][nth] (a selected problem that has finished stands at its best point, an
// unselected one at its theta0) and active [n] in; f [n], the gradient with respect to theta [n][nth] and feasible [n] out,
// for the active problems only.  Returns 0, or a code that ends the run.
using LbfgsBatchEval = std::function<int(const double *theta, const char *active, double *f, double *grad, char *feasible)>;

// n independent minimisations over theta > 0 (npos parameters each, Logexp-transformed; pgtol 1e-5, factr 1e7) that share one
// evaluation per round: each selected problem is the lbfgs_minimize run of its own transformed objective, where an infeasible
// point counts as +inf.  select == nullptr selects every problem; theta0 of a selected problem must be positive.  Ends when
// no problem is active, after max_evals + 40 rounds at the latest (max_evals <= 0: 1000).  Returns 0 or eval's code.
// nfree > 0: every problem has nfree further coordinates after the positive ones that are optimised as they stand (the inducing
// inputs of cgp_optimize_sparse_batch); theta, the gradient and out.theta then hold npos + nfree entries per problem.
inline int lbfgs_minimize_logexp_batch(int n, int npos, const double *theta0, size_t theta_stride, const unsigned char *select,
                                       int max_evals, const LbfgsBatchEval &eval, LbfgsBatchResult &out, int nfree = 0) {
  const int cap = max_evals > 0 ? max_evals : 1000;
  const int nth = npos + nfree;   // coordinates of a problem: npos positive ones, then nfree untransformed ones
  auto sel = [&](int b) { return !select || select[b] != 0; };
  std::vector<LbfgsStepper> st;
  st.reserve(n);
  std::vector<double> x0(nth);
  for (int b = 0; b < n; ++b) {
    for (int i = 0; i < nth; ++i) x0[i] = !sel(b) ? 0.0 : (i < npos ? logexp_x(theta0[b * theta_stride + i]) : theta0[b * theta_stride + i]);
    st.emplace_back(x0, cap, 1e-5, 1e7);
  }
  const size_t nt = (size_t)n * nth;
  std::vector<double> th(nt), f(n, 0.0), g(nt, 0.0), gx(nth, 0.0);
  std::vector<char> active(n, 0), feasible(n, 0);
  out.last_is_best.assign(n, 1);
  out.rounds = 0;
  for (int round = 0; round < cap + 40; ++round) {
    bool any = false;
    for (int b = 0; b < n; ++b) {
      active[b] = sel(b) && !st[b].done();
      any = any || active[b];
      const std::vector<double> &xx = active[b] ? st[b].trial() : st[b].best();
      for (int i = 0; i < nth; ++i)
        th[(size_t)b * nth + i] = !sel(b) ? theta0[b * theta_stride + i] : (i < npos ? logexp_theta_eval(xx[i]) : xx[i]);
    }
    if (!any) break;
    const int rc = eval(th.data(), active.data(), f.data(), g.data(), feasible.data());
    if (rc != 0) return rc;
    ++out.rounds;
    for (int b = 0; b < n; ++b) {
      if (!active[b]) continue;
      const std::vector<double> xt = st[b].trial();
      const double *tb = th.data() + (size_t)b * nth, *gb = g.data() + (size_t)b * nth;
      double fv = INFINITY;   // tell() gives an infeasible point a zero gradient itself
      if (feasible[b]) {
        for (int i = 0; i < nth; ++i) gx[i] = i < npos ? gb[i] * logexp_dtheta_dx(xt[i], tb[i]) : gb[i];
        fv = f[b];
      }
      st[b].tell(fv, gx);
      out.last_is_best[b] = st[b].best() == xt;
    }
  }
  out.theta.resize(nt);
  out.f.assign(n, 0.0);
  out.evals.assign(n, 0);
  out.status.assign(n, 0);
  for (int b = 0; b < n; ++b) {
    const std::vector<double> &xb = st[b].best();
    for (int i = 0; i < nth; ++i)
      out.theta[(size_t)b * nth + i] = !sel(b) ? theta0[b * theta_stride + i] : (i < npos ? logexp_theta(xb[i]) : xb[i]);
    if (!sel(b)) continue;
    const LbfgsResult r = st[b].result();
    out.f[b] = r.f;
    out.evals[b] = r.evals;
    out.status[b] = r.status;
  }
  return 0;
}

}  // namespace corenav
