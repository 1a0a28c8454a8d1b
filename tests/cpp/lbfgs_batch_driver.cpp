// The batched L-BFGS driver of lbfgs.hpp against lbfgs_minimize: five analytic problems over theta > 0 in one batch (one of
// them unselected), chosen so that they finish in different rounds.  Every selected problem must be, bitwise, the run of
// lbfgs_minimize alone on its own Logexp-transformed objective.  Stand-alone: built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lbfgs.hpp"

using corenav::logexp_dtheta_dx;
using corenav::logexp_theta;
using corenav::logexp_theta_eval;
using corenav::logexp_x;

namespace {

constexpr int NTH = 4;   // the batch's parameter count; a problem of fewer variables ignores the rest (zero gradient)

struct Problem {
  int kind, nvar;   // 0 quadratic, 1 quartic, 2 wall
  double start[NTH];
};

// value and gradient in theta; false: infeasible
bool objective(const Problem &p, const double *th, double &f, double *g) {
  for (int i = 0; i < NTH; ++i) g[i] = 0.0;
  f = 0.0;
  if (p.kind == 0) {
    for (int i = 0; i < p.nvar; ++i) {
      const double c = 0.5 + i, w = 1.0 + 3.0 * i;
      f += w * (th[i] - c) * (th[i] - c);
      g[i] = 2.0 * w * (th[i] - c);
    }
  } else if (p.kind == 1) {
    for (int i = 0; i < p.nvar; ++i) {
      const double c = 2.0 - 0.5 * i, e = th[i] - c;
      f += e * e * e * e + 0.01 * e * e;
      g[i] = 4.0 * e * e * e + 0.02 * e;
    }
    f += th[0] * th[1];
    g[0] += th[1];
    g[1] += th[0];
  } else {   // the wall of tests/test_optimizer_cpu.py: "not positive definite even with jitter" beyond theta_0 = 2
    if (th[0] > 2.0) return false;
    for (int i = 0; i < p.nvar; ++i) {
      f += (th[i] - 1.5) * (th[i] - 1.5) + 0.1 * th[i] * th[i] * th[i] * th[i];
      g[i] = 2.0 * (th[i] - 1.5) + 0.4 * th[i] * th[i] * th[i];
    }
  }
  return true;
}

const Problem PROBLEMS[] = {
    {0, 2, {3.0, 0.2, 1.0, 1.0}},
    {1, 4, {0.3, 4.0, 0.7, 2.5}},
    {2, 3, {0.1, 0.5, 4.0, 1.0}},     // the wall, feasible start
    {0, 4, {9.0, 9.0, 9.0, 9.0}},     // unselected
    {2, 3, {5.0, 1.0, 1.0, 1.0}},     // the wall, infeasible start
};
constexpr int NP = sizeof(PROBLEMS) / sizeof(PROBLEMS[0]);
const unsigned char SELECT[NP] = {1, 1, 1, 0, 1};

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL %s: ", #cond);   \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

struct Alone {
  std::vector<double> theta, last_x, best_x;
  corenav::LbfgsResult r;
};

Alone run_alone(const Problem &p, int max_evals) {
  Alone a;
  std::vector<double> x(NTH), th(NTH), g(NTH);
  for (int i = 0; i < NTH; ++i) x[i] = logexp_x(p.start[i]);
  auto fg = [&](const std::vector<double> &xx, std::vector<double> &gx) -> double {
    a.last_x = xx;
    for (int i = 0; i < NTH; ++i) th[i] = logexp_theta_eval(xx[i]);
    double f;
    if (!objective(p, th.data(), f, g.data())) return INFINITY;
    for (int i = 0; i < NTH; ++i) gx[i] = g[i] * logexp_dtheta_dx(xx[i], th[i]);
    return f;
  };
  a.r = corenav::lbfgs_minimize(fg, x, max_evals > 0 ? max_evals : 1000);
  a.best_x = x;
  a.theta.resize(NTH);
  for (int i = 0; i < NTH; ++i) a.theta[i] = logexp_theta(x[i]);
  return a;
}

// returns the number of problems whose last evaluated point was not their best one
int run_case(int max_evals) {
  std::vector<double> theta0((size_t)NP * NTH);
  for (int b = 0; b < NP; ++b)
    for (int i = 0; i < NTH; ++i) theta0[(size_t)b * NTH + i] = PROBLEMS[b].start[i];
  std::vector<Alone> alone;
  for (int b = 0; b < NP; ++b) alone.push_back(run_alone(PROBLEMS[b], max_evals));

  int calls = 0;
  std::vector<int> seen(NP, 0);   // evaluations the callback was asked for, per problem
  auto eval = [&](const double *th, const char *active, double *f, double *g, char *feasible) -> int {
    ++calls;
    for (int b = 0; b < NP; ++b) {
      if (!active[b]) {
        if (!SELECT[b])
          for (int i = 0; i < NTH; ++i) CHECK(same_bits(th[(size_t)b * NTH + i], PROBLEMS[b].start[i]), "unselected theta moved (problem %d)", b);
        continue;
      }
      CHECK(SELECT[b], "unselected problem %d marked active", b);
      CHECK(seen[b] < alone[b].r.evals, "finished problem %d marked active (evaluation %d)", b, seen[b] + 1);
      ++seen[b];
      feasible[b] = objective(PROBLEMS[b], th + (size_t)b * NTH, f[b], g + (size_t)b * NTH);
    }
    return 0;
  };
  corenav::LbfgsBatchResult res;
  const int rc = corenav::lbfgs_minimize_logexp_batch(NP, NTH, theta0.data(), NTH, SELECT, max_evals, eval, res);
  CHECK(rc == 0, "rc %d", rc);
  CHECK(calls == res.rounds, "%d calls, %d rounds", calls, res.rounds);
  int longest = 0, not_best = 0, distinct = 0;
  for (int b = 0; b < NP; ++b) {
    if (!SELECT[b]) {
      for (int i = 0; i < NTH; ++i) CHECK(same_bits(res.theta[(size_t)b * NTH + i], PROBLEMS[b].start[i]), "unselected theta returned changed");
      CHECK(seen[b] == 0, "unselected problem evaluated");
      continue;
    }
    const Alone &a = alone[b];
    for (int i = 0; i < NTH; ++i)
      CHECK(same_bits(res.theta[(size_t)b * NTH + i], a.theta[i]), "problem %d theta[%d] %.17g != %.17g", b, i, res.theta[(size_t)b * NTH + i], a.theta[i]);
    CHECK(same_bits(res.f[b], a.r.f), "problem %d f %.17g != %.17g", b, res.f[b], a.r.f);
    CHECK(res.evals[b] == a.r.evals && seen[b] == a.r.evals, "problem %d evals %d / seen %d != %d", b, res.evals[b], seen[b], a.r.evals);
    CHECK(res.status[b] == a.r.status, "problem %d status %d != %d", b, res.status[b], a.r.status);
    const bool last_is_best = a.last_x == a.best_x;
    CHECK((res.last_is_best[b] != 0) == last_is_best, "problem %d last_is_best %d != %d", b, (int)res.last_is_best[b], (int)last_is_best);
    not_best += !last_is_best;
    longest = std::max(longest, a.r.evals);
    bool first = true;
    for (int o = 0; o < b; ++o) first = first && !(SELECT[o] && alone[o].r.evals == a.r.evals);
    distinct += first;
    std::printf("max_evals %d problem %d: evals %d status %d f %.6g last_is_best %d\n", max_evals, b, a.r.evals, a.r.status, a.r.f, (int)last_is_best);
  }
  CHECK(calls == longest, "the callback ran %d times for a longest run of %d evaluations", calls, longest);   // once per round
  if (max_evals <= 0) CHECK(distinct >= 3, "the problems finish in %d distinct rounds only", distinct);
  return not_best;
}

}  // namespace

int main() {
  int not_best = run_case(0);
  not_best += run_case(4);
  CHECK(not_best > 0, "no problem ended on a rejected trial: last_is_best is not exercised");
  if (failures) std::printf("%d checks failed\n", failures);
  else std::printf("ok\n");
  return failures ? 1 : 0;
}
