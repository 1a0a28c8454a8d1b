/* ISO C11 caller of the multi-target windows' summed objective (cgp_window_multi_grad_reserve, cgp_window_multi_nll_grad,
 * cgp_window_optimize_multi): one window of capacity 4, SE-ARD (id 1) and RBF x Brownian (id 2), d = 1.
 * After ONE pushed tick (x1; y_1 .. y_P), with kxx = k(x1, x1), kyy = kxx + sigma_n^2 + 1e-8 and S = sum_p y_p^2:
 *   nll = S / (2 kyy) + P log(kyy) / 2 + P log(2 pi) / 2,     G = dnll / dkyy = -S / (2 kyy^2) + P / (2 kyy)
 *   dnll / dsigma_n^2 = G,  dnll / dell = 0,  SE-ARD: dnll / dsigma_f^2 = G;  RBF x Brownian (kxx = th0 th2 |x1|): G th2 |x1| and G th0 |x1|
 * Linearity: with every column of Y present twice (P -> 2 P) nll and the gradient double, to rounding, after four ticks. */
#include <math.h>
#include <stdio.h>

#include "corenav_gp.h"

#define CHECK(call)                                                                      \
  do {                                                                                   \
    int rc_ = (call);                                                                    \
    if (rc_ != CGP_OK) {                                                                 \
      fprintf(stderr, "%s -> %d (%s)\n", #call, rc_, cgp_strerror(rc_));                 \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

#define P 3
#define MAXTH 4

static int close_to(const char *what, const double *got, const double *want, int n, double tol, double scale) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(scale, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

static int run(cgp_ctx *ctx, int kid, const double *th, int nth) {
  const double x[4] = {5.0, 6.0, 7.0, 8.5};
  const double noise = th[nth - 1];
  double Y[4][P], Y2[4][2 * P], nll, grad[MAXTH], logml[P], wnll, wgrad[MAXTH], wlogml[P], pm[4], pv[4], lm[4];
  double nll2, grad2[MAXTH], logml2[2 * P], theta[MAXTH], best;
  int nev = 0;
  for (int t = 0; t < 4; ++t) {
    Y[t][0] = 0.7 - 0.2 * t;
    Y[t][1] = -0.3 + 0.05 * t * t;
    Y[t][2] = 0.1 + 0.3 * t;
    for (int p = 0; p < 2 * P; ++p) Y2[t][p] = Y[t][p % P];
  }
  CHECK(cgp_window_init(ctx, 1, 4, 1, kid, th, nth));
  if (cgp_window_multi_grad_reserve(ctx) != CGP_ESTATE) {
    fprintf(stderr, "cgp_window_multi_grad_reserve before cgp_window_multi_reserve must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_multi_reserve(ctx, P));
  if (cgp_window_multi_nll_grad(ctx, P, &nll, grad, nth, logml) != CGP_ESTATE ||
      cgp_window_optimize_multi(ctx, P, 10, NULL, NULL, 0, NULL, NULL) != CGP_ESTATE) {
    fprintf(stderr, "calls without the objective's reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_multi_grad_reserve(ctx));
  if (cgp_window_multi_nll_grad(ctx, P + 1, &nll, grad, nth, logml) != CGP_EINVAL ||
      cgp_window_multi_nll_grad(ctx, P, NULL, grad, nth, logml) != CGP_EINVAL ||
      cgp_window_multi_nll_grad(ctx, P, &nll, NULL, nth, logml) != CGP_EINVAL ||
      cgp_window_multi_nll_grad(ctx, P, &nll, grad, nth - 1, logml) != CGP_EINVAL) {
    fprintf(stderr, "a wrong P, a NULL nll or grad, grad_stride < ntheta must answer CGP_EINVAL\n");
    return 1;
  }
  /* the empty window */
  CHECK(cgp_window_multi_nll_grad(ctx, P, &nll, grad, nth, logml));
  int ok = nll == 0.0;
  for (int i = 0; i < nth; ++i) ok = ok && grad[i] == 0.0;
  for (int p = 0; p < P; ++p) ok = ok && logml[p] == 0.0;
  if (!ok) {
    fprintf(stderr, "kernel %d: the empty window does not answer 0, a zero gradient and logml 0\n", kid);
    return 1;
  }
  /* one tick: the closed form */
  CHECK(cgp_window_push_multi(ctx, 1, P, x, &Y[0][0], 0, pm, pv, lm));
  const double ax = fabs(x[0]);
  const double kxx = kid == CGP_KERNEL_SE_ARD ? th[0] : th[0] * th[2] * ax;
  const double kyy = kxx + noise + 1e-8, l2pi = log(2.0 * 3.14159265358979323846);
  double S = 0.0;
  for (int p = 0; p < P; ++p) {
    S += Y[0][p] * Y[0][p];
    wlogml[p] = -0.5 * Y[0][p] * Y[0][p] / kyy - 0.5 * log(kyy) - 0.5 * l2pi;
  }
  wnll = 0.5 * S / kyy + 0.5 * P * log(kyy) + 0.5 * P * l2pi;
  const double G = -0.5 * S / (kyy * kyy) + 0.5 * P / kyy;
  for (int i = 0; i < nth; ++i) wgrad[i] = 0.0;
  wgrad[0] = kid == CGP_KERNEL_SE_ARD ? G : G * th[2] * ax;
  if (kid == CGP_KERNEL_RBF_BROWNIAN) wgrad[2] = G * th[0] * ax;
  wgrad[nth - 1] = G;
  CHECK(cgp_window_multi_nll_grad(ctx, P, &nll, grad, nth, logml));
  printf("kernel %d: nll %.17g grad %.17g %.17g %.17g\n", kid, nll, grad[0], grad[1], grad[nth - 1]);
  if (!(close_to("nll", &nll, &wnll, 1, 1e-9, 1.0) && close_to("grad", grad, wgrad, nth, 1e-9, fabs(G)) &&
        close_to("logml", logml, wlogml, P, 1e-9, 1.0)))
    return 1;
  /* three more ticks, logml may be NULL; then every column twice */
  CHECK(cgp_window_push_multi(ctx, 3, P, x + 1, &Y[1][0], 0, pm, pv, lm));
  CHECK(cgp_window_multi_nll_grad(ctx, P, &nll, grad, nth, NULL));
  /* the optimiser runs and does not lower the summed logML */
  CHECK(cgp_window_optimize_multi(ctx, P, 50, NULL, theta, nth, &best, &nev));
  if (!(best >= -nll - 1e-9) || nev < 1) {
    fprintf(stderr, "kernel %d: optimiser: sum logml %.17g after %d evaluations, start %.17g\n", kid, best, nev, -nll);
    return 1;
  }
  for (int i = 0; i < nth; ++i)
    if (!(theta[i] > 0.0)) {
      fprintf(stderr, "kernel %d: optimiser: theta[%d] = %.17g\n", kid, i, theta[i]);
      return 1;
    }
  CHECK(cgp_window_init(ctx, 1, 4, 1, kid, th, nth));
  CHECK(cgp_window_multi_reserve(ctx, 2 * P));
  CHECK(cgp_window_multi_grad_reserve(ctx));
  CHECK(cgp_window_push_multi(ctx, 4, 2 * P, x, &Y2[0][0], 0, pm, pv, lm));
  CHECK(cgp_window_multi_nll_grad(ctx, 2 * P, &nll2, grad2, nth, logml2));
  double scale = 0.0;
  for (int i = 0; i < nth; ++i) scale = fmax(scale, fabs(grad[i]));
  ok = fabs(nll2 - 2.0 * nll) <= 1e-12 * fmax(1.0, fabs(nll2));
  for (int i = 0; i < nth; ++i) ok = ok && fabs(grad2[i] - 2.0 * grad[i]) <= 1e-11 * 2.0 * scale;
  for (int p = 0; p < P; ++p) ok = ok && logml2[p] == logml2[p + P];
  if (!ok) {
    fprintf(stderr, "kernel %d: linearity: nll %.17g against 2 x %.17g, grad[0] %.17g against 2 x %.17g\n", kid, nll2, nll, grad2[0], grad[0]);
    return 1;
  }
  return 0;
}

int main(void) {
  const double th_se[3] = {0.8, 2.5, 0.02}, th_rb[4] = {0.5, 30.0, 0.01, 0.002};
  double buf[8];
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  if (cgp_window_multi_grad_reserve(ctx) != CGP_ESTATE || cgp_window_multi_nll_grad(ctx, P, buf, buf, 4, buf) != CGP_ESTATE) {
    fprintf(stderr, "a call without windows must answer CGP_ESTATE\n");
    return 1;
  }
  if (run(ctx, CGP_KERNEL_SE_ARD, th_se, 3) || run(ctx, CGP_KERNEL_RBF_BROWNIAN, th_rb, 4)) return 1;
  cgp_destroy(ctx);
  printf("window_multi_opt.c ok\n");
  return 0;
}
