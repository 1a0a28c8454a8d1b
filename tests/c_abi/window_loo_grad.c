/* ISO C11 caller of the windows' leave-one-out objective (cgp_window_loo_grad_reserve, cgp_window_loo_nll_grad,
 * cgp_window_optimize_loo): one window of capacity 4, SE-ARD (id 1) and RBF x Brownian (id 2), d = 1.
 * After ONE pushed tick (x1, y), with kxx = k(x1, x1) and s = kxx + sigma_n^2 + 1e-8, the left-out prediction is the prior's:
 *   nlpd = log(2 pi s) / 2 + y^2 / (2 s),     G = dnlpd / ds = 1 / (2 s) - y^2 / (2 s^2)
 *   dnlpd / dsigma_n^2 = G,  dnlpd / dell = 0,  SE-ARD: dnlpd / dsigma_f^2 = G;  RBF x Brownian (kxx = th0 th2 |x1|): G th2 |x1| and G th0 |x1|
 * and logml = -nlpd (one sample: the two objectives coincide).  After three more ticks nlpd is cgp_window_loo's lpd_sum negated,
 * bit for bit, logml = NULL leaves nlpd and the gradient as they are, and the optimiser does not lower lpd_sum. */
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
  const double x[4] = {5.0, 6.0, 7.0, 8.5}, y[4] = {0.7, 0.45, 0.5, 0.1};
  const double noise = th[nth - 1];
  double nlpd, grad[MAXTH], logml, wnlpd, wgrad[MAXTH], wlogml, pm[4], pv[4], lm[4], nlpd2, grad2[MAXTH], tot, theta[MAXTH], best;
  int nev = 0;
  CHECK(cgp_window_init(ctx, 1, 4, 1, kid, th, nth));
  if (cgp_window_loo_nll_grad(ctx, &nlpd, grad, nth, &logml) != CGP_ESTATE ||
      cgp_window_optimize_loo(ctx, 10, NULL, NULL, 0, NULL, NULL) != CGP_ESTATE) {
    fprintf(stderr, "calls without the reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_loo_grad_reserve(ctx));
  if (cgp_window_loo_nll_grad(ctx, NULL, grad, nth, &logml) != CGP_EINVAL ||
      cgp_window_loo_nll_grad(ctx, &nlpd, NULL, nth, &logml) != CGP_EINVAL ||
      cgp_window_loo_nll_grad(ctx, &nlpd, grad, nth - 1, &logml) != CGP_EINVAL) {
    fprintf(stderr, "a NULL nlpd or grad, grad_stride < ntheta must answer CGP_EINVAL\n");
    return 1;
  }
  /* the empty window */
  CHECK(cgp_window_loo_nll_grad(ctx, &nlpd, grad, nth, &logml));
  int ok = nlpd == 0.0 && logml == 0.0;
  for (int i = 0; i < nth; ++i) ok = ok && grad[i] == 0.0;
  if (!ok) {
    fprintf(stderr, "kernel %d: the empty window does not answer 0, a zero gradient and logml 0\n", kid);
    return 1;
  }
  /* one tick: the closed form */
  CHECK(cgp_window_push(ctx, 1, x, y, 0, pm, pv, lm));
  const double ax = fabs(x[0]);
  const double kxx = kid == CGP_KERNEL_SE_ARD ? th[0] : th[0] * th[2] * ax;
  const double s = kxx + noise + 1e-8, l2pi = log(2.0 * 3.14159265358979323846);
  wnlpd = 0.5 * (l2pi + log(s)) + 0.5 * y[0] * y[0] / s;
  wlogml = -wnlpd;
  const double G = 0.5 / s - 0.5 * y[0] * y[0] / (s * s);
  for (int i = 0; i < nth; ++i) wgrad[i] = 0.0;
  wgrad[0] = kid == CGP_KERNEL_SE_ARD ? G : G * th[2] * ax;
  if (kid == CGP_KERNEL_RBF_BROWNIAN) wgrad[2] = G * th[0] * ax;
  wgrad[nth - 1] = G;
  CHECK(cgp_window_loo_nll_grad(ctx, &nlpd, grad, nth, &logml));
  printf("kernel %d: nlpd %.17g grad %.17g %.17g %.17g logml %.17g\n", kid, nlpd, grad[0], grad[1], grad[nth - 1], logml);
  if (!(close_to("nlpd", &nlpd, &wnlpd, 1, 1e-9, 1.0) && close_to("grad", grad, wgrad, nth, 1e-9, fabs(G)) &&
        close_to("logml", &logml, &wlogml, 1, 1e-9, 1.0)))
    return 1;
  /* three more ticks */
  CHECK(cgp_window_push(ctx, 3, x + 1, y + 1, 0, pm, pv, lm));
  CHECK(cgp_window_loo_nll_grad(ctx, &nlpd, grad, nth, &logml));
  CHECK(cgp_window_loo_nll_grad(ctx, &nlpd2, grad2, nth, NULL));
  CHECK(cgp_window_loo(ctx, NULL, NULL, NULL, &tot));
  ok = nlpd == nlpd2 && nlpd == -tot && fabs(logml - lm[2]) <= 1e-9 * fmax(1.0, fabs(lm[2]));
  for (int i = 0; i < nth; ++i) ok = ok && grad[i] == grad2[i] && grad[i] == grad[i];
  if (!ok) {
    fprintf(stderr, "kernel %d: four ticks: nlpd %.17g / %.17g, lpd_sum %.17g, logml %.17g against the push's %.17g\n", kid, nlpd, nlpd2,
            tot, logml, lm[2]);
    return 1;
  }
  /* the optimiser runs and does not lower lpd_sum */
  CHECK(cgp_window_optimize_loo(ctx, 50, NULL, theta, nth, &best, &nev));
  if (!(best >= -nlpd - 1e-9) || nev < 1) {
    fprintf(stderr, "kernel %d: optimiser: lpd_sum %.17g after %d evaluations, start %.17g\n", kid, best, nev, -nlpd);
    return 1;
  }
  for (int i = 0; i < nth; ++i)
    if (!(theta[i] > 0.0)) {
      fprintf(stderr, "kernel %d: optimiser: theta[%d] = %.17g\n", kid, i, theta[i]);
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
  if (cgp_window_loo_grad_reserve(ctx) != CGP_ESTATE || cgp_window_loo_nll_grad(ctx, buf, buf, 4, buf) != CGP_ESTATE) {
    fprintf(stderr, "a call without windows must answer CGP_ESTATE\n");
    return 1;
  }
  if (run(ctx, CGP_KERNEL_SE_ARD, th_se, 3) || run(ctx, CGP_KERNEL_RBF_BROWNIAN, th_rb, 4)) return 1;
  cgp_destroy(ctx);
  printf("window_loo_grad.c ok\n");
  return 0;
}
