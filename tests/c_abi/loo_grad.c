/* ISO C11 caller of the leave-one-out objective: cgp_loo_grad_reserve, cgp_loo_nll_grad and cgp_loo_nll_grad_batch on closed forms
 * the file writes out itself, squared-exponential kernel, d = 1.
 *   N = 1: v = k(x, x) + sigma_n^2 + 1e-8,  nlpd = 1/2 log(2 pi v) + 1/2 y^2 / v,  d nlpd / dv = 1/2 / v - 1/2 y^2 / v^2 (the
 *          marginal likelihood's at N = 1); sigma_f^2 and sigma_n^2 both enter through v, the length-scale not at all.
 *   N = 2: Ky = [[c, b], [b, c]],  Ky^-1 = [[c, -b], [-b, c]] / (c^2 - b^2): loo_mean = (b yb / c, b ya / c), loo_var = c - b^2 / c,
 *          nlpd = -sum_i log N(y_i; loo_mean_i, loo_var); its gradient by central differences of that expression. */
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

static const double PI = 3.14159265358979323846;
static const double XS[2] = {0.1, 0.9}, YS[2] = {0.5, -0.2};

static int close_to(const char *what, const double *got, const double *want, int n, double tol) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(1.0, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

static double nlpd2(const double *th) {
  const double c = th[0] + th[2] + 1e-8, r = XS[0] - XS[1], b = th[0] * exp(-0.5 * r * r / (th[1] * th[1]));
  const double v = c - b * b / c, m0 = b * YS[1] / c, m1 = b * YS[0] / c;
  return log(2.0 * PI * v) + 0.5 * ((YS[0] - m0) * (YS[0] - m0) + (YS[1] - m1) * (YS[1] - m1)) / v;
}

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02};
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 2, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double nl = 0.0, g[3] = {0.0, 0.0, 0.0};
  if (cgp_loo_nll_grad(ctx, XS, YS, 2, 1, CGP_KERNEL_SE_ISO, theta, &nl, g) != CGP_ESTATE) {
    fprintf(stderr, "a context without the reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_loo_grad_reserve(ctx, 2));
  if (cgp_loo_nll_grad(ctx, XS, YS, 2, 1, CGP_KERNEL_SE_ISO, theta, NULL, g) != CGP_EINVAL) {
    fprintf(stderr, "a NULL output must answer CGP_EINVAL\n");
    return 1;
  }
  /* N = 1 */
  const double x1 = 0.3, y1 = 0.7, v = theta[0] + theta[2] + 1e-8;
  const double w1 = 0.5 * log(2.0 * PI * v) + 0.5 * y1 * y1 / v, dv = 0.5 / v - 0.5 * y1 * y1 / (v * v);
  const double wg1[3] = {dv, 0.0, dv};
  CHECK(cgp_loo_nll_grad(ctx, &x1, &y1, 1, 1, CGP_KERNEL_SE_ISO, theta, &nl, g));
  printf("N = 1: nlpd %.17g (expected %.17g) grad %.17g %.17g %.17g (expected %.17g 0 %.17g)\n", nl, w1, g[0], g[1], g[2], dv, dv);
  int ok = close_to("nlpd", &nl, &w1, 1, 1e-12) && close_to("grad", g, wg1, 3, 1e-12);
  /* N = 2 */
  const double w2 = nlpd2(theta);
  double wg2[3];
  for (int i = 0; i < 3; ++i) {
    double tp[3] = {theta[0], theta[1], theta[2]}, tm[3] = {theta[0], theta[1], theta[2]};
    const double h = 1e-6 * theta[i];
    tp[i] += h;
    tm[i] -= h;
    wg2[i] = (nlpd2(tp) - nlpd2(tm)) / (2.0 * h);
  }
  CHECK(cgp_loo_nll_grad(ctx, XS, YS, 2, 1, CGP_KERNEL_SE_ISO, theta, &nl, g));
  printf("N = 2: nlpd %.17g (expected %.17g) grad %.17g %.17g %.17g (expected %.17g %.17g %.17g)\n", nl, w2, g[0], g[1], g[2], wg2[0],
         wg2[1], wg2[2]);
  ok = ok && close_to("nlpd", &nl, &w2, 1, 1e-12) && close_to("grad", g, wg2, 3, 1e-7);
  double pm = 0.0, pv = 0.0;
  CHECK(cgp_predict(ctx, XS, 1, 1, &pm, &pv));   /* the context is left fitted */
  /* the batch of two such windows: the same bits twice, a strided gradient */
  const double X2[4] = {XS[0], XS[1], XS[0], XS[1]}, Y2[4] = {YS[0], YS[1], YS[0], YS[1]};
  const double th2[8] = {theta[0], theta[1], theta[2], -1.0, theta[0], theta[1], theta[2], -1.0};
  double nb[2], gb[10] = {7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0}, lm[2];
  int info[2] = {-1, -1};
  CHECK(cgp_loo_nll_grad_batch(ctx, 2, 2, 1, CGP_KERNEL_SE_ISO, X2, Y2, th2, 4, nb, gb, 5, lm, info));
  ok = ok && nb[0] == nb[1] && close_to("batch nlpd", nb, &w2, 1, 1e-12) && close_to("batch grad", gb, wg2, 3, 1e-7) &&
       close_to("batch grad", gb + 5, wg2, 3, 1e-7) && gb[3] == 7.0 && gb[4] == 7.0 && gb[8] == 7.0 && info[0] == 0 && info[1] == 0 &&
       lm[0] == lm[1] && isfinite(lm[0]);
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("loo_grad.c ok\n");
  return 0;
}
