/* ISO C11 caller of the predictive gradients: the N = 1 closed form through cgp_fit_predict_grad_batch (host buffers) and through
 * cgp_fit -> cgp_predict_gradients, squared-exponential kernel, d = 1.
 *   c = sigma_f^2 + sigma_n^2 + 1e-8,  k = sigma_f^2 exp(-(x* - x1)^2 / (2 ell^2)),  k' = dk/dx* = k (x1 - x*) / ell^2
 *   mean = k y / c,  var = sigma_f^2 - k^2 / c,  dmean = k' y / c,  dvar = -2 k k' / c;  both gradients vanish at x* = x1 */
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

#define M 3

static int close_to(const char *what, const double *got, const double *want, int n, double tol) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(1.0, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x[1] = {0.4}, y[1] = {0.7}, xs[M] = {0.4, 1.1, -0.3};
  const double c = theta[0] + theta[2] + 1e-8;
  double wmean[M], wvar[M], wdm[M], wdv[M];
  for (int m = 0; m < M; ++m) {
    const double k = theta[0] * exp(-0.5 * (xs[m] - x[0]) * (xs[m] - x[0]) / (theta[1] * theta[1]));
    const double kp = k * (x[0] - xs[m]) / (theta[1] * theta[1]);
    wmean[m] = k * y[0] / c;
    wvar[m] = theta[0] - k * k / c;
    wdm[m] = kp * y[0] / c;
    wdv[m] = -2.0 * k * kp / c;
  }
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double mean[M], var[M], dm[M], dv[M], logml = 0.0;
  int info = -1;
  if (cgp_fit_predict_grad_batch(ctx, 1, 1, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, var, &logml, &info, dm, dv) != CGP_ESTATE) {
    fprintf(stderr, "a call without a reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_pgrad_reserve(ctx, 1, 8));
  if (cgp_fit_predict_grad_batch(ctx, 1, 1, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, var, &logml, &info, NULL, NULL) != CGP_EINVAL) {
    fprintf(stderr, "both gradients NULL must answer CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_fit_predict_grad_batch(ctx, 1, 1, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, var, &logml, &info, dm, dv));
  printf("batch: dmean %.17g %.17g %.17g dvar %.17g %.17g %.17g\n", dm[0], dm[1], dm[2], dv[0], dv[1], dv[2]);
  int ok = info == 0 && close_to("mean", mean, wmean, M, 1e-9) && close_to("var", var, wvar, M, 1e-9) &&
           close_to("dmean", dm, wdm, M, 1e-9) && close_to("dvar", dv, wdv, M, 1e-9);
  ok = ok && dm[0] == 0.0 && dv[0] == 0.0;   /* x* = x1: the difference is an exact zero */
  double l2 = 0.0, dm2[M], dv2[M], m2[M], v2[M];
  CHECK(cgp_fit(ctx, x, y, 1, 1, CGP_KERNEL_SE_ISO, theta, &l2));
  CHECK(cgp_predict_gradients(ctx, xs, M, m2, v2, dm2, dv2));
  printf("single: dmean %.17g %.17g %.17g dvar %.17g %.17g %.17g\n", dm2[0], dm2[1], dm2[2], dv2[0], dv2[1], dv2[2]);
  ok = ok && close_to("single mean", m2, wmean, M, 1e-9) && close_to("single var", v2, wvar, M, 1e-9) &&
       close_to("single dmean", dm2, wdm, M, 1e-9) && close_to("single dvar", dv2, wdv, M, 1e-9) && dm2[0] == 0.0 && dv2[0] == 0.0;
  CHECK(cgp_predict_gradients(ctx, xs, M, NULL, NULL, NULL, dv2));   /* one gradient alone */
  ok = ok && close_to("dvar alone", dv2, wdv, M, 1e-9);
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("pgrad.c ok\n");
  return 0;
}
