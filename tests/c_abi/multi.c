/* ISO C11 caller of the multi-target fits (cgp_multi_reserve, cgp_fit_predict_multi_batch), squared-exponential kernel, d = 1.
 *   N = 1 closed form:  mean[p] = k* / (k + sigma_n^2 + 1e-8) y_p,  k = sigma_f^2,  k* = sigma_f^2 exp(-(x - xs)^2 / (2 ell^2));
 *                       var = k + sigma_n^2 - k*^2 / (k + sigma_n^2 + 1e-8);  logml[p] = -y_p^2 / (2 c) - log(c) / 2 - log(2 pi) / 2
 *   linearity:          column 2 = column 0 + column 1 gives mean_2 = mean_0 + mean_1 to 1e-12 of its scale (the factor is shared) */
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

#define N2 9
#define M2 5

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x = 0.1, xs[2] = {0.4, -0.3}, y[3] = {0.5, -0.2, 0.3};
  const double pi = 3.14159265358979323846;
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double mean[3 * M2], var[M2], logml[3];
  int info = -1;
  if (cgp_fit_predict_multi_batch(ctx, 1, 1, 1, 2, 3, CGP_KERNEL_SE_ISO, &x, y, xs, theta, 3, 1, mean, var, logml, &info) != CGP_ESTATE) {
    fprintf(stderr, "a context without a reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_multi_reserve(ctx, 1, 3));
  if (cgp_fit_predict_multi_batch(ctx, 1, 1, 1, 2, 4, CGP_KERNEL_SE_ISO, &x, y, xs, theta, 3, 1, mean, var, logml, &info) != CGP_ECAPACITY) {
    fprintf(stderr, "P beyond the reservation must answer CGP_ECAPACITY\n");
    return 1;
  }
  CHECK(cgp_fit_predict_multi_batch(ctx, 1, 1, 1, 2, 3, CGP_KERNEL_SE_ISO, &x, y, xs, theta, 3, 1, mean, var, logml, &info));
  const double c = theta[0] + theta[2] + 1e-8;
  int ok = info == 0;
  for (int m = 0; m < 2; ++m) {
    const double ks = theta[0] * exp(-0.5 * (x - xs[m]) * (x - xs[m]) / (theta[1] * theta[1]));
    const double wv = theta[0] + theta[2] - ks * ks / c;
    printf("test point %d: var %.17g (expected %.17g)\n", m, var[m], wv);
    ok = ok && fabs(var[m] - wv) <= 1e-9 * wv;
    for (int p = 0; p < 3; ++p) {
      const double wm = ks / c * y[p];
      printf("  mean[%d] %.17g (expected %.17g)\n", p, mean[p * 2 + m], wm);
      ok = ok && fabs(mean[p * 2 + m] - wm) <= 1e-9 * fmax(1.0, fabs(wm));
    }
  }
  for (int p = 0; p < 3; ++p) {
    const double wl = -0.5 * y[p] * y[p] / c - 0.5 * log(c) - 0.5 * log(2.0 * pi);
    printf("logml[%d] %.17g (expected %.17g)\n", p, logml[p], wl);
    ok = ok && fabs(logml[p] - wl) <= 1e-9 * fmax(1.0, fabs(wl));
  }
  /* linearity in the targets: nine samples, five test points, column 2 = column 0 + column 1 */
  double X[N2], Y[3 * N2], Xs[M2];
  for (int i = 0; i < N2; ++i) {
    X[i] = 0.25 * i;
    Y[i] = sin(1.3 * X[i]);
    Y[N2 + i] = 0.4 * cos(2.1 * X[i]) - 0.1;
    Y[2 * N2 + i] = Y[i] + Y[N2 + i];
  }
  for (int m = 0; m < M2; ++m) Xs[m] = 0.11 + 0.4 * m;
  CHECK(cgp_fit_predict_multi_batch(ctx, 1, N2, 1, M2, 3, CGP_KERNEL_SE_ISO, X, Y, Xs, theta, 3, 0, mean, var, logml, NULL));
  double scale = 0.0;
  for (int m = 0; m < M2; ++m) scale = fmax(scale, fabs(mean[2 * M2 + m]));
  for (int m = 0; m < M2; ++m) {
    const double sum = mean[m] + mean[M2 + m];
    printf("mean_2[%d] %.17g  mean_0 + mean_1 %.17g\n", m, mean[2 * M2 + m], sum);
    ok = ok && fabs(mean[2 * M2 + m] - sum) <= 1e-12 * scale;
  }
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("multi.c ok\n");
  return 0;
}
