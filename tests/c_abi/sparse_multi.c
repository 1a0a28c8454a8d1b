/* ISO C11 caller of the sparse fits with P target columns (cgp_sparse_multi_reserve, cgp_fit_predict_sparse_multi_batch),
 * squared-exponential kernel, d = 1.
 *   status codes:       without the multi reservation CGP_ESTATE (the sparse one alone is not enough); P = 0 and P = 65 CGP_EINVAL; P
 *                       beyond the reservation CGP_ECAPACITY; a NULL array CGP_EINVAL
 *   N = 1, m = 1, P = 2 sparse.c's closed form per column, with k_uu = s_f^2 + 1e-8, sigma2 = s_n^2 + 1e-8, k = k(z, x), ks = k(z, xs):
 *                       mean[p] = ks k y_p / (k_uu sigma2 + k^2)
 *                       A = k^2 / (k_uu sigma2), B = 1 + A, c_p = k y_p / (sqrt(k_uu B) sigma2)
 *                       bound[p] = -1/2 log 2 pi - 1/2 log sigma2 - 1/2 log B - y_p^2 / (2 sigma2) + c_p^2 / 2 - s_f^2 / (2 sigma2) + A / 2
 *                       var = s_f^2 - ks^2 / k_uu + ks^2 / (k_uu B) + s_n^2, one row for both columns
 *   linearity:          N = 24, m = 2, columns (y1, y2, 2 y1 - 3 y2): the third mean row is 2 mean[0] - 3 mean[1]
 *   M = 0:              the P bounds alone, bitwise the same, with NULL test points and outputs */
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

#define EXPECT(call, code)                                                               \
  do {                                                                                   \
    int rc_ = (call);                                                                    \
    if (rc_ != (code)) {                                                                 \
      fprintf(stderr, "%s -> %d, expected %d\n", #call, rc_, (code));                    \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

static double se(double a, double b, double sf2, double ell) { return sf2 * exp(-0.5 * (a - b) * (a - b) / (ell * ell)); }

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x = 0.1, z = 0.35, xs[2] = {0.4, -0.3}, y[2] = {0.5, -1.25};
  double many[24], Y3[3 * 24];
  for (int i = 0; i < 24; ++i) {
    many[i] = 0.05 * i;
    Y3[i] = sin(3.0 * many[i]);
    Y3[24 + i] = 0.3 * cos(5.0 * many[i]) + 0.1;
    Y3[48 + i] = 2.0 * Y3[i] - 3.0 * Y3[24 + i];
  }
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);   /* max_n = 16 */
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double mean[6], var[2], bound[3] = {0.0, 0.0, 0.0}, bound0[2] = {0.0, 0.0};
  int info = -1;
  EXPECT(cgp_sparse_multi_reserve(ctx, 1, 3), CGP_ESTATE);
  CHECK(cgp_sparse_reserve(ctx, 1, 24, 2, 2));
  EXPECT(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, 2, 1, CGP_KERNEL_SE_ISO, &x, y, &z, xs, theta, 3, 1, mean, var, bound, &info), CGP_ESTATE);
  EXPECT(cgp_sparse_multi_reserve(ctx, 1, CGP_SPARSE_MAX_P + 1), CGP_EINVAL);
  CHECK(cgp_sparse_multi_reserve(ctx, 1, 3));
  EXPECT(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, 0, 1, CGP_KERNEL_SE_ISO, &x, y, &z, xs, theta, 3, 1, mean, var, bound, &info), CGP_EINVAL);
  EXPECT(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, CGP_SPARSE_MAX_P + 1, 1, CGP_KERNEL_SE_ISO, &x, y, &z, xs, theta, 3, 1, mean, var, bound, &info), CGP_EINVAL);
  EXPECT(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, 4, 1, CGP_KERNEL_SE_ISO, &x, y, &z, xs, theta, 3, 1, mean, var, bound, &info), CGP_ECAPACITY);
  EXPECT(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, 2, 1, CGP_KERNEL_SE_ISO, &x, NULL, &z, xs, theta, 3, 1, mean, var, bound, &info), CGP_EINVAL);
  /* linearity of the mean in Y: 24 samples (beyond the context's max_n = 16), two inducing inputs, three columns */
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 24, 1, 2, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, xs, xs, theta, 3, 1, mean, var, bound, &info));
  int ok = info == 0 && var[0] > 0.0 && var[1] > 0.0;
  for (int j = 0; j < 2; ++j) {
    const double want = 2.0 * mean[j] - 3.0 * mean[2 + j];
    printf("xs %.3g: mean of 2 y1 - 3 y2 %.17g, 2 mean1 - 3 mean2 %.17g\n", xs[j], mean[4 + j], want);
    ok = ok && isfinite(bound[j]) && fabs(mean[4 + j] - want) <= 1e-10 * fmax(1.0, fabs(want));
  }
  /* N = 1, m = 1, P = 2 */
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 2, 2, 1, CGP_KERNEL_SE_ISO, &x, y, &z, xs, theta, 3, 1, mean, var, bound, &info));
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 0, 2, 1, CGP_KERNEL_SE_ISO, &x, y, &z, NULL, theta, 3, 1, NULL, NULL, bound0, NULL));
  const double sf2 = theta[0], ell = theta[1], sn2 = theta[2], kuu = sf2 + 1e-8, sigma2 = sn2 + 1e-8, k = se(z, x, sf2, ell);
  const double A = k * k / (kuu * sigma2), B = 1.0 + A;
  ok = ok && info == 0;
  for (int p = 0; p < 2; ++p) {
    const double c = k * y[p] / (sqrt(kuu * B) * sigma2);
    const double want = -0.5 * log(2.0 * acos(-1.0)) - 0.5 * log(sigma2) - 0.5 * log(B) - y[p] * y[p] / (2.0 * sigma2) + 0.5 * c * c -
                        sf2 / (2.0 * sigma2) + 0.5 * A;
    printf("column %d: bound %.17g closed form %.17g bound-only call %.17g\n", p, bound[p], want, bound0[p]);
    ok = ok && fabs(bound[p] - want) <= 1e-10 * fmax(1.0, fabs(want)) && bound0[p] == bound[p];
    for (int j = 0; j < 2; ++j) {
      const double ks = se(z, xs[j], sf2, ell);
      const double wm = ks * k * y[p] / (kuu * sigma2 + k * k), wv = sf2 - ks * ks / kuu + ks * ks / (kuu * B) + sn2;
      printf("  xs %.3g: mean %.17g closed form %.17g var %.17g closed form %.17g\n", xs[j], mean[2 * p + j], wm, var[j], wv);
      ok = ok && fabs(mean[2 * p + j] - wm) <= 1e-10 * fmax(1.0, fabs(wm)) && fabs(var[j] - wv) <= 1e-10 * wv;
    }
  }
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("sparse_multi.c ok\n");
  return 0;
}
