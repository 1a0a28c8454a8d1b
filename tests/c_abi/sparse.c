/* ISO C11 caller of the sparse (inducing-point) fits (cgp_sparse_reserve, cgp_fit_predict_sparse_batch), squared-exponential
 * kernel, d = 1.
 *   status codes:       no reservation CGP_ESTATE; m = 0 and m = 513 CGP_EINVAL; N beyond the reservation CGP_ECAPACITY -- while N
 *                       beyond the CONTEXT's max_n is accepted; a NULL array CGP_EINVAL
 *   N = 1, m = 1 closed form, with k_uu = s_f^2 + 1e-8, sigma2 = s_n^2 + 1e-8, k = k(z, x), ks = k(z, xs):
 *                       mean = ks k y / (k_uu sigma2 + k^2)
 *                       A = k^2 / (k_uu sigma2), B = 1 + A, c = k y / (sqrt(k_uu B) sigma2)
 *                       bound = -1/2 log 2 pi - 1/2 log sigma2 - 1/2 log B - y^2 / (2 sigma2) + c^2 / 2 - s_f^2 / (2 sigma2) + A / 2
 *                       var = s_f^2 - ks^2 / k_uu + ks^2 / (k_uu B) + s_n^2
 *   M = 0:              the bound alone, bitwise the same, with NULL test points and outputs */
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
  const double theta[3] = {0.8, 0.9, 0.02}, x = 0.1, z = 0.35, xs[2] = {0.4, -0.3}, y = 0.5;
  double many[24];
  for (int i = 0; i < 24; ++i) many[i] = 0.05 * i;
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);   /* max_n = 16 */
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double mean[2], var[2], bound = 0.0, bound0 = 0.0;
  int info = -1;
  EXPECT(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, xs, theta, 3, 1, mean, var, &bound, &info), CGP_ESTATE);
  EXPECT(cgp_sparse_reserve(ctx, 1, 24, 513, 2), CGP_EINVAL);
  CHECK(cgp_sparse_reserve(ctx, 1, 24, 2, 2));
  EXPECT(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 2, 0, CGP_KERNEL_SE_ISO, &x, &y, &z, xs, theta, 3, 1, mean, var, &bound, &info), CGP_EINVAL);
  EXPECT(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 2, 513, CGP_KERNEL_SE_ISO, &x, &y, &z, xs, theta, 3, 1, mean, var, &bound, &info), CGP_EINVAL);
  EXPECT(cgp_fit_predict_sparse_batch(ctx, 1, 25, 1, 2, 1, CGP_KERNEL_SE_ISO, many, many, &z, xs, theta, 3, 1, mean, var, &bound, &info), CGP_ECAPACITY);
  EXPECT(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, &y, NULL, xs, theta, 3, 1, mean, var, &bound, &info), CGP_EINVAL);
  /* 24 samples in a context of max_n = 16: the sparse reservation alone bounds N */
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 24, 1, 2, 2, CGP_KERNEL_SE_ISO, many, many, xs, xs, theta, 3, 1, mean, var, &bound, &info));
  int ok = info == 0 && isfinite(bound) && isfinite(mean[0]) && var[0] > 0.0;
  /* N = 1, m = 1 */
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, xs, theta, 3, 1, mean, var, &bound, &info));
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 0, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, NULL, theta, 3, 1, NULL, NULL, &bound0, NULL));
  const double sf2 = theta[0], ell = theta[1], sn2 = theta[2], kuu = sf2 + 1e-8, sigma2 = sn2 + 1e-8, k = se(z, x, sf2, ell);
  const double A = k * k / (kuu * sigma2), B = 1.0 + A, c = k * y / (sqrt(kuu * B) * sigma2);
  const double want = -0.5 * log(2.0 * acos(-1.0)) - 0.5 * log(sigma2) - 0.5 * log(B) - y * y / (2.0 * sigma2) + 0.5 * c * c - sf2 / (2.0 * sigma2) +
                      0.5 * A;
  printf("bound %.17g closed form %.17g bound-only call %.17g\n", bound, want, bound0);
  ok = ok && info == 0 && fabs(bound - want) <= 1e-10 * fmax(1.0, fabs(want)) && bound0 == bound;
  for (int j = 0; j < 2; ++j) {
    const double ks = se(z, xs[j], sf2, ell);
    const double wm = ks * k * y / (kuu * sigma2 + k * k), wv = sf2 - ks * ks / kuu + ks * ks / (kuu * B) + sn2;
    printf("xs %.3g: mean %.17g closed form %.17g var %.17g closed form %.17g\n", xs[j], mean[j], wm, var[j], wv);
    ok = ok && fabs(mean[j] - wm) <= 1e-10 * fmax(1.0, fabs(wm)) && fabs(var[j] - wv) <= 1e-10 * wv;
  }
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("sparse.c ok\n");
  return 0;
}
