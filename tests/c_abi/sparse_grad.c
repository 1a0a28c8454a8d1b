/* ISO C11 caller of the sparse fits' objective (cgp_sparse_grad_reserve, cgp_sparse_nll_grad_batch, cgp_optimize_sparse_batch),
 * squared-exponential kernel, d = 1.
 *   status codes:       no reservation of either kind CGP_ESTATE; the gradient reservation without the sparse one CGP_ESTATE; m = 0
 *                       CGP_EINVAL; N beyond the reservation CGP_ECAPACITY; a NULL array CGP_EINVAL; a theta <= 0 in the optimiser
 *                       CGP_EINVAL
 *   N = 1, m = 1:       the closed-form bound of tests/c_abi/sparse.c,
 *                         k = s_f^2 exp(-(z - x)^2 / (2 ell^2)), k_uu = s_f^2 + 1e-8, sigma2 = s_n^2 + 1e-8,
 *                         A = k^2 / (k_uu sigma2), B = 1 + A, c^2 = k^2 y^2 / (k_uu B sigma2^2)
 *                         F = -1/2 log 2 pi - 1/2 log sigma2 - 1/2 log B - y^2 / (2 sigma2) + c^2 / 2 - s_f^2 / (2 sigma2) + A / 2
 *                       differentiated in (s_f^2, ell, s_n^2, z) by central differences in long double; nll = -F
 *   the optimiser:      a bound that is not below the start's, bitwise the forward call's at the returned point */
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

static long double bound_of(const long double v[4], long double x, long double y) {   /* v = (s_f^2, ell, s_n^2, z) */
  const long double sf2 = v[0], ell = v[1], sigma2 = v[2] + 1e-8L, z = v[3], kuu = sf2 + 1e-8L;
  const long double k = sf2 * expl(-0.5L * (z - x) * (z - x) / (ell * ell));
  const long double A = k * k / (kuu * sigma2), B = 1.0L + A, c2 = k * k * y * y / (kuu * B * sigma2 * sigma2);
  return -0.5L * logl(2.0L * acosl(-1.0L)) - 0.5L * logl(sigma2) - 0.5L * logl(B) - y * y / (2.0L * sigma2) + 0.5L * c2 - sf2 / (2.0L * sigma2) +
         0.5L * A;
}

int main(void) {
  double theta[3] = {0.8, 0.9, 0.02}, z = 0.35;
  const double x = 0.1, y = 0.5;
  double many[24];
  for (int i = 0; i < 24; ++i) many[i] = 0.05 * i;
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double nll = 0.0, grad[3], gz = 0.0, bound = 0.0;
  int info = -1, evals = 0;
  EXPECT(cgp_sparse_grad_reserve(ctx, 1), CGP_ESTATE);
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, theta, 3, &nll, grad, 3, &gz, &info), CGP_ESTATE);
  CHECK(cgp_sparse_reserve(ctx, 1, 24, 2, 0));
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, theta, 3, &nll, grad, 3, &gz, &info), CGP_ESTATE);
  EXPECT(cgp_sparse_grad_reserve(ctx, 2), CGP_EINVAL);
  CHECK(cgp_sparse_grad_reserve(ctx, 1));
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 0, CGP_KERNEL_SE_ISO, &x, &y, &z, theta, 3, &nll, grad, 3, &gz, &info), CGP_EINVAL);
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 25, 1, 1, CGP_KERNEL_SE_ISO, many, many, &z, theta, 3, &nll, grad, 3, &gz, &info), CGP_ECAPACITY);
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 1, CGP_KERNEL_SE_ISO, &x, &y, NULL, theta, 3, &nll, grad, 3, &gz, &info), CGP_EINVAL);
  EXPECT(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, theta, 3, &nll, grad, 2, &gz, &info), CGP_EINVAL);
  /* N = 1, m = 1 */
  CHECK(cgp_sparse_nll_grad_batch(ctx, 1, 1, 1, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, theta, 3, &nll, grad, 3, &gz, &info));
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 1, 1, 0, 1, CGP_KERNEL_SE_ISO, &x, &y, &z, NULL, theta, 3, 1, NULL, NULL, &bound, NULL));
  const long double v0[4] = {theta[0], theta[1], theta[2], z};
  long double want[4], big = 0.0L;
  for (int i = 0; i < 4; ++i) {
    long double a[4] = {v0[0], v0[1], v0[2], v0[3]}, b[4] = {v0[0], v0[1], v0[2], v0[3]};
    const long double h = 1e-6L * fabsl(v0[i]);
    a[i] += h;
    b[i] -= h;
    want[i] = -(bound_of(a, x, y) - bound_of(b, x, y)) / (2.0L * h);
    if (i < 3 && fabsl(want[i]) > big) big = fabsl(want[i]);
  }
  const double f0 = (double)bound_of(v0, x, y);
  printf("nll %.17g closed form %.17g forward call %.17g\n", nll, -f0, -bound);
  int ok = info == 0 && nll == -bound && fabs(nll + f0) <= 1e-10 * fmax(1.0, fabs(f0));
  for (int i = 0; i < 3; ++i) {
    printf("grad[%d] %.17g central difference %.17Lg\n", i, grad[i], want[i]);
    ok = ok && fabsl(grad[i] - want[i]) <= 1e-8L * big;
  }
  printf("gradZ %.17g central difference %.17Lg\n", gz, want[3]);
  ok = ok && fabsl(gz - want[3]) <= 1e-8L * fabsl(want[3]);
  /* the optimiser over theta and z on 24 samples with two inducing inputs */
  double Z2[2] = {0.3, 0.8}, start = 0.0, y24[24];
  for (int i = 0; i < 24; ++i) y24[i] = sin(3.0 * many[i]) + 0.05 * cos(40.0 * many[i]);
  double bad_theta[3] = {0.8, 0.0, 0.02};
  EXPECT(cgp_optimize_sparse_batch(ctx, 1, 24, 1, 2, CGP_KERNEL_SE_ISO, many, y24, Z2, bad_theta, 3, 1, 0, &bound, &evals), CGP_EINVAL);
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 24, 1, 0, 2, CGP_KERNEL_SE_ISO, many, y24, Z2, NULL, theta, 3, 1, NULL, NULL, &start, NULL));
  CHECK(cgp_optimize_sparse_batch(ctx, 1, 24, 1, 2, CGP_KERNEL_SE_ISO, many, y24, Z2, theta, 3, 1, 0, &bound, &evals));
  double again = 0.0;
  CHECK(cgp_fit_predict_sparse_batch(ctx, 1, 24, 1, 0, 2, CGP_KERNEL_SE_ISO, many, y24, Z2, NULL, theta, 3, 1, NULL, NULL, &again, NULL));
  printf("optimiser: bound %.17g -> %.17g in %d evaluations, theta %.6g %.6g %.6g, Z %.6g %.6g\n", start, bound, evals, theta[0], theta[1],
         theta[2], Z2[0], Z2[1]);
  ok = ok && bound >= start && again == bound && evals > 1 && theta[0] > 0.0 && theta[1] > 0.0 && theta[2] > 0.0;
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("sparse_grad.c ok\n");
  return 0;
}
