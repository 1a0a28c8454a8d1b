/* ISO C11 caller of the sparse fits' objective with P target columns (cgp_sparse_multi_grad_reserve,
 * cgp_sparse_multi_nll_grad_batch, cgp_optimize_sparse_multi_batch), squared-exponential kernel, d = 1.
 *   status codes:       without the multi-gradient reservation CGP_ESTATE, and that reservation without the three it needs
 *                       CGP_ESTATE; P = 0 CGP_EINVAL; P beyond the reservation CGP_ECAPACITY; a NULL array CGP_EINVAL
 *   N = 1, m = 1:       two columns y_1, y_2 on the closed-form bound of tests/c_abi/sparse_grad.c,
 *                         F = sum_p F(y_p),   F(y) = -1/2 log 2 pi - 1/2 log sigma2 - 1/2 log B - y^2 / (2 sigma2) + c(y)^2 / 2
 *                                                    - s_f^2 / (2 sigma2) + A / 2
 *                       differentiated in (s_f^2, ell, s_n^2, z) by central differences in long double; nll = -F, and the two
 *                       bounds returned are F(y_1) and F(y_2), bitwise the forward call's
 *   identical columns:  P = 3 copies of one column on 24 samples with two inducing inputs give 3 x the single-column nll, grad and
 *                       gradZ within 1e-9
 *   the optimiser:      a summed bound that is not below the start's, bitwise the column-order sum of the forward call's */
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
  const double x = 0.1, y2[2] = {0.5, -0.3};
  double many[24];
  for (int i = 0; i < 24; ++i) many[i] = 0.05 * i;
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double nll = 0.0, grad[3], gz = 0.0, lm[3], fwd[3];
  int info = -1, evals = 0;
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 1, 3), CGP_ESTATE);
  CHECK(cgp_sparse_reserve(ctx, 1, 24, 2, 0));
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 1, 3), CGP_ESTATE);
  CHECK(cgp_sparse_grad_reserve(ctx, 1));
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 1, 3), CGP_ESTATE);
  CHECK(cgp_sparse_multi_reserve(ctx, 1, 3));
  EXPECT(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, y2, &z, theta, 3, &nll, grad, 3, &gz, lm, &info), CGP_ESTATE);
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 1, 4), CGP_ESTATE);
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 2, 3), CGP_EINVAL);
  EXPECT(cgp_sparse_multi_grad_reserve(ctx, 1, CGP_SPARSE_MAX_P + 1), CGP_EINVAL);
  CHECK(cgp_sparse_multi_grad_reserve(ctx, 1, 3));
  EXPECT(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 0, 1, CGP_KERNEL_SE_ISO, &x, y2, &z, theta, 3, &nll, grad, 3, &gz, lm, &info), CGP_EINVAL);
  EXPECT(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 4, 1, CGP_KERNEL_SE_ISO, &x, many, &z, theta, 3, &nll, grad, 3, &gz, lm, &info), CGP_ECAPACITY);
  EXPECT(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, NULL, &z, theta, 3, &nll, grad, 3, &gz, lm, &info), CGP_EINVAL);
  EXPECT(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, y2, &z, theta, 3, &nll, grad, 2, &gz, lm, &info), CGP_EINVAL);
  /* N = 1, m = 1, P = 2 */
  CHECK(cgp_sparse_multi_nll_grad_batch(ctx, 1, 1, 1, 2, 1, CGP_KERNEL_SE_ISO, &x, y2, &z, theta, 3, &nll, grad, 3, &gz, lm, &info));
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 1, 1, 0, 2, 1, CGP_KERNEL_SE_ISO, &x, y2, &z, NULL, theta, 3, 1, NULL, NULL, fwd, NULL));
  const long double v0[4] = {theta[0], theta[1], theta[2], z};
  long double want[4], big = 0.0L;
  for (int i = 0; i < 4; ++i) {
    long double a[4] = {v0[0], v0[1], v0[2], v0[3]}, b[4] = {v0[0], v0[1], v0[2], v0[3]};
    const long double h = 1e-6L * fabsl(v0[i]);
    a[i] += h;
    b[i] -= h;
    want[i] = -(bound_of(a, x, y2[0]) + bound_of(a, x, y2[1]) - bound_of(b, x, y2[0]) - bound_of(b, x, y2[1])) / (2.0L * h);
    if (i < 3 && fabsl(want[i]) > big) big = fabsl(want[i]);
  }
  const double f0 = (double)(bound_of(v0, x, y2[0]) + bound_of(v0, x, y2[1]));
  printf("nll %.17g closed form %.17g forward call %.17g + %.17g\n", nll, -f0, -fwd[0], -fwd[1]);
  int ok = info == 0 && nll == -(fwd[0] + fwd[1]) && lm[0] == fwd[0] && lm[1] == fwd[1] && fabs(nll + f0) <= 1e-10 * fmax(1.0, fabs(f0));
  for (int p = 0; p < 2; ++p) ok = ok && fabs(lm[p] - (double)bound_of(v0, x, y2[p])) <= 1e-10 * fmax(1.0, fabs(lm[p]));
  for (int i = 0; i < 3; ++i) {
    printf("grad[%d] %.17g central difference %.17Lg\n", i, grad[i], want[i]);
    ok = ok && fabsl(grad[i] - want[i]) <= 1e-8L * big;
  }
  printf("gradZ %.17g central difference %.17Lg\n", gz, want[3]);
  ok = ok && fabsl(gz - want[3]) <= 1e-8L * fabsl(want[3]);
  /* P identical columns on 24 samples with two inducing inputs: P times the single-column call */
  double Z2[2] = {0.3, 0.8}, y24[24], Y3[72], n1 = 0.0, g1[3], gz1[2], n3 = 0.0, g3[3], gz3[2];
  for (int i = 0; i < 24; ++i) y24[i] = sin(3.0 * many[i]) + 0.05 * cos(40.0 * many[i]);
  for (int i = 0; i < 72; ++i) Y3[i] = y24[i % 24];
  CHECK(cgp_sparse_nll_grad_batch(ctx, 1, 24, 1, 2, CGP_KERNEL_SE_ISO, many, y24, Z2, theta, 3, &n1, g1, 3, gz1, NULL));
  CHECK(cgp_sparse_multi_nll_grad_batch(ctx, 1, 24, 1, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, Z2, theta, 3, &n3, g3, 3, gz3, NULL, NULL));
  double gbig = 0.0, zbig = 0.0;
  for (int i = 0; i < 3; ++i) gbig = fmax(gbig, fabs(3.0 * g1[i]));
  for (int i = 0; i < 2; ++i) zbig = fmax(zbig, fabs(3.0 * gz1[i]));
  printf("identical columns: nll %.17g against 3 x %.17g\n", n3, n1);
  ok = ok && fabs(n3 - 3.0 * n1) <= 1e-9 * fmax(1.0, fabs(3.0 * n1));
  for (int i = 0; i < 3; ++i) ok = ok && fabs(g3[i] - 3.0 * g1[i]) <= 1e-9 * gbig;
  for (int i = 0; i < 2; ++i) ok = ok && fabs(gz3[i] - 3.0 * gz1[i]) <= 1e-9 * zbig;
  /* the optimiser over theta and z */
  double start[3], again[3], sum = 0.0;
  double bad_theta[3] = {0.8, 0.0, 0.02};
  EXPECT(cgp_optimize_sparse_multi_batch(ctx, 1, 24, 1, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, Z2, bad_theta, 3, 1, 0, &sum, &evals), CGP_EINVAL);
  for (int i = 0; i < 24; ++i) {   /* three different columns */
    Y3[24 + i] = 0.7 * y24[i] + 0.1;
    Y3[48 + i] = -y24[i];
  }
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 24, 1, 0, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, Z2, NULL, theta, 3, 1, NULL, NULL, start, NULL));
  CHECK(cgp_optimize_sparse_multi_batch(ctx, 1, 24, 1, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, Z2, theta, 3, 1, 0, &sum, &evals));
  CHECK(cgp_fit_predict_sparse_multi_batch(ctx, 1, 24, 1, 0, 3, 2, CGP_KERNEL_SE_ISO, many, Y3, Z2, NULL, theta, 3, 1, NULL, NULL, again, NULL));
  printf("optimiser: summed bound %.17g -> %.17g in %d evaluations, theta %.6g %.6g %.6g, Z %.6g %.6g\n", start[0] + start[1] + start[2], sum,
         evals, theta[0], theta[1], theta[2], Z2[0], Z2[1]);
  ok = ok && sum >= start[0] + start[1] + start[2] && (again[0] + again[1]) + again[2] == sum && evals > 1 && theta[0] > 0.0 && theta[1] > 0.0 &&
       theta[2] > 0.0;
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("sparse_multi_grad.c ok\n");
  return 0;
}
