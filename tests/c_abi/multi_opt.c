/* ISO C11 caller of the multi-target objective (cgp_multi_grad_reserve, cgp_multi_nll_grad_batch, cgp_optimize_multi_batch),
 * squared-exponential kernel, d = 1.
 *   N = 1 closed form, P = 2:  c = sigma_f^2 + sigma_n^2 + 1e-8,  logml[p] = -y_p^2 / (2 c) - log(c) / 2 - log(2 pi) / 2,
 *                              nll = -(logml[0] + logml[1]),  d nll / d sigma_f^2 = d nll / d sigma_n^2 = -1/2 ((y_0^2 + y_1^2) / c^2 - 2 / c),
 *                              d nll / d ell = 0
 *   additivity in the columns: nll and gradient of Y = [y_0, y_1] are the sums of the two one-column calls, 1e-9 of their scale
 *                              (two routes through the same factor: the bar between two device routes) */
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

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x = 0.1, y[2] = {0.5, -0.2};
  const double pi = 3.14159265358979323846;
  cgp_ctx *ctx = cgp_create(0, 16, 16, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double nll = 0.0, grad[3], logml[2];
  int info = -1;
  if (cgp_multi_nll_grad_batch(ctx, 1, 1, 1, 2, CGP_KERNEL_SE_ISO, &x, y, theta, 3, &nll, grad, 3, logml, &info) != CGP_ESTATE ||
      cgp_multi_grad_reserve(ctx, 1, 2) != CGP_ESTATE) {
    fprintf(stderr, "a context without a reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_multi_reserve(ctx, 1, 2));
  CHECK(cgp_multi_grad_reserve(ctx, 1, 2));
  if (cgp_multi_nll_grad_batch(ctx, 1, 1, 1, 3, CGP_KERNEL_SE_ISO, &x, y, theta, 3, &nll, grad, 3, logml, &info) != CGP_ECAPACITY) {
    fprintf(stderr, "P beyond the reservation must answer CGP_ECAPACITY\n");
    return 1;
  }
  CHECK(cgp_multi_nll_grad_batch(ctx, 1, 1, 1, 2, CGP_KERNEL_SE_ISO, &x, y, theta, 3, &nll, grad, 3, logml, &info));
  const double c = theta[0] + theta[2] + 1e-8;
  int ok = info == 0;
  double wn = 0.0;
  for (int p = 0; p < 2; ++p) {
    const double wl = -0.5 * y[p] * y[p] / c - 0.5 * log(c) - 0.5 * log(2.0 * pi);
    printf("logml[%d] %.17g (expected %.17g)\n", p, logml[p], wl);
    ok = ok && fabs(logml[p] - wl) <= 1e-9 * fmax(1.0, fabs(wl));
    wn -= wl;
  }
  const double wg = -0.5 * ((y[0] * y[0] + y[1] * y[1]) / (c * c) - 2.0 / c);
  printf("nll %.17g (expected %.17g)\ngrad %.17g %.17g %.17g (expected %.17g 0 %.17g)\n", nll, wn, grad[0], grad[1], grad[2], wg, wg);
  ok = ok && fabs(nll - wn) <= 1e-9 * fmax(1.0, fabs(wn));
  ok = ok && fabs(grad[0] - wg) <= 1e-9 * fabs(wg) && fabs(grad[2] - wg) <= 1e-9 * fabs(wg) && fabs(grad[1]) <= 1e-12 * fabs(wg);
  /* additivity in the columns: nine samples, Y = [y_0, y_1] against the two one-column calls */
  double X[N2], Y[2 * N2], n1[2], g1[2][3], scale = 0.0;
  for (int i = 0; i < N2; ++i) {
    X[i] = 0.25 * i;
    Y[i] = sin(1.3 * X[i]);
    Y[N2 + i] = 0.4 * cos(2.1 * X[i]) - 0.1;
  }
  CHECK(cgp_multi_nll_grad_batch(ctx, 1, N2, 1, 2, CGP_KERNEL_SE_ISO, X, Y, theta, 3, &nll, grad, 3, NULL, NULL));
  for (int p = 0; p < 2; ++p) CHECK(cgp_multi_nll_grad_batch(ctx, 1, N2, 1, 1, CGP_KERNEL_SE_ISO, X, Y + p * N2, theta, 3, &n1[p], g1[p], 3, NULL, NULL));
  for (int i = 0; i < 3; ++i) scale = fmax(scale, fabs(g1[0][i] + g1[1][i]));
  printf("nll %.17g  sum of the columns' %.17g\n", nll, n1[0] + n1[1]);
  ok = ok && fabs(nll - (n1[0] + n1[1])) <= 1e-9 * fabs(nll);
  for (int i = 0; i < 3; ++i) {
    printf("grad[%d] %.17g  sum of the columns' %.17g\n", i, grad[i], g1[0][i] + g1[1][i]);
    ok = ok && fabs(grad[i] - (g1[0][i] + g1[1][i])) <= 1e-9 * scale;
  }
  /* the optimiser from the same start: it must not lose likelihood */
  double th[3] = {0.8, 0.9, 0.02}, lsum = 0.0;
  int nev = 0;
  CHECK(cgp_optimize_multi_batch(ctx, 1, N2, 1, 2, CGP_KERNEL_SE_ISO, X, Y, th, 3, 50, &lsum, &nev));
  printf("optimised: theta %.6g %.6g %.6g  sum logml %.17g after %d evaluations (start %.17g)\n", th[0], th[1], th[2], lsum, nev, -nll);
  ok = ok && lsum >= -nll && nev >= 1 && nev <= 50 && th[0] > 0.0 && th[1] > 0.0 && th[2] > 0.0;
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("multi_opt.c ok\n");
  return 0;
}
