/* ISO C11 caller of the windows' hyper-parameters replaced and re-estimated in place: cgp_window_init -> cgp_window_push ->
 * cgp_window_set_theta -> cgp_window_nll_grad -> cgp_window_optimize on a small deterministic stream (RBF x Brownian, d = 1);
 * logML under the new theta is checked against the number the test computed with the oracle and passed on the command line:
 *   window_adapt <N> <T> <expected logML under the new theta> <expected -logML gradient wrt theta[0]>
 * The stream is x_t = 11 + t, y_t = 0.1 sin(2 pi x_t / 40) + 0.02 cos(0.7 x_t). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "corenav_gp.h"

#define CHECK(call)                                                                      \
  do {                                                                                   \
    int rc_ = (call);                                                                    \
    if (rc_ != CGP_OK) {                                                                 \
      fprintf(stderr, "%s -> %d (%s)\n", #call, rc_, cgp_strerror(rc_));                 \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s N T logml grad0\n", argv[0]);
    return 2;
  }
  const int N = atoi(argv[1]), T = atoi(argv[2]);
  const double elogml = atof(argv[3]), egrad0 = atof(argv[4]);
  const double theta[4] = {0.5, 30.0, 0.01, 0.002}, theta_new[4] = {0.8, 45.0, 0.02, 0.004};
  const double bad_theta[4] = {0.5, 30.0, 0.01, -1.0e6};
  const double pi = 3.14159265358979323846;
  if (N < 2 || T < 1) return 2;
  double *x = malloc(sizeof(double) * (size_t)T), *y = malloc(sizeof(double) * (size_t)T);
  double *out = malloc(sizeof(double) * 3 * (size_t)T);
  if (!x || !y || !out) return 1;
  for (int t = 0; t < T; ++t) {
    x[t] = 11.0 + t;
    y[t] = 0.1 * sin(2.0 * pi * x[t] / 40.0) + 0.02 * cos(0.7 * x[t]);
  }
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double logml = 0.0, nll = 0.0, grad[4], theta_opt[4], logml_opt = 0.0;
  int info = -1, nev = 0, n = 0;
  if (cgp_window_set_theta(ctx, theta_new, 4, NULL, &logml, &info) != CGP_ESTATE || cgp_window_nll_grad(ctx, &nll, grad, 4) != CGP_ESTATE ||
      cgp_window_optimize(ctx, 10, NULL, theta_opt, 4, &logml_opt, &nev) != CGP_ESTATE) {
    fprintf(stderr, "a context without windows must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_init(ctx, 1, N, 1, CGP_KERNEL_RBF_BROWNIAN, theta, 4));
  CHECK(cgp_window_push(ctx, T, x, y, 1, out, out + T, out + 2 * T));
  if (cgp_window_set_theta(ctx, NULL, 4, NULL, &logml, &info) != CGP_EINVAL || cgp_window_set_theta(ctx, theta_new, 3, NULL, &logml, &info) != CGP_EINVAL ||
      cgp_window_nll_grad(ctx, &nll, grad, 3) != CGP_EINVAL) {
    fprintf(stderr, "a NULL theta and a short stride must answer CGP_EINVAL\n");
    return 1;
  }
  /* a theta under which Ky is not positive definite fails the window (its index comes back), a valid one revives it */
  if (cgp_window_set_theta(ctx, bad_theta, 4, NULL, &logml, &info) != 1 || info != 1) {
    fprintf(stderr, "a negative noise variance must fail window 1 at pivot 1 (info %d)\n", info);
    return 1;
  }
  CHECK(cgp_window_set_theta(ctx, theta_new, 4, NULL, &logml, &info));
  CHECK(cgp_window_state(ctx, 0, &n, &info));
  CHECK(cgp_window_nll_grad(ctx, &nll, grad, 4));
  printf("n %d info %d logml %.17g (expected %.17g) nll %.17g grad[0] %.17g (expected %.17g)\n", n, info, logml, elogml, nll, grad[0], egrad0);
  int ok = n == (T < N ? T : N) && info == 0 && fabs(logml - elogml) <= 1e-6 * fabs(elogml) && fabs(nll + elogml) <= 1e-6 * fabs(elogml) &&
           fabs(grad[0] - egrad0) <= 1e-6 * fmax(fabs(egrad0), 1e-3);
  CHECK(cgp_window_optimize(ctx, 30, NULL, theta_opt, 4, &logml_opt, &nev));
  printf("optimised: theta %.6g %.6g %.6g %.6g logml %.17g evaluations %d\n", theta_opt[0], theta_opt[1], theta_opt[2], theta_opt[3], logml_opt, nev);
  ok = ok && nev >= 1 && nev <= 30 && logml_opt >= logml - 1e-9 * fabs(logml) && theta_opt[0] > 0.0 && theta_opt[3] > 0.0;
  CHECK(cgp_window_push(ctx, 1, x, y, 1, out, out + 1, out + 2));   /* the stream simply continues */
  cgp_destroy(ctx);
  free(x); free(y); free(out);
  if (!ok) return 1;
  printf("window_adapt.c ok\n");
  return 0;
}
