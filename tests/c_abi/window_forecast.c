/* ISO C11 caller of the sliding-window forecast: cgp_window_init -> cgp_window_push -> cgp_window_predict on a small
 * deterministic stream (RBF x Brownian, d = 1), one forecast value checked against the number the test computed with the
 * oracle and passed on the command line:
 *   window_forecast <N> <T> <M> <j> <expected mean[j]> <expected var[j]>
 * The stream is x_t = 11 + t, y_t = 0.1 sin(2 pi x_t / 40) + 0.02 cos(0.7 x_t); the test points are the M ticks after it. */
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
  if (argc != 7) {
    fprintf(stderr, "usage: %s N T M j mean var\n", argv[0]);
    return 2;
  }
  const int N = atoi(argv[1]), T = atoi(argv[2]), M = atoi(argv[3]), j = atoi(argv[4]);
  const double emean = atof(argv[5]), evar = atof(argv[6]);
  const double theta[4] = {0.5, 30.0, 0.01, 0.002};
  const double pi = 3.14159265358979323846;
  if (N < 2 || T < 1 || M < 1 || j < 0 || j >= M) return 2;
  double *x = malloc(sizeof(double) * (size_t)T), *y = malloc(sizeof(double) * (size_t)T);
  double *out = malloc(sizeof(double) * 3 * (size_t)T), *xs = malloc(sizeof(double) * (size_t)M);
  double *mean = malloc(sizeof(double) * (size_t)M), *var = malloc(sizeof(double) * (size_t)M);
  if (!x || !y || !out || !xs || !mean || !var) return 1;
  for (int t = 0; t < T; ++t) {
    x[t] = 11.0 + t;
    y[t] = 0.1 * sin(2.0 * pi * x[t] / 40.0) + 0.02 * cos(0.7 * x[t]);
  }
  for (int m = 0; m < M; ++m) xs[m] = x[T - 1] + 1.0 + m;
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  if (cgp_window_predict(ctx, M, xs, 1, mean, var) != CGP_ESTATE) {
    fprintf(stderr, "a context without windows must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_init(ctx, 1, N, 1, CGP_KERNEL_RBF_BROWNIAN, theta, 4));
  CHECK(cgp_window_push(ctx, T, x, y, 1, out, out + T, out + 2 * T));
  if (cgp_window_predict(ctx, 0, xs, 1, mean, var) != CGP_EINVAL || cgp_window_predict(ctx, M, NULL, 1, mean, var) != CGP_EINVAL) {
    fprintf(stderr, "M < 1 and a NULL pointer must answer CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_window_predict(ctx, M, xs, 1, mean, var));
  int n = 0, info = -1;
  CHECK(cgp_window_state(ctx, 0, &n, &info));
  const double dm = fabs(mean[j] - emean), dv = fabs(var[j] - evar);
  printf("n %d info %d mean[%d] %.17g (expected %.17g) var %.17g (expected %.17g)\n", n, info, j, mean[j], emean, var[j], evar);
  const int ok = n == (T < N ? T : N) && info == 0 && dm <= 1e-6 * fmax(fabs(emean), 1e-3) && dv <= 1e-6 * evar;
  cgp_destroy(ctx);
  free(x); free(y); free(out); free(xs); free(mean); free(var);
  if (!ok) return 1;
  printf("window_forecast.c ok\n");
  return 0;
}
