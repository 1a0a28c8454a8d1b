/* ISO C11 caller of the Matern kernels: cgp_fit -> cgp_predict -> cgp_nll_grad on the two-sample, two-dimensional window of
 * tests/golden/matern_closed_m{32,52}_n2.npz; every output is checked against the fixture's closed-form numbers, which the
 * test passes in a text file:
 *   matern <file>
 * file: kernel_id, theta[4], X[2][2], y[2], xs[2], then the expected mean, var_latent, logml, dlogml_dtheta[4]. */
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

static int close_to(const char *what, double got, double want) {
  const double scale = fabs(want) > 1e-12 ? fabs(want) : 1e-12;
  if (fabs(got - want) <= 1e-9 * scale) return 1;
  fprintf(stderr, "%s: got %.17g, expected %.17g\n", what, got, want);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s file\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "r");
  int kid = -1;
  double v[19];
  if (!f || fscanf(f, "%d", &kid) != 1) return 2;
  for (int i = 0; i < 19; ++i)
    if (fscanf(f, "%lf", &v[i]) != 1) return 2;
  fclose(f);
  if (kid != CGP_KERNEL_MATERN32_ARD && kid != CGP_KERNEL_MATERN52_ARD) return 2;
  const double *theta = v, *X = v + 4, *y = v + 8, *xs = v + 10, *emean = v + 12, *evar = v + 13, *elogml = v + 14, *egrad = v + 15;
  int status = 0;
  cgp_ctx *ctx = cgp_create_ex(0, 8, 8, 2, 1, CGP_F64, &status);
  if (!ctx) {
    fprintf(stderr, "cgp_create_ex -> %d (%s)\n", status, cgp_strerror(status));
    return 1;
  }
  double logml = 0.0, mean = 0.0, var = 0.0, nll = 0.0, grad[4] = {0.0, 0.0, 0.0, 0.0};
  CHECK(cgp_fit(ctx, X, y, 2, 2, kid, theta, &logml));
  CHECK(cgp_predict(ctx, xs, 1, 0, &mean, &var));
  CHECK(cgp_nll_grad(ctx, X, y, 2, 2, kid, theta, &nll, grad));
  int ok = close_to("logml", logml, *elogml) & close_to("mean", mean, *emean) & close_to("var", var, *evar) & close_to("nll", nll, -*elogml);
  for (int i = 0; i < 4; ++i) ok &= close_to("grad", -grad[i], egrad[i]);
  /* a single-precision context refuses the kernel and stays usable */
  cgp_ctx *c32 = cgp_create(0, 8, 8, 2, 1, CGP_F32);
  if (!c32 || cgp_fit(c32, X, y, 2, 2, kid, theta, &logml) != CGP_EINVAL || cgp_fit(c32, X, y, 2, 2, CGP_KERNEL_SE_ARD, theta, &logml) != CGP_OK) {
    fprintf(stderr, "the fp32 refusal is not what the header says\n");
    ok = 0;
  }
  if (cgp_fit(ctx, X, y, 2, 2, 5, theta, &logml) != CGP_EINVAL) ok = 0;
  cgp_destroy(c32);
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("matern.c ok\n");
  return 0;
}
