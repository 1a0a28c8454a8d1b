/* ISO C11 caller of leave-one-out cross-validation: the N = 2 closed form through cgp_loo (a fit from host buffers) and through
 * cgp_window_loo (a resident window of capacity 4 holding the same two samples), squared-exponential kernel, d = 1.
 *   Ky = [[c, b], [b, c]],  c = sigma_f^2 + sigma_n^2 + 1e-8,  b = sigma_f^2 exp(-(xa - xb)^2 / (2 ell^2))
 *   loo_mean = (b yb / c, b ya / c),  loo_var = c - b^2 / c,  loo_lpd_i = log N(y_i; loo_mean_i, loo_var) */
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

static int close_to(const char *what, const double *got, const double *want, int n, double tol) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(1.0, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x[2] = {0.1, 0.9}, y[2] = {0.5, -0.2};
  const double pi = 3.14159265358979323846;
  const double c = theta[0] + theta[2] + 1e-8, b = theta[0] * exp(-0.5 * (x[0] - x[1]) * (x[0] - x[1]) / (theta[1] * theta[1]));
  double wm[2], wv[2], wl[2], ws;
  wm[0] = b * y[1] / c;
  wm[1] = b * y[0] / c;
  wv[0] = wv[1] = c - b * b / c;
  for (int i = 0; i < 2; ++i) wl[i] = -0.5 * log(2.0 * pi * wv[i]) - 0.5 * (y[i] - wm[i]) * (y[i] - wm[i]) / wv[i];
  ws = wl[0] + wl[1];
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double m[4], v[4], l[4], s = 0.0;
  if (cgp_window_loo(ctx, m, v, l, &s) != CGP_ESTATE) {
    fprintf(stderr, "a context without windows must answer CGP_ESTATE\n");
    return 1;
  }
  if (cgp_loo(ctx, x, y, 2, 1, CGP_KERNEL_SE_ISO, theta, NULL, NULL, NULL, NULL) != CGP_EINVAL) {
    fprintf(stderr, "all outputs NULL must answer CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_loo(ctx, x, y, 2, 1, CGP_KERNEL_SE_ISO, theta, m, v, l, &s));
  printf("cgp_loo: mean %.17g %.17g var %.17g lpd %.17g %.17g sum %.17g (expected %.17g)\n", m[0], m[1], v[0], l[0], l[1], s, ws);
  int ok = close_to("loo_mean", m, wm, 2, 1e-9) && close_to("loo_var", v, wv, 2, 1e-9) && close_to("loo_lpd", l, wl, 2, 1e-9) &&
           close_to("lpd_sum", &s, &ws, 1, 1e-9);
  double pm = 0.0, pv = 0.0;
  CHECK(cgp_predict(ctx, x, 1, 1, &pm, &pv));   /* the context is left fitted */
  double out[6];
  CHECK(cgp_window_init(ctx, 1, 4, 1, CGP_KERNEL_SE_ISO, theta, 3));
  CHECK(cgp_window_push(ctx, 2, x, y, 1, out, out + 2, out + 4));
  CHECK(cgp_window_loo(ctx, m, v, l, &s));
  printf("cgp_window_loo: mean %.17g %.17g var %.17g lpd %.17g %.17g sum %.17g tail %g %g\n", m[0], m[1], v[0], l[0], l[1], s, m[2], l[3]);
  ok = ok && close_to("window loo_mean", m, wm, 2, 1e-9) && close_to("window loo_var", v, wv, 2, 1e-9) &&
       close_to("window loo_lpd", l, wl, 2, 1e-9) && close_to("window lpd_sum", &s, &ws, 1, 1e-9);
  ok = ok && isnan(m[2]) && isnan(m[3]) && isnan(v[2]) && isnan(l[3]);   /* the window is still filling: entries [n, N) */
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("loo.c ok\n");
  return 0;
}
