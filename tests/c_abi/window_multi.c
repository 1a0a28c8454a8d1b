/* ISO C11 caller of the multi-target sliding windows (cgp_window_multi_reserve, cgp_window_push_multi,
 * cgp_window_predict_multi): one window of capacity 4 with P = 3 target columns, SE-ARD (id 1) and RBF x Brownian (id 2), d = 1.
 * Empty: the prior (mean 0, var k**, logml 0).  After ONE pushed tick (x1; y_p): with kyy = k(x1, x1) + sigma_n^2 + 1e-8,
 *   mean_p = k(x*, x1) y_p / kyy,  var = max(k** - k(x*, x1)^2 / kyy, 1e-15),  logml_p = -y_p^2 / (2 kyy) - log(kyy) / 2 - log(2 pi) / 2
 * The third column is a y_1 + b y_2: after three more ticks its mean row is a mean_1 + b mean_2 to 1e-12. */
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

#define M 5
#define P 3

static double sgn(double x) { return (double)((x > 0) - (x < 0)); }

static int close_to(const char *what, const double *got, const double *want, int n, double tol) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(1.0, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

static double kern(int kid, const double *th, double xs, double x1) {
  const double R = th[0] * exp(-0.5 * (xs - x1) * (xs - x1) / (th[1] * th[1]));
  if (kid == CGP_KERNEL_SE_ARD) return R;
  return sgn(xs) == sgn(x1) ? R * th[2] * fmin(fabs(xs), fabs(x1)) : 0.0;
}

static int run(cgp_ctx *ctx, int kid, const double *th, int nth) {
  const double ca = 0.7, cb = -1.9;
  const double x[4] = {5.0, 6.0, 7.0, 8.5}, xs[M] = {3.0, 5.0, 7.5, -2.0, 0.0};
  const double noise = th[nth - 1];
  double Y[4][P], mean[P * M], var[M], logml[P], wmean[P * M], wvar[M], wlogml[P], pm[4], pv[4], lm[4], m0[M], v0[M];
  for (int t = 0; t < 4; ++t) {
    Y[t][0] = 0.7 - 0.2 * t;
    Y[t][1] = -0.3 + 0.05 * t * t;
    Y[t][2] = ca * Y[t][0] + cb * Y[t][1];
  }
  CHECK(cgp_window_init(ctx, 1, 4, 1, kid, th, nth));
  if (cgp_window_predict_multi(ctx, M, P, xs, 0, mean, var, logml) != CGP_ESTATE ||
      cgp_window_push_multi(ctx, 1, P, x, &Y[0][0], 0, pm, pv, lm) != CGP_ESTATE) {
    fprintf(stderr, "calls without a reservation must answer CGP_ESTATE\n");
    return 1;
  }
  if (cgp_window_multi_reserve(ctx, 0) != CGP_EINVAL || cgp_window_multi_reserve(ctx, 65) != CGP_EINVAL) {
    fprintf(stderr, "P = 0 and P = 65 must answer CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_window_multi_reserve(ctx, P));
  if (cgp_window_predict_multi(ctx, M, P + 1, xs, 0, mean, var, logml) != CGP_EINVAL ||
      cgp_window_predict_multi(ctx, 0, P, xs, 0, mean, var, logml) != CGP_EINVAL ||
      cgp_window_predict_multi(ctx, M, P, NULL, 0, mean, var, logml) != CGP_EINVAL ||
      cgp_window_push(ctx, 1, x, &Y[0][0], 0, pm, pv, lm) != CGP_ESTATE) {
    fprintf(stderr, "a wrong P, M = 0, a NULL xs (CGP_EINVAL) or a plain push on a reserved context (CGP_ESTATE)\n");
    return 1;
  }
  /* the empty window: the prior */
  for (int m = 0; m < M; ++m) wvar[m] = kern(kid, th, xs[m], xs[m]) + noise;
  CHECK(cgp_window_predict_multi(ctx, M, P, xs, 1, mean, var, logml));
  int ok = close_to("prior var", var, wvar, M, 1e-14);
  for (int i = 0; i < P * M; ++i) ok = ok && mean[i] == 0.0;
  for (int p = 0; p < P; ++p) ok = ok && logml[p] == 0.0;
  if (!ok) {
    fprintf(stderr, "kernel %d: the empty window does not answer with the prior\n", kid);
    return 1;
  }
  /* one tick */
  CHECK(cgp_window_push_multi(ctx, 1, P, x, &Y[0][0], 0, pm, pv, lm));
  const double kyy = kern(kid, th, x[0], x[0]) + noise + 1e-8;
  for (int m = 0; m < M; ++m) {
    const double k = kern(kid, th, xs[m], x[0]);
    for (int p = 0; p < P; ++p) wmean[p * M + m] = k * Y[0][p] / kyy;
    wvar[m] = fmax(kern(kid, th, xs[m], xs[m]) - k * k / kyy, 1e-15);
  }
  for (int p = 0; p < P; ++p) wlogml[p] = -0.5 * Y[0][p] * Y[0][p] / kyy - 0.5 * log(kyy) - 0.5 * log(2.0 * 3.14159265358979323846);
  CHECK(cgp_window_predict_multi(ctx, M, P, xs, 0, mean, var, logml));
  printf("kernel %d: mean row 1 %.17g %.17g %.17g logml %.17g %.17g %.17g\n", kid, mean[M], mean[M + 1], mean[M + 2], logml[0], logml[1],
         logml[2]);
  ok = close_to("mean", mean, wmean, P * M, 1e-9) && close_to("var", var, wvar, M, 1e-9) && close_to("logml", logml, wlogml, P, 1e-9);
  ok = ok && fabs(lm[0] - wlogml[0]) <= 1e-9 * fmax(1.0, fabs(wlogml[0]));   /* the push's logML is column 0's */
  CHECK(cgp_window_predict(ctx, M, xs, 0, m0, v0));                          /* the single-target calls speak of column 0 */
  for (int m = 0; m < M; ++m) ok = ok && v0[m] == var[m] && fabs(m0[m] - mean[m]) <= 1e-12 * fmax(1.0, fabs(m0[m]));
  if (!ok) return 1;
  /* three more ticks: linearity of the mean in the targets; logml may be NULL */
  CHECK(cgp_window_push_multi(ctx, 3, P, x + 1, &Y[1][0], 0, pm, pv, lm));
  CHECK(cgp_window_predict_multi(ctx, M, P, xs, 0, mean, var, NULL));
  for (int m = 0; m < M; ++m) wmean[m] = ca * mean[m] + cb * mean[M + m];
  double scale = 0.0;
  for (int i = 0; i < P * M; ++i) scale = fmax(scale, fabs(mean[i]));
  for (int m = 0; m < M; ++m)
    if (!(fabs(mean[2 * M + m] - wmean[m]) <= 1e-12 * scale)) {
      fprintf(stderr, "kernel %d: linearity: %.17g against %.17g\n", kid, mean[2 * M + m], wmean[m]);
      return 1;
    }
  return 0;
}

int main(void) {
  const double th_se[3] = {0.8, 2.5, 0.02}, th_rb[4] = {0.5, 30.0, 0.01, 0.002};
  double buf[P * M];
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  if (cgp_window_multi_reserve(ctx, P) != CGP_ESTATE || cgp_window_predict_multi(ctx, 1, P, buf, 0, buf, buf, buf) != CGP_ESTATE) {
    fprintf(stderr, "a call without windows must answer CGP_ESTATE\n");
    return 1;
  }
  if (run(ctx, CGP_KERNEL_SE_ARD, th_se, 3) || run(ctx, CGP_KERNEL_RBF_BROWNIAN, th_rb, 4)) return 1;
  cgp_destroy(ctx);
  printf("window_multi.c ok\n");
  return 0;
}
