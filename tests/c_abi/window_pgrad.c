/* ISO C11 caller of the sliding windows' predictive gradients (cgp_window_predict_gradients): one window of capacity 4, first
 * empty (the prior), then after ONE pushed sample (x1, y1) against the n = 1 closed form, for SE-ARD (id 1) and RBF x Brownian
 * (id 2), d = 1.  With kyy = k(x1, x1) + sigma_n^2 + 1e-8, k* = k(x*, x1), dk* = dk(x*, x1)/dx*:
 *   mean = k* y1 / kyy,  var = max(k** - k*^2 / kyy, 1e-15),  dmean = dk* y1 / kyy,  dvar = dk** - 2 dk* k* / kyy
 *   id 1: k* = s exp(-(x* - x1)^2 / (2 l^2)), dk* = k* (x1 - x*) / l^2, k** = s, dk** = 0
 *   id 2: R = s exp(-(x* - x1)^2 / (2 l^2)), W = b min(|x*|, |x1|) for equal signs, else 0;  k* = R W,
 *         dk* = R W (x1 - x*) / l^2 + R b sign(x*) [|x*| < |x1| and equal signs],  k** = s b |x*|,  dk** = s b sign(x*)
 * (sign(0) = 0; at the tie |x*| = |x1| the bracket is 0).  Empty window: mean 0, var k**, dmean 0, dvar dk**. */
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

static double sgn(double x) { return (double)((x > 0) - (x < 0)); }

static int close_to(const char *what, const double *got, const double *want, int n, double tol) {
  for (int i = 0; i < n; ++i)
    if (!(fabs(got[i] - want[i]) <= tol * fmax(1.0, fabs(want[i])))) {
      fprintf(stderr, "%s[%d] = %.17g, expected %.17g\n", what, i, got[i], want[i]);
      return 0;
    }
  return 1;
}

/* k*, dk*, k**, dk** of kernel `kid` at x* against the sample x1 */
static void kern(int kid, const double *th, double xs, double x1, double *k, double *dk, double *kss, double *dkss) {
  const double l2 = th[1] * th[1], R = th[0] * exp(-0.5 * (xs - x1) * (xs - x1) / l2);
  if (kid == CGP_KERNEL_SE_ARD) {
    *k = R;
    *dk = R * (x1 - xs) / l2;
    *kss = th[0];
    *dkss = 0.0;
    return;
  }
  const int same = sgn(xs) == sgn(x1);
  const double W = same ? th[2] * fmin(fabs(xs), fabs(x1)) : 0.0;
  *k = R * W;
  *dk = R * W * (x1 - xs) / l2 + ((same && fabs(xs) < fabs(x1)) ? R * th[2] * sgn(xs) : 0.0);
  *kss = th[0] * th[2] * fabs(xs);
  *dkss = th[0] * th[2] * sgn(xs);
}

static int run(cgp_ctx *ctx, int kid, const double *th, int nth) {
  const double x1[1] = {5.0}, y1[1] = {0.7}, xs[M] = {3.0, 5.0, 7.5, -2.0, 0.0};
  const double noise = th[nth - 1];
  double mean[M], var[M], dm[M], dv[M], wmean[M], wvar[M], wdm[M], wdv[M], pm[1], pv[1], lm[1];
  double k, dk, kss, dkss, k11, unused;
  CHECK(cgp_window_init(ctx, 1, 4, 1, kid, th, nth));
  if (cgp_window_predict_gradients(ctx, M, xs, 0, mean, var, NULL, NULL) != CGP_EINVAL ||
      cgp_window_predict_gradients(ctx, 0, xs, 0, mean, var, dm, dv) != CGP_EINVAL ||
      cgp_window_predict_gradients(ctx, M, NULL, 0, mean, var, dm, dv) != CGP_EINVAL) {
    fprintf(stderr, "both gradients NULL, M = 0 and a NULL xs must answer CGP_EINVAL\n");
    return 1;
  }
  /* the empty window: the prior */
  for (int m = 0; m < M; ++m) {
    kern(kid, th, xs[m], x1[0], &k, &dk, &kss, &dkss);
    wmean[m] = 0.0;
    wvar[m] = kss + noise;
    wdm[m] = 0.0;
    wdv[m] = dkss;
  }
  CHECK(cgp_window_predict_gradients(ctx, M, xs, 1, mean, var, dm, dv));
  int ok = close_to("prior mean", mean, wmean, M, 1e-14) && close_to("prior var", var, wvar, M, 1e-14);
  for (int m = 0; m < M; ++m) ok = ok && mean[m] == 0.0 && dm[m] == 0.0 && dv[m] == wdv[m];
  if (!ok) {
    fprintf(stderr, "kernel %d: the empty window does not answer with the prior\n", kid);
    return 1;
  }
  /* one sample */
  CHECK(cgp_window_push(ctx, 1, x1, y1, 0, pm, pv, lm));
  kern(kid, th, x1[0], x1[0], &unused, &unused, &k11, &unused);
  const double kyy = k11 + noise + 1e-8;
  for (int m = 0; m < M; ++m) {
    kern(kid, th, xs[m], x1[0], &k, &dk, &kss, &dkss);
    wmean[m] = k * y1[0] / kyy;
    wvar[m] = fmax(kss - k * k / kyy, 1e-15);
    wdm[m] = dk * y1[0] / kyy;
    wdv[m] = dkss - 2.0 * dk * k / kyy;
  }
  CHECK(cgp_window_predict_gradients(ctx, M, xs, 0, mean, var, dm, dv));
  printf("kernel %d: dmean %.17g %.17g %.17g %.17g %.17g dvar %.17g %.17g %.17g %.17g %.17g\n", kid, dm[0], dm[1], dm[2], dm[3], dm[4],
         dv[0], dv[1], dv[2], dv[3], dv[4]);
  ok = close_to("mean", mean, wmean, M, 1e-9) && close_to("var", var, wvar, M, 1e-9) && close_to("dmean", dm, wdm, M, 1e-9) &&
       close_to("dvar", dv, wdv, M, 1e-9);
  double dv2[M], m2[M], v2[M];
  CHECK(cgp_window_predict_gradients(ctx, M, xs, 0, NULL, NULL, NULL, dv2));   /* one gradient alone */
  CHECK(cgp_window_predict(ctx, M, xs, 0, m2, v2));
  for (int m = 0; m < M; ++m) ok = ok && dv2[m] == dv[m] && m2[m] == mean[m] && v2[m] == var[m];
  return ok ? 0 : 1;
}

int main(void) {
  const double th_se[3] = {0.8, 2.5, 0.02}, th_rb[4] = {0.5, 30.0, 0.01, 0.002};
  double buf[M];
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  if (cgp_window_predict_gradients(ctx, 1, buf, 0, buf, buf, buf, buf) != CGP_ESTATE) {
    fprintf(stderr, "a call without windows must answer CGP_ESTATE\n");
    return 1;
  }
  if (run(ctx, CGP_KERNEL_SE_ARD, th_se, 3) || run(ctx, CGP_KERNEL_RBF_BROWNIAN, th_rb, 4)) return 1;
  cgp_destroy(ctx);
  printf("window_pgrad.c ok\n");
  return 0;
}
