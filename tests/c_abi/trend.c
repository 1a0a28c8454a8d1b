/* ISO C11 caller of the explicit-basis (trend) fits (cgp_trend_reserve, cgp_fit_predict_trend_batch), squared-exponential kernel,
 * d = 1.
 *   status codes:       no reservation CGP_ESTATE; q = 0 and q = CGP_MAX_TREND + 1 CGP_EINVAL; P beyond the reservation
 *                       CGP_ECAPACITY; a trend reservation without a multi-target one that covers max_p + CGP_MAX_TREND CGP_ESTATE
 *   N = 1 closed form:  q = 1, H = Hs = 1: the constant is the sample -- mean[p] = y_p, beta[p] = y_p, logml[p] = 0, tinfo = 0
 *   shift property:     nine samples, basis [1, x]: Y -> Y + c_0 + c_1 x moves beta by c and the mean by c_0 + c_1 xs (1e-9), leaves
 *                       var (bitwise) and logml (1e-9) alone */
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

#define N2 9
#define M2 5
#define P2 2
#define Q2 2

int main(void) {
  const double theta[3] = {0.8, 0.9, 0.02}, x = 0.1, xs[2] = {0.4, -0.3}, y[3] = {0.5, -0.2, 0.3};
  const double one[3] = {1.0, 1.0, 1.0};
  cgp_ctx *ctx = cgp_create(0, 16, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  double mean[3 * M2], var[M2], beta[3 * Q2], logml[3];
  int info = -1, tinfo = -1;
  EXPECT(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 3, 1, CGP_KERNEL_SE_ISO, &x, y, one, xs, one, theta, 3, 1, mean, var, beta, logml,
                                     &info, &tinfo), CGP_ESTATE);
  EXPECT(cgp_trend_reserve(ctx, 1, 3, 8), CGP_ESTATE);
  CHECK(cgp_multi_reserve(ctx, 1, 3 + CGP_MAX_TREND - 1));
  EXPECT(cgp_trend_reserve(ctx, 1, 3, 8), CGP_ESTATE);
  CHECK(cgp_multi_reserve(ctx, 1, 3 + CGP_MAX_TREND));
  EXPECT(cgp_trend_reserve(ctx, 1, 3, 9), CGP_EINVAL);
  CHECK(cgp_trend_reserve(ctx, 1, 3, 8));
  EXPECT(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 3, 0, CGP_KERNEL_SE_ISO, &x, y, one, xs, one, theta, 3, 1, mean, var, beta, logml,
                                     &info, &tinfo), CGP_EINVAL);
  EXPECT(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 3, CGP_MAX_TREND + 1, CGP_KERNEL_SE_ISO, &x, y, one, xs, one, theta, 3, 1, mean, var,
                                     beta, logml, &info, &tinfo), CGP_EINVAL);
  EXPECT(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 4, 1, CGP_KERNEL_SE_ISO, &x, y, one, xs, one, theta, 3, 1, mean, var, beta, logml,
                                     &info, &tinfo), CGP_ECAPACITY);
  EXPECT(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 3, 1, CGP_KERNEL_SE_ISO, &x, y, NULL, xs, one, theta, 3, 1, mean, var, beta, logml,
                                     &info, &tinfo), CGP_EINVAL);
  /* N = 1, q = 1, H = Hs = 1 */
  CHECK(cgp_fit_predict_trend_batch(ctx, 1, 1, 1, 2, 3, 1, CGP_KERNEL_SE_ISO, &x, y, one, xs, one, theta, 3, 1, mean, var, beta, logml,
                                    &info, &tinfo));
  int ok = info == 0 && tinfo == 0;
  for (int p = 0; p < 3; ++p) {
    printf("target %d: y %.17g beta %.17g logml %.3g mean %.17g %.17g\n", p, y[p], beta[p], logml[p], mean[p * 2], mean[p * 2 + 1]);
    ok = ok && fabs(beta[p] - y[p]) <= 1e-12 && fabs(logml[p]) <= 1e-12;
    for (int m = 0; m < 2; ++m) ok = ok && fabs(mean[p * 2 + m] - y[p]) <= 1e-12;
  }
  for (int m = 0; m < 2; ++m) ok = ok && var[m] > 0.0;
  /* the shift property */
  const double c[P2][Q2] = {{0.7, -0.3}, {-1.1, 0.25}};
  double X[N2], Y[P2 * N2], Ysh[P2 * N2], H[Q2 * N2], Xs[M2], Hs[Q2 * M2];
  double smean[P2 * M2], svar[M2], sbeta[P2 * Q2], slogml[P2];
  for (int i = 0; i < N2; ++i) {
    X[i] = 0.25 * i;
    H[i] = 1.0;
    H[N2 + i] = X[i] - 1.0;
    Y[i] = sin(1.3 * X[i]) + 0.4;
    Y[N2 + i] = 0.4 * cos(2.1 * X[i]) - 0.1 + 0.2 * X[i];
    for (int p = 0; p < P2; ++p) Ysh[p * N2 + i] = Y[p * N2 + i] + c[p][0] * H[i] + c[p][1] * H[N2 + i];
  }
  for (int m = 0; m < M2; ++m) {
    Xs[m] = 0.11 + 0.7 * m;
    Hs[m] = 1.0;
    Hs[M2 + m] = Xs[m] - 1.0;
  }
  CHECK(cgp_fit_predict_trend_batch(ctx, 1, N2, 1, M2, P2, Q2, CGP_KERNEL_SE_ISO, X, Y, H, Xs, Hs, theta, 3, 0, mean, var, beta, logml,
                                    &info, &tinfo));
  ok = ok && info == 0 && tinfo == 0;
  CHECK(cgp_fit_predict_trend_batch(ctx, 1, N2, 1, M2, P2, Q2, CGP_KERNEL_SE_ISO, X, Ysh, H, Xs, Hs, theta, 3, 0, smean, svar, sbeta, slogml,
                                    NULL, &tinfo));
  ok = ok && tinfo == 0;
  for (int p = 0; p < P2; ++p) {
    for (int r = 0; r < Q2; ++r) {
      printf("beta[%d][%d] %.17g shifted %.17g (c %.3g)\n", p, r, beta[p * Q2 + r], sbeta[p * Q2 + r], c[p][r]);
      ok = ok && fabs(sbeta[p * Q2 + r] - beta[p * Q2 + r] - c[p][r]) <= 1e-9;
    }
    for (int m = 0; m < M2; ++m) {
      const double want = mean[p * M2 + m] + c[p][0] * Hs[m] + c[p][1] * Hs[M2 + m];
      ok = ok && fabs(smean[p * M2 + m] - want) <= 1e-9 * fmax(1.0, fabs(want));
    }
    printf("logml[%d] %.17g shifted %.17g\n", p, logml[p], slogml[p]);
    ok = ok && fabs(slogml[p] - logml[p]) <= 1e-9 * fmax(1.0, fabs(logml[p]));
  }
  for (int m = 0; m < M2; ++m) ok = ok && svar[m] == var[m] && var[m] > 0.0;
  cgp_destroy(ctx);
  if (!ok) return 1;
  printf("trend.c ok\n");
  return 0;
}
