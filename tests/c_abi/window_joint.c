/* ISO C11 caller of the sliding windows' joint forecast: cgp_window_init -> cgp_window_joint_reserve -> cgp_window_push ->
 * cgp_window_predict_cov -> cgp_window_sample on the two-sample SE window of tests/golden/closed_joint_n2_se.npz; every output
 * is checked against the fixture's numbers, which the test passes in a text file:
 *   window_joint <file>
 * file: M S, theta[3], x[2], y[2], xs[M], xi[S M], jitter_rel, then the expected mean[M], cov_latent[M M], noise, paths[S M]. */
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

static int read_doubles(FILE *f, double *v, int n) {
  for (int i = 0; i < n; ++i)
    if (fscanf(f, "%lf", &v[i]) != 1) return 0;
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s file\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "r");
  int M = 0, S = 0;
  if (!f || fscanf(f, "%d %d", &M, &S) != 2 || M < 1 || M > 64 || S < 1 || S > 64) return 2;
  double theta[3], x[2], y[2], jitter = 0.0, noise = 0.0, out3[6];
  double *xs = malloc(sizeof(double) * (size_t)M), *xi = malloc(sizeof(double) * (size_t)(S * M));
  double *emean = malloc(sizeof(double) * (size_t)M), *ecov = malloc(sizeof(double) * (size_t)(M * M));
  double *epaths = malloc(sizeof(double) * (size_t)(S * M));
  double *mean = malloc(sizeof(double) * (size_t)M), *cov = malloc(sizeof(double) * (size_t)(M * M));
  double *paths = malloc(sizeof(double) * (size_t)(S * M));
  if (!xs || !xi || !emean || !ecov || !epaths || !mean || !cov || !paths) return 1;
  if (!read_doubles(f, theta, 3) || !read_doubles(f, x, 2) || !read_doubles(f, y, 2) || !read_doubles(f, xs, M) ||
      !read_doubles(f, xi, S * M) || !read_doubles(f, &jitter, 1) || !read_doubles(f, emean, M) || !read_doubles(f, ecov, M * M) ||
      !read_doubles(f, &noise, 1) || !read_doubles(f, epaths, S * M)) {
    fprintf(stderr, "short input file\n");
    return 2;
  }
  fclose(f);
  cgp_ctx *ctx = cgp_create(0, 8, 8, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  if (cgp_window_joint_reserve(ctx, M) != CGP_ESTATE) {
    fprintf(stderr, "a context without windows must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_init(ctx, 1, 2, 1, CGP_KERNEL_SE_ISO, theta, 3));
  if (cgp_window_predict_cov(ctx, M, xs, 0, mean, cov) != CGP_ESTATE) {
    fprintf(stderr, "no reservation must answer CGP_ESTATE\n");
    return 1;
  }
  CHECK(cgp_window_joint_reserve(ctx, M));
  CHECK(cgp_window_push(ctx, 2, x, y, 1, out3, out3 + 2, out3 + 4));
  if (cgp_window_predict_cov(ctx, M + 1, xs, 0, mean, cov) != CGP_ECAPACITY || cgp_window_sample(ctx, M, xs, 0, xi, 1, jitter, paths, NULL) != CGP_EINVAL) {
    fprintf(stderr, "M > max_m must answer CGP_ECAPACITY and S < 1 CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_window_predict_cov(ctx, M, xs, 0, mean, cov));
  int info = -1;
  CHECK(cgp_window_sample(ctx, M, xs, S, xi, 1, jitter, paths, &info));
  double em = 0.0, ec = 0.0, ep = 0.0;
  for (int i = 0; i < M; ++i) {
    em = fmax(em, fabs(mean[i] - emean[i]));
    for (int j = 0; j < M; ++j) {
      ec = fmax(ec, fabs(cov[i * M + j] - ecov[i * M + j]) / sqrt(ecov[i * M + i] * ecov[j * M + j]));
      if (cov[i * M + j] != cov[j * M + i]) ec = 1.0;
    }
  }
  for (int i = 0; i < S * M; ++i) ep = fmax(ep, fabs(paths[i] - epaths[i]));
  printf("info %d max errors: mean %.3g cov (relative) %.3g paths %.3g\n", info, em, ec, ep);
  const int ok = info == 0 && em <= 1e-6 && ec <= 1e-6 && ep <= 1e-6;
  cgp_destroy(ctx);
  free(xs); free(xi); free(emean); free(ecov); free(epaths); free(mean); free(cov); free(paths);
  if (!ok) return 1;
  printf("window_joint.c ok\n");
  return 0;
}
