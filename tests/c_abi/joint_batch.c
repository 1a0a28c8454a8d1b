/* ISO C11 caller of the joint forecast after batch / single fits: cgp_joint_reserve -> cgp_fit_predict_cov_batch ->
 * cgp_fit_sample_batch -> cgp_fit -> cgp_predict_cov -> cgp_sample on the two-sample SE window of
 * tests/golden/closed_joint_n2_se.npz; every output is checked against the fixture's numbers, which the test passes in a text file:
 *   joint_batch <file>
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

/* largest errors of (mean, cov, paths) against the expected values; cov relative to sqrt(cov_ii cov_jj), 1 if not symmetric */
static int compare(const char *what, int M, int S, const double *mean, const double *cov, const double *paths, const double *emean,
                   const double *ecov, const double *epaths) {
  double em = 0.0, ec = 0.0, ep = 0.0;
  for (int i = 0; i < M; ++i) {
    em = fmax(em, fabs(mean[i] - emean[i]));
    for (int j = 0; j < M; ++j) {
      ec = fmax(ec, fabs(cov[i * M + j] - ecov[i * M + j]) / sqrt(ecov[i * M + i] * ecov[j * M + j]));
      if (cov[i * M + j] != cov[j * M + i]) ec = 1.0;
    }
  }
  for (int i = 0; i < S * M; ++i) ep = fmax(ep, fabs(paths[i] - epaths[i]));
  printf("%s max errors: mean %.3g cov (relative) %.3g paths %.3g\n", what, em, ec, ep);
  return em <= 1e-6 && ec <= 1e-6 && ep <= 1e-6;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s file\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "r");
  int M = 0, S = 0;
  if (!f || fscanf(f, "%d %d", &M, &S) != 2 || M < 1 || M > 64 || S < 1 || S > 64) return 2;
  double theta[3], x[2], y[2], jitter = 0.0, noise = 0.0, logml = 0.0;
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
  cgp_ctx *ctx = cgp_create(0, 8, 64, 1, 1, CGP_F64);
  if (!ctx) {
    fprintf(stderr, "cgp_create failed\n");
    return 1;
  }
  int info = -1, sinfo = -1;
  if (cgp_fit_predict_cov_batch(ctx, 1, 2, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, cov, &logml, &info) != CGP_ESTATE) {
    fprintf(stderr, "no reservation must answer CGP_ESTATE\n");
    return 1;
  }
  if (cgp_joint_reserve(ctx, 2, M) != CGP_EINVAL || cgp_joint_reserve(ctx, 1, 65) != CGP_EINVAL) {
    fprintf(stderr, "a reservation beyond the context must answer CGP_EINVAL\n");
    return 1;
  }
  CHECK(cgp_joint_reserve(ctx, 1, M));
  if (M < 64 && cgp_fit_predict_cov_batch(ctx, 1, 2, 1, M + 1, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, cov, &logml, &info) != CGP_ECAPACITY) {
    fprintf(stderr, "M > max_m must answer CGP_ECAPACITY\n");
    return 1;
  }
  if (cgp_fit_sample_batch(ctx, 1, 2, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 1, 0, xi, jitter, paths, NULL, NULL, NULL) != CGP_EINVAL) {
    fprintf(stderr, "S < 1 must answer CGP_EINVAL\n");
    return 1;
  }
  /* the batch calls (a batch of one) */
  CHECK(cgp_fit_predict_cov_batch(ctx, 1, 2, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 0, mean, cov, &logml, &info));
  CHECK(cgp_fit_sample_batch(ctx, 1, 2, 1, M, CGP_KERNEL_SE_ISO, x, y, xs, theta, 3, 1, S, xi, jitter, paths, NULL, NULL, &sinfo));
  int ok = info == 0 && sinfo == 0 && compare("batch: ", M, S, mean, cov, paths, emean, ecov, epaths);
  /* the single-fit calls */
  CHECK(cgp_fit(ctx, x, y, 2, 1, CGP_KERNEL_SE_ISO, theta, &logml));
  CHECK(cgp_predict_cov(ctx, xs, M, 0, mean, cov));
  sinfo = -1;
  CHECK(cgp_sample(ctx, xs, M, S, xi, 1, jitter, paths, &sinfo));
  ok = ok && sinfo == 0 && compare("single:", M, S, mean, cov, paths, emean, ecov, epaths);
  (void)noise;
  cgp_destroy(ctx);
  free(xs); free(xi); free(emean); free(ecov); free(epaths); free(mean); free(cov); free(paths);
  if (!ok) return 1;
  printf("joint_batch.c ok\n");
  return 0;
}
