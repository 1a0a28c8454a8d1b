// cgp_joint_host.hpp -- host side of the joint forecast after batch / single fits (kernel: cgp_joint.hpp; the factorisation and the
// paths are the windows' k_window_joint_chol / k_window_joint_paths, launched with the fit index).  Not a translation unit of its
// own: cgp_engine.hip includes it after the fit entry points it builds on (fit_predict_device, fit_predict_batch_host,
// predict_enqueue) and after cgp_window_host.hpp, whose joint_cov_grid and joint_chol_paths_launch the launches here use.
// fp64 contexts only: every entry point answers CGP_EINVAL in a CGP_F32 context before anything is enqueued.
#pragma once

namespace {

// The arrays of a joint call on the device (all pointers: the call's first fit)
struct JointCall {
  const double *dXs, *dtheta, *dvar;
  const int *dinfo;   // or null: a single fit known to be good
  double *dcov;       // output form (batch, M, M); null: the scratch form for the factorisation
};

// the reservation: the matrices [max_batch][(mt * 16)^2], then the factorisations' failure words [max_batch]
inline size_t joint_mat_doubles(int max_batch, int max_m) {
  const size_t mpad = (size_t)cdiv(max_m, WPB) * WPB;
  return (size_t)max_batch * mpad * mpad;
}
inline int *joint_fail_words(const cgp_ctx *c) {
  return reinterpret_cast<int *>(static_cast<double *>(c->fj.buf) + joint_mat_doubles(c->fj.max_batch, c->fj.max_dim));
}

// The contraction of `nfit` fits whose panels are slabs slab, slab + 1, ... into the slots slot, slot + 1, ... of the call's
// arrays.  After run() has returned: a worker stream is joined by then.
int joint_cov_launch(cgp_ctx *c, const JointCall &jc, int N, int d, int M, int kid, int slab, int slot, int nfit, hipStream_t s) {
  JointFitArgs j{};
  const unsigned grid = joint_cov_grid(M, nfit, j.mt, j.nsup, j.npair, j.per_fit);
  if (grid == 0) return CGP_EINVAL;
  const size_t mpad = (size_t)j.mt * WPB;
  j.Lw = static_cast<const double *>(c->Lw) + (size_t)slab * c->lw_stride;
  j.lw_stride = c->lw_stride;
  j.row0 = (size_t)cdiv(N, TS) * TS;
  j.ld = c->ld;
  j.theta = jc.dtheta + (size_t)slot * CGP_MAX_THETA;
  j.Xs = jc.dXs + (size_t)slot * d * M;
  j.var = jc.dvar + (size_t)slot * M;
  j.info = jc.dinfo ? jc.dinfo + slot : nullptr;
  j.cov = jc.dcov ? jc.dcov + (size_t)slot * M * M : nullptr;
  j.C = static_cast<double *>(c->fj.buf) + (size_t)slot * mpad * mpad;
  j.N = N; j.d = d; j.M = M; j.kernel_id = kid; j.nfit = nfit;
  if (jc.dcov) hipLaunchKernelGGL(k_joint_cov<false>, dim3(grid), dim3(WJ_THREADS), 0, s, j);
  else hipLaunchKernelGGL(k_joint_cov<true>, dim3(grid), dim3(WJ_THREADS), 0, s, j);
  if (!hip_ok(c, hipGetLastError(), "joint covariance launch")) return CGP_EHIP;
  return CGP_OK;
}

// a call whose test points, theta and variance are the context's own copies (the host entry points)
inline JointCall joint_ctx_call(const cgp_ctx *c, const int *dinfo, double *dcov) {
  return JointCall{static_cast<const double *>(c->dXs), c->dtheta, static_cast<const double *>(c->dvar), dinfo, dcov};
}

// C C^T = scratch matrix + jitter I in place, then out = mean + C xi, for the fits in slots [0, nfit): the windows' kernels through
// the windows' launcher (joint_chol_paths_launch, cgp_window_host.hpp)
int joint_paths_launch(cgp_ctx *c, int nfit, int M, int S, const double *dmean, const double *dvar, const double *dxi, double jitter_rel,
                       double *dout, int *dsinfo, hipStream_t s) {
  JointArgs j{};
  j.C = static_cast<double *>(c->fj.buf);
  j.jinfo = joint_fail_words(c);
  j.mean = dmean; j.var = dvar; j.xi = dxi; j.out = dout; j.info = dsinfo;
  j.jitter_rel = jitter_rel;
  j.M = M; j.S = S; j.nwin = nfit;
  j.mt = cdiv(M, WPB);
  const int rc = joint_chol_paths_launch(j, nfit, s);
  if (rc != CGP_OK) return rc;
  if (!hip_ok(c, hipGetLastError(), "joint sample launches")) return CGP_EHIP;
  return CGP_OK;
}

// the checks every joint call starts with: dtype, reservation, the reservation's capacity
int joint_check(const cgp_ctx *c, int batch, int M) {
  if (!c || c->dtype != CGP_F64 || M < 1) return CGP_EINVAL;
  return scratch_check(c->fj, batch, M);
}

inline int first_flagged_fit(const int *info, size_t n) {
  for (size_t b = 0; b < n; ++b)
    if (info[b] != 0) return (int)b + 1;
  return CGP_OK;
}

}  // namespace

extern "C" int cgp_joint_reserve(cgp_ctx *c, int max_batch, int max_m) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_m < 1 || max_m > std::min(c->max_m, 1024)) return CGP_EINVAL;
  return scratch_reserve(c, c->fj, max_batch, max_m, joint_mat_doubles(max_batch, max_m) * sizeof(double) + (size_t)max_batch * sizeof(int));
}

extern "C" int cgp_fit_predict_cov_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *dX, const double *dy,
                                                const double *dXs, const double *dtheta, const double *djitter, int include_noise,
                                                double *dmean, double *dcov, double *dlogml, int *dinfo, void *hip_stream) {
  int rc = joint_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (!dXs || !dmean || !dcov) return CGP_EINVAL;
  double *dvar = static_cast<double *>(c->dvar);   // the fit's variance, the diagonal of cov: the context's own buffer
  rc = fit_predict_device(c, batch, N, d, M, kid, dX, dy, dXs, dtheta, djitter, include_noise, dmean, dvar, dlogml, dinfo, hip_stream, true);
  if (rc != CGP_OK) return rc;
  return joint_cov_launch(c, JointCall{dXs, dtheta, dvar, dinfo, dcov}, N, d, M, kid, 0, 0, batch, pick_stream(c, hip_stream));
}

extern "C" int cgp_fit_sample_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *dX, const double *dy,
                                           const double *dXs, const double *dtheta, const double *djitter, int include_noise, int S,
                                           const double *dxi, double jitter_rel, double *dout, double *dlogml, int *dinfo, int *dsinfo,
                                           void *hip_stream) {
  int rc = joint_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (S < 1 || !dXs || !dxi || !dout || !(jitter_rel >= 0.0)) return CGP_EINVAL;
  double *dmean = static_cast<double *>(c->dmean), *dvar = static_cast<double *>(c->dvar);   // the context's own: never the caller's
  rc = fit_predict_device(c, batch, N, d, M, kid, dX, dy, dXs, dtheta, djitter, include_noise, dmean, dvar, dlogml, dinfo, hip_stream, true);
  if (rc != CGP_OK) return rc;
  hipStream_t s = pick_stream(c, hip_stream);
  rc = joint_cov_launch(c, JointCall{dXs, dtheta, dvar, dinfo, nullptr}, N, d, M, kid, 0, 0, batch, s);
  if (rc != CGP_OK) return rc;
  return joint_paths_launch(c, batch, M, S, dmean, dvar, dxi, jitter_rel, dout, dsinfo, s);
}

extern "C" int cgp_fit_predict_cov_batch(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *X, const double *y,
                                         const double *Xs, const double *theta, int theta_stride, int include_noise, double *mean,
                                         double *cov, double *logml, int *info) {
  int rc = joint_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (!mean || !cov) return CGP_EINVAL;
  // the output form goes to the reservation, (M, M) per fit, and from there to the caller
  const JointCall jc = joint_ctx_call(c, c->dinfo, static_cast<double *>(c->fj.buf));
  const auto hook = [&](int slab, int slot, int nfit, hipStream_t s) { return joint_cov_launch(c, jc, N, d, M, kid, slab, slot, nfit, s); };
  const PostFit post = post_fit(hook);
  rc = fit_predict_batch_host(c, batch, N, d, M, kid, X, y, Xs, theta, theta_stride, include_noise, mean, nullptr, logml, info, &post);
  if (rc < 0) return rc;
  HIP_TRY(c, hipMemcpyAsync(cov, jc.dcov, (size_t)batch * M * M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return rc;
}

namespace {
// xi up, factorisation and paths of the fits in slots [0, nfit) on the context's stream, paths and failure words back: the tail
// the two host sampling calls share.  Returns 0 or the 1-based index of the first fit whose paths are NaN.
int joint_sample_host(cgp_ctx *c, int nfit, int M, int S, const double *xi, double jitter_rel, double *out, int *sinfo) {
  const size_t np = (size_t)nfit * S * M;
  if (!grow_device(c->fj.stage, c->fj.stage_cap, 2 * np * sizeof(double))) return CGP_ENOMEM;
  double *dxi = static_cast<double *>(c->fj.stage), *dout = dxi + np;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(dxi, xi, np * sizeof(double), hipMemcpyHostToDevice, s));
  int rc = joint_paths_launch(c, nfit, M, S, static_cast<const double *>(c->dmean), static_cast<const double *>(c->dvar), dxi, jitter_rel,
                              dout, nullptr, s);
  if (rc != CGP_OK) return rc;
  std::vector<int> hi(nfit);
  HIP_TRY(c, hipMemcpyAsync(out, dout, np * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(hi.data(), joint_fail_words(c), (size_t)nfit * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (sinfo) memcpy(sinfo, hi.data(), (size_t)nfit * sizeof(int));
  return first_flagged_fit(hi.data(), nfit);
}
}  // namespace

extern "C" int cgp_fit_sample_batch(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *X, const double *y, const double *Xs,
                                    const double *theta, int theta_stride, int include_noise, int S, const double *xi, double jitter_rel,
                                    double *out, double *logml, int *info, int *sinfo) {
  int rc = joint_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (S < 1 || !xi || !out || !(jitter_rel >= 0.0)) return CGP_EINVAL;
  const JointCall jc = joint_ctx_call(c, c->dinfo, nullptr);
  const auto hook = [&](int slab, int slot, int nfit, hipStream_t s) { return joint_cov_launch(c, jc, N, d, M, kid, slab, slot, nfit, s); };
  const PostFit post = post_fit(hook);
  rc = fit_predict_batch_host(c, batch, N, d, M, kid, X, y, Xs, theta, theta_stride, include_noise, nullptr, nullptr, logml, info, &post);
  if (rc < 0) return rc;
  return joint_sample_host(c, batch, M, S, xi, jitter_rel, out, sinfo);
}

// ---- after a single fit (cgp_fit / cgp_optimize): m.predict(full_cov=True), m.posterior_samples_f ----------------------------
extern "C" int cgp_predict_cov(cgp_ctx *c, const double *Xs, int M, int include_noise, double *mean, double *cov) {
  int rc = joint_check(c, 1, M);
  if (rc != CGP_OK) return rc;
  if (!Xs || !mean || !cov) return CGP_EINVAL;
  if ((rc = predict_enqueue(c, Xs, M, include_noise)) != CGP_OK) return rc;
  hipStream_t s = c->stream;
  const JointCall jc = joint_ctx_call(c, nullptr, static_cast<double *>(c->fj.buf));
  if ((rc = joint_cov_launch(c, jc, c->fN, c->fd, M, c->fkernel, 0, 0, 1, s)) != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(mean, c->dmean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(cov, jc.dcov, (size_t)M * M * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}

extern "C" int cgp_sample(cgp_ctx *c, const double *Xs, int M, int S, const double *xi, int include_noise, double jitter_rel, double *out,
                          int *info) {
  int rc = joint_check(c, 1, M);
  if (rc != CGP_OK) return rc;
  if (S < 1 || !Xs || !xi || !out || !(jitter_rel >= 0.0)) return CGP_EINVAL;
  if ((rc = predict_enqueue(c, Xs, M, include_noise)) != CGP_OK) return rc;
  if ((rc = joint_cov_launch(c, joint_ctx_call(c, nullptr, nullptr), c->fN, c->fd, M, c->fkernel, 0, 0, 1, c->stream)) != CGP_OK) return rc;
  return joint_sample_host(c, 1, M, S, xi, jitter_rel, out, info);
}
