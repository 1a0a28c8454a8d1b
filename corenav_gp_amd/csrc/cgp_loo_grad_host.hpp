// cgp_loo_grad_host.hpp -- host side of the leave-one-out objective: value and gradient of nlpd = -lpd_sum and its L-BFGS
// (kernels: cgp_loo_grad.hpp).  Not a translation unit of its own: cgp_engine.hip includes it after the leave-one-out entry
// points it builds on (loo_enqueue, loo_check) and beside cgp_multi_grad_host.hpp, whose shape it follows (upload_batch_xy,
// upload_theta, jitter_ladder, lbfgs_minimize_logexp_batch).  fp64 contexts only.
#pragma once

namespace {

// the reservation: S of every fit, then per fit loo_var | sqrt c | b / sqrt c | beta (L doubles each, L = NTmax 128), then
// lpd_sum and the logml of a call that passes none (max_batch each)
inline size_t loo_grad_doubles(const cgp_ctx *c, int max_batch) {
  const size_t L = (size_t)c->NTmax * TS;
  return (size_t)max_batch * (L * L + 4 * L + 2);
}

int loo_grad_check(const cgp_ctx *c, int batch, int N, int d, int kid) {
  if (!c || c->dtype != CGP_F64 || batch < 1) return CGP_EINVAL;
  const int rc = scratch_check(c->lg, batch, 1);
  if (rc != CGP_OK) return rc;
  return loo_check(c, batch, N, d, kid);
}

// One evaluation of `nfit` fits: slabs 0 .. nfit - 1 of the context and of the scratch, every pointer at the call's FIRST fit.
// loo_enqueue as it stands (the gradient-mode schedule, k_loo, k_loo_sum) with loo_var and lpd_sum into the scratch, then prep,
// kinv, beta, grad, finish.  All on s, nothing allocated, nothing synchronised.
int loo_grad_enqueue(cgp_ctx *c, int nfit, int N, int d, int kid, const double *dX, const double *dy, const double *dtheta,
                     const double *djitter, double *dnlpd, double *dgrad, int grad_stride, double *dlogml, int *dinfo, hipStream_t s) {
  const size_t L = (size_t)c->NTmax * TS, MB = c->lg.max_batch;
  double *S = static_cast<double *>(c->lg.buf), *vec = S + MB * L * L, *tail = vec + 4 * MB * L;
  if (!dlogml) dlogml = tail + MB;
  int rc = loo_enqueue(c, nfit, N, d, kid, dX, dy, dtheta, djitter, LooOut{nullptr, vec, nullptr, tail}, dlogml, dinfo, s);
  if (rc != CGP_OK) return rc;
  FitArgs a = grad_mode_args(c, N, d, kid, dX);
  a.y = dy;
  a.theta = dtheta;
  a.jitter = djitter;
  a.logml = dlogml;
  a.info = dinfo;
  LooGradArgs g{};
  g.lds = a.NT * TS;
  g.S = S;
  g.s_stride = (size_t)g.lds * g.lds;
  g.var = vec;
  g.lsum = tail;
  g.sc = vec + MB * L;
  g.u = vec + 2 * MB * L;
  g.beta = vec + 3 * MB * L;
  g.nlpd = dnlpd;
  g.grad = dgrad;
  g.grad_stride = grad_stride;
  const int npairs = a.NT * (a.NT + 1) / 2, lds = upd_lds_bytes<double>();
  hipLaunchKernelGGL(k_loo_prep, dim3(cdiv(g.lds, LG_PREP_THREADS), nfit), dim3(LG_PREP_THREADS), 0, s, a, g);
  hipLaunchKernelGGL(k_loo_kinv, dim3(npairs, nfit), dim3(256), lds, s, a, g);
  hipLaunchKernelGGL(k_loo_beta, dim3(g.lds / LG_EB, nfit), dim3(LG_WAVES * 64), 0, s, a, g);
  if (kid == K_MATERN32_ARD) hipLaunchKernelGGL(k_loo_grad<1>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  else if (kid == K_MATERN52_ARD) hipLaunchKernelGGL(k_loo_grad<2>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  else hipLaunchKernelGGL(k_loo_grad<0>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  hipLaunchKernelGGL(k_loo_grad_finish, dim3(nfit), dim3(LGF_THREADS), 0, s, a, g, npairs);
  if (!hip_ok(c, hipGetLastError(), "leave-one-out gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

// Host side of one evaluation of a batch whose X (c->dX), y (c->dy) and theta (c->dtheta) are on the device: the jitter zeroed,
// one batched call, then GPy's jitter ladder for the fits that failed, one at a time in slab 0 (loo_batch_host's policy); `skip`
// (or null) marks fits whose failure is not retried.  Results come back into nlpd (batch), grad (batch, CGP_MAX_THETA), logml
// (batch; may be null), info (batch); jit (batch) receives the jitter each fit was last tried with.
struct LooGradStage {
  double *dnlpd, *dgrad, *dlogml;
};
int loo_grad_stage(cgp_ctx *c, int batch, LooGradStage &st) {
  const size_t B = batch;
  if (!grow_device(c->lg.stage, c->lg.stage_cap, (2 * B + B * CGP_MAX_THETA) * sizeof(double))) return CGP_ENOMEM;
  st.dnlpd = static_cast<double *>(c->lg.stage);
  st.dgrad = st.dnlpd + B;
  st.dlogml = st.dgrad + B * CGP_MAX_THETA;
  return CGP_OK;
}
int loo_grad_eval_host(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *theta, int theta_stride,
                       const LooGradStage &st, const std::vector<char> *skip, double *nlpd, double *grad, double *logml, int *info,
                       double *jit) {
  hipStream_t s = c->stream;
  const double *dX = static_cast<const double *>(c->dX), *dy = static_cast<const double *>(c->dy);
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  int rc = loo_grad_enqueue(c, batch, N, d, kid, dX, dy, c->dtheta, c->djitter, st.dnlpd, st.dgrad, CGP_MAX_THETA, st.dlogml, c->dinfo, s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(info, c->dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  rc = jitter_ladder(c, batch, N, d, kid, theta, theta_stride, X, info, skip, jit, s, [&](int b) {
    const size_t off = (size_t)b * N;
    return loo_grad_enqueue(c, 1, N, d, kid, dX + off * d, dy + off, c->dtheta + (size_t)b * CGP_MAX_THETA, c->djitter + b, st.dnlpd + b,
                            st.dgrad + (size_t)b * CGP_MAX_THETA, CGP_MAX_THETA, st.dlogml + b, c->dinfo + b, s);
  });
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(nlpd, st.dnlpd, sizeof(double) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(grad, st.dgrad, sizeof(double) * batch * CGP_MAX_THETA, hipMemcpyDeviceToHost, s));
  if (logml) HIP_TRY(c, hipMemcpyAsync(logml, st.dlogml, sizeof(double) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}

// the upload and one evaluation of host buffers; returns the first non-zero per-fit status
int loo_grad_batch_host(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y, const double *theta,
                        int theta_stride, double *nlpd, double *grad, int grad_stride, double *logml, int *info, double *jit) {
  const int nth = ntheta(kid, d);
  c->have_fit = false;
  c->lazy_fit = false;
  LooGradStage st{};
  int rc = loo_grad_stage(c, batch, st);
  if (rc != CGP_OK) return rc;
  if ((rc = upload_batch_xy(c, batch, N, d, X, y, c->stream)) != CGP_OK) return rc;
  std::vector<double> hth, hg((size_t)batch * CGP_MAX_THETA);
  if ((rc = upload_theta(c, theta, theta_stride, nth, batch, c->stream, hth)) != CGP_OK) return rc;
  std::vector<int> hinfo(batch);
  rc = loo_grad_eval_host(c, batch, N, d, kid, X, theta, theta_stride, st, nullptr, nlpd, hg.data(), logml, hinfo.data(), jit);
  if (rc != CGP_OK) return rc;
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < nth; ++i) grad[(size_t)b * grad_stride + i] = hg[(size_t)b * CGP_MAX_THETA + i];
    if (info) info[b] = hinfo[b];
    if (hinfo[b] != 0) jit[b] = 0.0;   // only a fit that factored reports a jitter
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}

}  // namespace

extern "C" int cgp_loo_grad_reserve(cgp_ctx *c, int max_batch) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));   // (the attribute goes to the current device's function)
  for (const void *fn : {reinterpret_cast<const void *>(&k_loo_kinv), reinterpret_cast<const void *>(&k_loo_grad<0>),
                         reinterpret_cast<const void *>(&k_loo_grad<1>), reinterpret_cast<const void *>(&k_loo_grad<2>)})
    HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, upd_lds_bytes<double>()));
  return scratch_reserve(c, c->lg, max_batch, 1, loo_grad_doubles(c, max_batch) * sizeof(double));
}

extern "C" int cgp_loo_nll_grad_batch_device(cgp_ctx *c, int batch, int N, int d, int kid, const double *dX, const double *dy,
                                             const double *dtheta, const double *djitter, double *dnlpd, double *dgrad,
                                             int grad_stride, double *dlogml, int *dinfo, void *hip_stream) {
  int rc = loo_grad_check(c, batch, N, d, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dy || !dtheta || !dnlpd || !dgrad || !dinfo || grad_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  return loo_grad_enqueue(c, batch, N, d, kid, dX, dy, dtheta, djitter, dnlpd, dgrad, grad_stride, dlogml, dinfo, pick_stream(c, hip_stream));
}

extern "C" int cgp_loo_nll_grad_batch(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y,
                                      const double *theta, int theta_stride, double *nlpd, double *grad, int grad_stride,
                                      double *logml, int *info) {
  int rc = loo_grad_check(c, batch, N, d, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !y || !theta || !nlpd || !grad || theta_stride < nth || grad_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<double> jit(batch);
  return loo_grad_batch_host(c, batch, N, d, kid, X, y, theta, theta_stride, nlpd, grad, grad_stride, logml, info, jit.data());
}

extern "C" int cgp_loo_nll_grad(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta,
                                double *nlpd, double *grad) {
  int rc = loo_grad_check(c, 1, N, d, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta || !nlpd || !grad) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const int nth = ntheta(kid, d);
  int info = 0;
  double jit = 0.0;
  rc = loo_grad_batch_host(c, 1, N, d, kid, X, y, theta, nth, nlpd, grad, nth, nullptr, &info, &jit);
  if (rc < 0) return rc;
  // the factor panel of slab 0, alpha, the window, theta and the jitter are resident: fitted, as after cgp_loo
  c->fjitter = jit;
  c->have_fit = (info == 0);
  c->fN = N;
  c->fd = d;
  c->fkernel = kid;
  memcpy(c->ftheta, theta, sizeof(double) * nth);
  return info;
}

extern "C" int cgp_optimize_loo_batch(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y, double *theta,
                                      int theta_stride, int max_evals, double *lpd_sum, double *logml, int *n_evals) {
  int rc = loo_grad_check(c, batch, N, d, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !y || !theta || theta_stride < nth) return CGP_EINVAL;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < nth; ++i)
      if (!(theta[(size_t)b * theta_stride + i] > 0.0)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  LooGradStage stg{};
  if ((rc = loo_grad_stage(c, batch, stg)) != CGP_OK) return rc;
  if ((rc = upload_batch_xy(c, batch, N, d, X, y, c->stream)) != CGP_OK) return rc;
  // the batched L-BFGS driver over nlpd; a finished fit is evaluated at its best point and never retried
  std::vector<double> hth, nl(batch), hg((size_t)batch * CGP_MAX_THETA), hl(batch), jit(batch);
  std::vector<int> info(batch);
  std::vector<char> skip(batch, 0);
  auto round = [&](const double *th, const char *active, double *f, double *g, char *feasible) -> int {
    for (int b = 0; b < batch; ++b) skip[b] = !active[b];
    int rc = upload_theta(c, th, nth, nth, batch, c->stream, hth);
    if (rc != CGP_OK) return rc;
    // GPy jitchol inside m.optimize(): a trial point whose matrix is not positive definite climbs the ladder; one that stays
    // infeasible is +inf for the line search
    rc = loo_grad_eval_host(c, batch, N, d, kid, X, th, nth, stg, &skip, nl.data(), hg.data(), nullptr, info.data(), jit.data());
    if (rc != CGP_OK) return rc;
    for (int b = 0; b < batch; ++b) {
      if (!active[b]) continue;
      feasible[b] = info[b] == 0;
      f[b] = nl[b];
      std::copy(hg.data() + (size_t)b * CGP_MAX_THETA, hg.data() + (size_t)b * CGP_MAX_THETA + nth, g + (size_t)b * nth);
    }
    return CGP_OK;
  };
  corenav::LbfgsBatchResult res;
  if ((rc = corenav::lbfgs_minimize_logexp_batch(batch, nth, theta, theta_stride, nullptr, max_evals, round, res)) != CGP_OK) return rc;
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < nth; ++i) theta[(size_t)b * theta_stride + i] = res.theta[(size_t)b * nth + i];
    if (n_evals) n_evals[b] = res.evals[b];
  }
  if (lpd_sum || logml) {   // both objectives AT the returned theta: one evaluation more, not counted in n_evals
    if ((rc = upload_theta(c, res.theta.data(), nth, nth, batch, c->stream, hth)) != CGP_OK) return rc;
    rc = loo_grad_eval_host(c, batch, N, d, kid, X, res.theta.data(), nth, stg, nullptr, nl.data(), hg.data(), hl.data(), info.data(),
                            jit.data());
    if (rc != CGP_OK) return rc;
    for (int b = 0; b < batch; ++b) {
      if (lpd_sum) lpd_sum[b] = -nl[b];
      if (logml) logml[b] = hl[b];
    }
  }
  return CGP_OK;
}
