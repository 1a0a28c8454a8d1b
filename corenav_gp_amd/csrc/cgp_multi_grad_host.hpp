// cgp_multi_grad_host.hpp -- host side of the multi-target objective: value and gradient of -sum_p logml[p] over one shared theta
// and its L-BFGS (kernels: cgp_multi_grad.hpp).  Not a translation unit of its own: cgp_engine.hip includes it after
// cgp_multi_host.hpp and after the gradient-mode entry points it builds on (grad_mode_args / run as loo_enqueue uses them,
// upload_batch_xy, upload_theta, jitter_ladder).  fp64 contexts only.
#pragma once

namespace {

inline size_t multi_grad_a_doubles(const cgp_ctx *c, int max_batch, int max_p) {
  return (size_t)max_batch * c->NTmax * TS * ((size_t)cdiv(max_p, KT) * KT);
}

// the checks every call of this section starts with: dtype, P, both reservations, their capacity
int multi_grad_check(const cgp_ctx *c, int batch, int P) {
  if (!c || c->dtype != CGP_F64 || P < 1) return CGP_EINVAL;
  const int rz = scratch_check(c->mz, batch, P), ra = scratch_check(c->ma, batch, P);
  if (rz == CGP_ESTATE || ra == CGP_ESTATE) return CGP_ESTATE;   // a missing reservation before a small one
  return rz != CGP_OK ? rz : ra;
}

// One evaluation of `nfit` fits: slabs 0 .. nfit - 1 of the context, slots slot .. of the call's arrays (every pointer: the
// call's FIRST fit).  pack, the gradient-mode schedule on column 0 (loo_enqueue's FitArgs), solve, logml, alpha, grad, finish.
// All on s, nothing allocated, nothing synchronised.
int multi_grad_enqueue(cgp_ctx *c, int slot, int nfit, int N, int d, int P, int kid, const double *dX, const double *dY,
                       const double *dtheta, const double *djitter, double *dnll, double *dgrad, int grad_stride, double *dlogml,
                       int *dinfo, hipStream_t s) {
  double *dy0 = static_cast<double *>(c->dy);
  if (!dlogml) dlogml = static_cast<double *>(c->ma.buf) + multi_grad_a_doubles(c, c->ma.max_batch, c->ma.max_dim);   // the reservation's own (batch, P)
  MultiArgs ma = multi_args(c, N, 0, P, 0, slot, nfit, dY, dy0, nullptr, nullptr, dlogml, dinfo);
  int rc = multi_pack_launch(c, ma, s);
  if (rc != CGP_OK) return rc;
  FitArgs a = grad_mode_args(c, N, d, kid, dX + (size_t)slot * d * N);
  a.y = dy0 + (size_t)slot * N;
  a.theta = dtheta + (size_t)slot * CGP_MAX_THETA;
  a.jitter = djitter ? djitter + slot : nullptr;
  a.logml = c->dlogml + slot;   // column 0's own logML: a by-product
  a.info = dinfo + slot;
  rc = run(c, a, nfit, true, true, s);
  if (rc != CGP_OK) return rc;
  if ((rc = multi_solve_launch(c, ma, s)) != CGP_OK) return rc;
  hipLaunchKernelGGL(k_multi_logml, dim3(nfit), dim3(ML_THREADS), 0, s, ma);
  MultiGradArgs g{};
  g.Zw = ma.Zw;
  g.z_stride = ma.z_stride;
  g.ldz = ma.ldz;
  g.P = P;
  g.P16 = cdiv(P, KT) * KT;
  g.lda = a.NT * TS;
  g.a_stride = (size_t)g.lda * g.P16;
  g.Aw = static_cast<double *>(c->ma.buf);
  g.logml = ma.logml;
  g.nll = dnll + slot;
  g.grad = dgrad + (size_t)slot * grad_stride;
  g.grad_stride = grad_stride;
  const int npairs = a.NT * (a.NT + 1) / 2, lds = upd_lds_bytes<double>();
  hipLaunchKernelGGL(k_multi_alpha, dim3(a.NT, cdiv(P, TS), nfit), dim3(256), lds, s, a, g);
  if (kid == K_MATERN32_ARD) hipLaunchKernelGGL(k_multi_grad<1>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  else if (kid == K_MATERN52_ARD) hipLaunchKernelGGL(k_multi_grad<2>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  else hipLaunchKernelGGL(k_multi_grad<0>, dim3(npairs, nfit), dim3(256), lds, s, a, g, npairs);
  hipLaunchKernelGGL(k_multi_grad_finish, dim3(nfit), dim3(MGF_THREADS), 0, s, a, g, npairs);
  if (!hip_ok(c, hipGetLastError(), "multi-target gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

// Host side of one evaluation of a batch whose X (c->dX), Y and theta (c->dtheta) are on the device: the jitter zeroed, one batched
// call, then GPy's jitter ladder for the fits that failed, one at a time in slab 0 (loo_batch_host's policy); `skip` (or null)
// marks fits whose failure is not retried.  Results come back into nll (batch), grad (batch, CGP_MAX_THETA), logml (batch, P;
// may be null), info (batch).
struct MultiGradStage {
  double *dY, *dnll, *dgrad, *dlogml;
};
int multi_grad_stage(cgp_ctx *c, int batch, int N, int P, MultiGradStage &st) {
  const size_t B = batch, nY = B * P * N;
  if (!grow_device(c->ma.stage, c->ma.stage_cap, (nY + B + B * CGP_MAX_THETA + B * P) * sizeof(double))) return CGP_ENOMEM;
  st.dY = static_cast<double *>(c->ma.stage);
  st.dnll = st.dY + nY;
  st.dgrad = st.dnll + B;
  st.dlogml = st.dgrad + B * CGP_MAX_THETA;
  return CGP_OK;
}
int multi_grad_upload(cgp_ctx *c, int batch, int N, int d, int P, const double *X, const double *Y, const MultiGradStage &st) {
  const int rc = upload_batch_xy(c, batch, N, d, X, nullptr, c->stream);   // Y travels as it is: k_multi_pack reads it in place
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(st.dY, Y, (size_t)batch * P * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return CGP_OK;
}
int multi_grad_eval_host(cgp_ctx *c, int batch, int N, int d, int P, int kid, const double *X, const double *theta, int theta_stride,
                         const MultiGradStage &st, const std::vector<char> *skip, double *nll, double *grad, double *logml, int *info) {
  hipStream_t s = c->stream;
  const double *dX = static_cast<const double *>(c->dX);
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  int rc = multi_grad_enqueue(c, 0, batch, N, d, P, kid, dX, st.dY, c->dtheta, c->djitter, st.dnll, st.dgrad, CGP_MAX_THETA, st.dlogml,
                              c->dinfo, s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(info, c->dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  std::vector<double> jit(batch);
  rc = jitter_ladder(c, batch, N, d, kid, theta, theta_stride, X, info, skip, jit.data(), s, [&](int b) {
    return multi_grad_enqueue(c, b, 1, N, d, P, kid, dX, st.dY, c->dtheta, c->djitter, st.dnll, st.dgrad, CGP_MAX_THETA, st.dlogml,
                              c->dinfo, s);
  });
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(nll, st.dnll, sizeof(double) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(grad, st.dgrad, sizeof(double) * batch * CGP_MAX_THETA, hipMemcpyDeviceToHost, s));
  if (logml) HIP_TRY(c, hipMemcpyAsync(logml, st.dlogml, sizeof(double) * batch * P, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}

}  // namespace

extern "C" int cgp_multi_grad_reserve(cgp_ctx *c, int max_batch, int max_p) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_p < 1 || max_p > MULTI_MAX_P) return CGP_EINVAL;
  if (max_batch > c->mz.max_batch || max_p > c->mz.max_dim) return CGP_ESTATE;   // cgp_multi_reserve first, and one that covers this
  HIP_TRY(c, hipSetDevice(c->device));   // (the attribute goes to the current device's function)
  for (const void *fn : {reinterpret_cast<const void *>(&k_multi_alpha), reinterpret_cast<const void *>(&k_multi_grad<0>),
                         reinterpret_cast<const void *>(&k_multi_grad<1>), reinterpret_cast<const void *>(&k_multi_grad<2>)})
    HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, upd_lds_bytes<double>()));
  // A of every fit, then (max_batch, max_p) logml for the calls that pass none
  return scratch_reserve(c, c->ma, max_batch, max_p, (multi_grad_a_doubles(c, max_batch, max_p) + (size_t)max_batch * max_p) * sizeof(double));
}

extern "C" int cgp_multi_nll_grad_batch_device(cgp_ctx *c, int batch, int N, int d, int P, int kid, const double *dX, const double *dY,
                                               const double *dtheta, const double *djitter, double *dnll, double *dgrad,
                                               int grad_stride, double *dlogml, int *dinfo, void *hip_stream) {
  int rc = multi_grad_check(c, batch, P);
  if (rc != CGP_OK) return rc;
  if ((rc = check_shape(c, batch, N, d, N, kid)) != CGP_OK) return rc;
  if (!dX || !dY || !dtheta || !dnll || !dgrad || !dinfo || grad_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  return multi_grad_enqueue(c, 0, batch, N, d, P, kid, dX, dY, dtheta, djitter, dnll, dgrad, grad_stride, dlogml, dinfo,
                            pick_stream(c, hip_stream));
}

extern "C" int cgp_multi_nll_grad_batch(cgp_ctx *c, int batch, int N, int d, int P, int kid, const double *X, const double *Y,
                                        const double *theta, int theta_stride, double *nll, double *grad, int grad_stride,
                                        double *logml, int *info) {
  int rc = multi_grad_check(c, batch, P);
  if (rc != CGP_OK) return rc;
  if ((rc = check_shape(c, batch, N, d, N, kid)) != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !Y || !theta || !nll || !grad || theta_stride < nth || grad_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  MultiGradStage st{};
  if ((rc = multi_grad_stage(c, batch, N, P, st)) != CGP_OK) return rc;
  if ((rc = multi_grad_upload(c, batch, N, d, P, X, Y, st)) != CGP_OK) return rc;
  std::vector<double> hth, hg((size_t)batch * CGP_MAX_THETA);
  if ((rc = upload_theta(c, theta, theta_stride, nth, batch, c->stream, hth)) != CGP_OK) return rc;
  std::vector<int> hinfo(batch);
  rc = multi_grad_eval_host(c, batch, N, d, P, kid, X, theta, theta_stride, st, nullptr, nll, hg.data(), logml, hinfo.data());
  if (rc != CGP_OK) return rc;
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < nth; ++i) grad[(size_t)b * grad_stride + i] = hg[(size_t)b * CGP_MAX_THETA + i];
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}

extern "C" int cgp_optimize_multi_batch(cgp_ctx *c, int batch, int N, int d, int P, int kid, const double *X, const double *Y,
                                        double *theta, int theta_stride, int max_evals, double *logml_sum, int *n_evals) {
  int rc = multi_grad_check(c, batch, P);
  if (rc != CGP_OK) return rc;
  if ((rc = check_shape(c, batch, N, d, N, kid)) != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !Y || !theta || theta_stride < nth) return CGP_EINVAL;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < nth; ++i)
      if (!(theta[(size_t)b * theta_stride + i] > 0.0)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  MultiGradStage stg{};
  if ((rc = multi_grad_stage(c, batch, N, P, stg)) != CGP_OK) return rc;
  if ((rc = multi_grad_upload(c, batch, N, d, P, X, Y, stg)) != CGP_OK) return rc;
  // the batched L-BFGS driver over the summed objective; a finished fit is evaluated at its best point and never retried
  std::vector<double> hth, nll(batch), hg((size_t)batch * CGP_MAX_THETA);
  std::vector<int> info(batch);
  std::vector<char> skip(batch, 0);
  auto round = [&](const double *th, const char *active, double *f, double *g, char *feasible) -> int {
    for (int b = 0; b < batch; ++b) skip[b] = !active[b];
    int rc = upload_theta(c, th, nth, nth, batch, c->stream, hth);
    if (rc != CGP_OK) return rc;
    // GPy jitchol inside m.optimize(): a trial point whose matrix is not positive definite climbs the ladder; one that stays
    // infeasible is +inf for the line search
    rc = multi_grad_eval_host(c, batch, N, d, P, kid, X, th, nth, stg, &skip, nll.data(), hg.data(), nullptr, info.data());
    if (rc != CGP_OK) return rc;
    for (int b = 0; b < batch; ++b) {
      if (!active[b]) continue;
      feasible[b] = info[b] == 0;
      f[b] = nll[b];
      std::copy(hg.data() + (size_t)b * CGP_MAX_THETA, hg.data() + (size_t)b * CGP_MAX_THETA + nth, g + (size_t)b * nth);
    }
    return CGP_OK;
  };
  corenav::LbfgsBatchResult res;
  if ((rc = corenav::lbfgs_minimize_logexp_batch(batch, nth, theta, theta_stride, nullptr, max_evals, round, res)) != CGP_OK) return rc;
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < nth; ++i) theta[(size_t)b * theta_stride + i] = res.theta[(size_t)b * nth + i];
    if (logml_sum) logml_sum[b] = -res.f[b];
    if (n_evals) n_evals[b] = res.evals[b];
  }
  return CGP_OK;
}
