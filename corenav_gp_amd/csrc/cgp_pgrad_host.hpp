// cgp_pgrad_host.hpp -- host side of the predictive gradients after batch / single fits (kernels: cgp_pgrad.hpp).  Not a
// translation unit of its own: cgp_engine.hip includes it after the fit entry points it builds on (fit_predict_device,
// fit_predict_batch_host, predict_enqueue); it uses nothing of the other features' host headers.  fp64 contexts only: every entry
// point answers CGP_EINVAL in a CGP_F32 context before anything is enqueued.
#pragma once

namespace {

// The arrays of a predictive-gradient call on the device (all pointers: the call's first fit): what pgrad_launch needs beside the
// factor panel.
struct PgradCall {
  const double *dX, *dXs, *dtheta;
  const int *dinfo;          // or null: a single fit known to be good
  double *ddmean, *ddvar;    // (batch, M, d); either may be null
};

// Backward solve and contraction of `nfit` fits whose panels are slabs slab, slab + 1, ... into the slots slot, slot + 1, ... of
// the call's arrays and of the scratch.  After run() has returned: a worker stream is joined by then.
int pgrad_launch(cgp_ctx *c, const PgradCall &pc, int N, int d, int M, int kid, int slab, int slot, int nfit, hipStream_t s) {
  PgradArgs a{};
  a.NT = cdiv(N, TS);
  a.stiles = cdiv(M + 1, PG_TR);
  a.ldb = cdiv(M + 1, TS) * TS;
  a.b_stride = (size_t)a.NT * TS * a.ldb;
  a.Lw = static_cast<const double *>(c->Lw) + (size_t)slab * c->lw_stride;
  a.lw_stride = c->lw_stride;
  a.ld = c->ld;
  a.Winv = static_cast<const double *>(c->Winv) + (size_t)slab * c->winv_stride;
  a.winv_stride = c->winv_stride;
  a.Bw = static_cast<double *>(c->pg.buf) + (size_t)slot * a.b_stride;
  a.X = pc.dX + (size_t)slot * d * N;
  a.Xs = pc.dXs + (size_t)slot * d * M;
  a.theta = pc.dtheta + (size_t)slot * CGP_MAX_THETA;
  a.info = pc.dinfo ? pc.dinfo + slot : nullptr;
  a.dmean = pc.ddmean ? pc.ddmean + (size_t)slot * M * d : nullptr;
  a.dvar = pc.ddvar ? pc.ddvar + (size_t)slot * M * d : nullptr;
  a.row0 = (size_t)a.NT * TS;
  a.N = N; a.d = d; a.M = M; a.nfit = nfit;
  unsigned gs = 0;
  if (nfit > 65535 || xcd_grid((long long)nfit * a.stiles, gs) != CGP_OK) return CGP_EINVAL;
  hipLaunchKernelGGL(k_pgrad_solve, dim3(gs), dim3(256), 0, s, a);
  const dim3 gc(cdiv(M, 64), nfit);
  if (kid == K_RBF_BROWNIAN) hipLaunchKernelGGL(k_pgrad_contract<PGK_BROWN>, gc, dim3(256), 0, s, a, kid);
  else if (kid == K_MATERN32_ARD) hipLaunchKernelGGL(k_pgrad_contract<PGK_M32>, gc, dim3(256), 0, s, a, kid);
  else if (kid == K_MATERN52_ARD) hipLaunchKernelGGL(k_pgrad_contract<PGK_M52>, gc, dim3(256), 0, s, a, kid);
  else hipLaunchKernelGGL(k_pgrad_contract<PGK_SE>, gc, dim3(256), 0, s, a, kid);
  if (!hip_ok(c, hipGetLastError(), "predictive gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

// the checks every predictive-gradient call starts with: dtype, reservation, the reservation's capacity
int pgrad_check(const cgp_ctx *c, int batch, int M) {
  if (!c || c->dtype != CGP_F64 || M < 1) return CGP_EINVAL;
  return scratch_check(c->pg, batch, M);
}

}  // namespace

extern "C" int cgp_pgrad_reserve(cgp_ctx *c, int max_batch, int max_m) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_m < 1 || max_m > c->max_m) return CGP_EINVAL;
  return scratch_reserve(c, c->pg, max_batch, max_m, (size_t)max_batch * c->NTmax * TS * ((size_t)cdiv(max_m + 1, TS) * TS) * sizeof(double));
}

extern "C" int cgp_fit_predict_grad_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *dX, const double *dy,
                                                 const double *dXs, const double *dtheta, const double *djitter, int include_noise,
                                                 double *dmean, double *dvar, double *dlogml, int *dinfo, double *ddmean, double *ddvar,
                                                 void *hip_stream) {
  int rc = pgrad_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (!dXs || !dmean || !dvar || (!ddmean && !ddvar)) return CGP_EINVAL;
  rc = fit_predict_device(c, batch, N, d, M, kid, dX, dy, dXs, dtheta, djitter, include_noise, dmean, dvar, dlogml, dinfo, hip_stream, true);
  if (rc != CGP_OK) return rc;
  return pgrad_launch(c, PgradCall{dX, dXs, dtheta, dinfo, ddmean, ddvar}, N, d, M, kid, 0, 0, batch, pick_stream(c, hip_stream));
}

extern "C" int cgp_fit_predict_grad_batch(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *X, const double *y,
                                          const double *Xs, const double *theta, int theta_stride, int include_noise, double *mean,
                                          double *var, double *logml, int *info, double *dmean, double *dvar) {
  int rc = pgrad_check(c, batch, M);
  if (rc != CGP_OK) return rc;
  if (!mean || !var || (!dmean && !dvar)) return CGP_EINVAL;
  if ((rc = check_shape(c, batch, N, d, M, kid)) != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t ng = (size_t)batch * M * d;
  if (!grow_device(c->pg.stage, c->pg.stage_cap, 2 * ng * sizeof(double))) return CGP_ENOMEM;
  double *ddmean = static_cast<double *>(c->pg.stage), *ddvar = ddmean + ng;
  const PgradCall pc{static_cast<const double *>(c->dX), static_cast<const double *>(c->dXs), c->dtheta, c->dinfo, dmean ? ddmean : nullptr,
                     dvar ? ddvar : nullptr};
  const auto hook = [&](int slab, int slot, int nfit, hipStream_t s) { return pgrad_launch(c, pc, N, d, M, kid, slab, slot, nfit, s); };
  const PostFit post = post_fit(hook);
  rc = fit_predict_batch_host(c, batch, N, d, M, kid, X, y, Xs, theta, theta_stride, include_noise, mean, var, logml, info, &post);
  if (rc < 0) return rc;
  if (dmean) HIP_TRY(c, hipMemcpyAsync(dmean, ddmean, ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (dvar) HIP_TRY(c, hipMemcpyAsync(dvar, ddvar, ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return rc;
}

// ---- after a single fit (cgp_fit / cgp_optimize): m.predictive_gradients(Xnew) ------------------------------------------------
extern "C" int cgp_predict_gradients(cgp_ctx *c, const double *Xs, int M, double *mean, double *var, double *dmean, double *dvar) {
  int rc = pgrad_check(c, 1, M);
  if (rc != CGP_OK) return rc;
  if (!Xs || (!dmean && !dvar)) return CGP_EINVAL;
  if ((rc = predict_enqueue(c, Xs, M, 0)) != CGP_OK) return rc;
  hipStream_t s = c->stream;
  const size_t ng = (size_t)M * c->fd;
  if (!grow_device(c->pg.stage, c->pg.stage_cap, 2 * ng * sizeof(double))) return CGP_ENOMEM;
  double *ddmean = static_cast<double *>(c->pg.stage), *ddvar = ddmean + ng;
  const PgradCall pc{static_cast<const double *>(c->dX), static_cast<const double *>(c->dXs), c->dtheta, nullptr, dmean ? ddmean : nullptr,
                     dvar ? ddvar : nullptr};
  if ((rc = pgrad_launch(c, pc, c->fN, c->fd, M, c->fkernel, 0, 0, 1, s)) != CGP_OK) return rc;
  if (mean) HIP_TRY(c, hipMemcpyAsync(mean, c->dmean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  if (var) HIP_TRY(c, hipMemcpyAsync(var, c->dvar, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dmean) HIP_TRY(c, hipMemcpyAsync(dmean, ddmean, ng * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dvar) HIP_TRY(c, hipMemcpyAsync(dvar, ddvar, ng * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}
