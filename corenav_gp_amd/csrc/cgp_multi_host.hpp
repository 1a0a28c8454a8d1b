// cgp_multi_host.hpp -- host side of the multi-target fits (kernels: cgp_multi.hpp).  Not a translation unit of its own:
// cgp_engine.hip includes it after the fit entry points it builds on (fit_predict_device, fit_predict_batch_host) and after
// cgp_joint_host.hpp.  fp64 contexts only: every entry point answers CGP_EINVAL in a CGP_F32 context before anything is enqueued.
#pragma once

namespace {

constexpr int MULTI_MAX_P = 4096;   // corenav_gp.h states it

constexpr int multi_lds_bytes() { return std::max(upd_lds_bytes<double>(), WIMG * (int)sizeof(double)); }

// Tile height of the solve, from (fits, P) ONLY -- never from N or M, so a column's bits can be followed from the call's size.  Half
// tiles while 128-row tiles would leave CUs without a workgroup: the chain over all of N is the launch's length either way, and a
// half tile whose upper waves are padding issues no MFMA for them (the 128-row form computes all four waves).
inline bool multi_rows64(const cgp_ctx *c, int nfit, int P) {
  if (c->mz_form == 64) return true;
  if (c->mz_form == 128) return false;
  return (long long)nfit * cdiv(P, TS) < 256;
}

// The arguments of the launches for `nfit` fits whose panels are slabs slab, slab + 1, ... and whose targets, right-hand sides and
// outputs are the slots slot, slot + 1, ... of the call's arrays (all pointers: the call's first fit).
MultiArgs multi_args(cgp_ctx *c, int N, int M, int P, int slab, int slot, int nfit, const double *dY, double *dy0, double *dmean,
                     double *dvar, double *dlogml, const int *dinfo) {
  MultiArgs a{};
  a.NT = cdiv(N, TS);
  a.ldz = cdiv(P, TS) * TS;
  a.z_stride = (size_t)a.NT * TS * a.ldz;
  a.Lw = static_cast<const double *>(c->Lw) + (size_t)slab * c->lw_stride;
  a.lw_stride = c->lw_stride;
  a.ld = c->ld;
  a.Winv = static_cast<const double *>(c->Winv) + (size_t)slab * c->winv_stride;
  a.winv_stride = c->winv_stride;
  a.Zw = static_cast<double *>(c->mz.buf) + (size_t)slot * a.z_stride;
  a.Y = dY + (size_t)slot * P * N;
  a.y0 = dy0 ? dy0 + (size_t)slot * N : nullptr;
  a.mean = dmean ? dmean + (size_t)slot * P * M : nullptr;
  a.var = dvar ? dvar + (size_t)slot * M : nullptr;
  a.logml = dlogml ? dlogml + (size_t)slot * P : nullptr;
  a.info = dinfo ? dinfo + slot : nullptr;
  a.row0 = (size_t)a.NT * TS;
  a.N = N; a.M = M; a.P = P; a.nfit = nfit;
  a.pt = cdiv(P, WPB);
  a.mt = cdiv(M, WPB);
  a.nsm = cdiv(a.mt, WJ_ST);
  a.npair = cdiv(a.pt, WJ_ST) * a.nsm;
  a.per_fit = cdiv(a.npair, WJ_WAVES);
  return a;
}

// Y^T into the scratch (and column 0 into dy0, when given)
int multi_pack_launch(cgp_ctx *c, const MultiArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_multi_pack, dim3(a.NT * TS / MP_TILE, a.ldz / MP_TILE, a.nfit), dim3(MP_TILE * 8), 0, s, a);
  if (!hip_ok(c, hipGetLastError(), "multi-target pack launch")) return CGP_EHIP;
  return CGP_OK;
}

// Z = L^-1 Y in place: the tile height chosen (a.stiles follows it: the later launches of the call read it), one launch
int multi_solve_launch(cgp_ctx *c, MultiArgs &a, hipStream_t s) {
  const bool h64 = multi_rows64(c, a.nfit, a.P);
  a.stiles = cdiv(a.P, h64 ? HR : TS);
  unsigned gs = 0;
  if (xcd_grid((long long)a.nfit * a.stiles, gs) != CGP_OK) return CGP_EINVAL;
  if (h64) hipLaunchKernelGGL(k_multi_solve<true>, dim3(gs), dim3(256), multi_lds_bytes(), s, a);
  else hipLaunchKernelGGL(k_multi_solve<false>, dim3(gs), dim3(256), multi_lds_bytes(), s, a);
  return CGP_OK;
}

// after the fits: the solve, mean = V^T Z, logml; three launches
int multi_post_launch(cgp_ctx *c, MultiArgs a, hipStream_t s) {
  unsigned gm = 0;
  if (xcd_grid((long long)a.nfit * a.per_fit, gm) != CGP_OK || multi_solve_launch(c, a, s) != CGP_OK) return CGP_EINVAL;
  hipLaunchKernelGGL(k_multi_mean, dim3(gm), dim3(WJ_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_multi_logml, dim3(a.nfit), dim3(ML_THREADS), 0, s, a);
  if (!hip_ok(c, hipGetLastError(), "multi-target solve / mean launches")) return CGP_EHIP;
  return CGP_OK;
}

// the checks every multi-target call starts with: dtype, counts, reservation, the reservation's capacity
int multi_check(const cgp_ctx *c, int batch, int M, int P) {
  if (!c || c->dtype != CGP_F64 || M < 1 || P < 1) return CGP_EINVAL;
  return scratch_check(c->mz, batch, P);
}

}  // namespace

extern "C" int cgp_multi_reserve(cgp_ctx *c, int max_batch, int max_p) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_p < 1 || max_p > MULTI_MAX_P) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));   // (the attribute goes to the current device's function)
  for (const void *fn : {reinterpret_cast<const void *>(&k_multi_solve<true>), reinterpret_cast<const void *>(&k_multi_solve<false>)})
    HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, multi_lds_bytes()));
  return scratch_reserve(c, c->mz, max_batch, max_p, (size_t)max_batch * c->NTmax * TS * ((size_t)cdiv(max_p, TS) * TS) * sizeof(double));
}

extern "C" int cgp_multi_set_form(cgp_ctx *c, int rows) {
  if (!c || (rows != 0 && rows != HR && rows != TS)) return CGP_EINVAL;
  c->mz_form = rows;
  return CGP_OK;
}

extern "C" int cgp_fit_predict_multi_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int P, int kid, const double *dX,
                                                  const double *dY, const double *dXs, const double *dtheta, const double *djitter,
                                                  int include_noise, double *dmean, double *dvar, double *dlogml, int *dinfo,
                                                  void *hip_stream) {
  int rc = multi_check(c, batch, M, P);
  if (rc != CGP_OK) return rc;
  if (!dX || !dY || !dXs || !dtheta || !dmean || !dvar || !dlogml || !dinfo) return CGP_EINVAL;
  if ((rc = check_shape(c, batch, N, d, M, kid)) != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick_stream(c, hip_stream);
  // the fit schedule wants a y: column 0, gathered into the context's dy; its own mean / logml are by-products and stay there
  double *dy0 = static_cast<double *>(c->dy);
  const MultiArgs a = multi_args(c, N, M, P, 0, 0, batch, dY, dy0, dmean, dvar, dlogml, dinfo);
  if ((rc = multi_pack_launch(c, a, s)) != CGP_OK) return rc;
  rc = fit_predict_device(c, batch, N, d, M, kid, dX, dy0, dXs, dtheta, djitter, include_noise, c->dmean, dvar, c->dlogml, dinfo, hip_stream,
                          true);
  if (rc != CGP_OK) return rc;
  return multi_post_launch(c, a, s);
}

extern "C" int cgp_fit_predict_multi_batch(cgp_ctx *c, int batch, int N, int d, int M, int P, int kid, const double *X, const double *Y,
                                           const double *Xs, const double *theta, int theta_stride, int include_noise, double *mean,
                                           double *var, double *logml, int *info) {
  int rc = multi_check(c, batch, M, P);
  if (rc != CGP_OK) return rc;
  if (!X || !Y || !Xs || !theta || !mean || !var) return CGP_EINVAL;
  if ((rc = check_shape(c, batch, N, d, M, kid)) != CGP_OK) return rc;
  if (theta_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t B = batch, nY = B * P * N, nmean = B * P * M, nl = B * P;
  if (!grow_device(c->mz.stage, c->mz.stage_cap, (nY + nmean + nl) * sizeof(double))) return CGP_ENOMEM;
  double *dY = static_cast<double *>(c->mz.stage), *dmean = dY + nY, *dlogml = dmean + nmean;
  HIP_TRY(c, hipMemcpyAsync(dY, Y, nY * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::vector<double> y0(B * N);   // the fit schedule's y: each fit's column 0
  for (size_t b = 0; b < B; ++b) memcpy(&y0[b * N], Y + b * P * N, (size_t)N * sizeof(double));
  std::vector<int> hinfo(B);
  // after the fits: their targets are packed again (a retried fit's right-hand sides were solved in place against the factor that
  // failed), solved and contracted
  const auto hook = [&](int slab, int slot, int nfit, hipStream_t s) {
    const MultiArgs a = multi_args(c, N, M, P, slab, slot, nfit, dY, nullptr, dmean, static_cast<double *>(c->dvar), dlogml, c->dinfo);
    const int r = multi_pack_launch(c, a, s);
    return r != CGP_OK ? r : multi_post_launch(c, a, s);
  };
  const PostFit post = post_fit(hook);
  rc = fit_predict_batch_host(c, batch, N, d, M, kid, X, y0.data(), Xs, theta, theta_stride, include_noise, nullptr, var, nullptr,
                              hinfo.data(), &post);
  if (rc < 0) return rc;
  HIP_TRY(c, hipMemcpyAsync(mean, dmean, nmean * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  std::vector<double> hl(logml ? nl : 0);
  if (logml) HIP_TRY(c, hipMemcpyAsync(hl.data(), dlogml, nl * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (logml) memcpy(logml, hl.data(), nl * sizeof(double));
  if (info) memcpy(info, hinfo.data(), B * sizeof(int));
  return rc;
}
