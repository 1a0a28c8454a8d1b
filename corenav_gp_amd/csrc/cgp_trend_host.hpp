// cgp_trend_host.hpp -- host side of the explicit-basis (trend) fits (kernels: cgp_trend.hpp).  Not a translation unit of its own:
// cgp_engine.hip includes it after cgp_multi_host.hpp, whose launches it reuses on the P + q packed columns [Y | H].  fp64 contexts
// only: every entry point answers CGP_EINVAL in a CGP_F32 context before anything is enqueued.
#pragma once

namespace {

// The trend reservation's scratch, sized by (max_batch, max_p, max_m); a call's blocks start at the reservation's section bases and
// are strided by the call's own P, q, M:   [mean0 (fit, P + q, M) | logml0 (fit, P + q) | S (fit, ncol, 16) | Linv (fit, 16, 16)]
struct TrendLayout {
  size_t mean0, logml0, S, Linv, total;   // in doubles
};
inline TrendLayout trend_layout(int max_batch, int max_p, int max_m) {
  const size_t B = max_batch, W = (size_t)max_p + TR_MAX;
  TrendLayout l{};
  l.mean0 = 0;
  l.logml0 = l.mean0 + B * W * max_m;
  l.S = l.logml0 + B * W;
  l.Linv = l.S + B * (size_t)cdiv((int)W, TR_MAX) * TR_MAX * TR_MAX;
  l.total = l.Linv + B * TR_MAX * TR_MAX;
  return l;
}

struct TrendCall {   // the call's arrays (device, the call's first fit) and shape
  int N, M, P, q;
  const double *Y, *H, *Hs;
  double *mean, *var, *beta, *logml;
  const int *info;
  int *tinfo;
};

// The two argument records of the launches for `nfit` fits whose panels are slabs slab, slab + 1, ... and whose arrays are the
// slots slot, slot + 1, ...: the multi-target record over the P + q packed columns (its mean / logml: the trend scratch) and the
// trend record.
void trend_args(cgp_ctx *c, const TrendCall &k, int slab, int slot, int nfit, double *dy0, MultiArgs &ma, TrendArgs &ta) {
  const TrendLayout l = trend_layout(c->tr.max_batch, c->tr.max_dim, c->tr_max_m);
  double *buf = static_cast<double *>(c->tr.buf);
  const int W = k.P + k.q;
  // (the multi-target record's Y is not read: k_trend_pack packs)
  ma = multi_args(c, k.N, k.M, W, slab, slot, nfit, k.Y, nullptr, buf + l.mean0, k.var, buf + l.logml0, k.info);
  ma.Y = nullptr;
  ta = TrendArgs{};
  ta.Y = k.Y + (size_t)slot * k.P * k.N;
  ta.H = k.H + (size_t)slot * k.q * k.N;
  ta.y0 = dy0 ? dy0 + (size_t)slot * k.N : nullptr;
  ta.Zw = ma.Zw;
  ta.z_stride = ma.z_stride;
  ta.ldz = ma.ldz;
  ta.NT = ma.NT;
  ta.N = k.N; ta.M = k.M; ta.P = k.P; ta.q = k.q; ta.nfit = nfit;
  ta.ncol = cdiv(W, TR_MAX) * TR_MAX;
  ta.S = buf + l.S + (size_t)slot * ta.ncol * TR_MAX;
  ta.Linv = buf + l.Linv + (size_t)slot * TR_MAX * TR_MAX;
  ta.mean0 = ma.mean;
  ta.logml0 = ma.logml;
  ta.Hs = k.Hs + (size_t)slot * k.q * k.M;
  ta.mean = k.mean + (size_t)slot * k.P * k.M;
  ta.var = k.var + (size_t)slot * k.M;
  ta.beta = k.beta + (size_t)slot * k.P * k.q;
  ta.logml = k.logml + (size_t)slot * k.P;
  ta.info = k.info + slot;
  ta.info_stride = 1;
  ta.tinfo = k.tinfo + slot;
}

int trend_pack_launch(cgp_ctx *c, const TrendArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_trend_pack, dim3(a.NT * TS / MP_TILE, a.ldz / MP_TILE, a.nfit), dim3(MP_TILE * 8), 0, s, a);
  if (!hip_ok(c, hipGetLastError(), "trend pack launch")) return CGP_EHIP;
  return CGP_OK;
}

// after the fits: the multi-target solve / contraction / evidence over the P + q columns, then the three trend launches
int trend_post_launch(cgp_ctx *c, const MultiArgs &ma, const TrendArgs &a, hipStream_t s) {
  const int rc = multi_post_launch(c, ma, s);
  if (rc != CGP_OK) return rc;
  hipLaunchKernelGGL(k_trend_gram<false>, dim3(a.ncol / TR_MAX, a.nfit), dim3(TG_WAVES * 64), 0, s, a);
  hipLaunchKernelGGL(k_trend_solve, dim3(a.nfit), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_trend_apply, dim3(cdiv(a.M, TA_THREADS), cdiv(a.P, TA_PCH), a.nfit), dim3(TA_THREADS), 0, s, a);
  if (!hip_ok(c, hipGetLastError(), "trend gram / solve / apply launches")) return CGP_EHIP;
  return CGP_OK;
}

// the checks every trend call starts with: dtype, counts, the two reservations and their capacities
int trend_check(const cgp_ctx *c, int batch, int M, int P, int q) {
  if (!c || c->dtype != CGP_F64 || M < 1 || P < 1 || q < 1 || q > TR_MAX) return CGP_EINVAL;
  int rc = scratch_check(c->tr, batch, P);
  if (rc != CGP_OK) return rc;
  if (M > c->tr_max_m) return CGP_ECAPACITY;
  return scratch_check(c->mz, batch, P + q);
}

}  // namespace

extern "C" int cgp_trend_reserve(cgp_ctx *c, int max_batch, int max_p, int max_m) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_p < 1 || max_p > MULTI_MAX_P - TR_MAX || max_m < 1 || max_m > c->max_m)
    return CGP_EINVAL;
  if (max_batch > c->mz.max_batch || max_p + TR_MAX > c->mz.max_dim) return CGP_ESTATE;   // cgp_multi_reserve first, and one that covers this
  const int rc = scratch_reserve(c, c->tr, max_batch, max_p, trend_layout(max_batch, max_p, max_m).total * sizeof(double));
  c->tr_max_m = rc == CGP_OK ? max_m : 0;
  return rc;
}

extern "C" int cgp_fit_predict_trend_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int P, int q, int kid, const double *dX,
                                                  const double *dY, const double *dH, const double *dXs, const double *dHs,
                                                  const double *dtheta, const double *djitter, int include_noise, double *dmean,
                                                  double *dvar, double *dbeta, double *dlogml, int *dinfo, int *dtinfo,
                                                  void *hip_stream) {
  int rc = trend_check(c, batch, M, P, q);
  if (rc != CGP_OK) return rc;
  if (!dX || !dY || !dH || !dXs || !dHs || !dtheta || !dmean || !dvar || !dbeta || !dlogml || !dinfo || !dtinfo) return CGP_EINVAL;
  if ((rc = check_shape(c, batch, N, d, M, kid)) != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = pick_stream(c, hip_stream);
  double *dy0 = static_cast<double *>(c->dy);   // the fit schedule's y: target 0, as in the multi-target call
  const TrendCall k{N, M, P, q, dY, dH, dHs, dmean, dvar, dbeta, dlogml, dinfo, dtinfo};
  MultiArgs ma;
  TrendArgs ta;
  trend_args(c, k, 0, 0, batch, dy0, ma, ta);
  if ((rc = trend_pack_launch(c, ta, s)) != CGP_OK) return rc;
  rc = fit_predict_device(c, batch, N, d, M, kid, dX, dy0, dXs, dtheta, djitter, include_noise, c->dmean, dvar, c->dlogml, dinfo, hip_stream,
                          true);
  if (rc != CGP_OK) return rc;
  return trend_post_launch(c, ma, ta, s);
}

extern "C" int cgp_fit_predict_trend_batch(cgp_ctx *c, int batch, int N, int d, int M, int P, int q, int kid, const double *X,
                                           const double *Y, const double *H, const double *Xs, const double *Hs, const double *theta,
                                           int theta_stride, int include_noise, double *mean, double *var, double *beta, double *logml,
                                           int *info, int *tinfo) {
  int rc = trend_check(c, batch, M, P, q);
  if (rc != CGP_OK) return rc;
  if (!X || !Y || !H || !Xs || !Hs || !theta || !mean || !var) return CGP_EINVAL;
  if ((rc = check_shape(c, batch, N, d, M, kid)) != CGP_OK) return rc;
  if (theta_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // staging: [Y | H | Hs | mean | beta | logml | tinfo]
  const size_t B = batch, nY = B * P * N, nH = B * q * N, nHs = B * q * M, nmean = B * P * M, nb = B * P * q, nl = B * P;
  if (!grow_device(c->tr.stage, c->tr.stage_cap, (nY + nH + nHs + nmean + nb + nl) * sizeof(double) + B * sizeof(int))) return CGP_ENOMEM;
  double *dY = static_cast<double *>(c->tr.stage), *dH = dY + nY, *dHs = dH + nH, *dmean = dHs + nHs, *dbeta = dmean + nmean,
         *dlogml = dbeta + nb;
  int *dtinfo = reinterpret_cast<int *>(dlogml + nl);
  HIP_TRY(c, hipMemcpyAsync(dY, Y, nY * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dH, H, nH * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dHs, Hs, nHs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::vector<double> y0(B * N);   // the fit schedule's y: each fit's target 0
  for (size_t b = 0; b < B; ++b) memcpy(&y0[b * N], Y + b * P * N, (size_t)N * sizeof(double));
  std::vector<int> hinfo(B), htinfo(B);
  const TrendCall k{N, M, P, q, dY, dH, dHs, dmean, static_cast<double *>(c->dvar), dbeta, dlogml, c->dinfo, dtinfo};
  // after the fits: their columns are packed again (a retried fit's were solved in place against the factor that failed), solved,
  // contracted, and the trend is computed into the fit's own slot
  const auto hook = [&](int slab, int slot, int nfit, hipStream_t s) {
    MultiArgs ma;
    TrendArgs ta;
    trend_args(c, k, slab, slot, nfit, nullptr, ma, ta);
    const int r = trend_pack_launch(c, ta, s);
    return r != CGP_OK ? r : trend_post_launch(c, ma, ta, s);
  };
  const PostFit post = post_fit(hook);
  rc = fit_predict_batch_host(c, batch, N, d, M, kid, X, y0.data(), Xs, theta, theta_stride, include_noise, nullptr, var, nullptr,
                              hinfo.data(), &post);
  if (rc < 0) return rc;
  std::vector<double> hb(beta ? nb : 0), hl(logml ? nl : 0);
  HIP_TRY(c, hipMemcpyAsync(mean, dmean, nmean * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (beta) HIP_TRY(c, hipMemcpyAsync(hb.data(), dbeta, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (logml) HIP_TRY(c, hipMemcpyAsync(hl.data(), dlogml, nl * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(htinfo.data(), dtinfo, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (beta) memcpy(beta, hb.data(), nb * sizeof(double));
  if (logml) memcpy(logml, hl.data(), nl * sizeof(double));
  if (info) memcpy(info, hinfo.data(), B * sizeof(int));
  if (tinfo) memcpy(tinfo, htinfo.data(), B * sizeof(int));
  return rc;
}
