// cgp_sparse_host.hpp -- host side of the sparse (inducing-point) fits (kernels: cgp_sparse.hpp).  Not a translation unit of its
// own: cgp_engine.hip includes it after cgp_trend_host.hpp.  Nothing here touches the dense schedules or their buffers: the sparse
// reservation holds all the scratch of these calls, and N is bounded by it alone.  fp64 contexts only: every entry point answers
// CGP_EINVAL in a CGP_F32 context before anything is enqueued.
#pragma once

namespace {

constexpr int kSparseMaxN = 1 << 24;   // samples of a history (the index arithmetic of the kernels is 32-bit below d x N)

// The sparse reservation's scratch, sized by (max_batch, max_n, max_m_ind); a call's blocks start at the section bases and are
// strided by the call's own shape (sparse_shape).  In doubles, with mt = ceil((max_m_ind + 1) / 16), LD = 16 mt:
//   [rec (fit, 16) | part (fit, chunks(max_n), mt (mt + 1) / 2, 256) | U, F, W (fit, LD, LD) each | dinv (fit, 2, mt, 256) |
//    vec (fit, 4, LD) | scal (fit, 8)]
struct SparseLayout {
  size_t rec, part, U, F, W, dinv, vec, scal, total;
};
inline SparseLayout sparse_layout(int max_batch, int max_n, int max_m_ind) {
  const SparseShape sh = sparse_shape(max_n, max_m_ind, 1);
  const size_t B = max_batch, LD2 = (size_t)sh.LD * sh.LD;
  SparseLayout l{};
  l.rec = 0;
  l.part = l.rec + B * PREP_N;
  l.U = l.part + B * sh.nch * sh.ntile * 256;
  l.F = l.U + B * LD2;
  l.W = l.F + B * LD2;
  l.dinv = l.W + B * LD2;
  l.vec = l.dinv + B * 2 * sh.mt * 256;
  l.scal = l.vec + B * 4 * sh.LD;
  l.total = l.scal + B * 8;
  return l;
}

struct SparseCall {   // the call's arrays (device, the call's first fit) and shape
  int N, d, M, m, kid, include_noise;
  const double *X, *y, *Z, *Xs, *theta, *jitter;
  double *mean, *var, *logml;
  int *info;
  int P = 1;   // target columns: y (fit, P, N), mean (fit, P, M), logml (fit, P); more than one in cgp_sparse_multi_host.hpp's calls only
};

// the argument record of the launches for the `nfit` fits in slots slot, slot + 1, ... of the call's arrays and of the scratch
SparseArgs sparse_args(const cgp_ctx *c, const SparseCall &k, int slot, int nfit) {
  const SparseLayout l = sparse_layout(c->sp.max_batch, c->sp_max_n, c->sp.max_dim);
  double *buf = static_cast<double *>(c->sp.buf);
  const size_t s = slot;
  SparseArgs a{};
  a.sh = sparse_shape(k.N, k.m, k.d, k.P);
  const size_t LD = a.sh.LD, LD2 = LD * LD;
  a.X = k.X + s * k.d * k.N;
  a.y = k.y + s * k.P * k.N;
  a.Z = k.Z + s * k.d * k.m;
  a.Xs = k.Xs ? k.Xs + s * k.d * k.M : nullptr;
  a.theta = k.theta + s * MAX_THETA;
  a.jitter = k.jitter ? k.jitter + s : nullptr;
  a.mean = k.mean ? k.mean + s * k.P * k.M : nullptr;
  a.var = k.var ? k.var + s * k.M : nullptr;
  a.logml = k.logml + s * k.P;
  a.info = k.info + s;
  a.rec = buf + l.rec + s * PREP_N;
  a.part = buf + l.part + s * a.sh.nch * a.sh.nt0 * 256;
  a.U = buf + l.U + s * LD2;
  a.F = buf + l.F + s * LD2;
  a.W = buf + l.W + s * LD2;
  a.dinv = buf + l.dinv + s * 2 * a.sh.mt * 256;
  a.vec = buf + l.vec + s * 4 * LD;
  a.scal = buf + l.scal + s * 8;
  // one target column: b, c and yty where the gradient kernels read them (sparse_multi_args points several elsewhere)
  a.bm = a.vec;
  a.cm = a.vec + LD;
  a.yty = a.scal;
  a.bcs = (int)(4 * LD);
  a.ytys = 8;
  a.P = k.P;
  a.N = k.N; a.d = k.d; a.M = k.M; a.m = k.m; a.kid = k.kid; a.include_noise = k.include_noise; a.nfit = nfit;
  return a;
}

// the linear chain of a sparse call on s; profile slots (cgp_profile_read): 0 k_sparse_phi, 1 k_sparse_algebra, 2 k_sparse_reduce,
// 3 k_sparse_predict, 4 k_sparse_prep
int sparse_enqueue(cgp_ctx *c, const SparseArgs &a, hipStream_t s) {
  Launcher L{c, s};
  const SparseShape &sh = a.sh;
  const double mm = a.m, fits = a.nfit;
  L.begin(4, 0.0);
  hipLaunchKernelGGL(k_sparse_prep, dim3(cdiv(a.nfit, 64)), dim3(64), 0, s, a);
  L.end();
  L.begin(0, fits * a.N * (mm + a.P) * (mm + a.P + 1));
  hipLaunchKernelGGL(k_sparse_phi, dim3(sh.ngrp, sh.nch, a.nfit), dim3(SP_THREADS), sparse_phi_lds(a.d, sh.LDa, sh.S, sh.ldr), s, a);
  L.end();
  L.begin(2, fits * sh.nch * sh.ntile * 256);
  hipLaunchKernelGGL(k_sparse_reduce, dim3(sh.ntile, a.nfit), dim3(256), 0, s, a);
  L.end();
  L.begin(1, fits * (8.0 / 3.0) * mm * mm * mm);   // two factorisations, two m x m solves
  hipLaunchKernelGGL(k_sparse_algebra, dim3(a.nfit), dim3(SPA_THREADS), 0, s, a);
  L.end();
  if (a.M > 0) {
    const int nw = sparse_predict_waves(sh.LD);
    L.begin(3, fits * 2.0 * mm * mm * a.M);
    hipLaunchKernelGGL(k_sparse_predict, dim3(cdiv(cdiv(a.M, WPB), nw), a.nfit), dim3(64 * nw), (size_t)nw * sh.LD * WPB * sizeof(double), s, a);
    L.end();
  }
  if (!hip_ok(c, hipGetLastError(), "sparse launches")) return CGP_EHIP;
  return CGP_OK;
}

// the checks every sparse call starts with: dtype, the reservation and its capacities, then the shape
int sparse_check(const cgp_ctx *c, int batch, int N, int d, int M, int m, int kid) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (batch < 1 || N < 1 || d < 1 || M < 0 || m < 1 || m > SP_MAX_IND) return CGP_EINVAL;
  if (kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  const int rc = scratch_check(c->sp, batch, m);
  if (rc != CGP_OK) return rc;
  if (N > c->sp_max_n || M > c->sp_max_m || d > c->max_d || batch > c->max_batch) return CGP_ECAPACITY;
  return CGP_OK;
}

}  // namespace

extern "C" int cgp_sparse_chunk(void) { return SP_CHUNK; }

extern "C" int cgp_sparse_reserve(cgp_ctx *c, int max_batch, int max_n, int max_m_ind, int max_m) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_n < 1 || max_n > kSparseMaxN || max_m_ind < 1 || max_m_ind > SP_MAX_IND ||
      max_m < 0)
    return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));   // (the attribute goes to the current device's function)
  HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sparse_phi), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kLdsPerWorkgroup));
  HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sparse_predict), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kLdsPerWorkgroup));
  const int rc = scratch_reserve(c, c->sp, max_batch, max_m_ind, sparse_layout(max_batch, max_n, max_m_ind).total * sizeof(double));
  c->sp_max_n = rc == CGP_OK ? max_n : 0;
  c->sp_max_m = rc == CGP_OK ? max_m : 0;
  return rc;
}

extern "C" int cgp_fit_predict_sparse_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int m, int kid, const double *dX,
                                                   const double *dy, const double *dZ, const double *dXs, const double *dtheta,
                                                   const double *djitter, int include_noise, double *dmean, double *dvar,
                                                   double *dlogml, int *dinfo, void *hip_stream) {
  const int rc = sparse_check(c, batch, N, d, M, m, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dy || !dZ || !dtheta || !dlogml || !dinfo || (M > 0 && (!dXs || !dmean || !dvar))) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const SparseCall k{N, d, M, m, kid, include_noise, dX, dy, dZ, dXs, dtheta, djitter, dmean, dvar, dlogml, dinfo};
  return sparse_enqueue(c, sparse_args(c, k, 0, batch), pick_stream(c, hip_stream));
}

extern "C" int cgp_fit_predict_sparse_batch(cgp_ctx *c, int batch, int N, int d, int M, int m, int kid, const double *X, const double *y,
                                            const double *Z, const double *Xs, const double *theta, int theta_stride, int include_noise,
                                            double *mean, double *var, double *logml, int *info) {
  int rc = sparse_check(c, batch, N, d, M, m, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !Z || !theta || (M > 0 && (!Xs || !mean || !var))) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  if (theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // staging: the caller's row-major [X | Z | Xs], then what the device form takes: [dX | dZ | dXs | dy | theta | mean | var | logml]
  const size_t B = batch, nX = B * N * d, nZ = B * m * d, nXs = B * (size_t)M * d, ny = B * N, nth_all = B * CGP_MAX_THETA, nM = B * M;
  const size_t nraw = nX + nZ + nXs;
  if (!grow_device(c->sp.stage, c->sp.stage_cap, (2 * nraw + ny + nth_all + 2 * nM + B) * sizeof(double))) return CGP_ENOMEM;
  double *raw = static_cast<double *>(c->sp.stage), *dX = raw + nraw, *dZ = dX + nX, *dXs = dZ + nZ, *dy = dXs + nXs, *dth = dy + ny,
         *dmean = dth + nth_all, *dvar = dmean + nM, *dlogml = dvar + nM;
  std::vector<double> hth(nth_all, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (int q = 0; q < nth; ++q) hth[b * CGP_MAX_THETA + q] = theta[b * theta_stride + q];
  HIP_TRY(c, hipMemcpyAsync(raw, X, nX * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(raw + nX, Z, nZ * sizeof(double), hipMemcpyHostToDevice, s));
  if (M > 0) HIP_TRY(c, hipMemcpyAsync(raw + nX + nZ, Xs, nXs * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(dy, y, ny * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(dth, hth.data(), nth_all * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  auto pack = [&](const double *src, double *dst, int n) {
    hipLaunchKernelGGL(k_pack_soa<double>, dim3(std::min(64, cdiv(n * d, 256)), batch), dim3(256), 0, s, src, dst, n, d);
  };
  pack(raw, dX, N);
  pack(raw + nX, dZ, m);
  if (M > 0) pack(raw + nX + nZ, dXs, M);
  const SparseCall k{N, d, M, m, kid, include_noise, dX, dy, dZ, M > 0 ? dXs : nullptr, dth, c->djitter,
                     M > 0 ? dmean : nullptr, M > 0 ? dvar : nullptr, dlogml, c->dinfo};
  if ((rc = sparse_enqueue(c, sparse_args(c, k, 0, batch), s)) != CGP_OK) return rc;
  std::vector<int> hinfo(B);
  HIP_TRY(c, hipMemcpyAsync(hinfo.data(), c->dinfo, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  // the fits whose K_uu failed climb the jitter ladder of the dense calls, on K_uu's own diagonal: mean(diag) over the inducing
  // inputs.  (A failing pivot of B is not a matter of K_uu's jitter: it is reported as it is.)
  std::vector<char> skip(B, 0);
  for (size_t b = 0; b < B; ++b) skip[b] = hinfo[b] > m;
  std::vector<double> hjit(B, 0.0);
  rc = jitter_ladder(c, batch, m, d, kid, theta, theta_stride, Z, hinfo.data(), &skip, hjit.data(), s,
                     [&](int b) { return sparse_enqueue(c, sparse_args(c, k, b, 1), s); });
  if (rc != CGP_OK) return rc;
  std::vector<double> hl(B);
  if (M > 0) {
    HIP_TRY(c, hipMemcpyAsync(mean, dmean, nM * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(var, dvar, nM * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(c, hipMemcpyAsync(hl.data(), dlogml, B * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    if (logml) logml[b] = hl[b];
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}
