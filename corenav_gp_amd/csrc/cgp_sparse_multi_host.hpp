// cgp_sparse_multi_host.hpp -- host side of the sparse fits with P target columns on one (X, Z, theta): one Phi, one pair of
// factors and one variance for the P bounds and mean rows.  Not a translation unit of its own: cgp_engine.hip includes it after
// cgp_sparse_grad_host.hpp.  The kernels are the sparse section's own (cgp_sparse.hpp: the single-column calls run them with P = 1),
// the launches sparse_enqueue's; what is here is the reservation that holds what P columns add, and the two entry points.
#pragma once

namespace {

// The multi reservation's scratch, sized by (max_batch, max_p) and the sparse reservation's (max_n, max_m_ind) as they stood; a
// call's blocks start at the section bases and are strided by the call's own shape.  In doubles, with mt = ceil((max_m_ind + 1) /
// 16), LD = 16 mt, C = chunks(max_n) and k = ceil((max_p - 1) / 16), the tile rows that the targets of a call can add to its m x m
// objects' (the count is not monotone in m -- m = 14 with P = 3 adds a tile row, m = 17 does not -- so it is bounded, not evaluated
// at the maxima: a call's mta <= its mt + k, and (mt + k)(mt + k + 1) / 2 - mt (mt + 1) / 2 grows with mt):
//   [partx (fit, C, k mt + k (k + 1) / 2, 256) | bc (fit, 2, max_p, LD) | yty (fit, max_p)]
struct SparseMultiLayout {
  size_t partx, bc, yty, total;
};
inline SparseMultiLayout sparse_multi_layout(int max_batch, int max_n, int max_m_ind, int max_p) {
  const SparseShape sh = sparse_shape(max_n, max_m_ind, 1);
  const size_t B = max_batch, k = (max_p - 1 + 15) / 16;
  SparseMultiLayout l{};
  l.partx = 0;
  l.bc = l.partx + B * sh.nch * (k * sh.mt + k * (k + 1) / 2) * 256;
  l.yty = l.bc + B * 2 * max_p * sh.LD;
  l.total = l.yty + B * max_p;
  return l;
}

// sparse_args with the targets' vectors and the further tile rows in the multi reservation
SparseArgs sparse_multi_args(const cgp_ctx *c, const SparseCall &k, int slot, int nfit) {
  const SparseMultiLayout l = sparse_multi_layout(c->sm.max_batch, c->sm_max_n, c->sm_max_ind, c->sm.max_dim);
  double *buf = static_cast<double *>(c->sm.buf);
  const size_t s = slot;
  SparseArgs a = sparse_args(c, k, slot, nfit);
  a.bcs = 2 * k.P * a.sh.LD;
  a.ytys = k.P;
  a.partx = buf + l.partx + s * a.sh.nch * (a.sh.ntile - a.sh.nt0) * 256;
  a.bm = buf + l.bc + s * a.bcs;
  a.cm = a.bm + (size_t)k.P * a.sh.LD;
  a.yty = buf + l.yty + s * k.P;
  return a;
}

// the sparse section's checks, the column count among the counts and the multi reservation beside the sparse one
int sparse_multi_check(const cgp_ctx *c, int batch, int N, int d, int M, int P, int m, int kid) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (batch < 1 || N < 1 || d < 1 || M < 0 || P < 1 || P > SP_MAX_P || m < 1 || m > SP_MAX_IND) return CGP_EINVAL;
  if (kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  if (c->sp.max_dim < 1 || c->sm.max_dim < 1) return CGP_ESTATE;
  const int rc = sparse_check(c, batch, N, d, M, m, kid);
  if (rc != CGP_OK) return rc;
  if (batch > c->sm.max_batch || P > c->sm.max_dim || N > c->sm_max_n || m > c->sm_max_ind) return CGP_ECAPACITY;
  return CGP_OK;
}

}  // namespace

extern "C" int cgp_sparse_multi_reserve(cgp_ctx *c, int max_batch, int max_p) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_p < 1 || max_p > SP_MAX_P) return CGP_EINVAL;
  if (c->sp.max_dim < 1 || max_batch > c->sp.max_batch) return CGP_ESTATE;
  // sized by the sparse reservation as it stands now: a later, larger cgp_sparse_reserve does not widen this one
  const int rc = scratch_reserve(c, c->sm, max_batch, max_p,
                                 sparse_multi_layout(max_batch, c->sp_max_n, c->sp.max_dim, max_p).total * sizeof(double));
  c->sm_max_n = rc == CGP_OK ? c->sp_max_n : 0;
  c->sm_max_ind = rc == CGP_OK ? c->sp.max_dim : 0;
  return rc;
}

extern "C" int cgp_fit_predict_sparse_multi_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int P, int m, int kid,
                                                         const double *dX, const double *dY, const double *dZ, const double *dXs,
                                                         const double *dtheta, const double *djitter, int include_noise,
                                                         double *dmean, double *dvar, double *dlogml, int *dinfo, void *hip_stream) {
  const int rc = sparse_multi_check(c, batch, N, d, M, P, m, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dY || !dZ || !dtheta || !dlogml || !dinfo || (M > 0 && (!dXs || !dmean || !dvar))) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const SparseCall k{N, d, M, m, kid, include_noise, dX, dY, dZ, dXs, dtheta, djitter, dmean, dvar, dlogml, dinfo, P};
  return sparse_enqueue(c, sparse_multi_args(c, k, 0, batch), pick_stream(c, hip_stream));
}

extern "C" int cgp_fit_predict_sparse_multi_batch(cgp_ctx *c, int batch, int N, int d, int M, int P, int m, int kid, const double *X,
                                                  const double *Y, const double *Z, const double *Xs, const double *theta,
                                                  int theta_stride, int include_noise, double *mean, double *var, double *logml,
                                                  int *info) {
  int rc = sparse_multi_check(c, batch, N, d, M, P, m, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !Y || !Z || !theta || (M > 0 && (!Xs || !mean || !var))) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  if (theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // staging: the caller's row-major [X | Z | Xs], then what the device form takes: [dX | dZ | dXs | dY | theta | mean | var | logml]
  const size_t B = batch, nX = B * N * d, nZ = B * m * d, nXs = B * (size_t)M * d, nY = B * P * N, nth_all = B * CGP_MAX_THETA,
               nM = B * M, nPM = nM * P, nL = B * P;
  const size_t nraw = nX + nZ + nXs;
  if (!grow_device(c->sm.stage, c->sm.stage_cap, (2 * nraw + nY + nth_all + nPM + nM + nL) * sizeof(double))) return CGP_ENOMEM;
  double *raw = static_cast<double *>(c->sm.stage), *dX = raw + nraw, *dZ = dX + nX, *dXs = dZ + nZ, *dY = dXs + nXs, *dth = dY + nY,
         *dmean = dth + nth_all, *dvar = dmean + nPM, *dlogml = dvar + nM;
  std::vector<double> hth(nth_all, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (int q = 0; q < nth; ++q) hth[b * CGP_MAX_THETA + q] = theta[b * theta_stride + q];
  HIP_TRY(c, hipMemcpyAsync(raw, X, nX * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(raw + nX, Z, nZ * sizeof(double), hipMemcpyHostToDevice, s));
  if (M > 0) HIP_TRY(c, hipMemcpyAsync(raw + nX + nZ, Xs, nXs * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(dY, Y, nY * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(dth, hth.data(), nth_all * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  auto pack = [&](const double *src, double *dst, int n) {
    hipLaunchKernelGGL(k_pack_soa<double>, dim3(std::min(64, cdiv(n * d, 256)), batch), dim3(256), 0, s, src, dst, n, d);
  };
  pack(raw, dX, N);
  pack(raw + nX, dZ, m);
  if (M > 0) pack(raw + nX + nZ, dXs, M);
  const SparseCall k{N, d, M, m, kid, include_noise, dX, dY, dZ, M > 0 ? dXs : nullptr, dth, c->djitter,
                     M > 0 ? dmean : nullptr, M > 0 ? dvar : nullptr, dlogml, c->dinfo, P};
  if ((rc = sparse_enqueue(c, sparse_multi_args(c, k, 0, batch), s)) != CGP_OK) return rc;
  std::vector<int> hinfo(B);
  HIP_TRY(c, hipMemcpyAsync(hinfo.data(), c->dinfo, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  // cgp_fit_predict_sparse_batch's policy: the ladder is K_uu's, the fit goes again alone into its slot with all its columns
  std::vector<char> skip(B, 0);
  for (size_t b = 0; b < B; ++b) skip[b] = hinfo[b] > m;
  std::vector<double> hjit(B, 0.0);
  rc = jitter_ladder(c, batch, m, d, kid, theta, theta_stride, Z, hinfo.data(), &skip, hjit.data(), s,
                     [&](int b) { return sparse_enqueue(c, sparse_multi_args(c, k, b, 1), s); });
  if (rc != CGP_OK) return rc;
  std::vector<double> hl(nL);
  if (M > 0) {
    HIP_TRY(c, hipMemcpyAsync(mean, dmean, nPM * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(var, dvar, nM * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(c, hipMemcpyAsync(hl.data(), dlogml, nL * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (logml) std::copy(hl.begin(), hl.end(), logml);
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}
