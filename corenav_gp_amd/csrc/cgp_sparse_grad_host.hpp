// cgp_sparse_grad_host.hpp -- host side of the sparse fits' objective: value and gradient of nll = -bound in theta and in the
// inducing inputs Z, and its L-BFGS (kernels: cgp_sparse_grad.hpp).  Not a translation unit of its own: cgp_engine.hip includes it
// after cgp_sparse_host.hpp, whose forward chain (sparse_enqueue with M = 0) every evaluation starts with, and after the other
// optimisers, whose shape it follows (jitter_ladder, lbfgs_minimize_logexp_batch).  fp64 contexts only.
#pragma once

namespace {

// The gradient reservation's scratch, sized by max_batch and the sparse reservation's (max_n, max_m_ind); a call's blocks start at
// the section bases and are strided by the call's own shape.  In doubles, with mt = ceil((max_m_ind + 1) / 16), LD = 16 mt, C =
// chunks(max_n) and mr = ceil(max_m_ind / 16):
//   [A, Th, G (fit, LD, LD) each | tpart (fit, C, mr, 12) | zpart (fit, C, LD, 8) | upart (fit, mr, 12) | uz (fit, LD, 8) |
//    gs (fit, 4) | logml (fit)]
struct SparseGradLayout {
  size_t A, Th, G, tpart, zpart, upart, uz, gs, lml, total;
};
inline SparseGradLayout sparse_grad_layout(int max_batch, int max_n, int max_m_ind) {
  const SparseShape sh = sparse_shape(max_n, max_m_ind, 1);
  const SparseGradShape gh = sparse_grad_shape(max_m_ind);
  const size_t B = max_batch, LD2 = (size_t)sh.LD * sh.LD;
  SparseGradLayout l{};
  l.A = 0;
  l.Th = l.A + B * LD2;
  l.G = l.Th + B * LD2;
  l.tpart = l.G + B * LD2;
  l.zpart = l.tpart + B * sh.nch * gh.mtr * GRAD_N;
  l.upart = l.zpart + B * sh.nch * sh.LD * MAXD;
  l.uz = l.upart + B * gh.mtr * GRAD_N;
  l.gs = l.uz + B * sh.LD * MAXD;
  l.lml = l.gs + B * 4;
  l.total = l.lml + B;
  return l;
}

struct SparseGradCall {   // the call's arrays (device, the call's first fit) and shape
  int N, d, m, kid;
  const double *X, *y, *Z, *theta, *jitter;
  double *nll, *grad, *gradZ;
  int grad_stride;
  int *info;
};

// the gradient kernels' record for the fits in slots slot, slot + 1, ... of the gradient reservation's scratch, strided by the
// call's shape `sh`; the operand image of That in A's block (where it fits whenever the target rows add no tile row: LDa = LD)
SparseGradArgs sparse_grad_args(const cgp_ctx *c, const SparseShape &sh, int m, int slot) {
  const SparseGradLayout l = sparse_grad_layout(c->sg.max_batch, c->sg_max_n, c->sg.max_dim);
  double *buf = static_cast<double *>(c->sg.buf);
  const size_t sl = slot, LD = sh.LD, LD2 = LD * LD;
  SparseGradArgs g{};
  g.gh = sparse_grad_shape(m);
  g.A = buf + l.A + sl * LD2;
  g.Th = buf + l.Th + sl * LD2;
  g.G = buf + l.G + sl * LD2;
  g.tpart = buf + l.tpart + sl * sh.nch * g.gh.mtr * GRAD_N;
  g.zpart = buf + l.zpart + sl * sh.nch * LD * MAXD;
  g.upart = buf + l.upart + sl * g.gh.mtr * GRAD_N;
  g.uz = buf + l.uz + sl * LD * MAXD;
  g.gs = buf + l.gs + sl * 4;
  g.Ti = g.A;
  g.tifs = LD2;
  return g;
}

// the linear chain of a gradient call on s: the forward chain as it stands (M = 0, A kept), then algebra, panel, uu, finish; `a`
// carries the target columns (a.P), `g` the outputs.  Profile slots: 0 k_sparse_phi, 1 both algebra kernels, 2 k_sparse_reduce +
// k_sparse_grad_uu + k_sparse_grad_finish, 3 k_sparse_grad_panel, 4 k_sparse_prep
int sparse_grad_launch(cgp_ctx *c, SparseArgs &a, const SparseGradArgs &g, hipStream_t s) {
  const SparseShape &sh = a.sh;
  const int nfit = a.nfit;
  a.Acp = g.A;
  int rc = sparse_enqueue(c, a, s);
  if (rc != CGP_OK) return rc;
  Launcher L{c, s};
  const double mm = a.m, fits = nfit;
  L.begin(1, fits * 6.0 * mm * mm * mm);   // six m x m block solves
  hipLaunchKernelGGL(k_sparse_grad_algebra, dim3(nfit), dim3(SPA_THREADS), 0, s, a, g);
  L.end();
  const dim3 pg(g.gh.ngrp, sh.nch, nfit), ug(g.gh.mtr, nfit);
  const size_t lds = sparse_grad_panel_lds(a.d, sh.LDa, sh.S);
  const int kc = a.kid == K_RBF_BROWNIAN ? SGK_BROWN : a.kid == K_MATERN32_ARD ? SGK_M32 : a.kid == K_MATERN52_ARD ? SGK_M52 : SGK_SE;
  const bool wz = g.gradZ != nullptr;
  L.begin(3, fits * 2.0 * a.N * (mm + a.P) * sh.LDa);
#define CGP_SG_PANEL(KC)                                                                                             \
  if (wz) hipLaunchKernelGGL((k_sparse_grad_panel<KC, true>), pg, dim3(SG_THREADS), lds, s, a, g);                   \
  else hipLaunchKernelGGL((k_sparse_grad_panel<KC, false>), pg, dim3(SG_THREADS), lds, s, a, g)
  if (kc == SGK_BROWN) { CGP_SG_PANEL(SGK_BROWN); }
  else if (kc == SGK_M32) { CGP_SG_PANEL(SGK_M32); }
  else if (kc == SGK_M52) { CGP_SG_PANEL(SGK_M52); }
  else { CGP_SG_PANEL(SGK_SE); }
#undef CGP_SG_PANEL
  L.end();
  L.begin(2, fits * mm * mm * (2.0 * a.d + 2));
  if (kc == SGK_BROWN) hipLaunchKernelGGL(k_sparse_grad_uu<SGK_BROWN>, ug, dim3(SGU_THREADS), 0, s, a, g);
  else if (kc == SGK_M32) hipLaunchKernelGGL(k_sparse_grad_uu<SGK_M32>, ug, dim3(SGU_THREADS), 0, s, a, g);
  else if (kc == SGK_M52) hipLaunchKernelGGL(k_sparse_grad_uu<SGK_M52>, ug, dim3(SGU_THREADS), 0, s, a, g);
  else hipLaunchKernelGGL(k_sparse_grad_uu<SGK_SE>, ug, dim3(SGU_THREADS), 0, s, a, g);
  hipLaunchKernelGGL(k_sparse_grad_finish, dim3(nfit), dim3(256), 0, s, a, g, kc == SGK_BROWN ? 1 : 0);
  L.end();
  if (!hip_ok(c, hipGetLastError(), "sparse gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

// a single-column gradient call for the `nfit` fits in slots slot, slot + 1, ... of the call's arrays and of both scratches
int sparse_grad_enqueue(cgp_ctx *c, const SparseGradCall &k, int slot, int nfit, hipStream_t s) {
  const SparseGradLayout l = sparse_grad_layout(c->sg.max_batch, c->sg_max_n, c->sg.max_dim);
  const size_t sl = slot;
  const SparseCall fk{k.N, k.d, 0, k.m, k.kid, 0, k.X, k.y, k.Z, nullptr, k.theta, k.jitter, nullptr, nullptr,
                      static_cast<double *>(c->sg.buf) + l.lml, k.info};
  SparseArgs a = sparse_args(c, fk, slot, nfit);
  SparseGradArgs g = sparse_grad_args(c, a.sh, k.m, slot);
  g.nll = k.nll + sl;
  g.grad = k.grad + sl * k.grad_stride;
  g.gradZ = k.gradZ ? k.gradZ + sl * k.d * k.m : nullptr;
  g.grad_stride = k.grad_stride;
  return sparse_grad_launch(c, a, g, s);
}

// the checks every call of this section starts with: dtype, the two reservations, capacity, then the shape
int sparse_grad_check(const cgp_ctx *c, int batch, int N, int d, int m, int kid) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (batch < 1 || N < 1 || d < 1 || m < 1 || m > SP_MAX_IND) return CGP_EINVAL;
  if (kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  int rc = scratch_check(c->sp, batch, m);
  if (rc != CGP_OK) return rc;
  if ((rc = scratch_check(c->sg, batch, m)) != CGP_OK) return rc;
  if (N > c->sp_max_n || N > c->sg_max_n || d > c->max_d || batch > c->max_batch) return CGP_ECAPACITY;
  return CGP_OK;
}

// The staging of the host calls (P target columns: one here, several in cgp_sparse_multi_grad_host.hpp, each in its own
// reservation's staging block): the caller's row-major [X | Z], then what the device form takes and returns:
// [dX | dZ | dy (fit, P, N) | theta | nll | grad | gradZ | logml (fit, P)]; X and y are uploaded once, theta and Z per evaluation.
struct SparseGradStage {
  double *raw, *dX, *dZ, *dy, *dth, *dnll, *dgrad, *dgz, *dlm;
};
int sparse_grad_stage(cgp_ctx *c, Scratch &r, int batch, int N, int d, int m, int P, SparseGradStage &st) {
  const size_t B = batch, nX = B * N * d, nZ = B * m * d, ny = B * P * N, nth_all = B * CGP_MAX_THETA;
  if (!grow_device(r.stage, r.stage_cap, (2 * (nX + nZ) + ny + 2 * nth_all + B + nZ + B * P) * sizeof(double))) return CGP_ENOMEM;
  st.raw = static_cast<double *>(r.stage);
  st.dX = st.raw + nX + nZ;
  st.dZ = st.dX + nX;
  st.dy = st.dZ + nZ;
  st.dth = st.dy + ny;
  st.dnll = st.dth + nth_all;
  st.dgrad = st.dnll + B;
  st.dgz = st.dgrad + nth_all;
  st.dlm = st.dgz + nZ;
  return CGP_OK;
}
int sparse_grad_upload_xy(cgp_ctx *c, int batch, int N, int d, int P, const double *X, const double *y, const SparseGradStage &st) {
  hipStream_t s = c->stream;
  const size_t nX = (size_t)batch * N * d;
  HIP_TRY(c, hipMemcpyAsync(st.raw, X, nX * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(st.dy, y, (size_t)batch * P * N * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_pack_soa<double>, dim3(std::min(64, cdiv(N * d, 256)), batch), dim3(256), 0, s, st.raw, st.dX, N, d);
  return CGP_OK;
}
// One evaluation of the batch at host theta (batch, theta_stride) and Z (batch, m, d): upload, one batched call, the ladder on K_uu
// for the failed fits that `skip` (or null) does not mark, results back.  enqueue(slot, nfit) is the call's chain on the staged
// arrays (theta at CGP_MAX_THETA, jitter c->djitter, info c->dinfo, gradZ asked when hgz is).  hg (batch, CGP_MAX_THETA); hgz
// (batch, d, m) or null; hlm (batch, P) or null.
template <class Enqueue>
int sparse_grad_eval_host(cgp_ctx *c, int batch, int N, int d, int m, int P, int kid, const double *Z, const double *theta, int theta_stride,
                          const SparseGradStage &st, const std::vector<char> *skip, double *nll, double *hg, double *hgz, double *hlm,
                          int *info, Enqueue enqueue) {
  hipStream_t s = c->stream;
  const int nth = ntheta(kid, d);
  const size_t B = batch, nX = B * N * d, nZ = B * m * d;
  std::vector<double> hth(B * CGP_MAX_THETA, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (int q = 0; q < nth; ++q) hth[b * CGP_MAX_THETA + q] = theta[b * theta_stride + q];
  HIP_TRY(c, hipMemcpyAsync(st.raw + nX, Z, nZ * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(st.dth, hth.data(), hth.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  hipLaunchKernelGGL(k_pack_soa<double>, dim3(std::min(64, cdiv(m * d, 256)), batch), dim3(256), 0, s, st.raw + nX, st.dZ, m, d);
  int rc = enqueue(0, batch);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(info, c->dinfo, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  // cgp_fit_predict_sparse_batch's policy: the ladder is K_uu's; a failing pivot of B is reported as it is
  std::vector<char> sk(B, 0);
  for (size_t b = 0; b < B; ++b) sk[b] = info[b] > m || (skip && (*skip)[b]);
  std::vector<double> hjit(B, 0.0);
  rc = jitter_ladder(c, batch, m, d, kid, theta, theta_stride, Z, info, &sk, hjit.data(), s, [&](int b) { return enqueue(b, 1); });
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(nll, st.dnll, B * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(hg, st.dgrad, B * CGP_MAX_THETA * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hgz) HIP_TRY(c, hipMemcpyAsync(hgz, st.dgz, nZ * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hlm) HIP_TRY(c, hipMemcpyAsync(hlm, st.dlm, B * P * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}
// the staged single-column call
SparseGradCall sparse_grad_staged_call(cgp_ctx *c, int N, int d, int m, int kid, const SparseGradStage &st, bool want_gz) {
  return SparseGradCall{N, d, m, kid, st.dX, st.dy, st.dZ, st.dth, c->djitter, st.dnll, st.dgrad, want_gz ? st.dgz : nullptr, CGP_MAX_THETA,
                        c->dinfo};
}

// The batched L-BFGS of the sparse objectives over [theta | Z row-major]: theta Logexp-transformed, Z as it stands (free
// coordinates, optimize_z only).  eval(Z (batch, m, d), theta (batch, nth), skip or null, nll, hg (batch, CGP_MAX_THETA), hgz
// (batch, d, m) or null, info) is one evaluation of the batch with the ladder.  bound (or null): -nll at the returned point, from
// one evaluation more, not counted in n_evals.
template <class Eval>
int sparse_optimize_driver(int batch, int d, int m, int nth, double *Z, double *theta, int theta_stride, int optimize_z, int max_evals,
                           double *bound, int *n_evals, Eval eval) {
  const size_t B = batch, mz = (size_t)m * d;
  const int nfree = optimize_z ? (int)mz : 0, nx = nth + nfree;
  std::vector<double> x0(B * nx), hth(B * nth), hZ(Z, Z + B * mz), nl(B), hg(B * CGP_MAX_THETA), hgz(optimize_z ? B * mz : 0);
  std::vector<int> info(B);
  std::vector<char> skip(B, 0);
  for (size_t b = 0; b < B; ++b) {
    std::copy(theta + b * theta_stride, theta + b * theta_stride + nth, x0.begin() + b * nx);
    if (optimize_z) std::copy(Z + b * mz, Z + (b + 1) * mz, x0.begin() + b * nx + nth);
  }
  auto eval_at = [&](const double *x, const std::vector<char> *sk) -> int {
    for (size_t b = 0; b < B; ++b) {
      std::copy(x + b * nx, x + b * nx + nth, hth.begin() + b * nth);
      if (optimize_z) std::copy(x + b * nx + nth, x + (b + 1) * nx, hZ.begin() + b * mz);
    }
    return eval(hZ.data(), hth.data(), sk, nl.data(), hg.data(), optimize_z ? hgz.data() : nullptr, info.data());
  };
  auto round = [&](const double *x, const char *active, double *f, double *g, char *feasible) -> int {
    for (int b = 0; b < batch; ++b) skip[b] = !active[b];
    // a trial point whose K_uu is not positive definite climbs the ladder; one that stays infeasible (K_uu or B) is +inf
    const int rc = eval_at(x, &skip);
    if (rc != CGP_OK) return rc;
    for (size_t b = 0; b < B; ++b) {
      if (!active[b]) continue;
      feasible[b] = info[b] == 0;
      f[b] = nl[b];
      std::copy(hg.begin() + b * CGP_MAX_THETA, hg.begin() + b * CGP_MAX_THETA + nth, g + b * nx);
      if (optimize_z)   // the device's (d, m) into the row-major coordinates
        for (int r = 0; r < m; ++r)
          for (int q = 0; q < d; ++q) g[b * nx + nth + (size_t)r * d + q] = hgz[(b * d + q) * m + r];
    }
    return CGP_OK;
  };
  corenav::LbfgsBatchResult res;
  int rc = corenav::lbfgs_minimize_logexp_batch(batch, nth, x0.data(), nx, nullptr, max_evals, round, res, nfree);
  if (rc != CGP_OK) return rc;
  for (size_t b = 0; b < B; ++b) {
    std::copy(res.theta.begin() + b * nx, res.theta.begin() + b * nx + nth, theta + b * theta_stride);
    if (optimize_z) std::copy(res.theta.begin() + b * nx + nth, res.theta.begin() + (b + 1) * nx, Z + b * mz);
    if (n_evals) n_evals[b] = res.evals[b];
  }
  if (bound) {
    if ((rc = eval_at(res.theta.data(), nullptr)) != CGP_OK) return rc;
    for (size_t b = 0; b < B; ++b) bound[b] = -nl[b];
  }
  return CGP_OK;
}

}  // namespace

extern "C" int cgp_sparse_grad_reserve(cgp_ctx *c, int max_batch) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch) return CGP_EINVAL;
  if (c->sp.max_dim < 1 || max_batch > c->sp.max_batch) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));   // (the attribute goes to the current device's function)
  for (const void *fn : {reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_SE, false>), reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_SE, true>),
                         reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_M32, false>), reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_M32, true>),
                         reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_M52, false>), reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_M52, true>),
                         reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_BROWN, false>), reinterpret_cast<const void *>(&k_sparse_grad_panel<SGK_BROWN, true>)})
    HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerWorkgroup));
  // sized by the sparse reservation as it stands now: a later, larger cgp_sparse_reserve does not widen this one
  const int rc = scratch_reserve(c, c->sg, max_batch, c->sp.max_dim, sparse_grad_layout(max_batch, c->sp_max_n, c->sp.max_dim).total * sizeof(double));
  c->sg_max_n = rc == CGP_OK ? c->sp_max_n : 0;
  return rc;
}

extern "C" int cgp_sparse_nll_grad_batch_device(cgp_ctx *c, int batch, int N, int d, int m, int kid, const double *dX, const double *dy,
                                                const double *dZ, const double *dtheta, const double *djitter, double *dnll,
                                                double *dgrad, int grad_stride, double *dgradZ, int *dinfo, void *hip_stream) {
  const int rc = sparse_grad_check(c, batch, N, d, m, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dy || !dZ || !dtheta || !dnll || !dgrad || !dinfo || grad_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const SparseGradCall k{N, d, m, kid, dX, dy, dZ, dtheta, djitter, dnll, dgrad, dgradZ, grad_stride, dinfo};
  return sparse_grad_enqueue(c, k, 0, batch, pick_stream(c, hip_stream));
}

extern "C" int cgp_sparse_nll_grad_batch(cgp_ctx *c, int batch, int N, int d, int m, int kid, const double *X, const double *y,
                                         const double *Z, const double *theta, int theta_stride, double *nll, double *grad,
                                         int grad_stride, double *gradZ, int *info) {
  int rc = sparse_grad_check(c, batch, N, d, m, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !y || !Z || !theta || !nll || !grad || theta_stride < nth || grad_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  SparseGradStage st{};
  if ((rc = sparse_grad_stage(c, c->sg, batch, N, d, m, 1, st)) != CGP_OK) return rc;
  if ((rc = sparse_grad_upload_xy(c, batch, N, d, 1, X, y, st)) != CGP_OK) return rc;
  const size_t B = batch;
  std::vector<double> hg(B * CGP_MAX_THETA), hgz(gradZ ? B * m * d : 0);
  std::vector<int> hinfo(B);
  const SparseGradCall k = sparse_grad_staged_call(c, N, d, m, kid, st, gradZ != nullptr);
  rc = sparse_grad_eval_host(c, batch, N, d, m, 1, kid, Z, theta, theta_stride, st, nullptr, nll, hg.data(), gradZ ? hgz.data() : nullptr,
                             nullptr, hinfo.data(), [&](int slot, int nfit) { return sparse_grad_enqueue(c, k, slot, nfit, c->stream); });
  if (rc != CGP_OK) return rc;
  int first = 0;
  for (size_t b = 0; b < B; ++b) {
    for (int i = 0; i < nth; ++i) grad[b * grad_stride + i] = hg[b * CGP_MAX_THETA + i];
    if (gradZ)   // the device's (d, m) back to the caller's (m, d)
      for (int r = 0; r < m; ++r)
        for (int q = 0; q < d; ++q) gradZ[(b * m + r) * d + q] = hgz[(b * d + q) * m + r];
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}

extern "C" int cgp_optimize_sparse_batch(cgp_ctx *c, int batch, int N, int d, int m, int kid, const double *X, const double *y,
                                         double *Z, double *theta, int theta_stride, int optimize_z, int max_evals, double *logml,
                                         int *n_evals) {
  int rc = sparse_grad_check(c, batch, N, d, m, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !y || !Z || !theta || theta_stride < nth) return CGP_EINVAL;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < nth; ++i)
      if (!(theta[(size_t)b * theta_stride + i] > 0.0)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  SparseGradStage st{};
  if ((rc = sparse_grad_stage(c, c->sg, batch, N, d, m, 1, st)) != CGP_OK) return rc;
  if ((rc = sparse_grad_upload_xy(c, batch, N, d, 1, X, y, st)) != CGP_OK) return rc;
  const SparseGradCall kz = sparse_grad_staged_call(c, N, d, m, kid, st, optimize_z != 0), k0 = sparse_grad_staged_call(c, N, d, m, kid, st, false);
  // the bound AT the returned point comes from one evaluation more, not counted in n_evals
  return sparse_optimize_driver(batch, d, m, nth, Z, theta, theta_stride, optimize_z, max_evals, logml, n_evals,
                                [&](const double *hZ, const double *hth, const std::vector<char> *sk, double *nl, double *hg, double *hgz,
                                    int *info) {
                                  const SparseGradCall &k = hgz ? kz : k0;
                                  return sparse_grad_eval_host(c, batch, N, d, m, 1, kid, hZ, hth, nth, st, sk, nl, hg, hgz, nullptr, info,
                                                               [&](int slot, int nfit) { return sparse_grad_enqueue(c, k, slot, nfit, c->stream); });
                                });
}
