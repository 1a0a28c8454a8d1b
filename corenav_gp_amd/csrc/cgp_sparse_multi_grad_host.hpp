// cgp_sparse_multi_grad_host.hpp -- host side of the sparse fits' objective with P target columns on one (X, Z, theta): value and
// gradient of nll = -sum_p bound[p] in theta and in the inducing inputs Z, and its L-BFGS.  Not a translation unit of its own:
// cgp_engine.hip includes it after cgp_sparse_multi_host.hpp.  The kernels are the gradient section's own (cgp_sparse_grad.hpp: they
// take P from SparseArgs, and the single-column call runs them at P = 1 on the buffers it always used), the forward chain
// cgp_sparse_multi_host.hpp's at M = 0, the launches sparse_grad_launch's, the optimiser loop sparse_optimize_driver's; what is here
// is the reservation that holds what the columns add to the gradient scratch, the checks and the four entry points.
#pragma once

namespace {

// The multi-gradient reservation's scratch, sized by (max_batch, max_p) and the gradient reservation's max_m_ind as it stood; a
// call's blocks start at the section bases and are strided by the call's own shape.  In doubles, with LD = 16 ceil((max_m_ind + 1) /
// 16), mr = ceil(max_m_ind / 16) and k = ceil((max_p - 1) / 16) (the tile rows the targets of a call can add: its LDa <= its LD + 16 k):
//   [img (fit, mr, (LD + 16 k) / 4, 64) | logml (fit, max_p)]
// img: the operand image of That for the calls whose target rows add a tile row (LDa > LD) -- 16 mr LDa doubles no longer fit the
// LD^2 of A's block that the image takes otherwise; nothing at max_p = 1.
struct SparseMultiGradLayout {
  size_t img, lml, total;
};
inline SparseMultiGradLayout sparse_multi_grad_layout(int max_batch, int max_m_ind, int max_p) {
  const SparseShape sh = sparse_shape(1, max_m_ind, 1);
  const SparseGradShape gh = sparse_grad_shape(max_m_ind);
  const size_t B = max_batch, k = (max_p - 1 + 15) / 16;
  SparseMultiGradLayout l{};
  l.img = 0;
  l.lml = l.img + (k > 0 ? B * gh.mtr * WPB * (sh.LD + 16 * k) : 0);
  l.total = l.lml + B * max_p;
  return l;
}

struct SparseMultiGradCall {   // the call's arrays (device, the call's first fit) and shape
  int N, d, P, m, kid;
  const double *X, *Y, *Z, *theta, *jitter;
  double *nll, *grad, *gradZ, *logml;
  int grad_stride;
  int *info;
};

// the linear chain of a call for the `nfit` fits in slots slot, slot + 1, ... of the call's arrays and of the four scratches
int sparse_multi_grad_enqueue(cgp_ctx *c, const SparseMultiGradCall &k, int slot, int nfit, hipStream_t s) {
  const SparseMultiGradLayout l = sparse_multi_grad_layout(c->mg.max_batch, c->mg_max_ind, c->mg.max_dim);
  double *buf = static_cast<double *>(c->mg.buf);
  const size_t sl = slot;
  const SparseCall fk{k.N, k.d, 0, k.m, k.kid, 0, k.X, k.Y, k.Z, nullptr, k.theta, k.jitter, nullptr, nullptr, buf + l.lml, k.info, k.P};
  SparseArgs a = sparse_multi_args(c, fk, slot, nfit);
  SparseGradArgs g = sparse_grad_args(c, a.sh, k.m, slot);
  if (a.sh.LDa > a.sh.LD) {
    g.tifs = (size_t)g.gh.mtr * WPB * a.sh.LDa;
    g.Ti = buf + l.img + sl * g.tifs;
  }
  g.nll = k.nll + sl;
  g.grad = k.grad + sl * k.grad_stride;
  g.gradZ = k.gradZ ? k.gradZ + sl * k.d * k.m : nullptr;
  g.lout = k.logml ? k.logml + sl * k.P : nullptr;
  g.grad_stride = k.grad_stride;
  return sparse_grad_launch(c, a, g, s);
}

// the checks every call of this section starts with: dtype and counts, the four reservations, their capacities
int sparse_multi_grad_check(const cgp_ctx *c, int batch, int N, int d, int P, int m, int kid) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (batch < 1 || N < 1 || d < 1 || P < 1 || P > SP_MAX_P || m < 1 || m > SP_MAX_IND) return CGP_EINVAL;
  if (kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  if (c->sp.max_dim < 1 || c->sg.max_dim < 1 || c->sm.max_dim < 1 || c->mg.max_dim < 1) return CGP_ESTATE;
  int rc = sparse_grad_check(c, batch, N, d, m, kid);
  if (rc != CGP_OK) return rc;
  if ((rc = sparse_multi_check(c, batch, N, d, 0, P, m, kid)) != CGP_OK) return rc;
  if (batch > c->mg.max_batch || P > c->mg.max_dim || m > c->mg_max_ind) return CGP_ECAPACITY;
  return CGP_OK;
}

// the staged call of the host forms
SparseMultiGradCall sparse_multi_grad_staged_call(cgp_ctx *c, int N, int d, int P, int m, int kid, const SparseGradStage &st, bool want_gz) {
  return SparseMultiGradCall{N, d, P, m, kid, st.dX, st.dy, st.dZ, st.dth, c->djitter, st.dnll, st.dgrad, want_gz ? st.dgz : nullptr, st.dlm,
                             CGP_MAX_THETA, c->dinfo};
}

}  // namespace

extern "C" int cgp_sparse_multi_grad_reserve(cgp_ctx *c, int max_batch, int max_p) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;
  if (max_batch < 1 || max_batch > c->max_batch || max_p < 1 || max_p > SP_MAX_P) return CGP_EINVAL;
  if (c->sp.max_dim < 1 || max_batch > c->sp.max_batch || c->sg.max_dim < 1 || max_batch > c->sg.max_batch || c->sm.max_dim < 1 ||
      max_batch > c->sm.max_batch || max_p > c->sm.max_dim)
    return CGP_ESTATE;
  // sized by the gradient reservation as it stands now: a later, larger one does not widen this one
  const int rc = scratch_reserve(c, c->mg, max_batch, max_p, sparse_multi_grad_layout(max_batch, c->sg.max_dim, max_p).total * sizeof(double));
  c->mg_max_ind = rc == CGP_OK ? c->sg.max_dim : 0;
  return rc;
}

extern "C" int cgp_sparse_multi_nll_grad_batch_device(cgp_ctx *c, int batch, int N, int d, int P, int m, int kid, const double *dX,
                                                      const double *dY, const double *dZ, const double *dtheta, const double *djitter,
                                                      double *dnll, double *dgrad, int grad_stride, double *dgradZ, double *dlogml,
                                                      int *dinfo, void *hip_stream) {
  const int rc = sparse_multi_grad_check(c, batch, N, d, P, m, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dY || !dZ || !dtheta || !dnll || !dgrad || !dinfo || grad_stride < ntheta(kid, d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const SparseMultiGradCall k{N, d, P, m, kid, dX, dY, dZ, dtheta, djitter, dnll, dgrad, dgradZ, dlogml, grad_stride, dinfo};
  return sparse_multi_grad_enqueue(c, k, 0, batch, pick_stream(c, hip_stream));
}

extern "C" int cgp_sparse_multi_nll_grad_batch(cgp_ctx *c, int batch, int N, int d, int P, int m, int kid, const double *X,
                                               const double *Y, const double *Z, const double *theta, int theta_stride, double *nll,
                                               double *grad, int grad_stride, double *gradZ, double *logml, int *info) {
  int rc = sparse_multi_grad_check(c, batch, N, d, P, m, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !Y || !Z || !theta || !nll || !grad || theta_stride < nth || grad_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  SparseGradStage st{};
  if ((rc = sparse_grad_stage(c, c->mg, batch, N, d, m, P, st)) != CGP_OK) return rc;
  if ((rc = sparse_grad_upload_xy(c, batch, N, d, P, X, Y, st)) != CGP_OK) return rc;
  const size_t B = batch;
  std::vector<double> hg(B * CGP_MAX_THETA), hgz(gradZ ? B * m * d : 0);
  std::vector<int> hinfo(B);
  const SparseMultiGradCall k = sparse_multi_grad_staged_call(c, N, d, P, m, kid, st, gradZ != nullptr);
  rc = sparse_grad_eval_host(c, batch, N, d, m, P, kid, Z, theta, theta_stride, st, nullptr, nll, hg.data(), gradZ ? hgz.data() : nullptr,
                             logml, hinfo.data(), [&](int slot, int nfit) { return sparse_multi_grad_enqueue(c, k, slot, nfit, c->stream); });
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

extern "C" int cgp_optimize_sparse_multi_batch(cgp_ctx *c, int batch, int N, int d, int P, int m, int kid, const double *X,
                                               const double *Y, double *Z, double *theta, int theta_stride, int optimize_z, int max_evals,
                                               double *logml_sum, int *n_evals) {
  int rc = sparse_multi_grad_check(c, batch, N, d, P, m, kid);
  if (rc != CGP_OK) return rc;
  const int nth = ntheta(kid, d);
  if (!X || !Y || !Z || !theta || theta_stride < nth) return CGP_EINVAL;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < nth; ++i)
      if (!(theta[(size_t)b * theta_stride + i] > 0.0)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  SparseGradStage st{};
  if ((rc = sparse_grad_stage(c, c->mg, batch, N, d, m, P, st)) != CGP_OK) return rc;
  if ((rc = sparse_grad_upload_xy(c, batch, N, d, P, X, Y, st)) != CGP_OK) return rc;
  const SparseMultiGradCall kz = sparse_multi_grad_staged_call(c, N, d, P, m, kid, st, optimize_z != 0),
                            k0 = sparse_multi_grad_staged_call(c, N, d, P, m, kid, st, false);
  // the summed bound AT the returned point comes from one evaluation more, not counted in n_evals: -nll is the column-order sum
  return sparse_optimize_driver(batch, d, m, nth, Z, theta, theta_stride, optimize_z, max_evals, logml_sum, n_evals,
                                [&](const double *hZ, const double *hth, const std::vector<char> *sk, double *nl, double *hg, double *hgz,
                                    int *info) {
                                  const SparseMultiGradCall &k = hgz ? kz : k0;
                                  return sparse_grad_eval_host(c, batch, N, d, m, P, kid, hZ, hth, nth, st, sk, nl, hg, hgz, nullptr, info,
                                                               [&](int slot, int nfit) { return sparse_multi_grad_enqueue(c, k, slot, nfit, c->stream); });
                                });
}
