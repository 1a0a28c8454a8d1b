// cgp_joint.hpp -- joint forecast after a batch of fits (or a single fit): the full posterior covariance at the M test points
// (cgp_fit_predict_cov_batch, cgp_predict_cov) and sample paths drawn from it (cgp_fit_sample_batch, cgp_sample).
//
//   cov = K(Xs, Xs) - V^T V      C C^T = cov (+ sigma_n^2 I) + jitter I      path = mean + C xi
//
// After any tiled fit schedule the factor panel of fit b holds V^T = (L^-1 K*)^T as its M extra rows (cgp_kernels.hpp: rows
// [NT 128, NT 128 + M) of slab b, column-major, every block column stored), so the covariance needs no second solve:
//   k_joint_cov           cov(J, I) = K**(J, I) - sum_c V^T(J, c) V^T(I, c) on v_mfma_f64_16x16x4_f64, operands straight from the
//                         slab: for a fixed column c the 64 rows of a super-tile's side are 512 contiguous bytes.  The scheme is
//                         k_window_joint_cov's, written out a second time (a shared super-tile body was slower for the windows:
//                         docs/negatives.md item 20; a fix goes into both kernels): one WAVE owns a 64 x 64 super-tile of the lower
//                         triangle and runs the whole sum over c itself, in column order (no split over waves, no atomics: a fit's
//                         result is a function of its own data only, whatever its slot and its neighbours); the Gram tile,
//                         evaluated in registers from the SoA test points, is the accumulators' start value; the next 16 columns'
//                         operands are requested before this block's MFMAs; the workgroups of a fit run on one XCD, so its V rows
//                         come from HBM once.  The sum runs over the REAL N columns: the last, partial block of 16 is read masked,
//                         after the prefetched loop.  Output form: both triangles of the caller's (M, M) matrix from the same
//                         register, the diagonal replaced by the fit's own variance (clip and noise included).  Scratch form
//                         (sampling): the lower triangle, column-major, leading dimension M padded to 16, identity in the padding
//                         -- what k_window_joint_chol / k_window_joint_paths (cgp_window_joint.hpp) read; they are launched
//                         unchanged with the fit index where they take a window index.
// A fit whose info word is set gets NaN in all of its covariance (and, through the factorisation's failure word, in its paths).
// Read-only on the factor panel.  fp64 only.
#pragma once
#include "cgp_window_joint.hpp"

namespace cgp {

struct JointFitArgs {
  const double *Lw;      // slab of the call's first fit
  size_t lw_stride;      // elements per fit
  size_t row0;           // first extra row (NT 128)
  int ld;
  const double *theta;   // [nfit][MAX_THETA]
  const double *Xs;      // [nfit][d][M]
  const double *var;     // [nfit][M] the fit's variance: clipped, noise included when asked for
  const int *info;       // [nfit] the fits' status words, or null (a single fit known to be good)
  double *cov;           // output form: [nfit][M][M]
  double *C;             // scratch form: [nfit][mt * 16][mt * 16]
  int N, d, M, kernel_id, nfit;
  int mt, nsup, npair, per_fit;   // tiles of 16 test points, super-tiles per side, pairs of the lower triangle, workgroups per fit
};

template <bool SCRATCH>
__global__ __launch_bounds__(WJ_THREADS) void k_joint_cov(JointFitArgs p) {
  // workgroup -> (fit, group of super-tile pairs): consecutive ids on ONE XCD
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nfit * p.per_fit) return;
  const int f = lid / p.per_fit;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = (lid - f * p.per_fit) * WJ_WAVES + wave;
  if (pair >= p.npair) return;
  int BI = 0;
  while ((BI + 1) * (BI + 2) / 2 <= pair) ++BI;
  const int BJ = pair - BI * (BI + 1) / 2;   // BJ <= BI
  const int M = p.M, N = p.N, mt = p.mt, d = p.d, kid = p.kernel_id;
  const bool bad = p.info != nullptr && p.info[f] != 0;
  const WaCov cv = WaCov::from_theta(kid, d, p.theta + (size_t)f * MAX_THETA);
  const double *xs = p.Xs + (size_t)f * d * M;
  // tile (b, a): rows j = (BJ 4 + b) 16 + lq + 4 r (A operand), columns i = (BI 4 + a) 16 + l15 (B operand)
  auto live = [&](int b, int a) { return BI * WJ_ST + a < mt && BJ * WJ_ST + b <= BI * WJ_ST + a; };
  d4 acc[WJ_ST][WJ_ST];
  {
    double xc[WJ_ST][MAXD];
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) {
      const int i = (BI * WJ_ST + a) * WPB + l15;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) xc[a][q] = (q < d && i < M) ? xs[(size_t)q * M + i] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = (BJ * WJ_ST + b) * WPB + lq + 4 * r;
        double xr[MAXD], dq[MAXD];
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xr[q] = (q < d && j < M) ? xs[(size_t)q * M + j] : 0.0;
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a) acc[b][a][r] = live(b, a) ? cv.eval<false>(xr, xc[a], dq) : 0.0;
      }
  }
  // operands of column block kb: lane (l15, lq) holds V^T[tile 16 + l15][kb 16 + 4 ks + lq].  A tile index past the last one is
  // clamped to it (its products are never stored); the rows a last tile has beyond M are the y row and the panel's padding,
  // inside the slab, and reach only accumulator entries that are not stored either.
  const double *Vf = p.Lw + (size_t)f * p.lw_stride + p.row0 + (size_t)lq * p.ld + l15;
  const double *va[WJ_ST], *vb[WJ_ST];
#pragma unroll
  for (int t = 0; t < WJ_ST; ++t) {
    const int tj = BJ * WJ_ST + t < mt ? BJ * WJ_ST + t : mt - 1, ti = BI * WJ_ST + t < mt ? BI * WJ_ST + t : mt - 1;
    va[t] = Vf + tj * WPB;
    vb[t] = Vf + ti * WPB;
  }
  const size_t ld = p.ld;
  auto load = [&](int kb, double (&fa)[WJ_ST][4], double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = va[t][(size_t)(kb * WPB + 4 * ks) * ld];
        fb[t][ks] = vb[t][(size_t)(kb * WPB + 4 * ks) * ld];
      }
  };
  auto mac = [&](const double (&fa)[WJ_ST][4], const double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a)
          if (live(b, a)) acc[b][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(-fa[b][ks], fb[a][ks], acc[b][a], 0, 0, 0);
  };
  const int nfull = bad ? 0 : N / WPB;
  double fa[WJ_ST][4], fb[WJ_ST][4], ga[WJ_ST][4], gb[WJ_ST][4];
  if (nfull > 0) load(0, fa, fb);
  for (int kb = 0; kb < nfull; ++kb) {
    if (kb + 1 < nfull) load(kb + 1, ga, gb);
    mac(fa, fb);
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = ga[t][ks];
        fb[t][ks] = gb[t][ks];
      }
  }
  if (!bad && nfull * WPB < N) {   // the last columns, N not a multiple of 16: the columns from N on (the panel's identity padding) count as zero
    load(nfull, fa, fb);           // (inside the slab: its NT 128 columns cover the block)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bool in = nfull * WPB + 4 * ks + lq < N;
#pragma unroll
      for (int t = 0; t < WJ_ST; ++t) {
        fa[t][ks] = in ? fa[t][ks] : 0.0;
        fb[t][ks] = in ? fb[t][ks] : 0.0;
      }
    }
    mac(fa, fb);
  }
  const double *var = p.var + (size_t)f * M;
  const int mpad = mt * WPB;
#pragma unroll
  for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) {
      if (!live(b, a)) continue;
      const bool dtile = BJ * WJ_ST + b == BI * WJ_ST + a;
      const int i = (BI * WJ_ST + a) * WPB + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = (BJ * WJ_ST + b) * WPB + lq + 4 * r;
        if (i < M && j < M) {
          double v = acc[b][a][r];
          if (i == j) v = var[i];   // the fit's own variance
          if (bad) v = __builtin_nan("");
          if constexpr (SCRATCH) {
            p.C[(size_t)f * mpad * mpad + (size_t)j * mpad + i] = v;
          } else if (!dtile || j <= i) {
            double *cw = p.cov + (size_t)f * M * M;
            cw[(size_t)j * M + i] = v;
            if (i != j) cw[(size_t)i * M + j] = v;
          }
        } else if constexpr (SCRATCH) {
          p.C[(size_t)f * mpad * mpad + (size_t)j * mpad + i] = (i == j) ? 1.0 : 0.0;   // padding: identity
        }
      }
    }
}

}  // namespace cgp
