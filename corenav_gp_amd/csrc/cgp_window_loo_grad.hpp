// cgp_window_loo_grad.hpp -- value and gradient of the leave-one-out objective nlpd = -lpd_sum of the resident sliding windows
// (cgp_window_loo_nll_grad[_device], cgp_window_optimize_loo), from the factor, z, the inputs and the targets as they stand after
// any number of pushes, at the theta each window holds.  Algebra: cgp_loo_grad.hpp, on a window's resident factor:
//
//   c_i = 1/2 (1 / kd_i + alpha_i^2 / kd_i^2)      b_i = alpha_i / kd_i      beta = Ky^-1 b
//   w_ij = -2 sum_k Ky^-1_ik c_k Ky^-1_kj + beta_i alpha_j + alpha_i beta_j      grad = grad_from_sums(sum w o dK/dtheta)
//
// k_window_diag_inv, k_window_alpha, k_window_loo and k_window_loo_finish run first as they stand (loo_var = 1 / kd and lpd_sum
// go into the reservation's buffers), so nlpd is bitwise cgp_window_loo's lpd_sum negated and logml bitwise cgp_window_nll_grad's
// nll negated.  Then
//   k_window_loo_prep         c and b per sample; zeros from n on.
//   k_window_loo_kinv         Ky^-1 materialised once per window.  One WAVE = one window x one chunk of 16 columns, the work unit
//                             of k_window_kinv_grad: chunk_forward_solve, then that kernel's backward substitution written out
//                             again with the contraction replaced by stores: every finished 16 x 16 tile U(I, J) of Ky^-1 goes
//                             to the scratch matrix [NP][NP] (row-major, NP = N rounded up to 64) as block (I, J) and, for
//                             I != J, transposed as block (J, I), from the same register: the scratch is exactly symmetric off the
//                             diagonal tiles.  The chunk's V / U lives in the chunk's tile row of the slab's strict upper triangle
//                             as in k_window_kinv_grad; the lower triangle, the diagonal, z, the samples and the state words are
//                             NOT written.  Only elements (i < n, j < n) are stored: every reader masks the others.
//   k_window_loo_beta         beta = Ky^-1 b: workgroup (64 rows, window), the inner index dealt round-robin to four waves whose
//                             sums meet in LDS in wave order (k_loo_beta's shape); zeros from n on.
//   k_window_loo_grad         k_window_joint_cov's work unit and XCD numbering: one WAVE owns a 64 x 64 super-tile of the lower
//                             triangle (4 x 4 accumulator tiles, eight operand loads feed sixteen MFMAs per k-step) and runs the
//                             whole sum over k itself, in row order, operands from the scratch through L2 with c_k applied to the
//                             A operand as it is loaded and everything from n on masked to zero.  Then w = -2 acc + beta_i alpha_j
//                             + alpha_i beta_j is contracted in registers with K_ij and K_ij d_q^2 (WaCov's formulas): the GRAD_N
//                             sums of k_window_kinv_grad, off-diagonal tiles counted twice, the diagonal feeding the noise sum,
//                             tiles above the diagonal of a diagonal super-tile skipped.  One partial per (window, pair).
//   k_window_loo_grad_finish  per window: the pairs' partial sums in pair order (no atomics) -> grad_from_sums; nlpd = -lpd_sum;
//                             logml = -k_window_alpha's value; NaN for a failed window, zeros for an empty one.
// Origin, size and the failure word come from the window's state words: no host mirror, nothing depends on the slot.  fp64 only.
#pragma once
#include "cgp_window_loo.hpp"
#include "cgp_window_joint.hpp"

namespace cgp {

struct WindowLooGradArgs {
  double *kinv;          // [nwin][NP][NP] Ky^-1, row-major; elements from n on are never read unmasked
  const double *var;     // [nwin][N] loo_var = 1 / kd (k_window_loo's)
  const double *lsum;    // [nwin] lpd_sum (k_window_loo_finish's)
  double *cv, *bv, *beta;   // [nwin][NP]
  double *part;          // [nwin][npair][GRAD_N]
  double *nlpd, *logml;  // outputs [nwin]; logml may be null
  int NP, npair, per_win;   // padded size, super-tile pairs of the lower triangle, k_window_loo_grad's workgroups per window
};

__global__ __launch_bounds__(256) void k_window_loo_prep(AdaptArgs p, WindowLooGradArgs g) {
  const int w = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.NP) return;
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  double c = 0.0, b = 0.0;
  if (bad == 0 && e < n) {
    const double v = g.var[(size_t)w * p.N + e];
    const double al = p.alpha[(size_t)w * p.NB * WPB + e];
    b = al * v;
    c = 0.5 * (v + b * b);
  }
  g.cv[(size_t)w * g.NP + e] = c;
  g.bv[(size_t)w * g.NP + e] = b;
}

__global__ __launch_bounds__(256) void k_window_loo_kinv(AdaptArgs p, WindowLooGradArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gid = (long long)blockIdx.x * 4 + wave;
  if (gid >= (long long)p.nwin * p.NB) return;
  const int w = (int)(gid / p.NB), J = (int)(gid - (long long)w * p.NB);
  const int CAP = p.CAP, NP = g.NP;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const int nb = (n + WPB - 1) / WPB;
  if (bad != 0 || J >= nb) return;
  double *S = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0): lower triangle read, strict upper triangle scratch
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  double *Kw = g.kinv + (size_t)w * NP * NP;
  const int J0 = J * WPB;
  const int gj = J0 + l15;
  const bool colok = gj < n;
  double *Sc = S + J0 + l15;   // + row * CAP: element (row, chunk column l15) of V / U, transposed into the chunk's tile row
  double unused;
  const d4 VJ = chunk_forward_solve<false>(S, dinv, CAP, n, nb, J, l15, lq, unused);

  // ---- backward: U(I) = L(I, I)^-T (V(I) - sum_{K > I} L(K, I)^T U(K)), stored as it is finished (k_window_kinv_grad's step)
  for (int I = nb - 1; I >= J; --I) {
    const int I0 = I * WPB;
    d4 acc;
    if (I == J) {
      acc = VJ;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I0 + lq + 4 * r;
        acc[r] = (row < n && colok) ? Sc[(size_t)row * CAP] : 0.0;
      }
    }
    const double *Lt = S + (size_t)(I0 + l15) * CAP;   // column I0 + l15 of L: row l15 of L(K, I)^T
#pragma unroll 2
    for (int K = I + 1; K < nb; ++K) {
      const int k0 = K * WPB + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int kr = k0 + 4 * ks;
        const double a = kr < n ? -Lt[kr] : 0.0;
        const double b = (kr < n && colok) ? Sc[(size_t)kr * CAP] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
    }
    d4 u = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double dt = dinv[(size_t)I * (WPB * WPB) + l15 * WPB + lq + 4 * r];   // (L(I, I)^-1)[lq + 4 r][l15]
      u = __builtin_amdgcn_mfma_f64_16x16x4f64(dt, acc[r], u, 0, 0, 0);
    }
    if (I != J) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I0 + lq + 4 * r;
        if (row < n && colok) Sc[(size_t)row * CAP] = u[r];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // u[r] = Ky^-1(I0 + lq + 4 r, J0 + l15): block (I, J) in rows of 16 consecutive doubles, block (J, I) from the same register
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = I0 + lq + 4 * r;
      if (gi < n && colok) {
        Kw[(size_t)gi * NP + gj] = u[r];
        if (I != J) Kw[(size_t)gj * NP + gi] = u[r];
      }
    }
  }
}

constexpr int WLG_EB = 64, WLG_WAVES = 4, WLG_UNROLL = 8;
__global__ __launch_bounds__(WLG_WAVES * 64) void k_window_loo_beta(AdaptArgs p, WindowLooGradArgs g) {
  __shared__ double red[WLG_WAVES][WLG_EB];
  const int w = blockIdx.y, NP = g.NP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = blockIdx.x * WLG_EB + lane;   // < NP: the grid is NP / 64
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  double s = 0.0;
  if (bad == 0 && i < n) {
    const double *__restrict__ Kc = g.kinv + (size_t)w * NP * NP + i;
    const double *__restrict__ bw = g.bv + (size_t)w * NP;
    for (int k = wave; k < n; k += WLG_WAVES * WLG_UNROLL) {
      double v[WLG_UNROLL], u[WLG_UNROLL];
#pragma unroll
      for (int q = 0; q < WLG_UNROLL; ++q) {
        const int kk = k + q * WLG_WAVES;
        v[q] = kk < n ? Kc[(size_t)kk * NP] : 0.0;
        u[q] = kk < n ? bw[kk] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < WLG_UNROLL; ++q) s = fma(v[q], u[q], s);
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  g.beta[(size_t)w * NP + i] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(WJ_THREADS) void k_window_loo_grad(AdaptArgs p, WindowLooGradArgs g) {
  // workgroup -> (window, group of super-tile pairs): consecutive ids on ONE XCD
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nwin * g.per_win) return;
  const int w = lid / g.per_win;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = (lid - w * g.per_win) * WJ_WAVES + wave;
  if (pair >= g.npair) return;
  int BI = 0;
  while ((BI + 1) * (BI + 2) / 2 <= pair) ++BI;
  const int BJ = pair - BI * (BI + 1) / 2;   // BJ <= BI
  const int CAP = p.CAP, NP = g.NP, d = p.d, kid = p.kernel_id;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const int nb = (bad != 0 || n <= 0) ? 0 : (n + WPB - 1) / WPB;
  double *gp = g.part + ((size_t)w * g.npair + pair) * GRAD_N;
  if (BJ * WJ_ST >= nb) {   // (BI >= BJ: no live tile) every pair writes its partial on every call
    if (lane < GRAD_N) gp[lane] = 0.0;
    return;
  }
  // tile (b, a): rows j = (BJ 4 + b) 16 + lq + 4 r (A operand), columns i = (BI 4 + a) 16 + l15 (B operand)
  auto live = [&](int b, int a) { return BI * WJ_ST + a < nb && BJ * WJ_ST + b <= BI * WJ_ST + a; };
  d4 acc[WJ_ST][WJ_ST];
#pragma unroll
  for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) acc[b][a] = d4{0.0, 0.0, 0.0, 0.0};
  // operands of row block kb: lane (l15, lq) holds Ky^-1[kb 16 + 4 ks + lq][tile 16 + l15] -- 16 consecutive doubles per row
  const double *Kw = g.kinv + (size_t)w * NP * NP + (size_t)lq * NP + l15;
  const double *cw = g.cv + (size_t)w * NP + lq;
  bool oka[WJ_ST], okb[WJ_ST];
#pragma unroll
  for (int t = 0; t < WJ_ST; ++t) {
    oka[t] = (BJ * WJ_ST + t) * WPB + l15 < n;
    okb[t] = (BI * WJ_ST + t) * WPB + l15 < n;
  }
  auto load = [&](int kb, double (&fa)[WJ_ST][4], double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = kb * WPB + 4 * ks;   // + lq
      const bool kok = k + lq < n;
      const double ck = kok ? cw[k] : 0.0;
#pragma unroll
      for (int t = 0; t < WJ_ST; ++t) {
        fa[t][ks] = (kok && oka[t]) ? Kw[(size_t)k * NP + (BJ * WJ_ST + t) * WPB] * ck : 0.0;
        fb[t][ks] = (kok && okb[t]) ? Kw[(size_t)k * NP + (BI * WJ_ST + t) * WPB] : 0.0;
      }
    }
  };
  double fa[WJ_ST][4], fb[WJ_ST][4], ga[WJ_ST][4], gb[WJ_ST][4];
  load(0, fa, fb);
  for (int kb = 0; kb < nb; ++kb) {
    if (kb + 1 < nb) load(kb + 1, ga, gb);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a)
          if (live(b, a)) acc[b][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[b][ks], fb[a][ks], acc[b][a], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = ga[t][ks];
        fb[t][ks] = gb[t][ks];
      }
  }

  // ---- w = -2 acc + beta_j alpha_i + alpha_j beta_i contracted with K and K d_q^2 (k_window_kinv_grad's sums)
  const WaCov cv = WaCov::from_prep(kid, d, p.prep + (size_t)w * PREP_N);
  const double *xw = p.xw + (size_t)w * d * CAP + o;
  const double *alpha = p.alpha + (size_t)w * p.NB * WPB;
  const double *beta = g.beta + (size_t)w * NP;
  double xc[WJ_ST][MAXD], ac[WJ_ST], bc[WJ_ST];
#pragma unroll
  for (int a = 0; a < WJ_ST; ++a) {
    const int i = (BI * WJ_ST + a) * WPB + l15;
#pragma unroll
    for (int q = 0; q < MAXD; ++q) xc[a][q] = (q < d && i < n) ? xw[(size_t)q * CAP + i] : 0.0;
    ac[a] = i < n ? alpha[i] : 0.0;
    bc[a] = i < n ? beta[i] : 0.0;
  }
  double s_amp = 0.0, s_noise = 0.0, s_ell[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) s_ell[q] = 0.0;
#pragma unroll
  for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = (BJ * WJ_ST + b) * WPB + lq + 4 * r;
      double xr[MAXD];
#pragma unroll
      for (int q = 0; q < MAXD; ++q) xr[q] = (q < d && j < n) ? xw[(size_t)q * CAP + j] : 0.0;
      const double ar = j < n ? alpha[j] : 0.0, br = j < n ? beta[j] : 0.0;
#pragma unroll
      for (int a = 0; a < WJ_ST; ++a) {
        const int i = (BI * WJ_ST + a) * WPB + l15;
        if (live(b, a) && i < n && j < n) {
          const double wgt = BJ * WJ_ST + b == BI * WJ_ST + a ? 1.0 : 2.0;
          double dq2[MAXD];
          const double wij = __builtin_fma(-2.0, acc[b][a][r], __builtin_fma(br, ac[a], ar * bc[a]));
          double kv;
          if (i == j) {
            kv = cv.kss(xr[0]);
#pragma unroll
            for (int q = 0; q < MAXD; ++q) dq2[q] = 0.0;
            s_noise += wij;
          } else {
            kv = cv.eval<true>(xr, xc[a], dq2);
          }
          const double wk = wgt * wij * kv;
          s_amp += wk;
#pragma unroll
          for (int q = 0; q < MAXD; ++q) s_ell[q] = __builtin_fma(wk, dq2[q], s_ell[q]);
        }
      }
    }
  double vals[GRAD_N];
  vals[0] = s_amp;
#pragma unroll
  for (int q = 0; q < MAXD; ++q) vals[1 + q] = s_ell[q];
  vals[9] = s_noise;
  vals[10] = vals[11] = 0.0;
#pragma unroll
  for (int i = 0; i < GRAD_N; ++i) {
    double v = vals[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) gp[i] = v;
  }
}

// the pairs' sums in pair order -> gradient (natural parameters); nlpd = -lpd_sum, logml = -k_window_alpha's value
__global__ __launch_bounds__(64) void k_window_loo_grad_finish(AdaptArgs p, WindowLooGradArgs g) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= p.nwin) return;
  const int d = p.d, kid = p.kernel_id, nth = wa_ntheta(kid, d);
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  double *gr = p.grad + (size_t)w * p.grad_stride;
  if (bad != 0 || n <= 0) {
    const double v = bad != 0 ? __builtin_nan("") : 0.0;
    g.nlpd[w] = v;
    if (g.logml) g.logml[w] = v;
    for (int i = 0; i < nth; ++i) gr[i] = v;
    return;
  }
  double s[GRAD_N];
  for (int i = 0; i < GRAD_N; ++i) s[i] = 0.0;
  for (int pz = 0; pz < g.npair; ++pz)
    for (int i = 0; i < GRAD_N; ++i) s[i] += g.part[((size_t)w * g.npair + pz) * GRAD_N + i];
  g.nlpd[w] = -g.lsum[w];
  if (g.logml) g.logml[w] = -p.nllv[w];
  grad_from_sums(kid, d, p.theta + (size_t)w * MAX_THETA, s, gr);
}

}  // namespace cgp
