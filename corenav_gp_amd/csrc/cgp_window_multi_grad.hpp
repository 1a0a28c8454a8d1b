// cgp_window_multi_grad.hpp -- multi-target sliding windows: value and gradient of the P columns' summed log marginal likelihood
// from the resident factor (cgp_window_multi_grad_reserve, cgp_window_multi_nll_grad, cgp_window_optimize_multi).
//
// With Y (n x P) the window's targets, Z = L^-1 Y and A = L^-T Z = Ky^-1 Y:
//   nll  = - sum_p logml[p]
//   w_ij = sum_p A_ip A_jp - P (Ky^-1)_ij
//   grad = grad_from_sums(sums of w o dK/dtheta)          (cgp_window_nll_grad's sums with the rank-P term for alpha alpha^T)
// One pass over the factor serves all P columns.  The launches of an evaluation:
//   k_window_diag_inv          (cgp_window_forecast.hpp) as it stands
//   k_window_multi_z           (cgp_window_multi.hpp) as it stands: Z into the Z scratch [tile][row][16], logml[p]
//   k_window_multi_alpha       A = L^-T Z into the A scratch, the same tile order.  One WAVE = one window x one tile of 16 target
//                              columns -- the work unit of k_window_kinv_grad, and its backward block step: I from nb - 1 down,
//                              acc = Z(I), acc -= L(K, I)^T A(K) for K > I (A operand read across the slab's columns, B operand
//                              the finished A(K) from the scratch), A(I) = L(I, I)^-T acc (four MFMAs with the diagonal block's
//                              inverse), stored, then a wavefront fence.  Rows from n on and columns from P on come out as
//                              zeros (the Z scratch holds zeros there and the L operand is masked), so the next kernel reads whole
//                              tiles.  (The LDS-resident form of the predictive gradients' B = L^-T V keeps a chunk's whole V in
//                              128 KB of LDS per workgroup for 32 columns; P is 1 ... 64 and mostly a handful, the A tile is
//                              read back by the same wave only, and the wave-per-tile form needs no LDS and no barrier.)
//   k_window_multi_kinv_grad   k_window_kinv_grad's work unit (one wave per window x 16-column chunk): the same forward solve
//                              (chunk_forward_solve), backward substitution and dK/dtheta sums; w comes from the A scratch by
//                              ceil(P / 16) x 4 more MFMAs per tile.  A kernel of its own (see there why).
//   k_window_multi_grad_finish per window: the chunks' partial sums in chunk order -> gradient; nll = - sum_p logml[p] in p
//                              order; NaN for a failed window, zeros for an empty one.
// No atomics, every sum runs in a fixed order, plain vector stores only.
#pragma once
#include "cgp_window_adapt.hpp"
#include "cgp_window_multi.hpp"

namespace cgp {

constexpr int WA_MAX_PT = WM_MAX_P / WPB;   // target tiles of 16 columns a multi-target window can have
static_assert(WA_MAX_PT * WPB == WM_MAX_P && WA_MAX_PT == 4, "target tiles of the multi-target gradient");

__global__ __launch_bounds__(256) void k_window_multi_alpha(AdaptArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gid = (long long)blockIdx.x * 4 + wave;
  if (gid >= (long long)p.nwin * p.pt) return;
  const int w = (int)(gid / p.pt), tt = (int)(gid - (long long)w * p.pt);
  const int CAP = p.CAP;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  if (bad != 0 || n <= 0) return;   // the later kernels do not read a failed or empty window's tiles
  const int nb = (n + WPB - 1) / WPB;
  const double *S = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0): lower triangle and diagonal read
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  const size_t toff = ((size_t)w * p.pt + tt) * p.NB * WPB * WPB;
  const double *Zt = p.zs + toff;
  double *At = p.am + toff;
  for (int I = nb - 1; I >= 0; --I) {
    const int I0 = I * WPB;
    d4 acc;   // register r = row lq + 4 r of block I, target column l15 of the tile
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = Zt[(size_t)(I0 + lq + 4 * r) * WPB + l15];
    const bool rowok = I0 + l15 < n;   // (a column of the slab past the window is not read: rows from n on stay zeros)
    const double *Lt = S + (size_t)(I0 + l15) * CAP;   // column I0 + l15 of L: row l15 of L(K, I)^T
#pragma unroll 2
    for (int K = I + 1; K < nb; ++K) {
      const int k0 = K * WPB + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int kr = k0 + 4 * ks;
        const double a = (kr < n && rowok) ? -Lt[kr] : 0.0;
        const double b = At[(size_t)kr * WPB + l15];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
    }
    d4 u = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double dt = dinv[(size_t)I * (WPB * WPB) + l15 * WPB + lq + 4 * r];   // (L(I, I)^-1)[lq + 4 r][l15]
      u = __builtin_amdgcn_mfma_f64_16x16x4f64(dt, acc[r], u, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) At[(size_t)(I0 + lq + 4 * r) * WPB + l15] = u[r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the steps above this block read what other lanes stored
  }
}

// k_window_kinv_grad's work unit with the rank-P term.  A kernel of its own, NOT a shared body: with the two behind one
// __forceinline__ template the single-target kernel kept its resource line but not its instructions (551 of 3 323 changed, register
// numbering and contraction order), and cgp_window_nll_grad's gradient moved in the last bits (docs/negatives.md item 20 again).
// The forward half IS shared (chunk_forward_solve, as k_window_loo shares it); the backward substitution and the dK/dtheta sums
// below are k_window_kinv_grad's, statement for statement, and differ in where w comes from:
//   w_ij = (A(I) A(J)^T)_ij - P U_ij:  a operand A[tt][I0 + l15][lq + 4 ks], b operand A[tt][J0 + l15][lq + 4 ks] (loop-invariant:
//   at most 16 doubles per lane at P = 64); result register r is row lq + 4 r of block I, column l15 of the chunk, as u[r].
__global__ __launch_bounds__(256) void k_window_multi_kinv_grad(AdaptArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gid = (long long)blockIdx.x * 4 + wave;
  if (gid >= (long long)p.nwin * p.NB) return;
  const int w = (int)(gid / p.NB), J = (int)(gid - (long long)w * p.NB);
  const int CAP = p.CAP, d = p.d, kid = p.kernel_id;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const int nb = (n + WPB - 1) / WPB;
  double *gp = p.gpart + ((size_t)w * p.NB + J) * GRAD_N;
  if (bad != 0 || J >= nb) {
    if (lane < GRAD_N) gp[lane] = 0.0;
    return;
  }
  double *S = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0): lower triangle read, strict upper triangle scratch
  const double *xw = p.xw + (size_t)w * d * CAP + o;
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  const size_t tstride = (size_t)p.NB * WPB * WPB;   // one target tile of the A scratch
  const double *Am = p.am + (size_t)w * p.pt * tstride;
  const int J0 = J * WPB;
  const int gj = J0 + l15;
  const bool colok = gj < n;
  double *Sc = S + J0 + l15;   // + row * CAP: element (row, chunk column l15) of V / U, transposed into the chunk's tile row
  double unused;
  const d4 VJ = chunk_forward_solve<false>(S, dinv, CAP, n, nb, J, l15, lq, unused);

  // ---- backward: U(I) = L(I, I)^-T (V(I) - sum_{K > I} L(K, I)^T U(K)), contracted as it is finished
  const WaCov cv = WaCov::from_prep(kid, d, p.prep + (size_t)w * PREP_N);
  double xj[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) xj[q] = (q < d && colok) ? xw[(size_t)q * CAP + gj] : 0.0;
  double bj[WA_MAX_PT][4];   // A(J, .) as the B operand: targets lq + 4 ks of every tile (rows from n on are zeros in the scratch)
#pragma unroll
  for (int tt = 0; tt < WA_MAX_PT; ++tt)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bj[tt][ks] = tt < p.pt ? Am[tt * tstride + (size_t)gj * WPB + lq + 4 * ks] : 0.0;
  const double negp = -(double)p.P;
  double s_amp = 0.0, s_noise = 0.0, s_ell[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) s_ell[q] = 0.0;
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
    d4 aa = {0.0, 0.0, 0.0, 0.0};   // (A(I) A(J)^T): ceil(P / 16) x 4 MFMAs
#pragma unroll
    for (int tt = 0; tt < WA_MAX_PT; ++tt)
      if (tt < p.pt) {
        const double *ai = Am + tt * tstride + (size_t)(I0 + l15) * WPB + lq;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) aa = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[4 * ks], bj[tt][ks], aa, 0, 0, 0);
      }
    const double wgt = I == J ? 1.0 : 2.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = I0 + lq + 4 * r;
      if (gi < n && colok) {
        double xi[MAXD], dq2[MAXD];
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xi[q] = q < d ? xw[(size_t)q * CAP + gi] : 0.0;
        const double wij = __builtin_fma(negp, u[r], aa[r]);
        double kv;
        if (gi == gj) {
          kv = cv.kss(xi[0]);
#pragma unroll
          for (int q = 0; q < MAXD; ++q) dq2[q] = 0.0;
          s_noise += wij;
        } else {
          kv = cv.eval<true>(xi, xj, dq2);
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

// the chunks' sums in chunk order -> gradient (natural parameters, cgp_nll_grad's formulas); the value from the columns' logml
__global__ __launch_bounds__(64) void k_window_multi_grad_finish(AdaptArgs p) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= p.nwin) return;
  const int d = p.d, kid = p.kernel_id, nth = wa_ntheta(kid, d);
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  double *g = p.grad + (size_t)w * p.grad_stride;
  if (bad != 0 || n <= 0) {   // (k_window_multi_z has written the window's P logml entries: NaN resp. 0)
    p.nll[w] = bad != 0 ? __builtin_nan("") : 0.0;
    for (int i = 0; i < nth; ++i) g[i] = bad != 0 ? __builtin_nan("") : 0.0;
    return;
  }
  const int nb = (n + WPB - 1) / WPB;
  double s[GRAD_N];
  for (int i = 0; i < GRAD_N; ++i) s[i] = 0.0;
  for (int J = 0; J < nb; ++J)
    for (int i = 0; i < GRAD_N; ++i) s[i] += p.gpart[((size_t)w * p.NB + J) * GRAD_N + i];
  double lm = 0.0;
  for (int c = 0; c < p.P; ++c) lm += p.mlogml[(size_t)w * p.P + c];
  p.nll[w] = -lm;
  grad_from_sums(kid, d, p.theta + (size_t)w * MAX_THETA, s, g);
}

}  // namespace cgp
