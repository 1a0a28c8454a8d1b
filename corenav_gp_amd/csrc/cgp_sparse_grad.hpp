// cgp_sparse_grad.hpp -- sparse (inducing-point) fits: the gradient of the collapsed variational bound (cgp_sparse.hpp) in theta
// and in the inducing inputs Z.  With the forward chain's quantities (sigma2, K_uu = L_u L_u^T, A, B = I + A = L_B L_B^T, c, t, yty)
// and F the bound:
//   chat = L_B^-T c          Q = I - B^-1 - chat chat^T          mu = L_u^-T chat
//   T    = L_u^-T Q L_u^-1 / (2 sigma2)                (= dF/dPhi)
//   G_uu = 1/2 L_u^-T (Q - A) L_u^-1                   (= dF/dK_uu)
//   R    = 2 T K_uf + mu y^T / sigma2   (m x N)        (= dF/dK_uf; never stored: R = 2 That Phat, That = [T | mu / (2 sigma2)] and
//                                                        Phat = [K_uf; y] the augmented panel of k_sparse_phi)
//   dF/dtheta_p  = sum_rs G_uu[r,s] dk(z_r,z_s)/dtheta_p + sum_ri R[r,i] dk(z_r,x_i)/dtheta_p - sum_i dk(x_i,x_i)/dtheta_p / (2 sigma2)
//   dF/dsigma_n2 = (-N + (yty + t) / sigma2 - tr A + m - tr B^-1 - c^T c - chat^T chat) / (2 sigma2)
//   dF/dz_rq     = sum_i R[r,i] dk(z_r,x_i)/dz_rq + 2 sum_{s != r} G_uu[r,s] dk(z_r,z_s)/dz_rq + G_uu[r,r] dk(z_r,z_r)/dz_rq
// eps (the 1e-8 and any jitter on K_uu's diagonal) is a constant of the evaluation.  Outputs: nll = -F, grad = d nll / d theta in
// natural parameters (cgp_nll_grad's order, grad_from_sums), gradZ = d nll / d Z.
//
// The launches after the forward chain (prep, phi, reduce, algebra with M = 0; k_sparse_algebra also stores a copy of A):
//   k_sparse_grad_algebra  one workgroup per fit: chat and mu by backward vector solves, B^-1 = L_B^-T (L_B^-1 I), Q and Q - A, then T
//                          and G_uu by two backward block solves each (sparse_trsm_t: sparse_trsm run from the last block row up
//                          with the transposed blocks and the transposed diagonal inverses), all on the MFMA; the noise component;
//                          That is left as the MFMA A-operand image [row tile][k-step][lane] the panel pass reads.
//   k_sparse_grad_panel    the hot path: the second pass over N.  One workgroup (eight waves) per (fit, chunk, group of eight row
//                          tiles of That); a wave owns ONE row tile.  The chunk is walked in k_sparse_phi's sub-panels (the same
//                          sparse_shape chunking and S); the panel K(Z, x) | y for ALL LD rows goes to LDS ROW-major (row r of sample
//                          s at r S + s), because here the product contracts over the rows: the B operand of k-step ks is rows 4 ks +
//                          lq, sample l15 -- 64 consecutive doubles at S = 16, conflict-free.  Two buffers, one barrier per sub-panel.
//                          The wave's 16 x S tile of R / 2 is LD / 4 MFMAs into two accumulator chains; the A operand comes from the
//                          image in 512-byte coalesced loads.  The tile is contracted in registers: per (row, sample) k from the LDS
//                          panel, the scaled differences recomputed, one evaluation of the derivative factor (sg_factor), 1 + d
//                          multiply-adds for theta and d for Z (WITH_Z).  The Z sums are carried per lane (4 rows x d) across the
//                          chunk and meet over the 16 sample lanes by a butterfly at its end.  Partials per (chunk, row tile) for
//                          theta and per (chunk, row) for Z: no atomics.
//   k_sparse_grad_uu       one workgroup per (row tile, fit): the m^2 d contraction of G_uu with dK_uu/dtheta and dK_uu/dZ.
//   k_sparse_grad_finish   one workgroup per fit: the partials in chunk and tile order, the t-term (-t / (2 sigma2) on the amplitude
//                          sum: k(x, x) is linear in the amplitudes and free of the length-scales), nll, grad, gradZ; NaN for a
//                          fit whose info is not 0.
// Every sum has a fixed order and every output is a function of the fit's own data and of (N, m, d, kernel, WITH_Z) only; the theta
// sums are written with explicit fma so that the WITH_Z instantiation rounds them as the other one does.
//
// P target columns on one fit (SparseArgs::P; the formulas above are P = 1, and the single-column call runs these kernels at P = 1
// on the buffers it always used): F = sum_p bound[p], C = [c_1 ... c_P],
//   Chat = L_B^-T C      M = L_u^-T Chat      Q = P (I - B^-1) - Chat Chat^T      G_uu = 1/2 L_u^-T (Q - P A) L_u^-1
//   R = 2 T K_uf + M Y / sigma2 = 2 That Phat,   That = [T | M / (2 sigma2)] (m x (m + P)),   Phat = [K_uf; Y] ((m + P) x N)
//   dF/dsigma_n2 = (-N P + (sum_p yty_p + P t) / sigma2 - P tr A + P m - P tr B^-1 - ||C||^2 - ||Chat||^2) / (2 sigma2)
// and the t-term P times.  k_sparse_grad_algebra takes the columns through the vector solves SPV_COLS at a time (sixty-four
// vectors of length LD do not fit LDS): each pass folds its rank-nq term into Q in column order, adds to ||C||^2 and ||Chat||^2 in
// column order and leaves its columns of M in the forward chain's spent b vectors; every vector keeps its own partial sums, order
// and fma chain.  The image of That and the LDS panel have LDa = 16 ceil((m + P) / 16) columns / rows: k_sparse_grad_panel issues
// LDa / 4 MFMAs per sub-panel into the same 16 x S tile.  The image is 16 mtr LDa doubles: in A's spent block while LDa = LD, in the
// multi-gradient reservation's beyond (cgp_sparse_multi_grad_host.hpp).  nll is the columns' bounds summed in column order.
#pragma once
#include "cgp_sparse.hpp"
#include "cgp_window_pgrad.hpp"

namespace cgp {

constexpr int SG_THREADS = 512;               // k_sparse_grad_panel
constexpr int SG_WAVES = SG_THREADS / 64;     // row tiles of a workgroup: one per wave
constexpr int SGU_THREADS = 256;              // k_sparse_grad_uu
enum { SGK_SE = 0, SGK_M32 = 1, SGK_M52 = 2, SGK_BROWN = 3 };   // kernel case of the contractions, selected at the launch site

struct SparseGradShape {
  int mtr, ngrp;   // row tiles of T that hold an inducing input, groups of SG_WAVES of them
};
inline SparseGradShape sparse_grad_shape(int m) {
  SparseGradShape s{};
  s.mtr = (m + 15) / 16;
  s.ngrp = (s.mtr + SG_WAVES - 1) / SG_WAVES;
  return s;
}
inline size_t sparse_grad_panel_lds(int d, int LD, int S) { return ((size_t)d * LD + (size_t)2 * LD * S) * sizeof(double); }

struct SparseGradArgs {
  // the gradient reservation's scratch, at the call's first fit, strided by the call's own shape
  double *A;       // [fit][LD][LD] k_sparse_algebra's copy of A, row-major; then (LDa = LD) the operand image of That
  double *Th;      // [fit][LD][LD] work matrix (identity, B^-1, Q, T)
  double *G;       // [fit][LD][LD] Q - A, then G_uu, row-major
  double *tpart;   // [fit][nch][mtr][GRAD_N] the panel pass's theta sums
  double *zpart;   // [fit][nch][LD][MAXD] its Z sums (RBF x Brownian: slot 1 holds the term of min(|z|, |x|))
  double *upart;   // [fit][mtr][GRAD_N] k_sparse_grad_uu's theta sums
  double *uz;      // [fit][LD][MAXD] its Z sums
  double *gs;      // [fit][4] dF/dsigma_n^2, -P t / (2 sigma2)
  double *Ti;      // the operand image of That, [row tile][LDa / 4][64] per fit, fits tifs doubles apart: A's block where LDa = LD (A
  size_t tifs;     // is spent by then), the multi-gradient reservation's where the target rows add a tile row
  double *nll, *grad, *gradZ, *lout;   // outputs: (fit), (fit, grad_stride), (fit, d, m) or null, (fit, P) or null
  int grad_stride;
  SparseGradShape gh;
};

// x = L^-T x for the nq <= SPV_COLS vectors x[q][SP_LDMAX] in LDS, from the last block row up: sparse_vec_solve's scheme on the
// transposed blocks.  Each vector's arithmetic is its own and the same whatever nq is; L is read once for all.
__device__ __forceinline__ void sparse_vec_solve_t(const double *L, const double *dinv, double *x, int nq, double *red, double *rr, int ld,
                                                   int mt, int tid) {
  const int i = tid & 15, part = tid >> 4;
  for (int I = mt - 1; I >= 0; --I) {
    const double *col = L + (size_t)(I * WPB + i) * ld;   // column I 16 + i of L: row i of the transposed blocks
    double s[SPV_COLS];
#pragma unroll
    for (int q = 0; q < SPV_COLS; ++q) s[q] = 0.0;
    for (int k = (I + 1) * WPB + part; k < ld; k += SPA_THREADS / 16) {
      const double l = col[k];
#pragma unroll
      for (int q = 0; q < SPV_COLS; ++q)
        if (q < nq) s[q] = __builtin_fma(l, x[q * SP_LDMAX + k], s[q]);
    }
#pragma unroll
    for (int q = 0; q < SPV_COLS; ++q)
      if (q < nq) red[q * SPA_THREADS + part * WPB + i] = s[q];
    __syncthreads();
    if (tid < WPB * nq) {   // (here `part` is the vector)
      double r = x[part * SP_LDMAX + I * WPB + i];
      for (int q = 0; q < SPA_THREADS / 16; ++q) r -= red[part * SPA_THREADS + q * WPB + i];
      rr[tid] = r;
    }
    __syncthreads();
    if (tid < WPB * nq) {
      double v = 0.0;
      for (int j = i; j < WPB; ++j) v = __builtin_fma(dinv[I * (WPB * WPB) + i * WPB + j], rr[part * WPB + j], v);
      x[part * SP_LDMAX + I * WPB + i] = v;
    }
    __syncthreads();
  }
}

// Xo = L^-T R for all ld columns: sparse_trsm from the last block row up.  Block row I: acc = R(I, c) - sum_{K > I} L(K, I)^T Xo(K, c),
// then Xo(I, c) = L(I, I)^-T acc (the diagonal inverse read the other way round).  TRANS: the right-hand side is R^T.
template <bool TRANS>
__device__ __forceinline__ void sparse_trsm_t(const double *L, const double *dinv, const double *R, double *Xo, int ld, int mt, int tid) {
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int I = mt - 1; I >= 0; --I) {
    d4 acc[SPA_TPW];
#pragma unroll
    for (int t = 0; t < SPA_TPW; ++t) {
      const int c = wave + SPA_WAVES * t;
      acc[t] = d4{0.0, 0.0, 0.0, 0.0};
      if (c < mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[t][r] = TRANS ? R[(size_t)(c * WPB + l15) * ld + I * WPB + lq + 4 * r] : R[(size_t)(I * WPB + lq + 4 * r) * ld + c * WPB + l15];
      }
    }
    const double *Lc = L + (size_t)(I * WPB + l15) * ld + lq;   // column I 16 + l15 of L
    for (int K = I + 1; K < mt; ++K) {
      double a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[ks] = -Lc[K * WPB + 4 * ks];
#pragma unroll
      for (int t = 0; t < SPA_TPW; ++t) {
        const int c = wave + SPA_WAVES * t;
        if (c < mt) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = Xo[(size_t)(K * WPB + 4 * ks + lq) * ld + c * WPB + l15];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    double di[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) di[r] = dinv[I * (WPB * WPB) + l15 * WPB + lq + 4 * r];
#pragma unroll
    for (int t = 0; t < SPA_TPW; ++t) {
      const int c = wave + SPA_WAVES * t;
      if (c < mt) {
        d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[t][r], v, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Xo[(size_t)(I * WPB + lq + 4 * r) * ld + c * WPB + l15] = v[r];
      }
    }
    __syncthreads();   // block row I of Xo is in memory before block row I - 1 reads it
  }
}

__global__ __launch_bounds__(SPA_THREADS) void k_sparse_grad_algebra(SparseArgs p, SparseGradArgs g) {
  __shared__ double red[SPV_COLS * SPA_THREADS], rr[SPV_COLS * WPB], xv[SPV_COLS * SP_LDMAX];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (p.info[f] != 0) return;   // (k_sparse_grad_finish writes the NaNs)
  const int N = p.N, m = p.m, d = p.d, kid = p.kid, LD = p.sh.LD, mt = p.sh.mt, LDa = p.sh.LDa, P = p.P;
  const double Pd = (double)P;
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double sigma2 = pr[SP_R_SIGMA2];
  const double *X = p.X + (size_t)f * d * N;
  const double *U = p.U + (size_t)f * LD * LD, *F = p.F + (size_t)f * LD * LD;
  double *W = p.W + (size_t)f * LD * LD;
  const double *dU = p.dinv + (size_t)f * 2 * mt * (WPB * WPB), *dB = dU + (size_t)mt * (WPB * WPB);
  const double *cm = p.cm + (size_t)f * p.bcs, *da = p.vec + (size_t)f * 4 * LD + 2 * LD;
  double *mus = p.bm + (size_t)f * p.bcs;   // [P][LD] the columns of M: the b of the forward chain are spent
  double *A = g.A + (size_t)f * LD * LD, *Th = g.Th + (size_t)f * LD * LD, *G = g.G + (size_t)f * LD * LD;
  // B^-1 = L_B^-T (L_B^-1 I)
  for (int e = tid; e < LD * LD; e += SPA_THREADS) Th[e] = (e / LD == e % LD) ? 1.0 : 0.0;
  __syncthreads();
  sparse_trsm<false>(F, dB, Th, W, LD, mt, tid);
  sparse_trsm_t<false>(F, dB, W, Th, LD, mt, tid);
  // SPV_COLS target columns per pass: chat = L_B^-T c, the pass's rank-nq term of Q in column order, mu = L_u^-T chat.  Q is
  // built in Th pass by pass -- the first starts it from P (I - B^-1), the last also leaves Q - P A in G; zero in the padding --,
  // one sweep over the matrix per pass (P <= SPV_COLS: the one sweep the single column always took)
  double s_tb = 0.0, s_hh = 0.0, s_cc = 0.0;   // tr B^-1; ||Chat||^2 and ||C||^2, summed in column order
  for (int q0 = 0; q0 < P; q0 += SPV_COLS) {
    const int nq = P - q0 < SPV_COLS ? P - q0 : SPV_COLS;
    const bool first = q0 == 0, last = q0 + SPV_COLS >= P;
    __syncthreads();
    for (int q = 0; q < nq; ++q)
      for (int i = tid; i < LD; i += SPA_THREADS) xv[q * SP_LDMAX + i] = cm[(size_t)(q0 + q) * LD + i];
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
      double s = 0.0;
      for (int i = tid; i < m; i += SPA_THREADS) s += xv[q * SP_LDMAX + i] * xv[q * SP_LDMAX + i];
      s_cc += sparse_block_sum(s, red, tid);
    }
    __syncthreads();
    sparse_vec_solve_t(F, dB, xv, nq, red, rr, LD, mt, tid);
    for (int e = tid; e < LD * LD; e += SPA_THREADS) {
      const int i = e / LD, j = e - i * LD;
      double q = 0.0, qa = 0.0;
      if (i < m && j < m) {
        q = Th[e];
        if (first) {   // (Th holds B^-1)
          if (i == j) s_tb += q;
          q = Pd * ((i == j ? 1.0 : 0.0) - q);
        }
        for (int c = 0; c < nq; ++c) q = q - xv[c * SP_LDMAX + i] * xv[c * SP_LDMAX + j];
        if (last) qa = q - Pd * A[e];
      }
      Th[e] = q;
      if (last) G[e] = qa;
    }
    for (int q = 0; q < nq; ++q) {
      double s = 0.0;
      for (int i = tid; i < m; i += SPA_THREADS) s += xv[q * SP_LDMAX + i] * xv[q * SP_LDMAX + i];
      s_hh += sparse_block_sum(s, red, tid);
    }
    __syncthreads();   // (chat is spent: the columns of M are solved in its place)
    sparse_vec_solve_t(U, dU, xv, nq, red, rr, LD, mt, tid);
    for (int q = 0; q < nq; ++q)
      for (int i = tid; i < LD; i += SPA_THREADS) mus[(size_t)(q0 + q) * LD + i] = xv[q * SP_LDMAX + i];
  }
  __syncthreads();
  sparse_trsm_t<false>(U, dU, Th, W, LD, mt, tid);   // W = L_u^-T Q
  sparse_trsm_t<true>(U, dU, W, Th, LD, mt, tid);    // Th = L_u^-T W^T = L_u^-T Q L_u^-1
  sparse_trsm_t<false>(U, dU, G, W, LD, mt, tid);
  sparse_trsm_t<true>(U, dU, W, G, LD, mt, tid);     // G = L_u^-T (Q - P A) L_u^-1
  // That = [T | M] / (2 sigma2) as the operand image (A is spent), G_uu = G / 2
  const double h = 0.5 / sigma2;
  double *Ti = g.Ti + (size_t)f * g.tifs;
  const int nks = LDa / 4, tot = g.gh.mtr * WPB * LDa;
  for (int e = tid; e < tot || e < LD * LD; e += SPA_THREADS) {
    if (e < tot) {
      const int lane = e & 63, ks = (e >> 6) % nks, rt = (e >> 6) / nks;
      const int row = rt * WPB + (lane & 15), col = 4 * ks + (lane >> 4);
      double v = 0.0;
      if (row < m) v = col < m ? Th[(size_t)row * LD + col] * h : (col < m + P ? mus[(size_t)(col - m) * LD + row] * h : 0.0);
      Ti[e] = v;
    }
    if (e < LD * LD) G[e] = 0.5 * G[e];
  }
  // the noise component
  double s_tr = 0.0, s_t = 0.0;
  for (int i = tid; i < m; i += SPA_THREADS) s_tr += da[i];
  const WaCov kc = WaCov::from_prep(kid, d, pr);
  for (int i = tid; i < N; i += SPA_THREADS) s_t += kc.kss(X[i]);
  s_tb = sparse_block_sum(s_tb, red, tid);
  s_tr = sparse_block_sum(s_tr, red, tid);
  s_t = sparse_block_sum(s_t, red, tid);
  if (tid == 0) {
    double yty = p.yty[(size_t)f * p.ytys];
    for (int q = 1; q < P; ++q) yty += p.yty[(size_t)f * p.ytys + q];
    g.gs[(size_t)f * 4] = h * (-((double)N * Pd) + (yty + Pd * s_t) / sigma2 - Pd * s_tr + Pd * (double)m - Pd * s_tb - s_cc - s_hh);
    g.gs[(size_t)f * 4 + 1] = -(Pd * s_t) * h;
  }
}

// The derivative factor of one (z, x) pair from k and the scaled differences df[q] = (z_q - x_q) / ell_q (d2 = their squares' sum):
// w = -2 dk/dr^2 (k for the squared exponentials, k times WaCov::eval's quotient for the Matern pair), so that
//   dk/dell_q = w df_q^2 / ell_q          dk/dz_q = -w df_q / ell_q
// RBF x Brownian (d = 1): the same w = k for the RBF factor; `extra` is the term of min(|z|, |x|), k / z where |z| < |x| on the same
// side of zero (k_pgrad_contract's tie convention), which enters dk/dz unscaled.
template <int KC> __device__ __forceinline__ double sg_factor(double k, double d2) {
  if constexpr (KC == SGK_M32) {
    const double s = sqrt(3.0 * d2);
    return k * (3.0 / (1.0 + s));
  } else if constexpr (KC == SGK_M52) {
    const double s = sqrt(5.0 * d2);
    return k * ((5.0 / 3.0) * (1.0 + s) / __builtin_fma(5.0 / 3.0, d2, 1.0 + s));
  } else {
    return k;
  }
}
__device__ __forceinline__ double sg_brown_extra(double k, double z, double x) {
  const int sz = (z > 0) - (z < 0), sx = (x > 0) - (x < 0);
  return (sz == sx && fabs(z) < fabs(x)) ? k / z : 0.0;
}

template <int KC, bool WITH_Z>
__global__ __launch_bounds__(SG_THREADS) void k_sparse_grad_panel(SparseArgs p, SparseGradArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int grp = blockIdx.x, ch = blockIdx.y, f = blockIdx.z;
  if (p.info[f] != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, m = p.m, d = p.d, kid = p.kid;
  const int LD = p.sh.LDa, S = p.sh.S, nks = LD / 4, mP = m + p.P;   // (LD: the augmented panel's rows, m + P rounded up)
  double *Zl = reinterpret_cast<double *>(smem_raw);   // [d][LD] the inducing inputs, zero in the padding
  double *P = Zl + (size_t)d * LD;                     // [2][LD][S] the panel: row r of sample s at r * S + s
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double *X = p.X + (size_t)f * d * N, *y = p.y + (size_t)f * p.P * N, *Z = p.Z + (size_t)f * d * m;
  const int rt = grp * SG_WAVES + wave;                // the wave's row tile
  const bool live = rt < g.gh.mtr;
  for (int e = tid; e < d * LD; e += SG_THREADS) {
    const int q = e / LD, r = e - q * LD;
    Zl[e] = r < m ? Z[(size_t)q * m + r] : 0.0;
  }
  const int n0 = ch * p.sh.clen;
  const int n1 = n0 + p.sh.clen < N ? n0 + p.sh.clen : N;
  const int nsp = n1 > n0 ? (n1 - n0 + S - 1) / S : 0;
  __syncthreads();
  // sub-panel sp into buffer `buf`: K(z_r, x_i) for r < m, target column q of x_i in row m + q, zero in the padding and past the chunk
  auto eval = [&](int sp, int buf) {
    double *Pb = P + (size_t)buf * LD * S;
    const int tot = LD * S;
    for (int e = tid; e < tot; e += SG_THREADS) {
      const int r = e / S, s = e - r * S;
      const int i = n0 + sp * S + s;
      double v = 0.0;
      if (i < n1) {
        if (r < m) v = win_cov(kid, d, pr, Zl + r, LD, X + i, N, false);
        else if (r < mP) v = y[(size_t)(r - m) * N + i];
      }
      Pb[e] = v;
    }
  };
  double zr[4][MAXD], invl[MAXD];   // the lane's four rows lq + 4 r of the tile
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    invl[q] = q < d ? pr[q] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) zr[r][q] = (q < d && live) ? Zl[q * LD + rt * WPB + lq + 4 * r] : 0.0;
  }
  double s_amp = 0.0, s_ell[MAXD], az[WITH_Z ? 4 : 1][MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    s_ell[q] = 0.0;
#pragma unroll
    for (int r = 0; r < (WITH_Z ? 4 : 1); ++r) az[r][q] = 0.0;
  }
  const double *Ti = g.Ti + (size_t)f * g.tifs + (size_t)rt * WPB * LD + lane;   // the tile's operand image: k-step ks at ks * 64
  const int sl = l15 & (S - 1);
  const bool scol = l15 < S;
  if (nsp > 0) eval(0, 0);
  __syncthreads();
  for (int sp = 0; sp < nsp; ++sp) {
    const int buf = sp & 1;
    if (sp + 1 < nsp) eval(sp + 1, buf ^ 1);
    if (live) {
      const double *Pb = P + (size_t)buf * LD * S;
      const double *Bp = Pb + lq * S + sl;
      d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      for (int ks = 0; ks < nks; ks += 2) {   // (LD / 4 is even)
        const double a0 = Ti[(size_t)ks * 64], a1 = Ti[(size_t)(ks + 1) * 64];
        const double b0 = scol ? Bp[ks * 4 * S] : 0.0, b1 = scol ? Bp[(ks + 1) * 4 * S] : 0.0;
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
      }
      const int i = n0 + sp * S + l15;
      if (scol && i < n1) {
        double xi[MAXD];
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xi[q] = q < d ? X[(size_t)q * N + i] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * WPB + lq + 4 * r;
          if (row < m) {
            const double k = Pb[row * S + sl];
            const double Rv = 2.0 * (acc0[r] + acc1[r]);
            double df[MAXD], d2 = 0.0;
#pragma unroll
            for (int q = 0; q < MAXD; ++q) {
              df[q] = q < d ? (zr[r][q] - xi[q]) * invl[q] : 0.0;
              if (q < d) d2 = __builtin_fma(df[q], df[q], d2);
            }
            const double w = Rv * sg_factor<KC>(k, d2);
            s_amp = __builtin_fma(Rv, k, s_amp);
#pragma unroll
            for (int q = 0; q < MAXD; ++q) {
              if (q < d) {
                const double wd = w * df[q];
                s_ell[q] = __builtin_fma(wd, df[q], s_ell[q]);
                if constexpr (WITH_Z) az[r][q] += wd;
              }
            }
            if constexpr (WITH_Z && KC == SGK_BROWN) az[r][1] = __builtin_fma(Rv, sg_brown_extra(k, zr[r][0], xi[0]), az[r][1]);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  // the chunk's sums: theta over the whole wave, Z over the 16 sample lanes of each row, both in a fixed (butterfly) order
  double vals[1 + MAXD];
  vals[0] = s_amp;
#pragma unroll
  for (int q = 0; q < MAXD; ++q) vals[1 + q] = s_ell[q];
  double *tp = g.tpart + (((size_t)f * p.sh.nch + ch) * g.gh.mtr + rt) * GRAD_N;
#pragma unroll
  for (int i = 0; i < 1 + MAXD; ++i) {
    double v = vals[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) tp[i] = v;
  }
  if constexpr (WITH_Z) {
    double *zp = g.zpart + ((size_t)f * p.sh.nch + ch) * p.sh.LD * MAXD;
    const int nz = KC == SGK_BROWN ? 2 : d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rt * WPB + lq + 4 * r;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) {
        if (q < nz) {
          double v = az[r][q];
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
          if (l15 == 0 && row < m) zp[(size_t)row * MAXD + q] = v;
        }
      }
    }
  }
}

// One workgroup per (row tile of G_uu, fit): thread (i = tid & 15, part = tid >> 4) takes row rt 16 + i and the columns part, part +
// 16, ...; the sixteen parts of a row meet in LDS in part order, the rows of the tile in row order.
template <int KC>
__global__ __launch_bounds__(SGU_THREADS) void k_sparse_grad_uu(SparseArgs p, SparseGradArgs g) {
  __shared__ double red[SGU_THREADS / 16][WPB][1 + 2 * MAXD];
  const int rt = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  if (p.info[f] != 0) return;
  const int i = tid & 15, part = tid >> 4;
  const int m = p.m, d = p.d, kid = p.kid, LD = p.sh.LD;
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double *Z = p.Z + (size_t)f * d * m;
  const double *G = g.G + (size_t)f * LD * LD;
  const WaCov cv = WaCov::from_prep(kid, d, pr);
  const int row = rt * WPB + i;
  double zr[MAXD], zs[MAXD], dq[MAXD], s_amp = 0.0, s_ell[MAXD], az[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    zr[q] = (q < d && row < m) ? Z[(size_t)q * m + row] : 0.0;
    s_ell[q] = az[q] = 0.0;
  }
  if (row < m) {
    for (int col = part; col < m; col += SGU_THREADS / 16) {
      const double gv = G[(size_t)row * LD + col];
      if (col == row) {   // k(z, z): free of the length-scales; its derivative in z is RBF x Brownian's alone
        s_amp = __builtin_fma(gv, cv.kss(zr[0]), s_amp);
        if constexpr (KC == SGK_BROWN) az[1] = __builtin_fma(gv, window_grad_dkss(kid, pr, zr[0]), az[1]);
        continue;
      }
#pragma unroll
      for (int q = 0; q < MAXD; ++q) zs[q] = q < d ? Z[(size_t)q * m + col] : 0.0;
      const double k = cv.eval<false>(zr, zs, dq);
      double df[MAXD], d2 = 0.0;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) {
        df[q] = q < d ? (zr[q] - zs[q]) * cv.pr[q] : 0.0;
        if (q < d) d2 = __builtin_fma(df[q], df[q], d2);
      }
      const double w = gv * sg_factor<KC>(k, d2);
      s_amp = __builtin_fma(gv, k, s_amp);
#pragma unroll
      for (int q = 0; q < MAXD; ++q) {
        if (q < d) {
          const double wd = w * df[q];
          s_ell[q] = __builtin_fma(wd, df[q], s_ell[q]);
          az[q] = __builtin_fma(2.0, wd, az[q]);
        }
      }
      if constexpr (KC == SGK_BROWN) az[1] = __builtin_fma(2.0 * gv, sg_brown_extra(k, zr[0], zs[0]), az[1]);
    }
  }
  red[part][i][0] = s_amp;
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    red[part][i][1 + q] = s_ell[q];
    red[part][i][1 + MAXD + q] = az[q];
  }
  __syncthreads();
  if (tid < 1 + MAXD) {   // a theta sum of the tile
    double v = 0.0;
    for (int r = 0; r < WPB; ++r)
      for (int pt = 0; pt < SGU_THREADS / 16; ++pt) v += red[pt][r][tid];
    g.upart[((size_t)f * g.gh.mtr + rt) * GRAD_N + tid] = v;
  }
  if (tid >= 64 && tid < 64 + WPB * MAXD) {   // a Z sum of a row
    const int r = (tid - 64) / MAXD, q = (tid - 64) % MAXD;
    double v = 0.0;
    for (int pt = 0; pt < SGU_THREADS / 16; ++pt) v += red[pt][r][1 + MAXD + q];
    if (rt * WPB + r < m) g.uz[((size_t)f * LD + rt * WPB + r) * MAXD + q] = v;
  }
}

// One workgroup per fit.  Thread 0: the theta sums in (chunk, tile) order, then k_sparse_grad_uu's in tile order, then the t-term;
// every thread: entries of gradZ, the chunks in order, then k_sparse_grad_uu's.
__global__ __launch_bounds__(256) void k_sparse_grad_finish(SparseArgs p, SparseGradArgs g, int brown) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const int m = p.m, d = p.d, kid = p.kid, LD = p.sh.LD, nch = p.sh.nch, mtr = g.gh.mtr;
  const int nth = k_ntheta(kid, d);
  const bool bad = p.info[f] != 0;
  const double nan = __builtin_nan("");
  const double *pr = p.rec + (size_t)f * PREP_N;
  if (tid == 0) {
    double *gr = g.grad + (size_t)f * g.grad_stride;
    if (bad) {
      g.nll[f] = nan;
      for (int i = 0; i < nth; ++i) gr[i] = nan;
      if (g.lout)
        for (int q = 0; q < p.P; ++q) g.lout[(size_t)f * p.P + q] = nan;
    } else {
      double s[GRAD_N];
      for (int i = 0; i < GRAD_N; ++i) s[i] = 0.0;
      const double *tp = g.tpart + (size_t)f * nch * mtr * GRAD_N;
      for (int c = 0; c < nch * mtr; ++c)
        for (int i = 0; i < 1 + MAXD; ++i) s[i] += tp[(size_t)c * GRAD_N + i];
      const double *up = g.upart + (size_t)f * mtr * GRAD_N;
      for (int c = 0; c < mtr; ++c)
        for (int i = 0; i < 1 + MAXD; ++i) s[i] += up[(size_t)c * GRAD_N + i];
      s[0] += g.gs[(size_t)f * 4 + 1];
      // grad_from_sums states d(-logML) = -1/2 sum w dK; these sums carry dF/dK itself
      for (int i = 0; i < 1 + MAXD; ++i) s[i] *= 2.0;
      s[9] = 2.0 * g.gs[(size_t)f * 4];
      grad_from_sums(kid, d, p.theta + (size_t)f * MAX_THETA, s, gr);
      const double *lm = p.logml + (size_t)f * p.P;
      double bound = lm[0];   // the columns' bounds summed in column order
      for (int q = 1; q < p.P; ++q) bound += lm[q];
      g.nll[f] = -bound;
      if (g.lout)
        for (int q = 0; q < p.P; ++q) g.lout[(size_t)f * p.P + q] = lm[q];
    }
  }
  if (g.gradZ) {
    double *gz = g.gradZ + (size_t)f * d * m;
    for (int e = tid; e < d * m; e += 256) {
      const int q = e / m, row = e - q * m;
      double v = nan;
      if (!bad) {
        double sz = 0.0, sx = 0.0;   // the scaled-difference sums; RBF x Brownian's min(|z|, |x|) sums (slot 1, d = 1)
        for (int c = 0; c < nch; ++c) {
          const double *zp = g.zpart + (((size_t)f * nch + c) * LD + row) * MAXD;
          sz += zp[q];
          if (brown) sx += zp[1];
        }
        const double *uz = g.uz + ((size_t)f * LD + row) * MAXD;
        sz += uz[q];
        if (brown) sx += uz[1];
        v = sz * pr[q] - sx;   // d nll / dz = -dF/dz, dF/dz = -sz / ell + sx
      }
      gz[e] = v;
    }
  }
}

}  // namespace cgp
