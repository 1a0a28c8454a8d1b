// cgp_loo_grad.hpp -- value and gradient of the leave-one-out objective nlpd = -lpd_sum (cgp_loo_nll_grad[_batch[_device]],
// cgp_optimize_loo_batch; Rasmussen & Williams 5.4.2).  With Ky = L L^T, alpha = Ky^-1 y, kd_i = [Ky^-1]_ii (cgp_loo.hpp) and
//
//   c_i = 1/2 (1 / kd_i + alpha_i^2 / kd_i^2)      b_i = alpha_i / kd_i      beta = Ky^-1 b
//   d lpd_sum / dK = -Ky^-1 diag(c) Ky^-1 + 1/2 (beta alpha^T + alpha beta^T)
//
// the weight of k_grad's contraction (grad_from_sums returns -1/2 sum_ij w_ij dK_ij / dtheta, the gradient of the MINIMISED
// objective) is w_ij = -2 sum_k Ky^-1_ik c_k Ky^-1_kj + beta_i alpha_j + alpha_i beta_j.  With S = Ky^-1 diag(sqrt c) the first
// term is -2 S S^T, a symmetric product of ONE stored matrix, and beta = S (b / sqrt c) a matrix-vector product with the same one.
//
// After a gradient-mode fit (xid = 1, M = N) Wt = (L^-1)^T and alpha are resident; k_loo / k_loo_sum (cgp_loo.hpp) run as they
// stand and leave loo_var = 1 / kd and lpd_sum.  Then
//   k_loo_prep         sqrt c and b / sqrt c per sample; entries from N on are zeros.
//   k_loo_kinv         workgroup (pair, fit): k_grad's syrk over Wt leaves Ky^-1(ti, tj) in the accumulators; the tile goes into
//                      the scratch S in the row-panel layout of the next loop (element (row i, inner k) at i + k lds, lds = NT 128)
//                      twice: as block (i in ti, k in tj) scaled by sqrt c_k with 16-byte stores, and -- transposed through LDS,
//                      32 columns at a time per wave -- as block (i in tj, k in ti).  Diagonal pairs are stored once.  Rows and
//                      columns from N on are stored as ZEROS (the extra block's rows from N on hold the y row and padding), so
//                      every element of the lds x lds scratch is written by every call: nothing of an earlier call survives.
//   k_loo_beta         beta = S (b / sqrt c): workgroup (64 rows, fit), the inner index dealt round-robin to four waves whose
//                      sums meet in LDS in wave order (k_loo's shape).
//   k_loo_grad<MAT>    workgroup (pair, fit): mfma_rowpanel_loop over S, row panel tile ti, column panel tile tj, ALL NT 128 / 16
//                      chunks (the inner dimension is dense), the accumulators scaled by -2 on the VALU, alpha and beta of the
//                      tile's rows and columns in LDS where k_grad keeps alpha, then grad_tile_contract.
//   k_loo_grad_finish  one workgroup per fit: the pair partials in pair order -> grad_from_sums; nlpd = -lpd_sum; NaN into both
//                      for a fit whose info word is set.
// No atomics; every sum runs in a fixed order that involves neither the slot nor the neighbours.  fp64 only.
#pragma once
#include "cgp_kernels_fused.hpp"
#include "cgp_loo.hpp"

namespace cgp {

struct LooGradArgs {
  double *S;             // [nfit][lds][lds] Ky^-1 diag(sqrt c), row-panel layout
  size_t s_stride;       // lds lds
  int lds;               // NT 128: leading dimension of S and stride of the three vectors below
  const double *var;     // [nfit][N] loo_var = 1 / kd (k_loo's)
  const double *lsum;    // [nfit] lpd_sum (k_loo_sum's)
  double *sc, *u, *beta; // [nfit][lds] sqrt c, b / sqrt c, beta
  double *nlpd;          // [nfit]
  double *grad;          // [nfit][grad_stride]
  int grad_stride;
};

constexpr int LG_PREP_THREADS = 256;
__global__ __launch_bounds__(LG_PREP_THREADS) void k_loo_prep(FitArgs p, LooGradArgs g) {
  const int f = blockIdx.y, e = blockIdx.x * LG_PREP_THREADS + threadIdx.x;
  if (e >= g.lds) return;
  double s = 0.0, u = 0.0;
  if (e < p.N && p.info[f] == 0) {
    const double v = g.var[(size_t)f * p.N + e];
    const double al = reinterpret_cast<const double *>(p.alpha)[(size_t)f * p.alpha_stride + e];
    const double r = al * v;   // b_e
    s = sqrt(0.5 * (v + r * r));
    u = r / s;
  }
  g.sc[(size_t)f * g.lds + e] = s;
  g.u[(size_t)f * g.lds + e] = u;
}

constexpr int LG_TW = 33;   // LDS pitch of a wave's 32 x 32 transpose block, odd: the 8-byte reads of a half-wave (rows il, il + 1,
                            // columns 2 m) hit 64 distinct banks; the 8-byte writes of a 16-lane group (rows 2 l15 + j) are 2-way
                            // at any pitch (16 rows x 4 pitch dwords wrap the 32 banks twice); N^2 work beside an N^3 loop
__global__ __launch_bounds__(256, 2) void k_loo_kinv(FitArgs p, LooGradArgs g) {
  using P = Prec<double>;
  using acc_t = P::acc_t;
  typedef double d2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double *smem = reinterpret_cast<double *>(smem_raw);
  const int b = blockIdx.y, pair = blockIdx.x, tid = threadIdx.x;
  if (p.info[b] != 0) return;   // workgroup-uniform: nothing of a failed fit is read downstream
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ti, tj;
  grad_pair_tiles(pair, ti, tj);
  const double *Lw = reinterpret_cast<const double *>(p.Lw) + (size_t)b * p.lw_stride;
  const int ld = p.ld, N = p.N, lds = g.lds;
  const size_t rb = (size_t)p.NT * TS;

  acc_t acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = acc[cb][1] = acc_t{0, 0, 0, 0};
  const double *gR = Lw + rb + (size_t)ti * TS + (size_t)(ti * TS) * ld;
  const double *gC = Lw + rb + (size_t)tj * TS + (size_t)(ti * TS) * ld;
  mfma_rowpanel_loop<double, false>(acc, gR, (size_t)ld, gC, (size_t)ld, (p.NT - ti) * (TS / KT), smem, tid);   // Ky^-1(ti, tj)

  // acc[cb][j][r] = Ky^-1[ti 128 + wave 32 + 2 l15 + j][tj 128 + cb 16 + lq + 4 r]
  double *Sf = g.S + (size_t)b * g.s_stride;
  const double *scf = g.sc + (size_t)b * lds;
  const int i0 = ti * TS + wave * 32 + 2 * l15;
  const bool in0 = i0 < N, in1 = i0 + 1 < N;
  // block (i in ti, k in tj): a lane's two rows are adjacent
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = tj * TS + cb * DB + P::drow(lane, r);
      const bool ink = k < N;
      const double s = scf[k];
      *reinterpret_cast<d2 *>(Sf + (size_t)k * lds + i0) = d2{in0 && ink ? acc[cb][0][r] * s : 0.0, in1 && ink ? acc[cb][1][r] * s : 0.0};
    }
  if (ti == tj) return;
  // block (i in tj, k in ti) = the tile transposed, scaled by sqrt c of the tile's ROWS: two column blocks at a time through a
  // wave-private LDS block (the loop above ended on a barrier: its buffers are free), then rows of 32 contiguous doubles
  double *tw = smem + wave * (32 * LG_TW);
  const double s0 = scf[i0], s1 = scf[i0 + 1];
  const int m = lane & 15;
#pragma unroll
  for (int rd = 0; rd < NCB / 2; ++rd) {
#pragma unroll
    for (int cbl = 0; cbl < 2; ++cbl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cb = rd * 2 + cbl, cl = cbl * DB + P::drow(lane, r);
        const bool inc = tj * TS + cb * DB + P::drow(lane, r) < N;
        tw[(2 * l15) * LG_TW + cl] = in0 && inc ? acc[cb][0][r] * s0 : 0.0;
        tw[(2 * l15 + 1) * LG_TW + cl] = in1 && inc ? acc[cb][1][r] * s1 : 0.0;
      }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int il = lq + 4 * it;
      const d2 v{tw[il * LG_TW + 2 * m], tw[il * LG_TW + 2 * m + 1]};
      *reinterpret_cast<d2 *>(Sf + (size_t)(ti * TS + wave * 32 + il) * lds + tj * TS + rd * 32 + 2 * m) = v;
    }
    __syncthreads();
  }
}

constexpr int LG_EB = 64, LG_WAVES = 4, LG_UNROLL = 8;
__global__ __launch_bounds__(LG_WAVES * 64) void k_loo_beta(FitArgs p, LooGradArgs g) {
  __shared__ double red[LG_WAVES][LG_EB];
  const int b = blockIdx.y, N = p.N, lds = g.lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = blockIdx.x * LG_EB + lane;   // < lds: the grid is lds / 64
  double s = 0.0;
  if (p.info[b] == 0) {
    const double *__restrict__ Sf = g.S + (size_t)b * g.s_stride + i;
    const double *__restrict__ uf = g.u + (size_t)b * lds;
    for (int k = wave; k < N; k += LG_WAVES * LG_UNROLL) {
      double v[LG_UNROLL], w[LG_UNROLL];
#pragma unroll
      for (int q = 0; q < LG_UNROLL; ++q) {
        const int kk = k + q * LG_WAVES;
        v[q] = kk < N ? Sf[(size_t)kk * lds] : 0.0;
        w[q] = kk < N ? uf[kk] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < LG_UNROLL; ++q) s = fma(v[q], w[q], s);
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  g.beta[(size_t)b * lds + i] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

template <int MAT = 0>
__global__ __launch_bounds__(256, 2) void k_loo_grad(FitArgs p, LooGradArgs g, int npairs) {
  using T = double;
  using acc_t = typename Prec<T>::acc_t;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T *smem = reinterpret_cast<T *>(smem_raw);
  const int b = blockIdx.y, pair = blockIdx.x, tid = threadIdx.x;
  if (p.info[b] != 0) return;   // workgroup-uniform; k_loo_grad_finish reads no partial of a failed fit
  int ti, tj;
  grad_pair_tiles(pair, ti, tj);
  const int lds = g.lds, N = p.N;

  acc_t acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = acc[cb][1] = acc_t{0, 0, 0, 0};
  const T *Sf = g.S + (size_t)b * g.s_stride;
  mfma_rowpanel_loop<T, false>(acc, Sf + (size_t)ti * TS, (size_t)lds, Sf + (size_t)tj * TS, (size_t)lds, p.NT * (TS / KT), smem, tid);
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    acc[cb][0] *= T(-2);
    acc[cb][1] *= T(-2);
  }
  // alpha and beta of the tile's rows and columns, behind the coordinates that grad_tile_contract stages (its barrier covers both)
  T *ar = smem + 2 * MAXD * TS, *ac = ar + TS, *br = ac + TS, *bc = br + TS;
  const T *__restrict__ al = reinterpret_cast<const T *>(p.alpha) + (size_t)b * p.alpha_stride;
  const T *__restrict__ be = g.beta + (size_t)b * lds;
  if (tid < TS) {
    const int gi = ti * TS + tid, gj = tj * TS + tid;
    ar[tid] = gi < N ? al[gi] : T(0);
    ac[tid] = gj < N ? al[gj] : T(0);
    br[tid] = gi < N ? be[gi] : T(0);
    bc[tid] = gj < N ? be[gj] : T(0);
  }
  grad_tile_contract<T, MAT>(p, b, pair, npairs, ti, tj, acc, smem, smem_raw,
                             [&](T gg, int rl, int cl) { return gg + br[rl] * ac[cl] + ar[rl] * bc[cl]; });
}

constexpr int LGF_THREADS = 64;
__global__ __launch_bounds__(LGF_THREADS) void k_loo_grad_finish(FitArgs p, LooGradArgs g, int npairs) {
  __shared__ double s[GRAD_N];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int d = p.d, kid = p.kernel_id, nth = k_ntheta(kid, d);
  double *gr = g.grad + (size_t)f * g.grad_stride;
  if (p.info[f] != 0) {
    if (tid < nth) gr[tid] = __builtin_nan("");
    if (tid == 0) g.nlpd[f] = __builtin_nan("");
    return;
  }
  if (tid < GRAD_N) {   // the pairs' partial sums in pair order
    double v = 0.0;
    for (int pz = 0; pz < npairs; ++pz) v += p.gpart[((size_t)f * npairs + pz) * GRAD_N + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid == 0) grad_from_sums(kid, d, p.theta + (size_t)f * MAX_THETA, s, gr);
  else if (tid == 32) g.nlpd[f] = -g.lsum[f];
}

}  // namespace cgp
