// cgp_multi_grad.hpp -- multi-target fits: value and gradient of the SUMMED objective -sum_p logml[p] over one shared theta
// (cgp_multi_nll_grad_batch[_device], cgp_optimize_multi_batch).  GPy's ExactGaussianInference with P columns:
//
//   Ky = L L^T     Z = L^-1 Y  (N x P)     A = Ky^-1 Y = Wt Z     dL/dK = 1/2 (A A^T - P Ky^-1)     Ky^-1 = Wt Wt^T
//
// After a gradient-mode fit (xid = 1, M = N) L, the W_k images and Wt = (L^-1)^T (the panel's extra block, k_grad's header
// comment) are resident; Z comes from k_multi_pack / k_multi_solve and logml[p] from k_multi_logml (cgp_multi.hpp) as they stand.
//   k_multi_alpha        A = Wt Z.  Workgroup (row tile of 128 samples, tile of 128 targets, fit); Wt[e][c] = 0 for c < e, so the
//                        inner dimension starts at column block ti (as in k_grad).  mfma_rowpanel_loop's shape: row panel Wt,
//                        column panel the Z scratch.  The tile goes column-major over the targets into a second scratch,
//                        Aw[p lda + i], lda = NT 128, for p < P rounded up to 16 (targets from P on are zeros of the Z scratch, so
//                        they come out as zeros) with zeros in the samples from N on: the panel layout of the next loop.
//   k_multi_grad<MAT>    k_grad's tile-pair kernel with w_ij = sum_p A_ip A_jp - P Ky^-1_ij formed on the matrix cores: the syrk
//                        loop over Wt leaves Ky^-1(ti, tj) in the 8 x 2 accumulators, the VALU scales them by -P, and the SAME loop
//                        continues over Aw (row panel tile ti, column panel tile tj, P / 16 chunks of the inner dimension p) into
//                        the live accumulators -- mfma_rowpanel_loop never clears them and ends on a barrier, which is what
//                        k_panel relies on after its Gram tile.  Then grad_tile_contract (cgp_kernels_fused.hpp), the contraction
//                        with dK/dtheta and the fixed-order workgroup reduction into gpart that k_grad runs, with the
//                        accumulator itself as the weight.
//   k_multi_grad_finish  one workgroup per fit: the pair partials in pair order -> gradient of -sum_p logml[p] with respect to the
//                        natural parameters (grad_from_sums), logml[p] added in p order -> nll; NaN into nll, the gradient
//                        and logml of a fit whose info word is set.
// No atomics; every sum runs in a fixed order that does not involve the slot or the neighbours.  The sum over p IS the inner
// dimension of an MFMA loop: permuting the columns of Y changes the result to rounding, not bitwise.  fp64 only.
#pragma once
#include "cgp_multi.hpp"

namespace cgp {

struct MultiGradArgs {
  const double *Zw;      // [nfit][NT 128][ldz] Z of the call's first fit (k_multi_solve's)
  size_t z_stride;
  int ldz;
  double *Aw;            // [nfit][P16][lda] A = Ky^-1 Y of the call's first fit, column-major over the targets
  size_t a_stride;
  int lda;               // NT 128
  int P, P16;            // targets, rounded up to 16
  double *logml;         // [nfit][P]
  double *nll;           // [nfit]
  double *grad;          // [nfit][grad_stride]
  int grad_stride;
};

__global__ __launch_bounds__(256, 2) void k_multi_alpha(FitArgs p, MultiGradArgs m) {
  using P = Prec<double>;
  using acc_t = P::acc_t;
  typedef double d2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double *smem = reinterpret_cast<double *>(smem_raw);
  const int ti = blockIdx.x, pt = blockIdx.y, f = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ld = p.ld;
  const double *Lw = reinterpret_cast<const double *>(p.Lw) + (size_t)f * p.lw_stride;
  const size_t rb = (size_t)p.NT * TS;
  acc_t acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = acc[cb][1] = acc_t{0, 0, 0, 0};
  const double *gR = Lw + rb + (size_t)ti * TS + (size_t)(ti * TS) * ld;
  const double *gC = m.Zw + (size_t)f * m.z_stride + (size_t)pt * TS + (size_t)(ti * TS) * m.ldz;
  mfma_rowpanel_loop<double, false>(acc, gR, (size_t)ld, gC, (size_t)m.ldz, (p.NT - ti) * (TS / KT), smem, tid);
  // acc[cb][j][r] = A[sample ti 128 + wave 32 + 2 l15 + j][target pt 128 + cb 16 + drow(lane, r)]: a lane's two samples are adjacent
  const int i0 = ti * TS + wave * 32 + 2 * l15;
  const bool in0 = i0 < p.N, in1 = i0 + 1 < p.N;   // rows of the extra block from N on are the y row and padding
  double *Af = m.Aw + (size_t)f * m.a_stride + i0;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pc = pt * TS + cb * DB + P::drow(lane, r);
      if (pc < m.P16) *reinterpret_cast<d2 *>(Af + (size_t)pc * m.lda) = d2{in0 ? acc[cb][0][r] : 0.0, in1 ? acc[cb][1][r] : 0.0};
    }
}

template <int MAT = 0>
__global__ __launch_bounds__(256, 2) void k_multi_grad(FitArgs p, MultiGradArgs m, int npairs) {
  using T = double;
  using P = Prec<T>;
  using acc_t = typename P::acc_t;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T *smem = reinterpret_cast<T *>(smem_raw);
  const int b = blockIdx.y, pair = blockIdx.x, tid = threadIdx.x;
  int ti, tj;
  grad_pair_tiles(pair, ti, tj);
  const T *Lw = reinterpret_cast<const T *>(p.Lw) + (size_t)b * p.lw_stride;
  const int ld = p.ld;
  const size_t rb = (size_t)p.NT * TS;

  acc_t acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = acc[cb][1] = acc_t{0, 0, 0, 0};
  const T *gR = Lw + rb + (size_t)ti * TS + (size_t)(ti * TS) * ld;
  const T *gC = Lw + rb + (size_t)tj * TS + (size_t)(ti * TS) * ld;
  mfma_rowpanel_loop<T, false>(acc, gR, (size_t)ld, gC, (size_t)ld, (p.NT - ti) * (TS / KT), smem, tid);   // Ky^-1(ti, tj)
  const T mp = -(T)m.P;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    acc[cb][0] *= mp;
    acc[cb][1] *= mp;
  }
  // + A(ti, :) A(tj, :)^T over the targets (the loop above ended on a barrier: its LDS buffers are free)
  const T *Af = m.Aw + (size_t)b * m.a_stride;
  mfma_rowpanel_loop<T, false>(acc, Af + (size_t)ti * TS, (size_t)m.lda, Af + (size_t)tj * TS, (size_t)m.lda, m.P16 / KT, smem, tid);

  // acc = sum_p A_ip A_jp - P Ky^-1_ij is the weight itself
  grad_tile_contract<T, MAT>(p, b, pair, npairs, ti, tj, acc, smem, smem_raw, [](T w, int, int) { return w; });
}

constexpr int MGF_THREADS = 64;
__global__ __launch_bounds__(MGF_THREADS) void k_multi_grad_finish(FitArgs p, MultiGradArgs m, int npairs) {
  __shared__ double s[GRAD_N];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int d = p.d, kid = p.kernel_id, nth = k_ntheta(kid, d);
  double *g = m.grad + (size_t)f * m.grad_stride;
  double *lf = m.logml + (size_t)f * m.P;
  if (p.info[f] != 0) {
    for (int i = tid; i < m.P; i += MGF_THREADS) lf[i] = __builtin_nan("");
    if (tid < nth) g[tid] = __builtin_nan("");
    if (tid == 0) m.nll[f] = __builtin_nan("");
    return;
  }
  if (tid < GRAD_N) {   // the pairs' partial sums in pair order
    double v = 0.0;
    for (int pz = 0; pz < npairs; ++pz) v += p.gpart[((size_t)f * npairs + pz) * GRAD_N + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    grad_from_sums(kid, d, p.theta + (size_t)f * MAX_THETA, s, g);
  } else if (tid == 32) {   // the columns' logml in p order
    double t = 0.0;
#pragma unroll 8
    for (int i = 0; i < m.P; ++i) t += lf[i];
    m.nll[f] = -t;
  }
}

}  // namespace cgp
