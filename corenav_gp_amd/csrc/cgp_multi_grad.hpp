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
//                        k_panel relies on after its Gram tile.  Then k_grad's contraction with dK/dtheta (without the
//                        alpha_i alpha_j product) and its fixed-order workgroup reduction into gpart.
//   k_multi_grad_finish  one workgroup per fit: the pair partials in pair order -> gradient of -sum_p logml[p] with respect to the
//                        natural parameters (grad_from_sums' formulas), logml[p] added in p order -> nll; NaN into nll, the gradient
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
  const int b = blockIdx.y, pair = blockIdx.x;
  int ti = 0, rem = pair;
  while (rem > ti) {
    rem -= ti + 1;
    ++ti;
  }
  const int tj = rem;  // ti >= tj
  const T *Lw = reinterpret_cast<const T *>(p.Lw) + (size_t)b * p.lw_stride;
  const int ld = p.ld, N = p.N, d = p.d, kid = p.kernel_id;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
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

  // inputs of the tile: scaled coordinates [MAXD][128] of rows and columns
  const double *__restrict__ pr = p.prep + (size_t)b * PREP_N;
  T *xr = smem, *xc = smem + MAXD * TS;
  const T *__restrict__ Xb = reinterpret_cast<const T *>(p.X) + (size_t)b * d * N;
  const bool brown = kid == K_RBF_BROWNIAN;
  for (int idx = tid; idx < MAXD * TS; idx += 256) {
    const int q = idx >> 7, r = idx & 127;
    const T sc = brown ? T(1) : T(pr[q]);  // Brownian keeps the raw tick (GPy's r^2 expansion)
    const int gi = ti * TS + r, gj = tj * TS + r;
    xr[idx] = (q < d && gi < N) ? Xb[(size_t)q * N + gi] * sc : T(0);
    xc[idx] = (q < d && gj < N) ? Xb[(size_t)q * N + gj] * sc : T(0);
  }
  __syncthreads();
  const T amp = T(pr[9]), amp_b = T(pr[10]);
  const T inv_ell = T(pr[0]);
  double s_amp = 0, s_noise = 0, s_ell[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) s_ell[q] = 0;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cl = cb * DB + P::drow(lane, r);
      const int gcol = tj * TS + cl;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int rl = wave * 32 + 2 * l15 + j;
        const int grow = ti * TS + rl;
        const T w = acc[cb][j][r];   // sum_p A_ip A_jp - P Ky^-1_ij
        if (grow < N && gcol < N) {
          T kv, dq2[MAXD];
          T kg = T(0);   // what multiplies dq2 in the length-scale sums: k itself, Matern: -2 dk/dr^2
          if (!brown) {
            T d2 = 0;
#pragma unroll
            for (int q = 0; q < MAXD; ++q) {
              const T df = xr[q * TS + rl] - xc[q * TS + cl];
              dq2[q] = df * df;
              d2 += dq2[q];
            }
            if constexpr (MAT != 0) {
              double gm;
              kv = amp * matern_radial<MAT == 2, true>((double)d2, gm, [](double x) { return exp(x); });
              kg = amp * gm;
            } else {
              kv = amp * P::exp_(T(-0.5) * d2);
              kg = kv;
            }
          } else {
            const T x = xr[rl], xp = xc[cl];
            T r2 = (grow == gcol) ? T(0) : (T(-2) * x * xp + (x * x + xp * xp));
            r2 = r2 < T(0) ? T(0) : r2;
            const T rr = P::sqrt_(r2) * inv_ell;
            const int sx = (x > T(0)) - (x < T(0)), sp = (xp > T(0)) - (xp < T(0));
            const T ax = x < T(0) ? -x : x, ap = xp < T(0) ? -xp : xp;
            const T kb = (sx == sp) ? amp_b * (ax < ap ? ax : ap) : T(0);
            kv = amp * P::exp_(T(-0.5) * rr * rr) * kb;
#pragma unroll
            for (int q = 0; q < MAXD; ++q) dq2[q] = T(0);
            dq2[0] = rr * rr;
            kg = kv;
          }
          const double wk = w * kv;
          s_amp += wk;
          const double wg = MAT != 0 ? w * kg : wk;
#pragma unroll
          for (int q = 0; q < MAXD; ++q) s_ell[q] += wg * dq2[q];
          if (grow == gcol) s_noise += w;
        }
      }
    }
  }
  // workgroup reduction: wave shuffles, then LDS
  __syncthreads();
  double *red = reinterpret_cast<double *>(smem_raw);  // [4][GRAD_N]
  double vals[GRAD_N];
  vals[0] = s_amp;
#pragma unroll
  for (int q = 0; q < MAXD; ++q) vals[1 + q] = s_ell[q];
  vals[9] = s_noise;
  vals[10] = vals[11] = 0;
#pragma unroll
  for (int i = 0; i < GRAD_N; ++i) {
    double v = vals[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave * GRAD_N + i] = v;
  }
  __syncthreads();
  if (tid < GRAD_N) {
    const double wgt = (ti == tj) ? 1.0 : 2.0;
    const double v = (red[tid] + red[GRAD_N + tid]) + (red[2 * GRAD_N + tid] + red[3 * GRAD_N + tid]);
    p.gpart[((size_t)b * npairs + pair) * GRAD_N + tid] = wgt * v;
  }
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
    const double *th = p.theta + (size_t)f * MAX_THETA;
    g[0] = -0.5 * s[0] / th[0];
    if (kid == K_SE_ISO) {
      double se = 0.0;
      for (int q = 0; q < d; ++q) se += s[1 + q];
      g[1] = -0.5 * se / th[1];
      g[2] = -0.5 * s[9];
    } else if (k_is_ard(kid)) {
      for (int q = 0; q < d; ++q) g[1 + q] = -0.5 * s[1 + q] / th[1 + q];
      g[d + 1] = -0.5 * s[9];
    } else {
      g[1] = -0.5 * s[1] / th[1];
      g[2] = -0.5 * s[0] / th[2];
      g[3] = -0.5 * s[9];
    }
  } else if (tid == 32) {   // the columns' logml in p order
    double t = 0.0;
#pragma unroll 8
    for (int i = 0; i < m.P; ++i) t += lf[i];
    m.nll[f] = -t;
  }
}

}  // namespace cgp
