// Leave-one-out cross-validation in closed form from a gradient-mode factorisation (fp64; Rasmussen & Williams eq. 5.10-5.12,
// GPy's inference_method.LOO):
//     kd_e = [Ky^-1]_ee      loo_var_e = 1 / kd_e      loo_mean_e = y_e - alpha_e / kd_e
//     loo_lpd_e = -0.5 log(2 pi loo_var_e) - 0.5 (y_e - loo_mean_e)^2 / loo_var_e
// After run(..., xid = 1, M = N) the extra block of the factor panel holds Wt = (L^-1)^T (k_grad's header comment) and p.alpha
// holds alpha, so kd_e = sum_{c >= e} Wt[e][c]^2 is one pass over rows that are already there: N^2 / 2 doubles per fit, no
// matrix-core work.  Element (e, c) of Wt is at Lw[b * lw_stride + NT * TS + e + c * ld] -- e runs contiguously.
#pragma once
#include "cgp_kernels.hpp"

namespace cgp {

constexpr int LOO_EB = 64;      // samples per workgroup: one wave's width, so a wave reads 512 contiguous bytes per column
constexpr int LOO_WAVES = 4;    // the column range of a workgroup is dealt round-robin to its waves
constexpr int LOO_UNROLL = 8;   // loads in flight per lane

// Workgroup (eb, fit): lanes along e, wave w takes the columns c = c0 + w, c0 + w + 4, ... of [c0, N), c0 the start of e's
// 128-column block (Wt is zero in front of it, and nothing in front of it is read).  Rows e >= N and columns c >= N are masked,
// never trusted to hold zeros.  The four partial sums meet in LDS and are added in wave order; no atomics.  Several workgroups
// per fit (N / 64) come from the split along e, so a sum never crosses a workgroup.  lpd (batch, N) is never null (k_loo_sum
// reads it: the caller's loo_lpd, or scratch); loo_mean and loo_var may be.  A fit whose info is non-zero gets NaN.
__global__ __launch_bounds__(LOO_WAVES * 64) void k_loo(FitArgs p, double *__restrict__ loo_mean, double *__restrict__ loo_var,
                                                         double *__restrict__ lpd) {
  __shared__ double red[LOO_WAVES][LOO_EB];
  const int b = blockIdx.y, N = p.N, ld = p.ld;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e0 = blockIdx.x * LOO_EB, e = e0 + lane;
  const bool live = e < N;
  const bool bad = p.info[b] != 0;
  double s = 0.0;
  if (live && !bad) {
    const double *__restrict__ wt =
        reinterpret_cast<const double *>(p.Lw) + (size_t)b * p.lw_stride + (size_t)p.NT * TS + e;
    const int c0 = (e0 / TS) * TS;
    for (int c = c0 + wave; c < N; c += LOO_WAVES * LOO_UNROLL) {
      double v[LOO_UNROLL];
#pragma unroll
      for (int u = 0; u < LOO_UNROLL; ++u) {
        const int cc = c + u * LOO_WAVES;
        v[u] = cc < N ? wt[(size_t)cc * ld] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LOO_UNROLL; ++u) s = fma(v[u], v[u], s);
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || !live) return;
  const double kd = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  const double nan = __builtin_nan("");
  double m = nan, v = nan, l = nan;
  if (!bad) {
    const double al = reinterpret_cast<const double *>(p.alpha)[(size_t)b * p.alpha_stride + e];
    const double ye = reinterpret_cast<const double *>(p.y)[(size_t)b * N + e];
    v = 1.0 / kd;
    const double r = al * v;   // y_e - loo_mean_e
    m = ye - r;
    l = -0.5 * log(6.283185307179586476925286766559 * v) - 0.5 * r * al;   // r^2 / loo_var = alpha^2 / kd
  }
  const size_t o = (size_t)b * N + e;
  if (loo_mean) loo_mean[o] = m;
  if (loo_var) loo_var[o] = v;
  lpd[o] = l;
}

// lpd_sum of every fit, one wave per fit, in a fixed order: lane l adds entries l, l + 64, ... in index order, then the 64
// partial sums meet in a butterfly (both partners add the same pair, so every lane holds the same bits).
__global__ __launch_bounds__(64) void k_loo_sum(const double *__restrict__ lpd, const int *__restrict__ info, int N,
                                                double *__restrict__ lpd_sum) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int i = lane; i < N; i += 64) s += lpd[(size_t)b * N + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) lpd_sum[b] = info[b] != 0 ? __builtin_nan("") : s;
}

}  // namespace cgp
