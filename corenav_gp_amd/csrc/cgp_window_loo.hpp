// cgp_window_loo.hpp -- leave-one-out cross-validation of the resident sliding windows (cgp_window_loo), from the factor, z,
// the inputs and the targets as they stand after any number of pushes (formulas: cgp_loo.hpp).
//
//   k_window_loo          One WAVE = one window x one chunk of 16 columns [c0, c0 + 16): chunk_forward_solve<true>
//                         (cgp_window_adapt.hpp, the forward half k_window_kinv_grad also runs) gives V = L^-1 E for the chunk
//                         and the columns' sums of squares; V lives, transposed, in the chunk's tile row of the slab's strict
//                         upper triangle (the lower triangle, the diagonal, z, the samples and the state words are NOT
//                         written).  The 16 sums are kd = diag(Ky^-1) of the chunk's samples; with k_window_alpha's alpha and
//                         yw the wave writes its 16 entries of loo_mean / loo_var / loo_lpd at the window-order index
//                         (0 = oldest sample) and one partial sum of loo_lpd.
//   k_window_loo_finish   per window: the chunks' partial sums added in chunk order (no atomics); NaN for the entries [n, N) of a
//                         window still filling; NaN everywhere (sum included) for a failed window; NaN rows and sum 0 for an
//                         empty one.
// Origin and size come from the window's state words: no host mirror, nothing depends on the slot.
#pragma once
#include "cgp_window_adapt.hpp"

namespace cgp {

struct WindowLooOut {
  double *mean, *var, *lpd;   // [nwin][N], each may be null
  double *sum;                // [nwin] or null
  double *part;               // [nwin][NB] the chunks' partial sums of loo_lpd (scratch)
};

__global__ __launch_bounds__(256) void k_window_loo(AdaptArgs p, WindowLooOut out) {
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gid = (long long)blockIdx.x * 4 + wave;
  if (gid >= (long long)p.nwin * p.NB) return;
  const int w = (int)(gid / p.NB), J = (int)(gid - (long long)w * p.NB);
  const int CAP = p.CAP;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const int nb = (n + WPB - 1) / WPB;
  if (bad != 0 || J >= nb) {
    if (lane == 0) out.part[(size_t)w * p.NB + J] = 0.0;
    return;
  }
  double *S = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0): lower triangle read, strict upper triangle scratch
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  const int gj = J * WPB + l15;
  const bool colok = gj < n;
  double ss;   // this lane's share of column l15's sum of squares
  chunk_forward_solve<true>(S, dinv, CAP, n, nb, J, l15, lq, ss);

  // ---- kd of column l15: the four row groups' shares (fixed order), then this sample's three outputs
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);
  const double nan = __builtin_nan("");
  double m = nan, v = nan, l = 0.0;
  if (colok) {
    const double al = p.alpha[(size_t)w * p.NB * WPB + gj];
    const double ye = p.yw[(size_t)w * CAP + o + gj];
    v = 1.0 / ss;
    const double r = al * v;   // y_j - loo_mean_j
    m = ye - r;
    l = -0.5 * log(6.283185307179586476925286766559 * v) - 0.5 * r * al;
  }
  double ls = l;   // columns past the window add 0
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) ls += __shfl_xor(ls, off);
  if (lq == 0 && colok) {
    const size_t oi = (size_t)w * p.N + gj;
    if (out.mean) out.mean[oi] = m;
    if (out.var) out.var[oi] = v;
    if (out.lpd) out.lpd[oi] = l;
  }
  if (lane == 0) out.part[(size_t)w * p.NB + J] = ls;
}

__global__ __launch_bounds__(64) void k_window_loo_finish(AdaptArgs p, WindowLooOut out) {
  const int w = blockIdx.x, lane = threadIdx.x;
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const double nan = __builtin_nan("");
  const int first = (bad != 0 || n <= 0) ? 0 : n;   // entries [first, N) hold no sample (or the window failed)
  for (int i = first + lane; i < p.N; i += 64) {
    const size_t oi = (size_t)w * p.N + i;
    if (out.mean) out.mean[oi] = nan;
    if (out.var) out.var[oi] = nan;
    if (out.lpd) out.lpd[oi] = nan;
  }
  if (lane != 0 || !out.sum) return;
  double s = 0.0;
  if (bad != 0) {
    s = nan;
  } else if (n > 0) {
    const int nb = (n + WPB - 1) / WPB;
    for (int J = 0; J < nb; ++J) s += out.part[(size_t)w * p.NB + J];
  }
  out.sum[w] = s;
}

}  // namespace cgp
