// cgp_window_joint.hpp -- joint forecast from the sliding windows' resident state: the full posterior covariance at M test
// points (cgp_window_predict_cov) and sample paths drawn from it (cgp_window_sample).
//
//   V = L^-1 K(X, xs)      cov = K(xs, xs) - V^T V      C C^T = cov (+ sigma_n^2 I) + jitter I      path = mean + C xi
//
// Four stages, plain launches on one stream, every one a function of the window's own data only (no atomics, no split whose
// order depends on scheduling: a window's result depends neither on its slot nor on its neighbours):
//   k_window_forecast<.., KEEP>  the marginal forecast's solve (cgp_window_forecast.hpp) with every finished V(I) block also
//                         stored: [window][test-point tile of 16][row][16], so that a k-step of the contraction below reads 64
//                         consecutive doubles per operand.  Its mean is the joint mean and its variance the diagonal of cov:
//                         both are bitwise cgp_window_predict's.
//   k_window_joint_cov    cov(J, I) = K**(J, I) - sum_k V(k, J)^T V(k, I) on v_mfma_f64_16x16x4_f64.  One WAVE owns a 64 x 64
//                         super-tile (4 x 4 accumulator tiles: eight operand loads feed sixteen MFMAs per k-step) of the lower
//                         triangle and runs the whole sum over k itself, in row order; the Gram tile, evaluated in registers with
//                         win_cov's formulas, is the accumulators' start value and the next row block's operands are requested
//                         before this one's MFMAs.  Tiles above the diagonal of a diagonal super-tile are skipped.  The
//                         workgroups of a window run on one XCD (the forecast's numbering), so V comes from that XCD's L2.
//                         Output form: both triangles of the caller's (M, M) matrix from the same register (exactly symmetric),
//                         the diagonal replaced by the forecast's variance (clip and noise included).  Scratch form (sampling):
//                         the lower triangle, column-major with leading dimension M padded to 16, identity in the padding.
//   k_window_joint_chol   k_window_refactor's left-looking block Cholesky, written out a second time: a shared block-column step
//                         was slower (docs/negatives.md item 20), so a fix there goes into both kernels (transposed tiles, diagonal
//                         block by one wave in registers with factor_block16_repair, L(J, J)^-1 applied with four chained MFMAs)
//                         with the start tile read from the scratch matrix instead of evaluated, the jitter added to the diagonal
//                         as it is read; in place.  A non-positive pivot is repaired (nothing faults) and reported.
//   k_window_joint_paths  out = mean + C xi: one wave per (16 test points) x (16 paths) tile, sum over the block columns up to
//                         the diagonal one (masked above the diagonal).  NaN for a window whose factorisation failed.
// Forms by the window length N alone, as in the forecast (N <= 512 tuned, the two longer forms correct only); the Cholesky
// holds 4 / 8 tiles per wave for M <= 512 / 1024.  Read-only on the windows.
#pragma once
#include "cgp_window_adapt.hpp"

namespace cgp {

constexpr int WJ_THREADS = 256;   // k_window_joint_cov / _paths: four independent waves
constexpr int WJ_WAVES = WJ_THREADS / 64;
constexpr int WJ_ST = 4;          // tiles per side of a wave's super-tile

struct JointArgs {
  const int *state;
  const double *prep, *theta;
  const double *xs;     // [nwin][M][d]
  const double *V;      // [nwin][mt][nrow][16]  (k_window_forecast<.., true>)
  const double *mean;   // [nwin][M]
  const double *var;    // [nwin][M] the forecast's variance: clipped, noise included when asked for
  double *cov;          // output form: [nwin][M][M]
  double *C;            // scratch form: [nwin][mt * 16][mt * 16], lower triangle column-major; the factor overwrites it
  const double *xi;     // [nwin][S][M]
  double *out;          // [nwin][S][M]
  int *info, *jinfo;    // [nwin] caller's (may be null) and the context's own failure words
  double jitter_rel;
  int d, kernel_id, M, S, nwin;
  int mt, nrow;         // tiles of 16 test points, rows of a V tile (NB * 16)
  int nsup, npair, per_win;   // super-tiles per side, pairs of the lower triangle, workgroups per window
};

template <bool SCRATCH>
__global__ __launch_bounds__(WJ_THREADS) void k_window_joint_cov(JointArgs p) {
  // workgroup -> (window, group of super-tile pairs): consecutive ids on ONE XCD
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nwin * p.per_win) return;
  const int w = lid / p.per_win;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = (lid - w * p.per_win) * WJ_WAVES + wave;
  if (pair >= p.npair) return;
  int BI = 0;
  while ((BI + 1) * (BI + 2) / 2 <= pair) ++BI;
  const int BJ = pair - BI * (BI + 1) / 2;   // BJ <= BI
  const int M = p.M, mt = p.mt, d = p.d, kid = p.kernel_id;
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const int nb = (bad != 0 || n <= 0) ? 0 : (n + WPB - 1) / WPB;
  const WaCov cv = WaCov::from_prep(kid, d, p.prep + (size_t)w * PREP_N);
  const double *xs = p.xs + (size_t)w * M * d;
  // tile (b, a): rows j = (BJ 4 + b) 16 + lq + 4 r (A operand), columns i = (BI 4 + a) 16 + l15 (B operand)
  auto live = [&](int b, int a) { return BI * WJ_ST + a < mt && BJ * WJ_ST + b <= BI * WJ_ST + a; };
  d4 acc[WJ_ST][WJ_ST];
  {
    double xc[WJ_ST][MAXD];
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) {
      const int i = (BI * WJ_ST + a) * WPB + l15;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) xc[a][q] = (q < d && i < M) ? xs[(size_t)i * d + q] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = (BJ * WJ_ST + b) * WPB + lq + 4 * r;
        double xr[MAXD], dq[MAXD];
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xr[q] = (q < d && j < M) ? xs[(size_t)j * d + q] : 0.0;
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a) acc[b][a][r] = live(b, a) ? cv.eval<false>(xr, xc[a], dq) : 0.0;
      }
  }
  // operands of row block kb: lane (l15, lq) holds V[kb 16 + 4 ks + lq][tile 16 + l15] -- 64 consecutive doubles per k-step
  const double *Vw = p.V + (size_t)w * mt * p.nrow * WPB + (size_t)lq * WPB + l15;
  const double *va[WJ_ST], *vb[WJ_ST];
#pragma unroll
  for (int t = 0; t < WJ_ST; ++t) {
    const int tj = BJ * WJ_ST + t < mt ? BJ * WJ_ST + t : mt - 1, ti = BI * WJ_ST + t < mt ? BI * WJ_ST + t : mt - 1;
    va[t] = Vw + (size_t)tj * p.nrow * WPB;
    vb[t] = Vw + (size_t)ti * p.nrow * WPB;
  }
  auto load = [&](int kb, double (&fa)[WJ_ST][4], double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = va[t][(size_t)(kb * WPB + 4 * ks) * WPB];
        fb[t][ks] = vb[t][(size_t)(kb * WPB + 4 * ks) * WPB];
      }
  };
  double fa[WJ_ST][4], fb[WJ_ST][4], ga[WJ_ST][4], gb[WJ_ST][4];
  if (nb > 0) load(0, fa, fb);
  for (int kb = 0; kb < nb; ++kb) {
    if (kb + 1 < nb) load(kb + 1, ga, gb);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a)
          if (live(b, a)) acc[b][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(-fa[b][ks], fb[a][ks], acc[b][a], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = ga[t][ks];
        fb[t][ks] = gb[t][ks];
      }
  }
  const double *var = p.var + (size_t)w * M;
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
        double v = bad != 0 ? __builtin_nan("") : acc[b][a][r];
        if (i < M && j < M) {
          if (i == j) v = var[i];   // the shared solve's variance (NaN for a failed window)
          if constexpr (SCRATCH) {
            p.C[(size_t)w * mpad * mpad + (size_t)j * mpad + i] = v;
          } else if (!dtile || j <= i) {
            double *cw = p.cov + (size_t)w * M * M;
            cw[(size_t)j * M + i] = v;
            if (i != j) cw[(size_t)i * M + j] = v;
          }
        } else if constexpr (SCRATCH) {
          p.C[(size_t)w * mpad * mpad + (size_t)j * mpad + i] = (i == j) ? 1.0 : 0.0;   // padding: identity
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// In-place Cholesky of the scratch matrix (k_window_refactor's scheme, the start tile from memory).  One workgroup per window.
template <int TPW>
__global__ __launch_bounds__(WA_THREADS) void k_window_joint_chol(JointArgs p) {
  __shared__ double tile[WPB * WPB];   // the diagonal tile, [c * 16 + r]
  __shared__ double winv[WPB * WPB];   // L(J, J)^-1, element (row m, column k) at k * 16 + m
  const int w = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = p.M, mt = p.mt, mpad = mt * WPB;
  double *Cw = p.C + (size_t)w * mpad * mpad;
  // jitter = jitter_rel x the mean of the diagonal: every wave forms the same sum in the same order
  double jit;
  {
    const double *var = p.var + (size_t)w * M;
    double s = 0.0;
    for (int i = lane; i < M; i += 64) s += var[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    jit = p.jitter_rel * (s / (double)M);
  }
  int bad = 0;
  for (int J = 0; J < mt; ++J) {
    const int J0 = J * WPB;
    // the wave's tiles of block column J, transposed: acc[t][r] = element (row I_t 16 + l15, column J0 + lq + 4 r)
    d4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int I = J + wave + WA_WAVES * t;
      acc[t] = d4{0.0, 0.0, 0.0, 0.0};
      if (I < mt) {
        const int gi = I * WPB + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gj = J0 + lq + 4 * r;
          const double v = Cw[(size_t)gj * mpad + gi];
          acc[t][r] = (gi == gj && gi < M) ? v + jit : v;
        }
      }
    }
    for (int kb = 0; kb < J; ++kb) {
      const double *col = Cw + (size_t)(kb * WPB + lq) * mpad;
      double a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[ks] = -col[(size_t)(4 * ks) * mpad + J0 + l15];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int I = J + wave + WA_WAVES * t;
        if (I < mt) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = col[(size_t)(4 * ks) * mpad + I * WPB + l15];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    // wave 0: the diagonal block (its first tile) in registers, lane = row; the inverse goes to LDS
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(lq + 4 * r) * WPB + l15] = acc[0][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      double a[WPB], wv[WPB];
#pragma unroll
      for (int c = 0; c < WPB; ++c) a[c] = tile[c * WPB + l15];
      int badl = 0;
      factor_block16_repair<double>(a, wv, badl, J0, l15);
      if (bad == 0) bad = badl;
      if (lane < WPB) {
#pragma unroll
        for (int m = 0; m < WPB; ++m) winv[l15 * WPB + m] = wv[m];
#pragma unroll
        for (int c = 0; c < WPB; ++c)
          if (c <= l15) Cw[(size_t)(J0 + c) * mpad + J0 + l15] = a[c];
      }
    }
    __syncthreads();
    {
      double di[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) di[r] = winv[(lq + 4 * r) * WPB + l15];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int I = J + wave + WA_WAVES * t;
        if (I < mt && I > J) {
          d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[t][r], v, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) Cw[(size_t)(J0 + lq + 4 * r) * mpad + I * WPB + l15] = v[r];
        }
      }
    }
    __syncthreads();   // block column J is in memory before block column J + 1 reads it
  }
  if (wave == 0 && lane == 0) {   // lane 0 saw every pivot's verdict (the row broadcasts reach all lanes)
    p.jinfo[w] = bad;
    if (p.info) p.info[w] = bad;
  }
}

// out = mean + C xi.  One wave per (tile of 16 test points) x (tile of 16 paths).
__global__ __launch_bounds__(WJ_THREADS) void k_window_joint_paths(JointArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = p.M, S = p.S, mt = p.mt, mpad = mt * WPB;
  const int st = (S + WPB - 1) / WPB;
  const int w = blockIdx.x / p.per_win;
  const int unit = (blockIdx.x - w * p.per_win) * WJ_WAVES + wave;
  if (unit >= mt * st) return;
  const int I = mt - 1 - unit / st, T = unit % st;   // the long rows first
  const double *Cw = p.C + (size_t)w * mpad * mpad;
  const double *xi = p.xi + (size_t)w * S * M;
  const int s = T * WPB + l15, m0 = I * WPB;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int K = 0; K <= I; ++K) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = K * WPB + 4 * ks + lq;
      const double a = k <= m0 + l15 ? Cw[(size_t)k * mpad + m0 + l15] : 0.0;   // C(m0 + l15, k): zero above the diagonal
      const double b = (s < S && k < M) ? xi[(size_t)s * M + k] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
  }
  const bool failed = p.jinfo[w] != 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + lq + 4 * r;
    if (s < S && m < M)
      p.out[((size_t)w * S + s) * M + m] = failed ? __builtin_nan("") : p.mean[(size_t)w * M + m] + acc[r];
  }
}

}  // namespace cgp
