// cgp_window_forecast.hpp -- multi-point forecast from the sliding windows' resident state (cgp_window_predict).
//
// The push kernels (cgp_window.hpp) keep, per window, the factor L of Ky = K + (sigma_n^2 + 1e-8) I, z = L^-1 y and the
// window's inputs up to date; a forecast at M test points needs nothing else:
//   K*[i][j] = k(x_i, xs_j)        V = L^-1 K*        mean_j = sum_i V_ij z_i        var_j = k(xs_j, xs_j) - sum_i V_ij^2
// (no back-substitution: z is maintained by every tick).  This is what the reference's producer publishes
// (gp_slip_node.py:45-61: mean and variance over the next 600 ticks), on a window that is maintained instead of refitted.
//
// The work is n^2 M flops per window -- a blocked forward substitution on the fp64 MFMA (v_mfma_f64_16x16x4_f64):
//   k_window_diag_inv   pre-pass, one 16-lane row per 16 x 16 diagonal block of every window: the block's inverse (lane j
//                       = column j, sixteen substitution steps in registers) into a context scratch buffer.  The blocks are
//                       counted from the window's origin, which moves every tick, so the inverses are formed per call; the
//                       strict upper triangle of the slab is NOT read (the push kernels leave by-products there).
//   k_window_forecast   one workgroup (eight waves) = one window x one chunk of test points.  Left-looking over the row
//                       blocks I:  acc = K*(I, chunk) - sum_{J<I} L(I, J) V(J, chunk);  V(I) = L(I, I)^-1 acc.
//                       The chunk's V stays in LDS in the MFMA's B-operand order ([column tile][row][16]: the 64 lanes of a
//                       k-step read 64 consecutive doubles), L(I, J) is the A operand straight from memory (lanes run down a
//                       column: four 128-byte segments per k-step) and K* is evaluated in registers.  The sum over J is split
//                       over the waves of a column tile (J = q, q + SPLIT, ...: a fixed order, so a window's result depends
//                       neither on its slot nor on its neighbours); the partial tiles meet in LDS, wave `ct` of tile ct adds
//                       them, applies the diagonal block's inverse with four more MFMAs -- register r of an MFMA result holds
//                       rows lq + 4 r, which is the B operand of a k-step whose A operand is columns lq + 4 r of the inverse,
//                       so the product chains in registers -- and writes V(I).  sum v z and sum v^2 are accumulated as rows are
//                       finished.  The next step's L blocks (and this step's inverse) are requested BEFORE the barrier that
//                       ends a step: they do not depend on V, so the serial part of a step hides their latency.
// Forms (picked by the window length N alone, so that results do not depend on how many windows a context holds):
//   N <=  512   32 test points per workgroup: two column tiles x four-way split of J       V = 128 KB of LDS at N = 512
//   N <= 1024   16 test points:              one column tile  x eight-way split             V = 128 KB at N = 1024
//   N <= 2048    8 test points: as above with half of the tile's columns empty (the "still correct" form; V = 128 KB at N = 2048)
// Workgroups are numbered so that the chunks of a window run on the same XCD at the same time (blockIdx.x round-robins over
// the eight XCDs): a window's factor is then fetched from HBM once and served to its other chunks by that XCD's L2.
// Read-only on the windows: L, z, xw, yw and state are not written.
// The kernel has two more forms of the same block step: KEEP also stores V for the joint forecast (cgp_window_joint.hpp), GRAD
// goes on from V to the predictive gradients (cgp_window_pgrad.hpp: B = L^-T V in place, then the contraction with dk/dx*).
// The multi-target windows (cgp_window_multi.hpp) add two: WM_Z solves Z = L^-1 Y for the P target columns (the start tile comes
// from the target store instead of K*), WM_MEAN is the forecast whose P mean rows are contracted from V and Z after the loop.
#pragma once
#include "cgp_window.hpp"

namespace cgp {

constexpr int WF_THREADS = 512;
constexpr int WF_WAVES = WF_THREADS / 64;
constexpr int WF_PREF = 8;     // L blocks of a step a wave requests at once (N <= 512 / 1024: ALL of the step's blocks of the wave)
constexpr int WF_XCDS = 8;

struct ForecastArgs {
  const double *L, *z, *xw;   // the windows' state (WindowArgs)
  const int *state;
  const double *prep, *theta;
  const double *xs;           // [nwin][M][d] test points
  double *mean, *var;         // [nwin][M]
  double *dinv;               // [nwin][NB][16 * 16] inverses of the diagonal blocks, element (row m, column k) at k * 16 + m
  int N, CAP, d, kernel_id, M, include_noise;
  int nwin, nchunk, NB;       // NB = ceil(N / 16) block rows the buffers are sized for
  // KEEP form only (cgp_window_joint.hpp): V is also stored, [nwin][mt][NB * 16][16] (test-point tile, row, column of the tile)
  double *vkeep;
  int mt;                     // test-point tiles of 16 the store is sized for: ceil(M / 16)
  // GRAD form only (cgp_window_pgrad.hpp): mean / var may each be null there
  const double *alpha;        // [nwin][NB * 16] k_window_alpha's alpha = L^-T z
  double *gdmean, *gdvar;     // [nwin][M][d] d mean / d x*, d var / d x*; either may be null
  // multi-target forms only (cgp_window_multi.hpp); in the WM_Z form M = P and the "test points" are the target columns
  const double *ystore;       // [nwin][P][N] the targets of the last N ticks, tick t at index t mod N
  const int *ycount;          // [nwin] ticks stored so far, mod N
  double *zs;                 // [nwin][pt][NB * 16][16] Z = L^-1 Y in the B-operand order (target tile, row, column of the tile)
  double *mlogml;             // [nwin][P] or null (WM_Z)
  int P, pt;                  // targets, target tiles of 16: ceil(P / 16); WM_MEAN: mean is [nwin][P][M]
};
enum { WM_NONE = 0, WM_Z = 1, WM_MEAN = 2 };   // forms of k_window_forecast for the multi-target windows

// Inverse of every 16 x 16 diagonal block of the windows' factors (blocks counted from the window's origin).  Rows past the
// window are identity rows.  One 16-lane row per block, four blocks per workgroup.
__global__ __launch_bounds__(64) void k_window_diag_inv(ForecastArgs p) {
  __shared__ double blk[4][WPB * WPB];   // [c * 16 + r], strictly lower part and diagonal; zero above
  const int nbx = (p.NB + 3) / 4;
  const int w = blockIdx.x / nbx, lane = threadIdx.x, g = lane >> 4, j = lane & 15;
  const int b = (blockIdx.x - w * nbx) * 4 + g;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1];
  const double *L = p.L + (size_t)w * p.CAP * p.CAP;
  const int r0 = b * WPB;
  {   // lane j = row j of the block
    const bool in = r0 + j < n;
#pragma unroll
    for (int c = 0; c < WPB; ++c) {
      double v = (c == j) ? 1.0 : 0.0;
      if (in && c <= j) v = L[(size_t)(o + r0 + c) * p.CAP + o + r0 + j];
      blk[g][c * WPB + j] = v;
    }
  }
  __syncthreads();
  if (b >= p.NB) return;
  // lane j = column j of the inverse: B x = e_j
  double x[WPB];
#pragma unroll
  for (int i = 0; i < WPB; ++i) {
    double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; ++k) s = __builtin_fma(-blk[g][k * WPB + i], x[k], s);
    x[i] = s / blk[g][i * WPB + i];
  }
  double *out = p.dinv + ((size_t)w * p.NB + b) * (WPB * WPB) + j * WPB;
#pragma unroll
  for (int i = 0; i < WPB; ++i) out[i] = x[i];
}

// NCT column tiles per workgroup (the waves of a tile split the sum over J WF_WAVES / NCT ways); VW = columns of a tile in use
// KEEP: every finished V(I) block is also stored for the joint forecast (cgp_window_joint.hpp); the forms cgp_window_predict
// launches are the KEEP = false ones
// GRAD: the gradient form (cgp_window_pgrad.hpp, cgp_window_predict_gradients): the same solve, then the tail declared below
// goes on from the chunk's finished V in LDS; p.mean / p.var may each be null.  The forms cgp_window_predict and the joint
// forecast launch are the GRAD = false ones; the block step is written once for all of them.
template <int NCT, int VW, bool MAT>
__device__ __forceinline__ void window_grad_tail(const ForecastArgs &p, double *V, double *red, const double *L, const double *xw,
                                                 const double *dinv, const double *pr, const double (&xq)[MAXD], int w, int col,
                                                 bool colok, int n, int nb, double (&a)[WF_PREF][4]);
__device__ __forceinline__ void window_grad_prior(const ForecastArgs &p, size_t oi, bool bad, double x0, const double *pr);
// MULTI: the two multi-target forms (cgp_window_multi.hpp): the pieces below are theirs, the block step is the kernel's own.
// WM_Z has no test points: lane l15 of a tile is a target column, the start tile is read from the target store, every finished
// block goes to the Z scratch, and the tail writes logml[p].  WM_MEAN leaves the mean to its tail; var is the kernel's own.
template <int MULTI> __device__ __forceinline__ void window_multi_prior(const ForecastArgs &p, int w, int col, bool bad, double prior_var);
__device__ __forceinline__ double window_multi_target(const ForecastArgs &p, int w, int col, int n, int row);
__device__ __forceinline__ void window_multi_z_tail(const ForecastArgs &p, double *red, const double *L, int w, int col, bool writer,
                                                    int n, double sv2);
template <int NCT, int VW>
__device__ __forceinline__ void window_multi_mean_tail(const ForecastArgs &p, const double *V, double *red, int w, int ch, int n, int nb);

template <int NCT, int VW, bool KEEP = false, bool MAT = false, bool GRAD = false, int MULTI = WM_NONE>   // MAT: the windows hold a Matern kernel (an instantiation of its own)
__global__ __launch_bounds__(WF_THREADS, 1) void k_window_forecast(ForecastArgs p) {
  static_assert((NCT == 1 || NCT == 2) && (VW == 16 || VW == 8), "forms of the forecast kernel");
  constexpr int SPLIT = WF_WAVES / NCT, MC = NCT * VW;
  typedef double d4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int nrow = p.NB * WPB;
  double *V = reinterpret_cast<double *>(smem_raw);   // [NCT][nrow][VW]
  double *red = V + (size_t)NCT * nrow * VW;          // [WF_WAVES][4][64] the waves' partial tiles
  // workgroup -> (window, chunk): consecutive ids on ONE XCD
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nwin * p.nchunk) return;
  const int w = lid / p.nchunk, ch = lid - w * p.nchunk;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = wave % NCT, jq = wave / NCT;
  const int CAP = p.CAP, d = p.d, kid = p.kernel_id, M = p.M;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  const double *pr = p.prep + (size_t)w * PREP_N;
  const double *th = p.theta + (size_t)w * MAX_THETA;
  const int nth = k_ntheta(kid, d);
  const double noise = p.include_noise ? th[nth - 1] : 0.0;
  // this lane's test point (solver waves: column l15 of tile ct)
  const int col = ch * MC + ct * VW + l15;
  const bool colok = l15 < VW && col < M;
  double xq[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) xq[q] = (MULTI != WM_Z && colok && q < d) ? p.xs[((size_t)w * M + col) * d + q] : 0.0;
  const double kss = (kid == K_RBF_BROWNIAN) ? pr[9] * pr[10] * fabs(xq[0]) : pr[9];
  if (bad != 0 || n <= 0) {   // a failed window answers NaN, an empty one with the prior
    if (jq == 0 && lq == 0 && colok) {
      if constexpr (MULTI != WM_NONE) {
        window_multi_prior<MULTI>(p, w, col, bad != 0, kss + noise);
      } else {
        const size_t oi = (size_t)w * M + col;
        if (!GRAD || p.mean) p.mean[oi] = bad != 0 ? __builtin_nan("") : 0.0;
        if (!GRAD || p.var) p.var[oi] = bad != 0 ? __builtin_nan("") : kss + noise;
        if constexpr (GRAD) window_grad_prior(p, oi, bad != 0, xq[0], pr);
      }
    }
    return;
  }
  const double *L = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0)
  const double *z = p.z + (size_t)w * CAP + o;
  const double *xw = p.xw + (size_t)w * d * CAP + o;
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  double *Vt = V + (size_t)ct * nrow * VW;
  const int nb = (n + WPB - 1) / WPB;

  // L(I, J) as the MFMA's A operand: lane (l15, lq) holds rows I 16 + l15, columns J 16 + 4 ks + lq; rows past the window are zero
  auto load_blk = [&](int I, int J, double (&a)[4]) {
    const int row = I * WPB + l15;
    const double *src = L + (size_t)(J * WPB + lq) * CAP + row;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a[ks] = row < n ? src[(size_t)(4 * ks) * CAP] : 0.0;
  };
  // the wave's blocks of step I: J = jq + SPLIT s, s < cnt(I)
  auto count = [&](int I) { return I > jq ? (I - jq + SPLIT - 1) / SPLIT : 0; };
  auto load_group = [&](int I, int s0, double (&a)[WF_PREF][4]) {
    const int cnt = count(I);
#pragma unroll
    for (int s = 0; s < WF_PREF; ++s)
      if (s0 + s < cnt) load_blk(I, jq + SPLIT * (s0 + s), a[s]);
  };

  // K*(I, tile) is formed by the tile's LAST wave of the split (the one with the fewest blocks of a step), which starts its
  // partial sum from it; the rows' inputs are requested a step ahead like the L blocks, so no load sits on a step's path
  const bool kwave = jq == SPLIT - 1;
  double prr[MAXD], xr[4][MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) prr[q] = q < d ? pr[q] : 0.0;
  const double amp = pr[9], ampb = pr[10];
  auto load_x = [&](int I) {
    if constexpr (MULTI == WM_Z) {   // the start tile itself: rows lq + 4 r of target column `col`
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I * WPB + lq + 4 * r;
        xr[r][0] = (colok && row < n) ? window_multi_target(p, w, col, n, row) : 0.0;
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = I * WPB + lq + 4 * r;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) xr[r][q] = (q < d && row < n) ? xw[(size_t)q * CAP + row] : 0.0;
    }
  };
  auto cov = [&](const double (&xa)[MAXD]) {   // win_cov's formulas on registers
    if (kid != K_RBF_BROWNIAN) {
      double d2 = 0;
#pragma unroll
      for (int q = 0; q < MAXD; ++q)
        if (q < d) {
          const double df = (xa[q] - xq[q]) * prr[q];
          d2 += df * df;
        }
      if constexpr (MAT) {
        double unused;
        return amp * matern_radial_rt<false>(kid, d2, unused);
      }
      return amp * exp(-0.5 * d2);
    }
    const double x = xa[0], xp = xq[0];
    double r2 = -2.0 * x * xp + (x * x + xp * xp);
    r2 = r2 < 0.0 ? 0.0 : r2;
    const double rr = sqrt(r2) * prr[0];
    const int sx = (x > 0) - (x < 0), sp = (xp > 0) - (xp < 0);
    const double kb = (sx == sp) ? ampb * fmin(fabs(x), fabs(xp)) : 0.0;
    return amp * exp(-0.5 * rr * rr) * kb;
  };

  double a[WF_PREF][4];
  double svz = 0.0, sv2 = 0.0;
  if (kwave) load_x(0);
  for (int I = 0; I < nb; ++I) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    double di[4] = {0.0, 0.0, 0.0, 0.0};
    if (kwave) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MULTI == WM_Z) acc[r] = xr[r][0];
        else acc[r] = I * WPB + lq + 4 * r < n ? cov(xr[r]) : 0.0;
      }
    }
    if (jq == 0) {   // the tile's solver wave requests the diagonal block's inverse (used after the barrier)
#pragma unroll
      for (int r = 0; r < 4; ++r) di[r] = dinv[(size_t)I * (WPB * WPB) + (lq + 4 * r) * WPB + l15];
    }
    const int cnt = count(I);
    for (int s0 = 0; s0 < cnt; s0 += WF_PREF) {
      if (s0 > 0) load_group(I, s0, a);   // (windows of more than WF_PREF SPLIT block rows only)
#pragma unroll
      for (int s = 0; s < WF_PREF; ++s) {
        if (s0 + s < cnt) {
          const double *vb = Vt + (size_t)((jq + SPLIT * (s0 + s)) * WPB) * VW + lq * VW + l15;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = (VW == 16 || l15 < VW) ? vb[4 * ks * VW] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[s][ks], b, acc, 0, 0, 0);
          }
        }
      }
    }
    if (jq != 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    if (I + 1 < nb) {   // in flight across the serial part of this step
      load_group(I + 1, 0, a);
      if (kwave) load_x(I + 1);
    }
    __syncthreads();
    if (jq == 0) {
#pragma unroll
      for (int q = 1; q < SPLIT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += red[((ct + NCT * q) * 4 + r) * 64 + lane];
      d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[r], v, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I * WPB + lq + 4 * r;
        if (VW == 16 || l15 < VW) Vt[(size_t)row * VW + l15] = v[r];
        if constexpr (KEEP) {   // rows lq + 4 r of the four lane groups are consecutive: 512 contiguous bytes per store
          const int gc = ch * MC + ct * VW + l15;
          if ((VW == 16 || l15 < VW) && (gc >> 4) < p.mt)
            p.vkeep[(((size_t)w * p.mt + (gc >> 4)) * nrow + row) * WPB + (gc & 15)] = v[r];
        }
        if constexpr (MULTI == WM_Z) {   // the KEEP store's order, into the Z scratch
          const int gc = ch * MC + ct * VW + l15;
          if ((VW == 16 || l15 < VW) && (gc >> 4) < p.pt) p.zs[(((size_t)w * p.pt + (gc >> 4)) * nrow + row) * WPB + (gc & 15)] = v[r];
        }
        if constexpr (MULTI == WM_NONE) {
          const double zr = row < n ? z[row] : 0.0;
          svz = __builtin_fma(v[r], zr, svz);
        }
        sv2 = __builtin_fma(v[r], v[r], sv2);
      }
    }
    __syncthreads();
  }
  if (jq == 0) {
    svz += __shfl_xor(svz, 16);
    sv2 += __shfl_xor(sv2, 16);
    svz += __shfl_xor(svz, 32);
    sv2 += __shfl_xor(sv2, 32);
    if (lq == 0 && colok) {
      const size_t oi = (size_t)w * M + col;
      double pv = kss - sv2;
      pv = pv < 1e-15 ? 1e-15 : pv;
      if (MULTI == WM_NONE && (!GRAD || p.mean)) p.mean[oi] = svz;
      if (MULTI != WM_Z && (!GRAD || p.var)) p.var[oi] = pv + noise;
    }
  }
  if constexpr (GRAD) window_grad_tail<NCT, VW, MAT>(p, V, red, L, xw, dinv, pr, xq, w, col, colok, n, nb, a);
  if constexpr (MULTI == WM_Z) window_multi_z_tail(p, red, L, w, col, jq == 0 && lq == 0 && colok, n, sv2);
  if constexpr (MULTI == WM_MEAN) window_multi_mean_tail<NCT, VW>(p, V, red, w, ch, n, nb);
}

}  // namespace cgp
