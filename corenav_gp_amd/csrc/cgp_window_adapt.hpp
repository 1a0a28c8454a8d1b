// cgp_window_adapt.hpp -- hyper-parameters of the resident sliding windows re-estimated and replaced in place
// (cgp_window_set_theta, cgp_window_nll_grad, cgp_window_optimize).
//
// The push kernels (cgp_window.hpp) keep a window's samples, the factor L of Ky = K + (sigma_n^2 + 1e-8) I and z = L^-1 y on
// the device under a theta that cgp_window_init fixed.  The reference re-estimates theta on every window
// (gp_slip_node.py:36, m.optimize()); the kernels here do the same for a window that is maintained instead of refitted:
//
//   k_window_refactor     new theta -> prep record, Ky from the resident inputs (win_cov's formulas), its Cholesky factor at the
//                         window's current origin, z = L^-1 y, logML, and the failure word state[2] from the result.
//                         One workgroup of eight waves per window, left-looking over 16-column block columns on
//                         v_mfma_f64_16x16x4_f64:  tile (I, J) = Ky(I, J) - sum_{k < J} L(I, k) L(J, k)^T  is formed TRANSPOSED
//                         (A operand = L(J, k), B operand = L(I, k)^T, both read down the slab's columns: 128-byte segments),
//                         with the Gram tile evaluated in registers as the accumulator's start value.  In that orientation
//                         register r of the result holds rows lq + 4 r of the transposed tile, which is the B operand of the
//                         k-step whose A operand is columns lq + 4 r of L(J, J)^-1, so L(I, J)^T = L(J, J)^-1 tile^T chains in
//                         registers (four more MFMAs) and the store runs down the slab's columns again.  Wave 0 factors the
//                         16 x 16 diagonal block in registers (factor_block16_repair: DPP row broadcasts) and hands its inverse
//                         to the others through LDS; y rides along as one more row (wave 7, the one with the fewest tiles);
//                         the log-determinant is a mantissa / exponent product of the pivots as in the pushes.
//                         Wave v owns tiles I = J + v, J + v + 8, ...: TPW accumulators per wave, TPW = 4 / 8 / 16 for
//                         N <= 512 / 1024 / 2048 (a function of N alone; the two long forms are correct, not tuned).
//   k_window_alpha        alpha = L^-T z (blocked back-substitution with the diagonal blocks' inverses of k_window_diag_inv)
//                         and the value 0.5 z'z + sum log L_ii + 0.5 n log 2 pi.  One workgroup per window, n^2 / 2 loads.
//   k_window_kinv_grad    Ky^-1 contracted with dK/dtheta without a materialised inverse.  One WAVE = one window x one chunk of
//                         16 columns [c0, c0 + 16): forward substitution V = L^-1 E (rows above the chunk are zero: it starts
//                         at the chunk's block), back-substitution L^T U = V stopped at the chunk's first row, and as every
//                         16 x 16 tile of U = Ky^-1 is finished, w = alpha_i alpha_j - U_ij is contracted with K_ij and
//                         K_ij d_q^2 in registers (off-diagonal tiles count twice): k_grad's sums.  The chunk's V / U lives,
//                         transposed, in the chunk's own tile row of the slab's strict upper triangle (nothing reads that
//                         triangle; the lower triangle, the diagonal, z, the samples and the state words are NOT written), the
//                         diagonal tile stays in registers.  Forward: L(I, K) is the A operand down the slab's columns, V(K) the
//                         B operand.  Backward: L(K, I)^T is the A operand read across the columns (32-byte segments, L2).
//   k_window_grad_finish  per window: the chunks' partial sums added in chunk order (no atomics) -> gradient with respect to
//                         the natural parameters (cgp_nll_grad's formulas); NaN for a failed window, zeros for an empty one.
// Every kernel reads origin and size from the window's state words: no host mirror, nothing depends on the slot.
#pragma once
#include "cgp_window_forecast.hpp"

namespace cgp {

constexpr int WA_THREADS = 512;
constexpr int WA_WAVES = WA_THREADS / 64;
constexpr double WA_LOG_2PI = 1.8378770664093453;

struct AdaptArgs {
  double *L, *z;              // the windows' state (WindowArgs); k_window_kinv_grad writes the strict upper triangle only
  const double *xw, *yw;
  int *state;
  double *prep, *theta;       // written by k_window_refactor, read by the others
  // k_window_refactor
  const double *new_theta;    // [nwin][theta_stride]
  int theta_stride;
  const unsigned char *select;   // [nwin] or nullptr = every window
  double *logml;              // [nwin] or nullptr
  int *info;                  // [nwin] or nullptr: 1-based index of the first non-positive pivot, 0 = none
  // value and gradient
  const double *dinv;         // [nwin][NB][256] k_window_diag_inv's inverses
  double *alpha;              // [nwin][NB * 16]
  double *gpart;              // [nwin][NB][GRAD_N]
  double *nllv;               // [nwin] k_window_alpha's value
  double *nll, *grad;         // outputs: [nwin], [nwin][grad_stride]
  int grad_stride;
  int N, CAP, d, kernel_id, nwin, NB;
  // multi-target objective (cgp_window_multi_grad.hpp)
  const double *zs;           // [nwin][pt][NB * 16][16] k_window_multi_z's Z = L^-1 Y
  double *am;                 // [nwin][pt][NB * 16][16] A = L^-T Z, the same tile order
  const double *mlogml;       // [nwin][P] k_window_multi_z's per-column values
  int P, pt;                  // targets, target tiles of 16
};

typedef double d4 __attribute__((ext_vector_type(4)));   // one lane's share of a 16 x 16 fp64 MFMA tile

// the covariance of two points held in registers: win_cov's formulas (as k_window_forecast evaluates K*)
struct WaCov {
  double pr[MAXD], amp, ampb;
  int kid, d;
  // from theta in natural parameters: the prep record's fields as cgp_window_init derives them on the host
  static __device__ __forceinline__ WaCov from_theta(int kid, int d, const double *th) {
    WaCov cv;
    cv.kid = kid;
    cv.d = d;
#pragma unroll
    for (int q = 0; q < MAXD; ++q) cv.pr[q] = q < d ? 1.0 / (k_is_ard(kid) ? th[1 + q] : th[1]) : 0.0;
    cv.amp = th[0];
    cv.ampb = kid == K_RBF_BROWNIAN ? th[2] : 0.0;
    return cv;
  }
  // from a window's prep record
  static __device__ __forceinline__ WaCov from_prep(int kid, int d, const double *pr) {
    WaCov cv;
    cv.kid = kid;
    cv.d = d;
#pragma unroll
    for (int q = 0; q < MAXD; ++q) cv.pr[q] = q < d ? pr[q] : 0.0;
    cv.amp = pr[9];
    cv.ampb = pr[10];
    return cv;
  }
  __device__ __forceinline__ double kss(double x0) const { return kid == K_RBF_BROWNIAN ? amp * ampb * fabs(x0) : amp; }
  // k(a, b) for a != b; dq2[q] = the squared length-scaled differences (Brownian: dq2[0] = r^2 / ell^2) for the gradient.
  // Matern: dq2 comes back times (-2 dk/dr^2) / k = 3 / (1 + s) resp. (5/3) (1 + s) / (1 + s + s^2 / 3) -- a quotient whose
  // denominator is >= 1 -- so that the caller's sums of w k dq2 are the length-scale sums of that kernel as they stand.
  template <bool WITH_DQ, bool MAT = true> __device__ __forceinline__ double eval(const double (&xa)[MAXD], const double (&xb)[MAXD], double (&dq2)[MAXD]) const {
    if (kid != K_RBF_BROWNIAN) {
      double d2 = 0;
#pragma unroll
      for (int q = 0; q < MAXD; ++q) {
        if (q < d) {
          const double df = (xa[q] - xb[q]) * pr[q];
          d2 += df * df;
          if (WITH_DQ) dq2[q] = df * df;
        } else if (WITH_DQ) {
          dq2[q] = 0.0;
        }
      }
      if (MAT && k_is_matern(kid)) {   // MAT = false: an instantiation that never sees a Matern window (k_window_refactor)
        double unused;
        const double k1 = matern_radial_rt<false>(kid, d2, unused);
        if (WITH_DQ) {
          const double s = sqrt((kid == K_MATERN52_ARD ? 5.0 : 3.0) * d2);
          const double ratio = kid == K_MATERN52_ARD ? (5.0 / 3.0) * (1.0 + s) / __builtin_fma(5.0 / 3.0, d2, 1.0 + s) : 3.0 / (1.0 + s);
#pragma unroll
          for (int q = 0; q < MAXD; ++q) dq2[q] *= ratio;
        }
        return amp * k1;
      }
      return amp * exp(-0.5 * d2);
    }
    const double x = xa[0], xp = xb[0];
    double r2 = -2.0 * x * xp + (x * x + xp * xp);
    r2 = r2 < 0.0 ? 0.0 : r2;
    const double rr = sqrt(r2) * pr[0];
    const int sx = (x > 0) - (x < 0), sp = (xp > 0) - (xp < 0);
    const double kb = (sx == sp) ? ampb * fmin(fabs(x), fabs(xp)) : 0.0;
    if (WITH_DQ) {
#pragma unroll
      for (int q = 0; q < MAXD; ++q) dq2[q] = 0.0;
      dq2[0] = rr * rr;
    }
    return amp * exp(-0.5 * rr * rr) * kb;
  }
};

__device__ __forceinline__ int wa_ntheta(int kid, int d) { return k_ntheta(kid, d); }

// ---------------------------------------------------------------------------------------------------------------------
template <int TPW, bool MAT = false>   // MAT: the windows hold a Matern kernel (an instantiation of its own)
__global__ __launch_bounds__(WA_THREADS) void k_window_refactor(AdaptArgs p) {
  __shared__ double tile[WPB * WPB];   // the diagonal tile, [c * 16 + r]
  __shared__ double winv[WPB * WPB];   // L(J, J)^-1, element (row m, column k) at k * 16 + m
  __shared__ double red[4];
  __shared__ int sbad;
  const int w = blockIdx.x;
  if (p.select && !p.select[w]) return;   // an unselected window is not touched
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int CAP = p.CAP, d = p.d, kid = p.kernel_id;
  const int nth = wa_ntheta(kid, d);
  int *st = p.state + w * 4;
  const int o = st[0], n = st[1];
  // the new theta and its derived record (what cgp_window_init computes on the host)
  const double *tn = p.new_theta + (size_t)w * p.theta_stride;
  // written out, not WaCov::from_theta: the factory compiles this kernel to another, slower listing (docs/negatives.md item 20)
  WaCov cv;
  cv.kid = kid;
  cv.d = d;
#pragma unroll
  for (int q = 0; q < MAXD; ++q) cv.pr[q] = q < d ? 1.0 / (k_is_ard(kid) ? tn[1 + q] : tn[1]) : 0.0;
  cv.amp = tn[0];
  cv.ampb = (kid == K_RBF_BROWNIAN) ? tn[2] : 0.0;
  const double noise = tn[nth - 1];
  if (tid < PREP_N) {
    double v = 0.0;
    if (tid < d) v = 1.0 / (k_is_ard(kid) ? tn[1 + tid] : tn[1]);
    if (tid == 9) v = tn[0];
    if (tid == 10) v = (kid == K_RBF_BROWNIAN) ? tn[2] : 0.0;
    p.prep[(size_t)w * PREP_N + tid] = v;
  }
  if (tid < MAX_THETA) p.theta[(size_t)w * MAX_THETA + tid] = tid < nth ? tn[tid] : 0.0;
  if (n <= 0) {   // an empty window: theta stored, logML 0, nothing failed
    if (tid == 0) {
      st[2] = 0;
      if (p.logml) p.logml[w] = 0.0;
      if (p.info) p.info[w] = 0;
    }
    return;
  }
  double *L = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;   // the window's (0, 0)
  double *z = p.z + (size_t)w * CAP + o;
  const double *xw = p.xw + (size_t)w * d * CAP + o;
  const double *yw = p.yw + (size_t)w * CAP + o;
  const int nb = (n + WPB - 1) / WPB;
  const bool zwave = wave == WA_WAVES - 1;
  int bad = 0;
  double pmant = 1.0, zz = 0.0;
  int pexp = 0;

  for (int J = 0; J < nb; ++J) {
    const int J0 = J * WPB;
    // ---- the wave's tiles of block column J, transposed: acc[t][r] = tile(c = lq + 4 r, row l15 of block I_t)
    d4 acc[TPW], zacc = {0.0, 0.0, 0.0, 0.0};
    {
      double xj[4][MAXD];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gj = J0 + lq + 4 * r;
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xj[r][q] = (q < d && gj < n) ? xw[(size_t)q * CAP + gj] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int I = J + wave + WA_WAVES * t;
        acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        if (I < nb) {
          const int gi = I * WPB + l15;
          double xi[MAXD];
#pragma unroll
          for (int q = 0; q < MAXD; ++q) xi[q] = (q < d && gi < n) ? xw[(size_t)q * CAP + gi] : 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gj = J0 + lq + 4 * r;
            double dq[MAXD], v;
            if (gi < n && gj < n) v = (gi == gj) ? cv.kss(xi[0]) + noise + 1e-8 : cv.template eval<false, MAT>(xj[r], xi, dq);
            else v = (gi == gj) ? 1.0 : 0.0;   // rows past the window: identity
            acc[t][r] = v;
          }
        }
      }
      if (zwave) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gj = J0 + lq + 4 * r;
          zacc[r] = (l15 == 0 && gj < n) ? yw[gj] : 0.0;
        }
      }
    }
    {
      const int rowJ = J0 + l15;
      for (int kb = 0; kb < J; ++kb) {
        const double *col = L + (size_t)(kb * WPB + lq) * CAP;
        double a[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = rowJ < n ? -col[(size_t)(4 * ks) * CAP + rowJ] : 0.0;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int I = J + wave + WA_WAVES * t;
          if (I < nb) {
            const int rowI = I * WPB + l15;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              const double b = rowI < n ? col[(size_t)(4 * ks) * CAP + rowI] : 0.0;
              acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, acc[t], 0, 0, 0);
            }
          }
        }
        if (zwave) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = l15 == 0 ? z[kb * WPB + 4 * ks + lq] : 0.0;
            zacc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, zacc, 0, 0, 0);
          }
        }
      }
    }
    // ---- wave 0: the diagonal block (its first tile) in registers, lane = row; the inverse goes to LDS
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
      const int row = J0 + l15;
      if (lane < WPB) {
#pragma unroll
        for (int m = 0; m < WPB; ++m) winv[l15 * WPB + m] = wv[m];
        double dg = 1.0;
#pragma unroll
        for (int c = 0; c < WPB; ++c) dg = (c == l15) ? a[c] : dg;
        if (row < n) {
#pragma unroll
          for (int c = 0; c < WPB; ++c)
            if (c <= l15) L[(size_t)(J0 + c) * CAP + row] = a[c];
          pmant *= dg;
          pexp += __builtin_amdgcn_frexp_exp(pmant);
          pmant = __builtin_amdgcn_frexp_mant(pmant);
        }
      }
    }
    __syncthreads();
    // ---- L(I, J)^T = L(J, J)^-1 tile^T for the tiles below the diagonal, and the z row
    {
      double di[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) di[r] = winv[(lq + 4 * r) * WPB + l15];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int I = J + wave + WA_WAVES * t;
        if (I < nb && I > J) {
          d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[t][r], v, 0, 0, 0);
          const int rowI = I * WPB + l15;
          if (rowI < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) L[(size_t)(J0 + lq + 4 * r) * CAP + rowI] = v[r];
          }
        }
      }
      if (zwave) {
        d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], zacc[r], v, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gj = J0 + lq + 4 * r;
          if (l15 == 0 && gj < n) {
            z[gj] = v[r];
            zz = __builtin_fma(v[r], v[r], zz);
          }
        }
      }
    }
    __syncthreads();   // block column J (and its rows of z) are in memory before block column J + 1 reads them
  }
  if (wave == 0) {
    double lg = log(pmant) + (double)pexp * 0.6931471805599453;   // lanes that never multiplied: log(1) + 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lg += __shfl_xor(lg, off);
    if (lane == 0) {
      red[0] = lg;
      sbad = bad;
    }
  }
  if (zwave) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) zz += __shfl_xor(zz, off);
    if (lane == 0) red[1] = zz;
  }
  __syncthreads();
  if (tid == 0) {
    const int b = sbad;
    st[2] = b;   // 0 revives a window an earlier push or set_theta failed; non-zero marks it failed for pushes and forecasts
    if (p.logml) p.logml[w] = b != 0 ? __builtin_nan("") : -0.5 * red[1] - red[0] - 0.5 * (double)n * WA_LOG_2PI;
    if (p.info) p.info[w] = b;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// alpha = L^-T z and the value.  Right-looking over the row blocks from the bottom: alpha(I) = L(I, I)^-T t(I), then
// t(rows above) -= L(I, rows above)^T alpha(I) -- row r of that update reads 16 consecutive doubles of the slab's column r.
__global__ __launch_bounds__(256) void k_window_alpha(AdaptArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double *t = reinterpret_cast<double *>(smem_raw);   // [NB * 16]
  __shared__ double red[2][4];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CAP = p.CAP;
  const int o = p.state[w * 4], n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  if (bad != 0 || n <= 0) {
    if (tid == 0) p.nllv[w] = bad != 0 ? __builtin_nan("") : 0.0;
    return;
  }
  const double *L = p.L + (size_t)w * CAP * CAP + (size_t)o * CAP + o;
  const double *z = p.z + (size_t)w * CAP + o;
  const double *dinv = p.dinv + (size_t)w * p.NB * (WPB * WPB);
  double *alpha = p.alpha + (size_t)w * p.NB * WPB;
  const int nb = (n + WPB - 1) / WPB;
  double szz = 0.0, slog = 0.0;
  for (int i = tid; i < nb * WPB; i += 256) {
    const double zi = i < n ? z[i] : 0.0;
    t[i] = zi;
    szz = __builtin_fma(zi, zi, szz);
    if (i < n) slog += log(L[(size_t)i * CAP + i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    szz += __shfl_xor(szz, off);
    slog += __shfl_xor(slog, off);
  }
  if (lane == 0) {
    red[0][wave] = szz;
    red[1][wave] = slog;
  }
  __syncthreads();
  if (tid == 0)
    p.nllv[w] = 0.5 * ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) + ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) +
                0.5 * (double)n * WA_LOG_2PI;
  for (int I = nb - 1; I >= 0; --I) {
    const int I0 = I * WPB;
    double ai = 0.0;
    if (tid < WPB) {   // alpha_i = sum_k (L(I, I)^-1)[k][i] t_k; element (row k, column i) of the inverse at i * 16 + k
      const double *dc = dinv + (size_t)I * (WPB * WPB) + tid * WPB;
#pragma unroll
      for (int k = 0; k < WPB; ++k) ai = __builtin_fma(dc[k], t[I0 + k], ai);
    }
    __syncthreads();
    if (tid < WPB) {
      t[I0 + tid] = ai;
      if (I0 + tid < n) alpha[I0 + tid] = ai;
    }
    __syncthreads();
    const int nk = min(WPB, n - I0);
    for (int r = tid; r < I0; r += 256) {
      const double *src = L + (size_t)r * CAP + I0;
      double s = t[r];
      for (int k = 0; k < nk; ++k) s = __builtin_fma(-src[k], t[I0 + k], s);
      t[r] = s;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward half of a wave's work unit (one window x the chunk of 16 columns of block J), shared by k_window_kinv_grad and
// k_window_loo (cgp_window_loo.hpp): V = L^-1 E for the chunk.  V(J) = L(J, J)^-1 stays in registers and is returned (register r =
// rows lq + 4 r, column l15); V(I) = L(I, I)^-1 (- sum_{J <= K < I} L(I, K) V(K)) for I > J goes, transposed, into the chunk's
// tile row of S's strict upper triangle.  L(I, K) is the A operand down the slab's columns, V(K) the B operand.
// SUMSQ: ss = this lane's share of column l15's sum of squares over the window's rows (identity rows past it are not counted).
template <bool SUMSQ>
__device__ __forceinline__ d4 chunk_forward_solve(double *S, const double *dinv, int CAP, int n, int nb, int J, int l15, int lq, double &ss) {
  const int J0 = J * WPB;
  const bool colok = J0 + l15 < n;
  double *Sc = S + J0 + l15;
  d4 VJ;
  if (SUMSQ) ss = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    VJ[r] = dinv[(size_t)J * (WPB * WPB) + l15 * WPB + lq + 4 * r];
    if (SUMSQ && J0 + lq + 4 * r < n && colok) ss = __builtin_fma(VJ[r], VJ[r], ss);
  }
  for (int I = J + 1; I < nb; ++I) {
    const int rowI = I * WPB + l15;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int K = J; K < I; ++K) {
      const int k0 = K * WPB + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double a = rowI < n ? -S[(size_t)(k0 + 4 * ks) * CAP + rowI] : 0.0;
        double b;
        if (K == J) b = VJ[ks];
        else b = colok ? Sc[(size_t)(k0 + 4 * ks) * CAP] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
    }
    d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double di = dinv[(size_t)I * (WPB * WPB) + (lq + 4 * r) * WPB + l15];
      v = __builtin_amdgcn_mfma_f64_16x16x4f64(di, acc[r], v, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = I * WPB + lq + 4 * r;
      if (row < n && colok) {
        Sc[(size_t)row * CAP] = v[r];
        if (SUMSQ) ss = __builtin_fma(v[r], v[r], ss);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // later steps of this wave read what other lanes stored
  }
  return VJ;
}

__global__ __launch_bounds__(256) void k_window_kinv_grad(AdaptArgs p) {
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
  const double *alpha = p.alpha + (size_t)w * p.NB * WPB;
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
  const double aj = colok ? alpha[gj] : 0.0;
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
    const double wgt = I == J ? 1.0 : 2.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = I0 + lq + 4 * r;
      if (gi < n && colok) {
        double xi[MAXD], dq2[MAXD];
#pragma unroll
        for (int q = 0; q < MAXD; ++q) xi[q] = q < d ? xw[(size_t)q * CAP + gi] : 0.0;
        const double wij = __builtin_fma(alpha[gi], aj, -u[r]);
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

// the chunks' sums in chunk order -> value and gradient (natural parameters, cgp_nll_grad's formulas)
__global__ __launch_bounds__(64) void k_window_grad_finish(AdaptArgs p) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= p.nwin) return;
  const int d = p.d, kid = p.kernel_id, nth = wa_ntheta(kid, d);
  const int n = p.state[w * 4 + 1], bad = p.state[w * 4 + 2];
  double *g = p.grad + (size_t)w * p.grad_stride;
  if (bad != 0 || n <= 0) {
    p.nll[w] = bad != 0 ? __builtin_nan("") : 0.0;
    for (int i = 0; i < nth; ++i) g[i] = bad != 0 ? __builtin_nan("") : 0.0;
    return;
  }
  const int nb = (n + WPB - 1) / WPB;
  double s[GRAD_N];
  for (int i = 0; i < GRAD_N; ++i) s[i] = 0.0;
  for (int J = 0; J < nb; ++J)
    for (int i = 0; i < GRAD_N; ++i) s[i] += p.gpart[((size_t)w * p.NB + J) * GRAD_N + i];
  p.nll[w] = p.nllv[w];
  grad_from_sums(kid, d, p.theta + (size_t)w * MAX_THETA, s, g);
}

}  // namespace cgp
