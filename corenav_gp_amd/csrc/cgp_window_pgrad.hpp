// cgp_window_pgrad.hpp -- predictive gradients from the sliding windows' resident state (cgp_window_predict_gradients):
// d mean / d x* and d var / d x* of every window at M test points of its own, the window form of cgp_pgrad.hpp.
//
//   alpha = L^-T z          B = L^-T V,  V = L^-1 K(X, xs)   (n x M)
//   dmean[m][q] =                sum_i dk(x*_m, x_i)/dx*_q alpha_i
//   dvar [m][q] = dk**/dx*_q - 2 sum_i dk(x*_m, x_i)/dx*_q B[i][m]
//
// Three launches: k_window_diag_inv and k_window_alpha as cgp_window_nll_grad runs them (alpha into AdaptArgs::alpha; its value
// is a by-product), then the GRAD = true instantiation of k_window_forecast (cgp_window_forecast.hpp): the same workgroup = one
// window x one chunk of test points, the same forms by N alone, the same XCD numbering -- and the same forward pass, the kernel's
// own, so mean / var are cgp_window_predict's bit for bit.  The tail below (declared in cgp_window_forecast.hpp, called at the
// end of the GRAD form) goes on from the chunk's finished V in LDS:
//   backward   I = nb - 1 .. 0:  B(I) = L(I, I)^-T (V(I) - sum_{J > I} L(J, I)^T B(J)), in place, on v_mfma_f64_16x16x4_f64.
//              The sum over J is split over the waves of a column tile as the forward pass splits it, counted from the last
//              block (J = nb - 1 - jq - SPLIT s: a fixed order); the partial tiles meet in `red`; the tile's solver wave adds
//              them to V(I), applies the diagonal block's inverse READ THE OTHER WAY ROUND (element (row m, column k) of the
//              inverse at k 16 + m is the transpose's (k, m)) and writes B(I).
//              The A operand is L(J, I)^T.  In the column-major slab the inner index -- the row inside block J -- is the
//              contiguous direction, so lane (l15, lq) takes rows 4 lq .. 4 lq + 3 of column I 16 + l15 as ONE 32-byte item and
//              k-step ks uses its element ks.  The B operand has to present row 4 lq + ks to lane group lq at k-step ks; a
//              finished B(I) is therefore stored with the rows of the block transposed as a 4 x 4 grid (row 4 a + b in slot
//              a + 4 b), which makes the operand read the forward pass's own conflict-free one (slot lq + 4 ks: 64 lanes, 512
//              consecutive bytes).  V(I), still in natural order, is read by the solver wave alone before it is replaced.
//              Rows >= n are zero in every operand; the next step's L blocks are requested before the step's barrier.
//   contract   after the loop, all 512 threads: wave (ct, jq) takes the blocks jq, jq + SPLIT, ... of column tile ct, lane
//              (l15, lq) test point l15 and the rows 4 lq .. 4 lq + 3 of a block.  Per (test point, sample) one evaluation of
//              g = -2 dk/dr^2 (k_pgrad_contract's formulas: k itself for the squared exponentials, matern_radial's g for the
//              Matern pair, the id-2 case with its tie convention), then 2 d multiply-adds on the scaled differences against
//              alpha_i and B[i][j]; 1 / ell_q leaves the loop.  The lane groups meet by two shuffles, the waves of a tile in
//              `red` in wave order: no LDS beyond the forecast's, no atomics, every sum in a fixed order.
// A failed window gets NaN in every output that was passed, an empty one the prior (dmean 0, dvar = dk**/dx*).  Read-only on
// the windows: L, z, xw, yw and state are not written, the slabs' strict upper triangle is neither read nor written.
#pragma once
#include "cgp_window_forecast.hpp"

namespace cgp {

// d k(x*, x*) / d x*: sigma_r^2 sigma_b^2 sign(x*) for RBF x Brownian (sign(0) = 0), zero for the stationary kernels
__device__ __forceinline__ double window_grad_dkss(int kid, const double *pr, double x0) {
  return kid == K_RBF_BROWNIAN ? pr[9] * pr[10] * (double)((x0 > 0) - (x0 < 0)) : 0.0;
}

// rows of a failed (NaN) or empty (prior) window; oi = w M + column
__device__ __forceinline__ void window_grad_prior(const ForecastArgs &p, size_t oi, bool bad, double x0, const double *pr) {
  const double nan = __builtin_nan("");
  const double dk = window_grad_dkss(p.kernel_id, pr, x0);   // (id 2 has d = 1)
  for (int q = 0; q < p.d; ++q) {
    if (p.gdmean) p.gdmean[oi * p.d + q] = bad ? nan : 0.0;
    if (p.gdvar) p.gdvar[oi * p.d + q] = bad ? nan : (q == 0 ? dk : 0.0);
  }
}

template <int NCT, int VW, bool MAT>
__device__ __forceinline__ void window_grad_tail(const ForecastArgs &p, double *V, double *red, const double *L, const double *xw,
                                                 const double *dinv, const double *pr, const double (&xq)[MAXD], int w, int col,
                                                 bool colok, int n, int nb, double (&a)[WF_PREF][4]) {
  constexpr int SPLIT = WF_WAVES / NCT;
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = wave % NCT, jq = wave / NCT;
  const int CAP = p.CAP, d = p.d, kid = p.kernel_id;
  const int nrow = p.NB * WPB;
  double *Vt = V + (size_t)ct * nrow * VW;
  const bool vok = VW == 16 || l15 < VW;

  // ---- backward substitution, in place ----
  // L(J, I)^T as the A operand: lane (l15, lq) holds column I 16 + l15, rows J 16 + 4 lq + ks (one 32-byte item)
  auto load_blk_t = [&](int I, int J, double (&b)[4]) {
    const int c = I * WPB + l15, r0 = J * WPB + 4 * lq;
    const double *src = L + (size_t)c * CAP + r0;
    if (c < n && r0 + 3 < n) {
      d4 v;
      __builtin_memcpy(&v, src, sizeof(v));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) b[ks] = v[ks];
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) b[ks] = (c < n && r0 + ks < n) ? src[ks] : 0.0;
    }
  };
  // the wave's blocks of step I: J = nb - 1 - jq - SPLIT s, s < count(I)
  auto count = [&](int I) { return nb - 1 - I > jq ? (nb - 1 - I - jq + SPLIT - 1) / SPLIT : 0; };
  auto load_group = [&](int I, int s0, double (&g)[WF_PREF][4]) {
    const int cnt = count(I);
#pragma unroll
    for (int s = 0; s < WF_PREF; ++s)
      if (s0 + s < cnt) load_blk_t(I, nb - 1 - jq - SPLIT * (s0 + s), g[s]);
  };
  for (int I = nb - 1; I >= 0; --I) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    double di[4] = {0.0, 0.0, 0.0, 0.0};
    if (jq == 0) {   // the tile's solver wave starts from V(I) (natural row order) and requests the inverse, transposed
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r] = vok ? Vt[(size_t)(I * WPB + lq + 4 * r) * VW + l15] : 0.0;
        di[r] = dinv[(size_t)I * (WPB * WPB) + l15 * WPB + lq + 4 * r];
      }
    }
    const int cnt = count(I);
    for (int s0 = 0; s0 < cnt; s0 += WF_PREF) {
      if (s0 > 0) load_group(I, s0, a);   // (windows of more than WF_PREF SPLIT block rows only)
#pragma unroll
      for (int s = 0; s < WF_PREF; ++s) {
        if (s0 + s < cnt) {
          const double *vb = Vt + (size_t)((nb - 1 - jq - SPLIT * (s0 + s)) * WPB) * VW + lq * VW + l15;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = vok ? vb[4 * ks * VW] : 0.0;   // slot lq + 4 ks = row 4 lq + ks
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[s][ks], b, acc, 0, 0, 0);
          }
        }
      }
    }
    if (jq != 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    if (I > 0) load_group(I - 1, 0, a);   // in flight across the serial part of this step
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
      for (int r = 0; r < 4; ++r)   // row lq + 4 r goes to slot r + 4 lq
        if (vok) Vt[(size_t)(I * WPB + r + 4 * lq) * VW + l15] = v[r];
    }
    __syncthreads();
  }

  // ---- contraction with dk/dx* ----
  double sm[MAXD], sv[MAXD], prr[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    sm[q] = sv[q] = 0.0;
    prr[q] = q < d ? pr[q] : 0.0;
  }
  const double amp = pr[9], ampb = pr[10];
  const double x0 = xq[0], ax0 = fabs(x0);
  const int sg0 = (x0 > 0) - (x0 < 0);
#ifndef CGP_WPG_NO_CONTRACT   // (a measurement build times the kernel without this loop; the shipped library never defines it)
  const double *al = p.alpha + (size_t)w * nrow;
  for (int blk = jq; blk < nb; blk += SPLIT) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int i = blk * WPB + 4 * lq + ks;
      const bool in = i < n;
      const double bm = (in && vok) ? Vt[(size_t)(blk * WPB + lq + 4 * ks) * VW + l15] : 0.0;
      const double ai = in ? al[i] : 0.0;
      if (kid == K_RBF_BROWNIAN) {
        const double xi = in ? xw[i] : 0.0, axi = fabs(xi);
        const int sgi = (xi > 0) - (xi < 0);
        const double df = (xi - x0) * prr[0];
        const double R = amp * exp(-0.5 * df * df);
        const bool same = sg0 == sgi;
        const double W = same ? ampb * fmin(ax0, axi) : 0.0;
        const double br = (same && ax0 < axi) ? ampb * (double)sg0 : 0.0;
        const double c = __builtin_fma(R * W, df * prr[0], R * br);
        sm[0] = __builtin_fma(c, ai, sm[0]);
        sv[0] = __builtin_fma(c, bm, sv[0]);
      } else {
        double df[MAXD], r2 = 0.0;
#pragma unroll
        for (int q = 0; q < MAXD; ++q) {
          if (q < d) {
            df[q] = ((in ? xw[(size_t)q * CAP + i] : 0.0) - xq[q]) * prr[q];
            r2 = __builtin_fma(df[q], df[q], r2);
          }
        }
        double g;
        if constexpr (MAT) (void)matern_radial_rt<true>(kid, r2, g);
        else g = exp(-0.5 * r2);
        g *= amp;
        const double ga = g * ai, gb = g * bm;
#pragma unroll
        for (int q = 0; q < MAXD; ++q) {
          if (q < d) {
            sm[q] = __builtin_fma(df[q], ga, sm[q]);
            sv[q] = __builtin_fma(df[q], gb, sv[q]);
          }
        }
      }
    }
  }
#endif
  // the four lane groups of a test point, then the waves of its tile in wave order (`red` is free: the loop's last barrier)
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    if (q < d) {
      sm[q] += __shfl_xor(sm[q], 16);
      sv[q] += __shfl_xor(sv[q], 16);
      sm[q] += __shfl_xor(sm[q], 32);
      sv[q] += __shfl_xor(sv[q], 32);
    }
  }
  if (jq != 0 && lq == 0) {
#pragma unroll
    for (int q = 0; q < MAXD; ++q) {
      if (q < d) {
        red[wave * 256 + q * WPB + l15] = sm[q];
        red[wave * 256 + (MAXD + q) * WPB + l15] = sv[q];
      }
    }
  }
  __syncthreads();
  if (jq == 0 && lq == 0 && colok) {
    const double dk = window_grad_dkss(kid, pr, x0);
    const size_t oi = ((size_t)w * p.M + col) * d;
#pragma unroll
    for (int q = 0; q < MAXD; ++q) {
      if (q < d) {
        double tm = sm[q], tv = sv[q];
#pragma unroll
        for (int s = 1; s < SPLIT; ++s) {
          tm += red[(ct + NCT * s) * 256 + q * WPB + l15];
          tv += red[(ct + NCT * s) * 256 + (MAXD + q) * WPB + l15];
        }
        const double sc = kid == K_RBF_BROWNIAN ? 1.0 : prr[q];
        if (p.gdmean) p.gdmean[oi + q] = tm * sc;
        if (p.gdvar) p.gdvar[oi + q] = dk - 2.0 * (tv * sc);
      }
    }
  }
}

}  // namespace cgp
