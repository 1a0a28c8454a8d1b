// cgp_pgrad.hpp -- predictive gradients after a batch of fits (or a single fit): d mean / d x* and d var / d x* at the M test
// points (cgp_fit_predict_grad_batch[_device], cgp_predict_gradients; GPy's m.predictive_gradients).
//
//   B = Ky^-1 K(X, Xs) = L^-T V  (N x M)      alpha = Ky^-1 y = L^-T z
//   dmean[m][q] =                sum_i dk(x*_m, x_i)/dx*_q alpha_i
//   dvar [m][q] = dk**/dx*_q - 2 sum_i dk(x*_m, x_i)/dx*_q B[i][m]
//
// After any tiled fit schedule the factor panel of fit b holds V^T and z^T as its M + 1 extra rows and Winv the images of
// W_k = L(k,k)^-1 (cgp_kernels.hpp).  Two launches follow:
//   k_pgrad_solve      the mirror image of k_multi_solve: B^T(t, k) = (V^T(t, k) - sum_{j>k} B^T(t, j) L(j, k)) W_k for
//                      k = NT - 1 .. 0 in ONE launch, one workgroup per (fit, tile t of 64 extra rows), on
//                      v_mfma_f64_16x16x4_f64.  The z row is solved with the rest, so row M of B^T is alpha and no k_alpha launch
//                      is needed.  V^T stays as it is (the joint calls and cgp_predict read it); B^T goes to a scratch of its own
//                      in the panel's layout, column-major over the samples: Bw[c ldb + row], ldb = M + 1 rounded up to 128,
//                      NT 128 columns.  A wave owns 16 rows and all 128 columns of the step (64 accumulator registers: two
//                      workgroups per CU, which measured faster than 32 rows per wave and one workgroup -- DESIGN 9f), the
//                      accumulators hold -S transposed (sample on the MFMA row, extra row on the lane, as every panel kernel
//                      has them), so the products of a step are D(c, row) += L(j, k)(i, c) B^T(row, j 128 + i):
//                        * L(j, k) is the A operand.  For a fixed output column c the inner index i runs along a column of the
//                          panel -- the contiguous direction -- so a PAIR of consecutive i is one 16-byte item and feeds two
//                          MFMAs; lane group lq of MFMA e (e = 0, 1) of a block of eight inner indices holds i = i0 + 2 lq + e.
//                          The B operand (the rows solved at the earlier steps, read back from the scratch straight to
//                          registers) uses the same order.  The four waves need the same L(j, k): it is staged
//                          through LDS in chunks of 16 inner indices x 128 columns (a thread fetches four items, eight lanes
//                          cover a column's 128 contiguous bytes), laid out [pair][column] so that an operand read is one
//                          conflict-free ds_read_b128, three buffers with ONE LDS-only barrier per chunk; both operands are
//                          requested two chunks (128 MFMAs of a wave) ahead.  Plain loads and stores: the compiler counts
//                          the waits.
//                        * the product with W_k (not W_k^T, as the forward solve has it) reads the negated block image the
//                          other way round: the A operand of output block cb and inner block qb >= cb is
//                          -W[qb 16 + lq + 4 r][cb 16 + l15] = Wimg[blk(qb, cb)][l15][lq + 4 r], straight from the image in L2;
//                          the output blocks are formed in ascending order, each from accumulator blocks not yet overwritten.
//                      A wave reads back what its own lanes stored one step earlier: release / acquire at agent scope around
//                      a barrier (multi_step_handoff).  A wave whose rows are all padding stages and keeps the barriers, and
//                      issues no MFMA.  Rows >= M + 1 and
//                      samples >= N are masked in every operand and stored as zeros / not stored: the panel's identity padding
//                      is not relied on.  A row's sums run in a fixed order that involves neither its tile nor its neighbours.
//   k_pgrad_contract   the two sums.  For a fixed sample the M rows of B^T are contiguous: a lane owns a test point, the sample's
//                      coordinates and alpha_i are wave-uniform reads.  Per (m, i): one evaluation of g = -2 dk/dr^2 (k itself for
//                      the squared exponentials, matern_radial's g for the Matern pair; exp_nonpos), then 2 d FMAs on the scaled
//                      differences; the factor 1 / ell_q leaves the loop.  The four waves take the samples i = wave, wave + 4, ...
//                      and their partial sums meet in LDS in wave order.  RBF x Brownian (d = 1):
//                        dk/dx* = R W (x_i - x*) / ell^2 + R sigma_b^2 sign(x*) [|x*| < |x_i| and equal signs],   dk**/dx* = sigma_r^2 sigma_b^2 sign(x*)
//                      with R = sigma_r^2 exp(-(x* - x_i)^2 / 2 ell^2), W = sigma_b^2 min(|x*|, |x_i|) for equal signs, else 0.
//                      CONVENTION: at a tie |x*| = |x_i| the bracket is 0 (min's derivative is taken from the side where x* is
//                      the larger), and sign(0) = 0.  Test points on the tick grid inside a window hit such ties.
// A fit whose info word is set gets NaN in all of its gradients.  The clip of the variance at 1e-15 and include_noise do not enter.
// No atomics; every sum runs in a fixed order that does not involve the slot, the batch or the neighbours.  fp64 only.
#pragma once
#include "cgp_multi.hpp"

namespace cgp {

struct PgradArgs {
  const double *Lw;      // slab of the call's first fit
  size_t lw_stride;
  int ld;
  const double *Winv;    // W images of the call's first fit
  size_t winv_stride;
  double *Bw;            // [nfit][NT 128][ldb] B^T (rows < M) and alpha (row M) of the call's first fit
  size_t b_stride;
  int ldb;               // M + 1 rounded up to 128
  const double *X;       // [nfit][d][N]
  const double *Xs;      // [nfit][d][M]
  const double *theta;   // [nfit][MAX_THETA]
  const int *info;       // [nfit] the fits' status words, or null (a single fit known to be good)
  double *dmean, *dvar;  // [nfit][M][d]; either may be null
  size_t row0;           // first extra row of the factor panel (NT 128)
  int N, d, M, NT, nfit;
  int stiles;            // k_pgrad_solve: tiles of PG_TR extra rows per fit
};

constexpr int PG_RB = 1;    // row blocks of 16 per wave
constexpr int PG_TR = 4 * PG_RB * DB;   // rows of a workgroup's tile: four waves
constexpr int PG_IB = 16;   // inner indices of L(j, k) staged per barrier: for one output column 128 contiguous bytes
constexpr int PG_PS = TS + 2;                         // LDS stride of a pair of inner indices, in 16-byte items: eight pairs x two
                                                      // columns of a quarter wave's store land in 64 different banks
constexpr int PG_SR = TS / (256 / (PG_IB / 2));       // staging rounds: 16-byte items per thread and chunk

__global__ __launch_bounds__(256, 2) void k_pgrad_solve(PgradArgs p) {
  using P = Prec<double>;
  using acc_t = P::acc_t;
  typedef double d2 __attribute__((ext_vector_type(2)));
  __shared__ d2 lsm[3][PG_IB / 2][PG_PS];   // three chunks of L(j, k): [pair of inner indices][output column]
  // workgroup -> (fit, row tile): consecutive ids on ONE XCD, so a fit's tiles share its L and W_k in one L2
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nfit * p.stiles) return;
  const int f = lid / p.stiles, t = lid - f * p.stiles;
  if (p.info != nullptr && p.info[f] != 0) return;   // (the whole workgroup) a failed fit: the contraction writes NaN
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, NT = p.NT, P1 = p.M + 1;
  const size_t ld = p.ld, ldb = p.ldb;
  const double *Lf = p.Lw + (size_t)f * p.lw_stride;
  const double *Vf = Lf + p.row0;
  const double *Wf = p.Winv + (size_t)f * p.winv_stride;
  double *Bf = p.Bw + (size_t)f * p.b_stride;
  const int wrow0 = t * PG_TR + wave * (PG_RB * DB);
  bool live[PG_RB], rok[PG_RB];   // live: wave-uniform, the block has a row < M + 1; rok: this lane's row is one
  int row[PG_RB];
#pragma unroll
  for (int rb = 0; rb < PG_RB; ++rb) {
    row[rb] = wrow0 + rb * DB + l15;
    live[rb] = wrow0 + rb * DB < P1;
    rok[rb] = row[rb] < P1;
  }
  acc_t acc[PG_RB][NCB];
  const int sp = tid & (PG_IB / 2 - 1), sc = tid / (PG_IB / 2);   // staging: this thread's pair of inner indices and first column
  for (int k = NT - 1; k >= 0; --k) {
    if (live[0]) {
      // -V^T(rows, k): D layout, sample k 128 + cb 16 + lq + 4 r on the MFMA row, the extra row on the lane
#pragma unroll
      for (int rb = 0; rb < PG_RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = k * TS + cb * DB + P::drow(lane, r);
            double v = 0.0;
            if (live[rb]) v = Vf[(size_t)c * ld + row[rb]];   // (inside the slab: the extra tiles are whole)
            acc[rb][cb][r] = (rok[rb] && c < N) ? -v : 0.0;
          }
    }
    // + sum_{j > k} L(j, k)^T B^T(rows, j)^T, j = NT - 1 .. k + 1, in chunks of 16 inner indices staged through LDS for the four
    // waves (a dead wave stages its share and keeps the barriers), two blocks of eight inner indices per chunk
    const double *Lg = Lf + (size_t)(k * TS + sc) * ld + 2 * sp;   // + 32 r ld + inner index
    const double *Bb = Bf + (size_t)(2 * lq) * ldb;                 // + inner index * ldb + row
    const int nchunk = (NT - 1 - k) * (TS / PG_IB);
    auto fetch = [&](int ch, d2 (&g)[PG_SR]) {
      const int i = (NT - 1 - ch / (TS / PG_IB)) * TS + (ch % (TS / PG_IB)) * PG_IB;   // first inner index of the chunk (a sample)
      const bool in0 = i + 2 * sp < N, in1 = i + 2 * sp + 1 < N;                          // samples >= N: not summed
#pragma unroll
      for (int r = 0; r < PG_SR; ++r) {
        const d2 v = *reinterpret_cast<const d2 *>(Lg + (size_t)(r * (256 / (PG_IB / 2))) * ld + i);
        g[r] = d2{in0 ? v.x : 0.0, in1 ? v.y : 0.0};
      }
    };
    auto stash = [&](int buf, const d2 (&g)[PG_SR]) {
#pragma unroll
      for (int r = 0; r < PG_SR; ++r) lsm[buf][sp][sc + r * (256 / (PG_IB / 2))] = g[r];
    };
    auto loadb = [&](int s, double (&b)[PG_RB][2]) {   // block s of eight inner indices
      const int i = (NT - 1 - s / (TS / 8)) * TS + (s % (TS / 8)) * 8;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int rb = 0; rb < PG_RB; ++rb) b[rb][e] = live[rb] ? Bb[(size_t)(i + e) * ldb + row[rb]] : 0.0;
    };
    auto mac = [&](int buf, int q, const double (&b)[PG_RB][2]) {
      d2 a[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) a[cb] = lsm[buf][4 * q + lq][cb * DB + l15];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        double fb[PG_RB];
#pragma unroll
        for (int rb = 0; rb < PG_RB; ++rb) fb[rb] = rok[rb] ? b[rb][e] : 0.0;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int rb = 0; rb < PG_RB; ++rb)
            if (live[rb]) acc[rb][cb] = P::mfma(a[cb][e], fb[rb], acc[rb][cb]);
      }
    };
    // Both operands are requested TWO chunks ahead (a chunk is 64 MFMAs of a wave, about 1.7 us: one chunk did not cover the
    // latency of a miss to HBM with one wave per SIMD).  L: chunk ch + 2 is fetched to registers in iteration ch and written to
    // LDS buffer (ch + 2) % 3 at the top of iteration ch + 1 -- the buffer chunk ch - 1 was read from, free since every wave
    // passed the barrier of iteration ch.  B^T: four register slots, chunk ch in slot ch & 3 (nchunk is a multiple of 8).
    d2 g[PG_SR];
    double bq[4][2][PG_RB][2];
    auto loadb_chunk = [&](int ch, double (&b)[2][PG_RB][2]) {
      loadb(2 * ch, b[0]);
      loadb(2 * ch + 1, b[1]);
    };
    auto body = [&](int ch, auto slot) {
      constexpr int S = decltype(slot)::value;
      if (ch + 1 < nchunk) stash((ch + 1) % 3, g);
      if (ch + 2 < nchunk) fetch(ch + 2, g);
      lds_barrier();   // chunk ch (and ch + 1) is staged; every wave is done with chunk ch - 1
      if (live[0]) {
        if (ch + 2 < nchunk) loadb_chunk(ch + 2, bq[(S + 2) & 3]);
        mac(ch % 3, 0, bq[S][0]);
        mac(ch % 3, 1, bq[S][1]);
      }
    };
    if (nchunk > 0) {   // (then nchunk >= 8)
      fetch(0, g);
      stash(0, g);
      fetch(1, g);
      if (live[0]) {
        loadb_chunk(0, bq[0]);
        loadb_chunk(1, bq[1]);
      }
    }
    for (int ch = 0; ch < nchunk; ch += 4) {
      body(ch, std::integral_constant<int, 0>{});
      body(ch + 1, std::integral_constant<int, 1>{});
      body(ch + 2, std::integral_constant<int, 2>{});
      body(ch + 3, std::integral_constant<int, 3>{});
    }
    if (live[0]) {
      // B^T(rows, k) = S W_k: output block cb from the accumulator blocks qb >= cb, in ascending cb
      const double *Wk = Wf + (size_t)k * WIMG + l15 * DB + lq;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        acc_t t0[PG_RB];
#pragma unroll
        for (int rb = 0; rb < PG_RB; ++rb) t0[rb] = acc_t{0, 0, 0, 0};
#pragma unroll
        for (int qb = cb; qb < NCB; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double w = Wk[wimg_blk(qb, cb) + 4 * r];   // -W[qb 16 + lq + 4 r][cb 16 + l15]
            w = (k * TS + qb * DB + lq + 4 * r < N) ? w : 0.0;
#pragma unroll
            for (int rb = 0; rb < PG_RB; ++rb)
              if (live[rb]) t0[rb] = P::mfma(w, acc[rb][qb][r], t0[rb]);
          }
#pragma unroll
        for (int rb = 0; rb < PG_RB; ++rb) acc[rb][cb] = t0[rb];
      }
#pragma unroll
      for (int rb = 0; rb < PG_RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = k * TS + cb * DB + P::drow(lane, r);
            if (rok[rb]) Bf[(size_t)c * ldb + row[rb]] = c < N ? acc[rb][cb][r] : 0.0;
          }
    }
    if (k > 0) multi_step_handoff();
  }
}

// kernel case of the contraction, selected at the launch site
enum { PGK_SE = 0, PGK_M32 = 1, PGK_M52 = 2, PGK_BROWN = 3 };

template <int KC>
__global__ __launch_bounds__(256) void k_pgrad_contract(PgradArgs p, int kid) {
  __shared__ double red[3][2 * MAXD][64];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, M = p.M, d = p.d;
  const int m = blockIdx.x * 64 + lane;
  const bool bad = p.info != nullptr && p.info[f] != 0;
  const double *th = p.theta + (size_t)f * MAX_THETA;
  const double amp = th[0], ampb = KC == PGK_BROWN ? th[2] : 0.0;
  double invl[MAXD], xs[MAXD], sm[MAXD], sv[MAXD];
#pragma unroll
  for (int q = 0; q < MAXD; ++q) {
    invl[q] = q < d ? 1.0 / (k_is_ard(kid) ? th[1 + q] : th[1]) : 0.0;
    xs[q] = (q < d && m < M) ? p.Xs[((size_t)f * d + q) * M + m] : 0.0;
    sm[q] = sv[q] = 0.0;
  }
  const double *Bf = p.Bw + (size_t)f * p.b_stride;
  const double *Xf = p.X + (size_t)f * d * N;
  const size_t ldb = p.ldb;
  ExpC ec;
  ec.load();
  auto ex = [&](double x) { return exp_nonpos(x, ec); };
  const double x0 = xs[0], ax0 = fabs(x0);
  const int sg0 = (x0 > 0) - (x0 < 0);
  if (!bad) {
    for (int i = wave; i < N; i += 4) {
      const double al = Bf[(size_t)i * ldb + M];
      const double bm = m < M ? Bf[(size_t)i * ldb + m] : 0.0;
      if constexpr (KC == PGK_BROWN) {
        const double xi = Xf[i], axi = fabs(xi);
        const int sgi = (xi > 0) - (xi < 0);
        const double df = (xi - x0) * invl[0];
        const double R = amp * ex(-0.5 * df * df);
        const bool same = sg0 == sgi;
        const double W = same ? ampb * fmin(ax0, axi) : 0.0;
        const double br = (same && ax0 < axi) ? ampb * (double)sg0 : 0.0;
        const double c = __builtin_fma(R * W, df * invl[0], R * br);
        sm[0] = __builtin_fma(c, al, sm[0]);
        sv[0] = __builtin_fma(c, bm, sv[0]);
      } else {
        double df[MAXD], r2 = 0.0;
#pragma unroll
        for (int q = 0; q < MAXD; ++q) {
          if (q < d) {
            df[q] = (Xf[(size_t)q * N + i] - xs[q]) * invl[q];
            r2 = __builtin_fma(df[q], df[q], r2);
          }
        }
        double g;
        if constexpr (KC == PGK_SE) g = ex(-0.5 * r2);
        else (void)matern_radial<KC == PGK_M52, true>(r2, g, ex);
        g *= amp;
        const double ga = g * al, gb = g * bm;
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
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < MAXD; ++q) {
      red[wave - 1][q][lane] = sm[q];
      red[wave - 1][MAXD + q][lane] = sv[q];
    }
  }
  __syncthreads();
  if (wave == 0 && m < M) {
    const double nan = __builtin_nan("");
    const double dkss = KC == PGK_BROWN ? amp * ampb * (double)sg0 : 0.0;
#pragma unroll
    for (int q = 0; q < MAXD; ++q) {
      if (q < d) {
        const double tm = ((sm[q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane];
        const double tv = ((sv[q] + red[0][MAXD + q][lane]) + red[1][MAXD + q][lane]) + red[2][MAXD + q][lane];
        const double sc = KC == PGK_BROWN ? 1.0 : invl[q];
        const size_t o = ((size_t)f * M + m) * d + q;
        if (p.dmean) p.dmean[o] = bad ? nan : tm * sc;
        if (p.dvar) p.dvar[o] = bad ? nan : dkss - 2.0 * (tv * sc);
      }
    }
  }
}

}  // namespace cgp
