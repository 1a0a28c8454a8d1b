// cgp_trend.hpp -- explicit basis functions (a trend with a vague prior on its coefficients, Rasmussen & Williams 2.7) after the
// multi-target machinery: f(x) = g(x) + h(x)^T beta.  The q basis columns H ride through the solve and the contraction as q more
// target columns ([Y | H] packed as P + q columns: cgp_multi.hpp); what is new is everything after that:
//
//   Z = L^-1 Y     G = L^-1 H     V = L^-1 K(X, Xs)
//   A = G^T G (q x q) = L_A L_A^T      B = G^T Z (q x P)      beta[:, p] = A^-1 B[:, p]      R = Hs^T - G^T V  (q x M)
//   mean[p, m] = sum_i V[i, m] Z[i, p] + sum_r R[r, m] beta[r, p]
//   var[m]     = the fit's own variance + |L_A^-1 R[:, m]|^2
//   logml[p]   = -1/2 |Z_p|^2 + 1/2 B_p^T beta_p - sum log L_ii - sum log (L_A)_rr - (N - q)/2 log 2 pi
//
//   k_trend_pack    [Y | H] (P + q, N) row-major -> Zw (k_multi_pack's transposition with two sources); column 0 also to the fit's y.
//   k_trend_gram    S = G^T [Z | G], 16 x (P + q) per fit, on the fp64 matrix cores (16x16x4): the basis columns are the 16 rows of the
//                   A operand (zero beyond q), one workgroup per (fit, 16 result columns), K over the REAL samples in sample order.
//                   The samples are dealt to the four waves as four contiguous runs of 4-sample blocks (a function of n only); the
//                   four partial sums meet in one fixed tree, (w0 + w1) + (w2 + w3).  One body over a column accessor, so that the
//                   batch scratch and the windows' Z scratch (the last q columns of a multi-target window: cgp_window_multi.hpp)
//                   are both read in place.  No atomics.
//   k_trend_solve   one wave per fit: the unpivoted Cholesky of A in index order under the rank rule (pivot r fails when it is not
//                   > 1e-10 A[r][r], A[r][r] the entry before elimination; NaN and negative pivots fail the same test), L_A^-1 (kept
//                   for the variance), beta and the evidence terms of all P columns, tinfo and the NaN rule.
//   k_trend_apply   per (fit, m): R[:, m] from Hs and the contraction's basis rows, the quadratic form onto var, sum_r R beta onto
//                   every target's mean row in fixed order over r.
// A column's results depend on its own data and the basis only: never on p, P, the slot or the neighbours.  fp64 only.
#pragma once
#include "cgp_multi.hpp"

namespace cgp {

constexpr int TR_MAX = 16;            // CGP_MAX_TREND: the basis columns are the 16 rows of one MFMA tile
constexpr double TR_RANK_TOL = 1e-10;

struct TrendArgs {
  const double *Y;        // [nfit][P][N]   (k_trend_pack)
  const double *H;        // [nfit][q][N]
  double *y0;             // [nfit][N] column 0 for the fit schedule, or null
  double *Zw;             // the multi-target scratch of the call's first fit: [nfit][NT 128][ldz]
  size_t z_stride;
  int ldz, NT;
  int N, M, P, q, nfit;   // P targets, q basis columns: column j of the source is target j (j < P) or basis column j - P
  int ncol;               // P + q rounded up to 16
  double *S;              // [nfit][ncol][16]   S[j][r] = sum_c G[c][r] X[c][j]
  double *Linv;           // [nfit][16][16]     L_A^-1, zero above the diagonal and beyond q
  const double *mean0;    // [nfit][P + q][M]   the contraction V^T [Z | G]
  const double *logml0;   // [nfit][P + q]      the multi-target evidence of every column
  const double *Hs;       // [nfit][q][M]
  double *mean;           // [nfit][P][M]
  double *var;            // [nfit][M]  in: the fit's own variance; out: + the quadratic form
  double *beta;           // [nfit][P][q]
  double *logml;          // [nfit][P]
  const int *info;        // the fit's failing pivot: word f info_stride (the windows: word 2 of the state words, stride 4)
  int info_stride;
  int *tinfo;             // [nfit] the 1-based failing pivot of A
  // the resident windows as the source (cgp_window_predict_trend): the Z scratch of cgp_window_multi.hpp, [nwin][pt][nrow][16], row =
  // sample (oldest first), and the state words [nwin][4] whose word 1 is the window's number of samples
  const double *zs;
  const int *state;
  int pt, nrow;
};

__global__ __launch_bounds__(MP_TILE * 8) void k_trend_pack(TrendArgs p) {
  __shared__ double t[MP_TILE][MP_TILE + 1];
  const int f = blockIdx.z, c0 = blockIdx.x * MP_TILE, p0 = blockIdx.y * MP_TILE;
  const int tx = threadIdx.x & (MP_TILE - 1), ty = threadIdx.x / MP_TILE;
  const double *Y = p.Y + (size_t)f * p.P * p.N, *H = p.H + (size_t)f * p.q * p.N;
#pragma unroll
  for (int i = 0; i < MP_TILE / 8; ++i) {
    const int pp = p0 + ty + 8 * i, c = c0 + tx;
    double v = 0.0;
    if (c < p.N) {
      if (pp < p.P) v = Y[(size_t)pp * p.N + c];
      else if (pp < p.P + p.q) v = H[(size_t)(pp - p.P) * p.N + c];
    }
    t[ty + 8 * i][tx] = v;
    if (pp == 0 && p.y0 != nullptr && c < p.N) p.y0[(size_t)f * p.N + c] = v;
  }
  __syncthreads();
  double *Zf = p.Zw + (size_t)f * p.z_stride;
#pragma unroll
  for (int i = 0; i < MP_TILE / 8; ++i) Zf[(size_t)(c0 + ty + 8 * i) * p.ldz + p0 + tx] = t[tx][ty + 8 * i];   // (c0 + 32 <= NT 128, p0 + 32 <= ldz)
}

// Column accessors of k_trend_gram: value of column j at sample c (c < n, j < P + q), n = the number of real samples.
struct TrendBatchCols {   // the multi-target scratch after k_multi_solve
  const double *Zf;
  int ldz, n;
  __device__ __forceinline__ double operator()(int c, int j) const { return Zf[(size_t)c * ldz + j]; }
};
struct TrendWindowCols {   // the windows' Z scratch after k_window_multi_z; rows from n on are not read
  const double *Zw;
  int nrow, n;
  __device__ __forceinline__ double operator()(int c, int j) const { return Zw[((size_t)(j >> 4) * nrow + c) * 16 + (j & 15)]; }
};
template <bool WIN> __device__ __forceinline__ auto trend_cols(const TrendArgs &p, int f) {
  if constexpr (WIN) return TrendWindowCols{p.zs + (size_t)f * p.pt * p.nrow * 16, p.nrow, p.state[f * 4 + 1]};
  else return TrendBatchCols{p.Zw + (size_t)f * p.z_stride, p.ldz, p.N};
}

constexpr int TG_WAVES = 4, TG_DEPTH = 8;
// S rows [16 chunk, 16 chunk + 16) of one fit: Sf[j][r], r = basis column.  Called by all TG_WAVES waves of the workgroup.
template <class Cols>
__device__ __forceinline__ void trend_gram_body(const Cols &X, int P, int q, int chunk, double *Sf, double (*red)[4][64]) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = X.n, j = chunk * TR_MAX + l15;
  const bool acol = l15 < q, bcol = j < P + q;
  // blocks of 4 samples: wave w takes the w-th contiguous quarter of them
  const int nblk = (n + 3) / 4, per = (nblk + TG_WAVES - 1) / TG_WAVES;
  const int b0 = wave * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  d4 acc = d4{0, 0, 0, 0};
  for (int kb = b0; kb < b1; kb += TG_DEPTH) {   // TG_DEPTH blocks' operands requested before the first product; a block past
    double a[TG_DEPTH], b[TG_DEPTH];             // the wave's run or a sample past n contributes exact zeros
#pragma unroll
    for (int u = 0; u < TG_DEPTH; ++u) {
      const int c = (kb + u) * 4 + lq;
      const bool in = kb + u < b1 && c < n;
      a[u] = (in && acol) ? X(c, P + l15) : 0.0;   // A operand: G[c][basis l15]
      b[u] = (in && bcol) ? X(c, j) : 0.0;         // B operand: X[c][column j]
    }
#pragma unroll
    for (int u = 0; u < TG_DEPTH; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
  if (wave == 0 && bcol) {
#pragma unroll
    for (int r = 0; r < 4; ++r)   // register r of lane (l15, lq): basis row lq + 4 r, column j
      Sf[(size_t)j * TR_MAX + lq + 4 * r] = (red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]);
  }
}

template <bool WIN> __global__ __launch_bounds__(TG_WAVES * 64) void k_trend_gram(TrendArgs p) {
  __shared__ double red[TG_WAVES][4][64];
  const int f = blockIdx.y;
  trend_gram_body(trend_cols<WIN>(p, f), p.P, p.q, blockIdx.x, p.S + (size_t)f * p.ncol * TR_MAX, red);
}

// The factorisation of A and everything that follows from it for one fit; S = this fit's block, outputs = this fit's.  One wave.
// `bad`: the fit itself failed (tinfo = 0, NaN); n_lt_q has no separate rule: A is then rank-deficient and a pivot fails.
__device__ __forceinline__ void trend_solve_body(const double *Sf, int P, int q, bool bad, const double *logml0, double *Linv, double *beta,
                                                 double *logml, int *tinfo) {
  __shared__ double A[TR_MAX][TR_MAX + 1], L[TR_MAX][TR_MAX + 1], Li[TR_MAX][TR_MAX + 1], d0[TR_MAX];
  const int tid = threadIdx.x;   // 64 threads
  for (int e = tid; e < TR_MAX * TR_MAX; e += 64) {
    const int i = e / TR_MAX, jj = e - i * TR_MAX;
    A[i][jj] = (i < q && jj < q) ? Sf[(size_t)(P + i) * TR_MAX + jj] : 0.0;
    L[i][jj] = 0.0;
    Li[i][jj] = 0.0;
  }
  __syncthreads();
  if (tid < TR_MAX) d0[tid] = A[tid][tid];
  int fail = 0;
  const int i = tid;
  for (int r = 0; r < q; ++r) {
    __syncthreads();
    const double piv = A[r][r];
    if (!(piv > TR_RANK_TOL * d0[r])) {   // (uniform: every thread reads the same two words)
      fail = r + 1;
      break;
    }
    const double lrr = sqrt(piv);
    if (i == r) L[r][r] = lrr;
    if (i > r && i < q) L[i][r] = A[i][r] / lrr;
    __syncthreads();
    if (i > r && i < q)
      for (int jj = r + 1; jj <= i; ++jj) A[i][jj] = __builtin_fma(-L[i][r], L[jj][r], A[i][jj]);
  }
  __syncthreads();
  const bool nan_out = bad || fail != 0;
  if (tid == 0) *tinfo = bad ? 0 : fail;
  double sumlog = 0.0;
  if (!nan_out) {
    if (tid < q) {   // column tid of L_A^-1 by forward substitution
      const int c = tid;
      for (int r = c; r < q; ++r) {
        double s = r == c ? 1.0 : 0.0;
        for (int k = c; k < r; ++k) s = __builtin_fma(-L[r][k], Li[k][c], s);
        Li[r][c] = s / L[r][r];
      }
    }
    for (int r = 0; r < q; ++r) sumlog += log(L[r][r]);
  }
  __syncthreads();
  for (int e = tid; e < TR_MAX * TR_MAX; e += 64) Linv[e] = nan_out ? __builtin_nan("") : Li[e / TR_MAX][e % TR_MAX];
  for (int pp = tid; pp < P; pp += 64) {
    if (nan_out) {
      for (int r = 0; r < q; ++r) beta[(size_t)pp * q + r] = __builtin_nan("");
      logml[pp] = __builtin_nan("");
      continue;
    }
    // w = L_A^-1 B_p, beta_p = L_A^-T w, B_p^T beta_p = |w|^2.  Entries beyond q are zero in S and in Li: the loops run to 16.
    double b[TR_MAX], w[TR_MAX];
#pragma unroll
    for (int r = 0; r < TR_MAX; ++r) b[r] = Sf[(size_t)pp * TR_MAX + r];
    double ww = 0.0;
#pragma unroll
    for (int r = 0; r < TR_MAX; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k <= r; ++k) s = __builtin_fma(Li[r][k], b[k], s);
      w[r] = s;
      ww = __builtin_fma(s, s, ww);
    }
#pragma unroll
    for (int r = 0; r < TR_MAX; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = r; k < TR_MAX; ++k) s = __builtin_fma(Li[k][r], w[k], s);
      if (r < q) beta[(size_t)pp * q + r] = s;
    }
    logml[pp] = logml0[pp] + 0.5 * ww - sumlog + 0.5 * q * 1.8378770664093453;   // logml0 carries -N/2 log 2 pi
  }
}

__global__ __launch_bounds__(64) void k_trend_solve(TrendArgs p) {
  const int f = blockIdx.x;
  trend_solve_body(p.S + (size_t)f * p.ncol * TR_MAX, p.P, p.q, p.info[(size_t)f * p.info_stride] != 0, p.logml0 + (size_t)f * (p.P + p.q),
                   p.Linv + (size_t)f * TR_MAX * TR_MAX, p.beta + (size_t)f * p.P * p.q, p.logml + (size_t)f * p.P, p.tinfo + f);
}

constexpr int TA_THREADS = 128, TA_PCH = 32;
// One fit's test points [blockIdx.x 128, + 128) and targets [blockIdx.y 32, + 32).  mean0 rows: [P targets | q basis rows] of M.
__device__ __forceinline__ void trend_apply_body(const double *mean0, const double *Hs, const double *Linv, const double *beta, int M, int P,
                                                 int q, bool nan_out, double *mean, double *var) {
  __shared__ double Li[TR_MAX * TR_MAX];
  const int tid = threadIdx.x, m = blockIdx.x * TA_THREADS + tid;
  const int p0 = blockIdx.y * TA_PCH, p1 = p0 + TA_PCH < P ? p0 + TA_PCH : P;
  for (int e = tid; e < TR_MAX * TR_MAX; e += TA_THREADS) Li[e] = Linv[e];
  __syncthreads();
  if (m >= M) return;
  if (nan_out) {
    if (blockIdx.y == 0) var[m] = __builtin_nan("");
    for (int pp = p0; pp < p1; ++pp) mean[(size_t)pp * M + m] = __builtin_nan("");
    return;
  }
  double R[TR_MAX];
#pragma unroll
  for (int r = 0; r < TR_MAX; ++r) R[r] = r < q ? Hs[(size_t)r * M + m] - mean0[(size_t)(P + r) * M + m] : 0.0;
  if (blockIdx.y == 0) {
    double quad = 0.0;
#pragma unroll
    for (int r = 0; r < TR_MAX; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k <= r; ++k) s = __builtin_fma(Li[r * TR_MAX + k], R[k], s);
      quad = __builtin_fma(s, s, quad);
    }
    var[m] = var[m] + quad;
  }
  for (int pp = p0; pp < p1; ++pp) {
    double s = mean0[(size_t)pp * M + m];
    const double *bp = beta + (size_t)pp * q;
#pragma unroll
    for (int r = 0; r < TR_MAX; ++r)
      if (r < q) s = __builtin_fma(R[r], bp[r], s);
    mean[(size_t)pp * M + m] = s;
  }
}

__global__ __launch_bounds__(TA_THREADS) void k_trend_apply(TrendArgs p) {
  const int f = blockIdx.z;
  trend_apply_body(p.mean0 + (size_t)f * (p.P + p.q) * p.M, p.Hs + (size_t)f * p.q * p.M, p.Linv + (size_t)f * TR_MAX * TR_MAX,
                   p.beta + (size_t)f * p.P * p.q, p.M, p.P, p.q, p.info[(size_t)f * p.info_stride] != 0 || p.tinfo[f] != 0, p.mean + (size_t)f * p.P * p.M,
                   p.var + (size_t)f * p.M);
}

}  // namespace cgp
