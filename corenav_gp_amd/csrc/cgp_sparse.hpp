// cgp_sparse.hpp -- sparse (inducing-point) fits: the collapsed variational bound of Titsias (2009) -- GPy's
// SparseGPRegression / VarDTC -- and its forecast.  Per fit: samples X (N, d), y (N), inducing inputs Z (m, d), test points Xs (M, d).
//
//   sigma2 = sigma_n^2 + 1e-8      eps = 1e-8 + jitter      K_uu = K(Z, Z) + eps I = L_u L_u^T
//   Phi = K_uf K_fu (m x m)        b = K_uf y               yty = y^T y            t = sum_i k(x_i, x_i)
//   A = L_u^-1 Phi L_u^-T / sigma2         B = I + A = L_B L_B^T           c = L_B^-1 L_u^-1 b / sigma2
//   bound = -N/2 log 2 pi - N/2 log sigma2 - sum log diag(L_B) - yty / (2 sigma2) + c^T c / 2 - t / (2 sigma2) + tr(A) / 2
//   V1 = L_u^-1 K(Z, Xs)   V2 = L_B^-1 V1   mean = V2^T c   var = k** - colsum(V1^2) + colsum(V2^2)  (clipped at 1e-15, + sigma_n^2)
//
// No N x N object anywhere: the cost is N m^2 for Phi and m^3 for the rest, and N is bounded by the sparse reservation only.
// Five launches on one stream, each a function of the fit's own data and of (N, m, M, d, kernel) only -- no atomics, every sum in
// a fixed order -- so a fit's outputs do not depend on the batch, its slot or its neighbours:
//   k_sparse_prep     the fit's parameter record (the prep record of the other kernels: win_cov's formulas read it).
//   k_sparse_phi      the hot path.  The augmented matrix [K_uf; y] [K_uf; y]^T -- row m is y, so b and yty come out of the same
//                     product -- is cut into 16 x 16 tiles of its lower triangle, the sum over N into at most SP_MAX_CHUNKS chunks
//                     (a function of N alone).  One workgroup (eight waves) per (fit, chunk, group of at most SP_GROUP tiles): it
//                     walks its chunk in sub-panels of S samples, evaluates the panel K(Z, x) (rows: the inducing inputs its tiles
//                     need, staged in LDS once) into LDS, sample-major with a row stride of an odd number of 16-double groups (the
//                     four k-rows of an MFMA operand then fall on different banks), and every wave accumulates its up to SP_TPW
//                     tiles with both operands from LDS on v_mfma_f64_16x16x4_f64.  Two panel buffers: sub-panel s + 1 is
//                     evaluated (VALU) before the MFMAs of sub-panel s are issued, one barrier per sub-panel.  The chunk's tiles
//                     go to the partial buffer.  At m = 512 the triangle is 561 tiles: four groups, each evaluating only the rows
//                     up to its last tile's.  The sum over a tile's samples is one chain in sample order whatever S is.
//   k_sparse_reduce   sums a fit's partial tiles in chunk order and unpacks them: Phi (both triangles, zero in the padding), b, yty.
//   k_sparse_algebra  one workgroup per fit, in place in scratch: K_uu evaluated and factored, W = L_u^-1 Phi and L_u^-1 W^T by
//                     blocked forward substitutions on the MFMA (diagonal-inverse tiles, the product with the inverse chained in
//                     registers as k_window_joint_chol applies L(J, J)^-1), B factored, the two vector solves for c, tr(A), the
//                     log-determinant, t and the bound.  The blocked Cholesky is k_window_joint_chol's scheme written out here
//                     (sparse_chol): it also keeps the diagonal blocks' inverses, and a shared block-column step has already been
//                     measured slower for that kernel (docs/negatives.md item 20).  Non-positive pivots are repaired and reported.
//   k_sparse_predict  one WAVE per (fit, 16 test points): the K(Z, xs) tile in LDS, forward solves against L_u and L_B in place
//                     (L blocks from memory, one block ahead in registers), the two column sums and V2^T c as the rows finish.
// Padding: m + 1 is rounded up to LD = 16 mt; the padding is zero in Phi and identity in K_uu and B.
#pragma once
#include "cgp_window_adapt.hpp"

namespace cgp {

constexpr int SP_MAX_IND = 512;                 // inducing inputs of a fit
constexpr int SP_THREADS = 512;                 // k_sparse_phi
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_TPW = 20;                      // accumulator tiles of a wave (160 of its 256 registers)
constexpr int SP_GROUP = SP_WAVES * SP_TPW;     // tiles of a workgroup
constexpr int SP_CHUNK = 512;                   // samples of the shortest chunk
constexpr int SP_MAX_CHUNKS = 16;               // chunks of the longest history
constexpr int SPA_THREADS = 256;                // k_sparse_algebra
constexpr int SPA_WAVES = SPA_THREADS / 64;
constexpr int SPA_TPW = 9;                      // tiles of a wave per block column / block row: ceil(33 / 4)
constexpr int SPP_WAVES = 4;                    // k_sparse_predict: waves (column tiles) of a workgroup, fewer when LDS is short
constexpr int SP_LDMAX = ((SP_MAX_IND + 1 + 15) / 16) * 16;
constexpr int SP_MAX_P = 64;                    // target columns of a fit (cgp_sparse_multi.hpp's calls; the other calls have one)
constexpr int SPV_COLS = 8;                     // target columns of one pass of sparse_vec_solve
static_assert(SPA_TPW * SPA_WAVES * 16 >= SP_LDMAX, "a wave holds every tile of its share");
// the fit's record: PREP_N doubles in the prep record's layout ([0..7] 1 / ell_q, [9] amp, [10] amp_b), then
constexpr int SP_R_SIGMA2 = 11, SP_R_EPS = 12, SP_R_NOISE = 13;   // sigma_n^2 + 1e-8, 1e-8 + jitter, sigma_n^2

// what follows from a call's (N, m, d) alone
struct SparseShape {
  int mt, LD, nt0;        // tiles per side of the m x m objects (m + 1 rounded up), 16 mt, tiles of their lower triangle
  int mta, LDa, ntile;    // the same of the augmented matrix of m + P rows (P target rows; at P = 1 they are the three above)
  int nch, clen;          // chunks of the sum over N, samples per chunk (a multiple of 16)
  int ngrp, tpg;          // tile groups (workgroups per chunk), tiles per group
  int S, ldr;             // samples of a sub-panel, row stride of the LDS panel
};
__host__ __device__ inline int sparse_chunks(int N) {
  const int n = (N + SP_CHUNK - 1) / SP_CHUNK;
  return n < SP_MAX_CHUNKS ? n : SP_MAX_CHUNKS;
}
inline size_t sparse_phi_lds(int d, int LD, int S, int ldr) { return ((size_t)d * LD + (size_t)2 * S * ldr) * sizeof(double); }
inline SparseShape sparse_shape(int N, int m, int d, int P = 1) {
  SparseShape s{};
  s.mt = (m + 1 + 15) / 16;
  s.LD = s.mt * 16;
  s.nt0 = s.mt * (s.mt + 1) / 2;
  s.mta = (m + P + 15) / 16;
  s.LDa = s.mta * 16;
  s.ntile = s.mta * (s.mta + 1) / 2;
  s.nch = sparse_chunks(N);
  s.clen = (((N + s.nch - 1) / s.nch) + 15) / 16 * 16;
  s.ngrp = (s.ntile + SP_GROUP - 1) / SP_GROUP;
  s.tpg = (s.ntile + s.ngrp - 1) / s.ngrp;
  s.ldr = 16 * (s.mta | 1);
  s.S = sparse_phi_lds(d, s.LDa, 16, s.ldr) <= (size_t)160 * 1024 ? 16 : 8;
  return s;
}
inline int sparse_predict_waves(int LD) {
  const int fit = (int)(((size_t)160 * 1024) / ((size_t)LD * 16 * sizeof(double)));
  return fit < SPP_WAVES ? fit : SPP_WAVES;
}

struct SparseArgs {
  // the call's arrays, at its first fit: X (fit, d, N), y (fit, N), Z (fit, d, m), Xs (fit, d, M), theta (fit, MAX_THETA)
  // the P target columns of a fit: y (fit, P, N), mean (fit, P, M), logml (fit, P); P = 1 in every call but the multi-column ones
  const double *X, *y, *Z, *Xs, *theta, *jitter;   // jitter (fit) or null
  double *mean, *var, *logml;                      // (fit, P, M), (fit, M), (fit, P)
  int *info;                                       // (fit)
  // the reservation's scratch, at the call's first fit, strided by the call's own shape
  double *rec;     // [fit][PREP_N]
  double *part;    // [fit][nch][nt0][256] a chunk's tiles, element (row lq + 4 r, column l15) of a tile at r * 64 + lane
  double *partx;   // [fit][nch][ntile - nt0][256] the tiles of the tile rows that P > 1 targets add (the multi reservation's)
  double *U;       // [fit][LD][LD] K_uu, then L_u: column-major lower triangle
  double *F;       // [fit][LD][LD] Phi, then L_u^-1 W^T, then B and L_B
  double *W;       // [fit][LD][LD] W = L_u^-1 Phi, row-major
  double *dinv;    // [fit][2][mt][256] inverses of the diagonal blocks of L_u, L_B: element (row i, column k) at k * 16 + i
  double *vec;     // [fit][4][LD] b, c, diag(A)
  double *scal;    // [fit][8] yty
  // the targets' vectors, column p of fit f: b at bm + f bcs + p LD, c at cm + f bcs + p LD, yty at yty[f ytys + p].  One column:
  // the b and c of vec and scal[0] (what the gradient kernels read); several: the multi reservation's [fit][2][P][LD] and [fit][P]
  double *bm, *cm, *yty;
  int bcs, ytys, P;
  double *Acp;     // [fit][LD][LD] or null: a copy of A, row-major, for the gradient call (cgp_sparse_grad.hpp)
  int N, d, M, m, kid, include_noise, nfit;
  SparseShape sh;
};

__device__ __forceinline__ void sparse_tile(int idx, int &I, int &J) {   // tile idx of the lower triangle, row by row
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= idx) ++I;
  J = idx - I * (I + 1) / 2;
}
__device__ __forceinline__ void sparse_wave_sync() {   // LDS / memory written by this wave's lanes is read by its other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void k_sparse_prep(SparseArgs p) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= p.nfit) return;
  const double *th = p.theta + (size_t)f * MAX_THETA;
  double *o = p.rec + (size_t)f * PREP_N;
  const int kid = p.kid, d = p.d;
  for (int q = 0; q < MAXD; ++q) o[q] = q < d ? 1.0 / (k_is_ard(kid) ? th[1 + q] : th[1]) : 0.0;
  const double noise = th[k_ntheta(kid, d) - 1];
  o[8] = 0.0;
  o[9] = th[0];
  o[10] = kid == K_RBF_BROWNIAN ? th[2] : 0.0;
  o[SP_R_SIGMA2] = noise + 1e-8;
  o[SP_R_EPS] = 1e-8 + (p.jitter ? p.jitter[f] : 0.0);
  o[SP_R_NOISE] = noise;
  o[14] = o[15] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void k_sparse_phi(SparseArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int g = blockIdx.x, ch = blockIdx.y, f = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, m = p.m, d = p.d, kid = p.kid;
  const int LD = p.sh.LDa, S = p.sh.S, ldr = p.sh.ldr, ntile = p.sh.ntile, nt0 = p.sh.nt0, tpg = p.sh.tpg, mP = m + p.P;
  double *Zl = reinterpret_cast<double *>(smem_raw);   // [d][LD] the inducing inputs, zero in the padding
  double *P = Zl + (size_t)d * LD;                     // [2][S][ldr] the panel: row r of sample s at s * ldr + r
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double *X = p.X + (size_t)f * d * N, *y = p.y + (size_t)f * p.P * N, *Z = p.Z + (size_t)f * d * m;
  // the group's tiles; wave w holds tiles w, w + SP_WAVES, ... of the group
  const int first = g * tpg;
  const int last = (first + tpg < ntile ? first + tpg : ntile) - 1;
  int nrows;   // the panel rows the group's tiles read
  {
    int I, J;
    sparse_tile(last, I, J);
    nrows = (I + 1) * WPB;
  }
  int ab[SP_TPW];   // the tiles' panel rows, wave-uniform: I 16 | J 16 << 16
  unsigned live = 0;
#pragma unroll
  for (int t = 0; t < SP_TPW; ++t) {
    const int u = wave + SP_WAVES * t;
    const bool ok = u < tpg && first + u <= last;
    int I = 0, J = 0;
    if (ok) sparse_tile(first + u, I, J);
    ab[t] = __builtin_amdgcn_readfirstlane(I * WPB | (J * WPB) << 16);
    live |= ok ? 1u << t : 0u;
  }
  for (int e = tid; e < d * LD; e += SP_THREADS) {
    const int q = e / LD, r = e - q * LD;
    Zl[e] = r < m ? Z[(size_t)q * m + r] : 0.0;
  }
  const int n0 = ch * p.sh.clen;
  const int n1 = n0 + p.sh.clen < N ? n0 + p.sh.clen : N;
  const int nsp = n1 > n0 ? (n1 - n0 + S - 1) / S : 0;
  __syncthreads();
  // sub-panel sp into buffer `buf`: K(z_r, x_i) for r < m, target column q of x_i in row m + q, zero in the padding and past the chunk
  auto eval = [&](int sp, int buf) {
    double *Pb = P + (size_t)buf * S * ldr;
    const int tot = nrows * S;
    for (int e = tid; e < tot; e += SP_THREADS) {
      const int s = e / nrows, r = e - s * nrows;
      const int i = n0 + sp * S + s;
      double v = 0.0;
      if (i < n1) {
        if (r < m) v = win_cov(kid, d, pr, Zl + r, LD, X + i, N, false);
        else if (r < mP) v = y[(size_t)(r - m) * N + i];
      }
      Pb[s * ldr + r] = v;
    }
  };
  d4 acc[SP_TPW];
#pragma unroll
  for (int t = 0; t < SP_TPW; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  if (nsp > 0) eval(0, 0);
  __syncthreads();
  for (int sp = 0; sp < nsp; ++sp) {
    const int buf = sp & 1;
    if (sp + 1 < nsp) eval(sp + 1, buf ^ 1);
    // A operand: lane (l15, lq) holds row I 16 + l15 of sample 4 ks + lq; B operand: row J 16 + l15 of the same sample
    const double *Pb = P + (size_t)buf * S * ldr + lq * ldr + l15;
    for (int ks = 0; ks < S / 4; ++ks) {
      const double *row = Pb + ks * 4 * ldr;
#pragma unroll
      for (int t = 0; t < SP_TPW; ++t)
        if (live >> t & 1u) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[ab[t] & 0xffff], row[ab[t] >> 16], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // tiles of the m x m objects' tile rows to the partial buffer, those of the tile rows further targets add to theirs
  const size_t fc = (size_t)f * p.sh.nch + ch;
#pragma unroll
  for (int t = 0; t < SP_TPW; ++t)
    if (live >> t & 1u) {
      const int u = first + wave + SP_WAVES * t;
      double *o = (u < nt0 ? p.part + (fc * nt0 + u) * 256 : p.partx + (fc * (ntile - nt0) + (u - nt0)) * 256) + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r * 64] = acc[t][r];
    }
}

// One workgroup per (tile, fit): the chunks' tiles summed in chunk order, unpacked into Phi (in the m x m objects' layout, whatever
// P is), the b of every target column and its yty.
__global__ __launch_bounds__(256) void k_sparse_reduce(SparseArgs p) {
  const int idx = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int m = p.m, LD = p.sh.LD, ntile = p.sh.ntile, nt0 = p.sh.nt0, nch = p.sh.nch;
  int I, J;
  sparse_tile(idx, I, J);
  const int lane = tid & 63, r = tid >> 6;
  const int i = I * WPB + (lane >> 4) + 4 * r, j = J * WPB + (lane & 15);
  const int nt = idx < nt0 ? nt0 : ntile - nt0;   // tiles of a chunk in the buffer that holds this one
  const double *src = (idx < nt0 ? p.part + ((size_t)f * nch * nt + idx) * 256 : p.partx + ((size_t)f * nch * nt + (idx - nt0)) * 256) + tid;
  double v = 0.0;
  for (int c = 0; c < nch; ++c) v += src[(size_t)c * nt * 256];
  if (i < LD && j < LD) {
    double *F = p.F + (size_t)f * LD * LD;
    const double phi = (i < m && j < m) ? v : 0.0;
    F[(size_t)i * LD + j] = phi;
    if (I != J) F[(size_t)j * LD + i] = phi;   // (a diagonal tile holds both of its triangles itself)
  }
  if (i >= m && i < m + p.P && j < LD) {   // a target's row: its tiles cover every column of the padded m x m objects
    double *b = p.bm + (size_t)f * p.bcs + (size_t)(i - m) * LD;
    b[j] = j < m ? v : 0.0;
  }
  if (i >= m && i < m + p.P && j == i) p.yty[(size_t)f * p.ytys + (i - m)] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// In-place blocked Cholesky of the column-major matrix Cw (leading dimension ld = 16 mt, lower triangle): k_window_joint_chol's
// scheme with the diagonal blocks' inverses kept in dinv.  Returns (to every thread) the first failing pivot, 1-based, or 0.
__device__ __forceinline__ int sparse_chol(double *Cw, int ld, int mt, double *dinv, double *tile, double *winv, int *sbad, int tid) {
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bad = 0;
  for (int J = 0; J < mt; ++J) {
    const int J0 = J * WPB;
    // the wave's tiles of block column J, transposed: acc[t][r] = element (row I_t 16 + l15, column J0 + lq + 4 r)
    d4 acc[SPA_TPW];
#pragma unroll
    for (int t = 0; t < SPA_TPW; ++t) {
      const int I = J + wave + SPA_WAVES * t;
      acc[t] = d4{0.0, 0.0, 0.0, 0.0};
      if (I < mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = Cw[(size_t)(J0 + lq + 4 * r) * ld + I * WPB + l15];
      }
    }
    for (int kb = 0; kb < J; ++kb) {
      const double *col = Cw + (size_t)(kb * WPB + lq) * ld;
      double a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[ks] = -col[(size_t)(4 * ks) * ld + J0 + l15];
#pragma unroll
      for (int t = 0; t < SPA_TPW; ++t) {
        const int I = J + wave + SPA_WAVES * t;
        if (I < mt) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = col[(size_t)(4 * ks) * ld + I * WPB + l15];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    // wave 0: the diagonal block (its first tile) in registers, lane = row; the inverse goes to LDS and to dinv
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(lq + 4 * r) * WPB + l15] = acc[0][r];
      sparse_wave_sync();
      double a[WPB], wv[WPB];
#pragma unroll
      for (int c = 0; c < WPB; ++c) a[c] = tile[c * WPB + l15];
      int badl = 0;
      factor_block16_repair<double>(a, wv, badl, J0, l15);
      if (bad == 0) bad = badl;
      if (lane < WPB) {
#pragma unroll
        for (int k = 0; k < WPB; ++k) {
          winv[l15 * WPB + k] = wv[k];
          dinv[J * (WPB * WPB) + l15 * WPB + k] = wv[k];
        }
#pragma unroll
        for (int c = 0; c < WPB; ++c)
          if (c <= l15) Cw[(size_t)(J0 + c) * ld + J0 + l15] = a[c];
      }
    }
    __syncthreads();
    {
      double di[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) di[r] = winv[(lq + 4 * r) * WPB + l15];
#pragma unroll
      for (int t = 0; t < SPA_TPW; ++t) {
        const int I = J + wave + SPA_WAVES * t;
        if (I < mt && I > J) {
          d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[t][r], v, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) Cw[(size_t)(J0 + lq + 4 * r) * ld + I * WPB + l15] = v[r];
        }
      }
    }
    __syncthreads();   // block column J is in memory before block column J + 1 reads it
  }
  if (tid == 0) *sbad = bad;   // lane 0 of wave 0 saw every pivot's verdict (the row broadcasts reach all lanes)
  __syncthreads();
  return *sbad;
}

// Xo = L^-1 R for all ld columns: L column-major with the inverses of its diagonal blocks in dinv, Xo row-major (element (i, j) at
// i * ld + j).  TRANS: the right-hand side is R^T, R row-major.  Wave w owns the column tiles w, w + SPA_WAVES, ...; block row I:
// acc = R(I, c) - sum_{K < I} L(I, K) Xo(K, c), then Xo(I, c) = L(I, I)^-1 acc with four chained MFMAs.
template <bool TRANS>
__device__ __forceinline__ void sparse_trsm(const double *L, const double *dinv, const double *R, double *Xo, int ld, int mt, int tid) {
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int I = 0; I < mt; ++I) {
    d4 acc[SPA_TPW];
#pragma unroll
    for (int t = 0; t < SPA_TPW; ++t) {
      const int c = wave + SPA_WAVES * t;
      acc[t] = d4{0.0, 0.0, 0.0, 0.0};
      if (c < mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[t][r] = TRANS ? R[(size_t)(c * WPB + l15) * ld + I * WPB + lq + 4 * r] : R[(size_t)(I * WPB + lq + 4 * r) * ld + c * WPB + l15];
      }
    }
    for (int K = 0; K < I; ++K) {
      double a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[ks] = -L[(size_t)(K * WPB + 4 * ks + lq) * ld + I * WPB + l15];
#pragma unroll
      for (int t = 0; t < SPA_TPW; ++t) {
        const int c = wave + SPA_WAVES * t;
        if (c < mt) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double b = Xo[(size_t)(K * WPB + 4 * ks + lq) * ld + c * WPB + l15];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    double di[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) di[r] = dinv[I * (WPB * WPB) + (lq + 4 * r) * WPB + l15];
#pragma unroll
    for (int t = 0; t < SPA_TPW; ++t) {
      const int c = wave + SPA_WAVES * t;
      if (c < mt) {
        d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) v = __builtin_amdgcn_mfma_f64_16x16x4f64(di[r], acc[t][r], v, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Xo[(size_t)(I * WPB + lq + 4 * r) * ld + c * WPB + l15] = v[r];
      }
    }
    __syncthreads();   // block row I of Xo is in memory before block row I + 1 reads it
  }
}

// x = L^-1 x for the nq <= SPV_COLS vectors x[q][SP_LDMAX] in LDS, block row by block row: sixteen partial sums per row and vector in
// a fixed order, then the block's inverse.  Each vector's arithmetic is its own and the same whatever nq is; L is read once for all.
__device__ __forceinline__ void sparse_vec_solve(const double *L, const double *dinv, double *x, int nq, double *red, double *rr, int ld,
                                                 int mt, int tid) {
  const int i = tid & 15, part = tid >> 4;
  for (int I = 0; I < mt; ++I) {
    double s[SPV_COLS];
#pragma unroll
    for (int q = 0; q < SPV_COLS; ++q) s[q] = 0.0;
    for (int k = part; k < I * WPB; k += SPA_THREADS / 16) {
      const double l = L[(size_t)k * ld + I * WPB + i];
#pragma unroll
      for (int q = 0; q < SPV_COLS; ++q)
        if (q < nq) s[q] = __builtin_fma(l, x[q * SP_LDMAX + k], s[q]);
    }
#pragma unroll
    for (int q = 0; q < SPV_COLS; ++q)
      if (q < nq) red[q * SPA_THREADS + part * WPB + i] = s[q];
    __syncthreads();
    if (tid < WPB * nq) {
      double r = x[part * SP_LDMAX + I * WPB + i];
      for (int q = 0; q < SPA_THREADS / 16; ++q) r -= red[part * SPA_THREADS + q * WPB + i];
      rr[tid] = r;
    }
    __syncthreads();
    if (tid < WPB * nq) {
      double v = 0.0;
      for (int j = 0; j <= i; ++j) v = __builtin_fma(dinv[I * (WPB * WPB) + j * WPB + i], rr[part * WPB + j], v);
      x[part * SP_LDMAX + I * WPB + i] = v;
    }
    __syncthreads();
  }
}

// the sum of every thread's v, the same in every thread: each lane of wave 0 adds four values, then a butterfly
__device__ __forceinline__ double sparse_block_sum(double v, double *red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  double s = 0.0;
  const int lane = tid & 63;
#pragma unroll
  for (int q = 0; q < SPA_THREADS / 64; ++q) s += red[lane + 64 * q];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

__global__ __launch_bounds__(SPA_THREADS) void k_sparse_algebra(SparseArgs p) {
  __shared__ double tile[WPB * WPB], winv[WPB * WPB], red[SPV_COLS * SPA_THREADS], rr[SPV_COLS * WPB], xv[SPV_COLS * SP_LDMAX];
  __shared__ int sbad;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int N = p.N, m = p.m, d = p.d, kid = p.kid, LD = p.sh.LD, mt = p.sh.mt;
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double sigma2 = pr[SP_R_SIGMA2], eps = pr[SP_R_EPS];
  const double *Z = p.Z + (size_t)f * d * m, *X = p.X + (size_t)f * d * N;
  double *U = p.U + (size_t)f * LD * LD, *F = p.F + (size_t)f * LD * LD, *W = p.W + (size_t)f * LD * LD;
  double *dU = p.dinv + (size_t)f * 2 * mt * (WPB * WPB), *dB = dU + (size_t)mt * (WPB * WPB);
  double *da = p.vec + (size_t)f * 4 * LD + 2 * LD;
  const double *bm = p.bm + (size_t)f * p.bcs;
  double *cm = p.cm + (size_t)f * p.bcs, *logml = p.logml + (size_t)f * p.P;
  const int P = p.P;
  const double nan = __builtin_nan("");
  // K_uu + eps I, lower triangle (zero above the diagonal), identity in the padding
  for (int e = tid; e < LD * LD; e += SPA_THREADS) {
    const int col = e / LD, row = e - col * LD;
    double v = row == col ? 1.0 : 0.0;
    if (row < m && col < m) {
      v = 0.0;
      if (row >= col) v = win_cov(kid, d, pr, Z + row, m, Z + col, m, row == col) + (row == col ? eps : 0.0);
    }
    U[e] = v;
  }
  __syncthreads();
  int bad = sparse_chol(U, LD, mt, dU, tile, winv, &sbad, tid);
  if (bad != 0) {
    if (tid == 0) p.info[f] = bad;
    if (tid < P) logml[tid] = nan;
    return;
  }
  sparse_trsm<false>(U, dU, F, W, LD, mt, tid);   // W = L_u^-1 Phi
  sparse_trsm<true>(U, dU, W, F, LD, mt, tid);    // F = L_u^-1 W^T = sigma2 A
  // B = I + A in place (the padding of A is zero: identity there), diag(A) aside
  for (int e = tid; e < LD * LD; e += SPA_THREADS) {
    const int i = e / LD, j = e - i * LD;
    const double a = F[e] / sigma2;
    if (i == j) da[i] = a;
    if (p.Acp) p.Acp[(size_t)f * LD * LD + e] = a;
    F[e] = i == j ? 1.0 + a : a;
  }
  __syncthreads();
  bad = sparse_chol(F, LD, mt, dB, tile, winv, &sbad, tid);
  if (bad != 0) {
    if (tid == 0) p.info[f] = m + bad;
    if (tid < P) logml[tid] = nan;
    return;
  }
  // the terms every target column shares
  double s_ld = 0.0, s_tr = 0.0, s_t = 0.0;
  for (int i = tid; i < LD; i += SPA_THREADS)
    if (i < m) {
      s_ld += log(F[(size_t)i * LD + i]);
      s_tr += da[i];
    }
  const WaCov kc = WaCov::from_prep(kid, d, pr);
  for (int i = tid; i < N; i += SPA_THREADS) s_t += kc.kss(X[i]);
  s_ld = sparse_block_sum(s_ld, red, tid);
  s_tr = sparse_block_sum(s_tr, red, tid);
  s_t = sparse_block_sum(s_t, red, tid);
  // c = L_B^-1 (L_u^-1 b) / sigma2 and the bound, SPV_COLS target columns per pass over the block rows
  for (int q0 = 0; q0 < P; q0 += SPV_COLS) {
    const int nq = P - q0 < SPV_COLS ? P - q0 : SPV_COLS;
    __syncthreads();
    for (int q = 0; q < nq; ++q)
      for (int i = tid; i < LD; i += SPA_THREADS) xv[q * SP_LDMAX + i] = bm[(size_t)(q0 + q) * LD + i];
    __syncthreads();
    sparse_vec_solve(U, dU, xv, nq, red, rr, LD, mt, tid);
    for (int q = 0; q < nq; ++q)
      for (int i = tid; i < LD; i += SPA_THREADS) xv[q * SP_LDMAX + i] = xv[q * SP_LDMAX + i] / sigma2;
    __syncthreads();
    sparse_vec_solve(F, dB, xv, nq, red, rr, LD, mt, tid);
    for (int q = 0; q < nq; ++q) {
      double s_cc = 0.0;
      for (int i = tid; i < LD; i += SPA_THREADS) {
        const double c = xv[q * SP_LDMAX + i];
        cm[(size_t)(q0 + q) * LD + i] = c;
        if (i < m) s_cc += c * c;
      }
      s_cc = sparse_block_sum(s_cc, red, tid);
      if (tid == 0) {
        const double yty = p.yty[(size_t)f * p.ytys + q0 + q];
        const double LOG_2PI = 1.8378770664093454836;
        logml[q0 + q] = -0.5 * N * LOG_2PI - 0.5 * N * log(sigma2) - s_ld - yty / (2.0 * sigma2) + 0.5 * s_cc - s_t / (2.0 * sigma2) + 0.5 * s_tr;
      }
    }
  }
  if (tid == 0) p.info[f] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// One wave per (fit, tile of 16 test points); the waves of a workgroup share nothing but the launch.
__global__ __launch_bounds__(SPP_WAVES * 64) void k_sparse_predict(SparseArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f = blockIdx.y, ct = blockIdx.x * (blockDim.x / 64) + wave;
  const int M = p.M, m = p.m, d = p.d, kid = p.kid, LD = p.sh.LD, mt = p.sh.mt;
  if (ct * WPB >= M) return;
  const int col = ct * WPB + l15;
  const bool colok = col < M;
  double *mean = p.mean + (size_t)f * p.P * M, *var = p.var + (size_t)f * M;
  if (p.info[f] != 0) {   // a failed fit: NaN in the variance and in every column's mean
    if (lq == 0 && colok) {
      var[col] = __builtin_nan("");
      for (int q = 0; q < p.P; ++q) mean[(size_t)q * M + col] = __builtin_nan("");
    }
    return;
  }
  double *V = reinterpret_cast<double *>(smem_raw) + (size_t)wave * LD * WPB;   // [LD][16] the tile, solved in place
  const double *pr = p.rec + (size_t)f * PREP_N;
  const double *Z = p.Z + (size_t)f * d * m, *Xs = p.Xs + (size_t)f * d * M;
  for (int row = lq; row < LD; row += 4)
    V[row * WPB + l15] = (row < m && colok) ? win_cov(kid, d, pr, Z + row, m, Xs + col, M, false) : 0.0;
  sparse_wave_sync();
  double s1 = 0.0, s2 = 0.0;
  // V = L^-1 V, block row by block row; the next L block is requested before this one's MFMAs
  auto solve = [&](const double *L, const double *dinv, bool second) {
    for (int I = 0; I < mt; ++I) {
      d4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = V[(I * WPB + lq + 4 * r) * WPB + l15];
      const double *Lr = L + (size_t)lq * LD + I * WPB + l15;
      double a[4], an[4];
      if (I > 0) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = Lr[(size_t)(4 * ks) * LD];
      }
      for (int K = 0; K < I; ++K) {
        if (K + 1 < I) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) an[ks] = Lr[(size_t)((K + 1) * WPB + 4 * ks) * LD];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[ks], V[(K * WPB + 4 * ks + lq) * WPB + l15], acc, 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = an[ks];
      }
      d4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double di = dinv[I * (WPB * WPB) + (lq + 4 * r) * WPB + l15];
        v = __builtin_amdgcn_mfma_f64_16x16x4f64(di, acc[r], v, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        V[(I * WPB + lq + 4 * r) * WPB + l15] = v[r];   // (the lane's own four elements of the block row)
        if (second) s2 = __builtin_fma(v[r], v[r], s2);
        else s1 = __builtin_fma(v[r], v[r], s1);
      }
      sparse_wave_sync();
    }
  };
  const double *U = p.U + (size_t)f * LD * LD, *B = p.F + (size_t)f * LD * LD;
  const double *dU = p.dinv + (size_t)f * 2 * mt * (WPB * WPB), *dB = dU + (size_t)mt * (WPB * WPB);
  solve(U, dU, false);
  solve(B, dB, true);
  // the four row groups of a column meet: a fixed order
  s1 += __shfl_xor(s1, 16);
  s1 += __shfl_xor(s1, 32);
  s2 += __shfl_xor(s2, 16);
  s2 += __shfl_xor(s2, 32);
  if (lq == 0 && colok) {
    const WaCov kc = WaCov::from_prep(kid, d, pr);
    double v = kc.kss(Xs[col]) - s1 + s2;
    v = v < 1e-15 ? 1e-15 : v;
    var[col] = p.include_noise ? v + pr[SP_R_NOISE] : v;
  }
  // mean = V2^T c, column by column from the finished tile: one fma chain down the lane's rows, as the rows were finished
  for (int q = 0; q < p.P; ++q) {
    const double *cvec = p.cm + (size_t)f * p.bcs + (size_t)q * LD;
    double mu = 0.0;
    for (int I = 0; I < mt; ++I) {
#pragma unroll
      for (int r = 0; r < 4; ++r) mu = __builtin_fma(V[(I * WPB + lq + 4 * r) * WPB + l15], cvec[I * WPB + lq + 4 * r], mu);
    }
    mu += __shfl_xor(mu, 16);
    mu += __shfl_xor(mu, 32);
    if (lq == 0 && colok) mean[(size_t)q * M + col] = mu;
  }
}

}  // namespace cgp
