// cgp_multi.hpp -- multi-target fits: P target columns of a fit share its factor (cgp_fit_predict_multi_batch[_device]).
//
//   Ky = L L^T      Z = L^-1 Y  (N x P)      V = L^-1 K(X, Xs)      mean = V^T Z  (P x M)      logml[p] = -1/2 |Z_p|^2 - sum log L_ii - N/2 log 2 pi
//
// After any tiled fit schedule everything but Z is resident: L in the factor panel, the images of W_k = L(k,k)^-1 in Winv, V^T as
// the panel's M extra rows (cgp_kernels.hpp).  The P targets are treated as P more extra rows of the trapezoid, kept in a scratch
// of their own -- the panel's layout, column-major over the samples: Zw[c ldz + p], ldz = P rounded up to 128, NT 128 columns:
//   k_multi_pack    Y (P, N) row-major -> Zw (transposed through LDS), zeros in the samples [N, NT 128) and the rows [P, ldz);
//                   column 0 also goes to the fit's y (the fit schedule wants one).
//   k_multi_solve   Z(t, k) = (Y(t, k) - sum_{j<k} Z(t, j) L(k, j)^T) W_k^T for k = 0 .. NT - 1, ONE launch, one workgroup per (fit,
//                   row tile t): a tile's rows depend on their own earlier block columns and on the finished L / W_k only, so there is
//                   no hand-off between workgroups and no flag.  The step is k_panel's for an extra tile with the Gram tile replaced
//                   by the stored right-hand side: 128-row form = load_tile (negated), mfma_rowpanel_loop, trmm_in_registers,
//                   store_tile; 64-row form (H64) = k_rows64's: a wave per 16 rows, its rows straight to registers, the column panel
//                   through a ring of four LDS-DMA slots.  Rows are independent and both forms add a row's products in the same
//                   order, so they agree bitwise per element; the host picks the form from (fits, P) only (multi_rows64).
//   k_multi_mean    mean(p, m) = sum_{c<N} Z(p, c) V^T(m, c): k_joint_cov's scheme on a rectangle.  One WAVE owns a 64 x 64 super-tile
//                   and runs the whole sum over c in column order, operands straight from the two slabs (for a fixed c both are
//                   contiguous runs of rows), the next 16 columns requested before this block's MFMAs, the last partial block of 16
//                   masked; the workgroups of a fit run on one XCD.
//   k_multi_logml   one workgroup per fit: sum log L_ii from the factor's diagonal (strided partial sums, one fixed tree), |Z_p|^2
//                   over the real N samples in sample order; NaN into var and logml of a fit whose info word is set.
// No atomics; every sum runs in a fixed order that does not involve p, P, the slot or the neighbours.  fp64 only.
#pragma once
#include "cgp_joint.hpp"

namespace cgp {

struct MultiArgs {
  const double *Lw;      // slab of the call's first fit
  size_t lw_stride;
  int ld;
  const double *Winv;    // W images of the call's first fit
  size_t winv_stride;
  double *Zw;            // [nfit][NT 128][ldz] right-hand sides / Z of the call's first fit
  size_t z_stride;
  int ldz;               // P rounded up to 128
  const double *Y;       // [nfit][P][N]
  double *y0;            // [nfit][N] column 0 for the fit schedule, or null
  double *mean;          // [nfit][P][M]
  double *var;           // [nfit][M] the fit's own variance: only touched (NaN) for a failed fit
  double *logml;         // [nfit][P]
  const int *info;       // [nfit]
  size_t row0;           // first extra row of the factor panel (NT 128)
  int N, M, P, NT, nfit;
  int stiles;            // k_multi_solve: row tiles per fit (of 128 or 64 rows)
  int pt, mt, nsm, npair, per_fit;   // k_multi_mean: tiles of 16 targets / test points, super-tiles along M, super-tiles, workgroups per fit
};

constexpr int MP_TILE = 32;
__global__ __launch_bounds__(MP_TILE * 8) void k_multi_pack(MultiArgs p) {
  __shared__ double t[MP_TILE][MP_TILE + 1];
  const int f = blockIdx.z, c0 = blockIdx.x * MP_TILE, p0 = blockIdx.y * MP_TILE;
  const int tx = threadIdx.x & (MP_TILE - 1), ty = threadIdx.x / MP_TILE;
  const double *Y = p.Y + (size_t)f * p.P * p.N;
#pragma unroll
  for (int i = 0; i < MP_TILE / 8; ++i) {
    const int pp = p0 + ty + 8 * i, c = c0 + tx;
    const double v = (pp < p.P && c < p.N) ? Y[(size_t)pp * p.N + c] : 0.0;
    t[ty + 8 * i][tx] = v;
    if (pp == 0 && p.y0 != nullptr && c < p.N) p.y0[(size_t)f * p.N + c] = v;
  }
  __syncthreads();
  double *Zf = p.Zw + (size_t)f * p.z_stride;
#pragma unroll
  for (int i = 0; i < MP_TILE / 8; ++i) Zf[(size_t)(c0 + ty + 8 * i) * p.ldz + p0 + tx] = t[tx][ty + 8 * i];   // (c0 + 32 <= NT 128, p0 + 32 <= ldz)
}

// One chunk of the 64-row form: r16_step (cgp_kernels_fused.hpp) without the running sums and with the dead-wave rule -- a wave
// whose 16 rows are all padding stages its share of the column panel and keeps the barriers, and issues no MFMA.
template <int S, bool ISSUE, int WAITN>
__device__ __forceinline__ void multi_r16_step(Prec<double>::acc_t (&acc)[NCB][1], double (&f)[4][KT / 4], const double *gRl, size_t ldR,
                                               const double *gC, size_t ldC, int c, double *smem, int lane, int wave, bool live) {
  using P = Prec<double>;
  constexpr int CH = KT * LDST;
  const int l15 = lane & 15, lq = lane >> 4;
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WAITN) : "memory");
#pragma unroll
  for (int ks = 0; ks < KT / 4; ++ks) asm volatile("" : "+v"(f[S][ks]));
  if constexpr (ISSUE) {
    cpanel_stage<double>(gC, ldC, c + 2, smem + ((S + 2) & 3) * CH, lane, wave);
    r16_load<double, (S + 2) & 3>(f, gRl, ldR, c + 2, lq);
  }
  if (!live) return;
  const double *cur = smem + S * CH + lq * LDST + l15;
  double fa[2][NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) fa[0][cb] = cur[cb * DB];
#pragma unroll
  for (int ks = 0; ks < KT / 4; ++ks) {
    if (ks + 1 < KT / 4) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) fa[(ks + 1) & 1][cb] = cur[(ks + 1) * 4 * LDST + cb * DB];
    }
    const double fb = f[S][ks];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = P::mfma(fa[ks & 1][cb], fb, acc[cb][0]);
  }
}

// What a step leaves for the next one.  Step k + 1 reads, as its row panel, the block column this workgroup stored at step k -- and
// the CU read the same lines at step k, as right-hand sides, so its vector L1 may still hold them as they were (a store does not
// update a line the L1 holds, and the LDS-DMA and straight-to-register loads of the loops go through that L1 like any other
// load).  Release at agent scope: the stores are in L2 before anyone passes the barrier; acquire at agent scope after it: this
// CU's L1 is invalidated before the next step's first load.  The barrier also ends the step's use of the W image in LDS.
// (k_sched / sched_run_tile hand tiles over inside a launch the same way, between workgroups.)
__device__ __forceinline__ void multi_step_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

template <bool H64>
__global__ __launch_bounds__(256, 2) void k_multi_solve(MultiArgs p) {
  using P = Prec<double>;
  using acc_t = P::acc_t;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double *smem = reinterpret_cast<double *>(smem_raw);
  // workgroup -> (fit, row tile): consecutive ids on ONE XCD, so a fit's tiles share its L and W_k in one L2
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nfit * p.stiles) return;
  const int f = lid / p.stiles, t = lid - f * p.stiles;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const double *Lf = p.Lw + (size_t)f * p.lw_stride;
  double *Zf = p.Zw + (size_t)f * p.z_stride;
  const int ld = p.ld, ldz = p.ldz, NT = p.NT;
  if constexpr (!H64) {
    FitArgs fa{};   // trmm_in_registers reads the W images through it, nothing else
    fa.Winv = const_cast<double *>(p.Winv);
    fa.winv_stride = p.winv_stride;
    double *Zt = Zf + (size_t)t * TS;
    acc_t acc[NCB][2];
    for (int k = 0; k < NT; ++k) {
      double *zk = Zt + (size_t)(k * TS) * ldz;
      load_tile<double, false>(acc, zk, ldz, tid);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        acc[cb][0] = -acc[cb][0];
        acc[cb][1] = -acc[cb][1];
      }
      mfma_rowpanel_loop<double, false>(acc, Zt, (size_t)ldz, Lf + (size_t)k * TS, (size_t)ld, k * (TS / KT), smem, tid);
      __syncthreads();   // every wave is done with the staged chunks before W_k overwrites them
      trmm_in_registers<double>(fa, acc, smem, f, k, tid);
      store_tile<double>(acc, zk, ldz, tid);
      if (k + 1 < NT) multi_step_handoff();
    }
  } else {
    constexpr int CH = KT * LDST, L = cpanel_loads<double>() + KT / 4;
    const int row0 = t * HR + wave * DB;      // this wave's 16 rows
    const bool live = row0 < p.P;             // (wave-uniform) rows [P, ldz) are padding: zeros, left as packed
    double *gRl = Zf + row0 + l15;
    acc_t acc[NCB][1];
    double rf[4][KT / 4];
    for (int k = 0; k < NT; ++k) {
      double *zk = gRl + (size_t)(k * TS) * ldz;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[cb][0][r] = -zk[(size_t)(cb * DB + P::drow(lane, r)) * ldz];
      const int nchunk = k * (TS / KT);
      const double *gC = Lf + (size_t)k * TS;
      if (nchunk > 0) {   // (then nchunk >= 8)
        cpanel_stage<double>(gC, (size_t)ld, 0, smem, lane, wave);
        r16_load<double, 0>(rf, gRl, (size_t)ldz, 0, lq);
        cpanel_stage<double>(gC, (size_t)ld, 1, smem + CH, lane, wave);
        r16_load<double, 1>(rf, gRl, (size_t)ldz, 1, lq);
        int c = 0;
        for (; c + 4 < nchunk; c += 4) {
          multi_r16_step<0, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c, smem, lane, wave, live);
          multi_r16_step<1, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 1, smem, lane, wave, live);
          multi_r16_step<2, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 2, smem, lane, wave, live);
          multi_r16_step<3, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 3, smem, lane, wave, live);
        }
        multi_r16_step<0, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c, smem, lane, wave, live);
        multi_r16_step<1, true, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 1, smem, lane, wave, live);
        multi_r16_step<2, false, L>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 2, smem, lane, wave, live);
        multi_r16_step<3, false, 0>(acc, rf, gRl, (size_t)ldz, gC, (size_t)ld, c + 3, smem, lane, wave, live);
      }
      __syncthreads();   // every wave is done with the staged chunks before W_k overwrites them
      // Z(:, k) = S W_k^T in registers (trmm_in_registers with one row block per wave, as k_rows64)
      const double *__restrict__ Wk = p.Winv + (size_t)f * p.winv_stride + (size_t)k * WIMG;
      {
        typedef __attribute__((address_space(3))) void lds_void;
        typedef const __attribute__((address_space(1))) void gbl_void;
        constexpr int PER = 1024 / (int)sizeof(double), NI = WIMG / PER / 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int off = (i * 4 + wave) * PER;
          __builtin_amdgcn_global_load_lds((gbl_void *)(Wk + off + lane * 2), (lds_void *)(smem + off), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
      if (live) {
#pragma unroll
        for (int cb = NCB - 1; cb >= 0; --cb) {
          acc_t t0 = acc_t{0, 0, 0, 0};
          const double *wrow = smem + (cb * (cb + 1) / 2) * DB * DB + l15;
#pragma unroll
          for (int qb = 0; qb <= cb; ++qb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) t0 = P::mfma(wrow[qb * DB * DB + P::drow(lane, r) * DB], acc[qb][0][r], t0);
          }
          acc[cb][0] = t0;
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) zk[(size_t)(cb * DB + P::drow(lane, r)) * ldz] = acc[cb][0][r];
      }
      if (k + 1 < NT) multi_step_handoff();
    }
  }
}

__global__ __launch_bounds__(WJ_THREADS) void k_multi_mean(MultiArgs p) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  // workgroup -> (fit, group of super-tiles): consecutive ids on ONE XCD
  const int per = gridDim.x / WF_XCDS;
  const int lid = (blockIdx.x % WF_XCDS) * per + blockIdx.x / WF_XCDS;
  if (lid >= p.nfit * p.per_fit) return;
  const int f = lid / p.per_fit;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int st = (lid - f * p.per_fit) * WJ_WAVES + wave;
  if (st >= p.npair) return;
  const int BP = st / p.nsm, BM = st - BP * p.nsm;
  const int M = p.M, N = p.N, Pn = p.P, mt = p.mt, pt = p.pt;
  const bool bad = p.info[f] != 0;
  // tile (b, a): targets j = (BP 4 + b) 16 + lq + 4 r (A operand), test points i = (BM 4 + a) 16 + l15 (B operand)
  auto live = [&](int b, int a) { return BP * WJ_ST + b < pt && BM * WJ_ST + a < mt; };
  d4 acc[WJ_ST][WJ_ST];
#pragma unroll
  for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) acc[b][a] = d4{0, 0, 0, 0};
  // operands of column block kb: lane (l15, lq) holds Z[tile 16 + l15][kb 16 + 4 ks + lq] and V^T[tile 16 + l15][the same].  A tile
  // index past the last one is clamped to it (its products are never stored); the rows a last tile has beyond P are zeros inside
  // the scratch, those beyond M the y row and the panel's padding inside the slab: they reach only entries that are not stored.
  const double *Zl = p.Zw + (size_t)f * p.z_stride + (size_t)lq * p.ldz + l15;
  const double *Vl = p.Lw + (size_t)f * p.lw_stride + p.row0 + (size_t)lq * p.ld + l15;
  const double *za[WJ_ST], *vb[WJ_ST];
#pragma unroll
  for (int t = 0; t < WJ_ST; ++t) {
    const int tj = BP * WJ_ST + t < pt ? BP * WJ_ST + t : pt - 1, ti = BM * WJ_ST + t < mt ? BM * WJ_ST + t : mt - 1;
    za[t] = Zl + tj * WPB;
    vb[t] = Vl + ti * WPB;
  }
  const size_t ld = p.ld, ldz = p.ldz;
  auto load = [&](int kb, double (&fa)[WJ_ST][4], double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = za[t][(size_t)(kb * WPB + 4 * ks) * ldz];
        fb[t][ks] = vb[t][(size_t)(kb * WPB + 4 * ks) * ld];
      }
  };
  auto mac = [&](const double (&fa)[WJ_ST][4], const double (&fb)[WJ_ST][4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
        for (int a = 0; a < WJ_ST; ++a)
          if (live(b, a)) acc[b][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[b][ks], fb[a][ks], acc[b][a], 0, 0, 0);
  };
  const int nfull = bad ? 0 : N / WPB;
  double fa[WJ_ST][4], fb[WJ_ST][4], ga[WJ_ST][4], gb[WJ_ST][4];
  if (nfull > 0) load(0, fa, fb);
  for (int kb = 0; kb < nfull; ++kb) {
    if (kb + 1 < nfull) load(kb + 1, ga, gb);
    mac(fa, fb);
#pragma unroll
    for (int t = 0; t < WJ_ST; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa[t][ks] = ga[t][ks];
        fb[t][ks] = gb[t][ks];
      }
  }
  if (!bad && nfull * WPB < N) {   // the last columns, N not a multiple of 16: the samples from N on are not summed
    load(nfull, fa, fb);           // (inside both slabs: their NT 128 columns cover the block)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bool in = nfull * WPB + 4 * ks + lq < N;
#pragma unroll
      for (int t = 0; t < WJ_ST; ++t) {
        fa[t][ks] = in ? fa[t][ks] : 0.0;
        fb[t][ks] = in ? fb[t][ks] : 0.0;
      }
    }
    mac(fa, fb);
  }
  double *mf = p.mean + (size_t)f * Pn * M;
#pragma unroll
  for (int b = 0; b < WJ_ST; ++b)
#pragma unroll
    for (int a = 0; a < WJ_ST; ++a) {
      if (!live(b, a)) continue;
      const int i = (BM * WJ_ST + a) * WPB + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = (BP * WJ_ST + b) * WPB + lq + 4 * r;
        if (i < M && j < Pn) mf[(size_t)j * M + i] = bad ? __builtin_nan("") : acc[b][a][r];
      }
    }
}

constexpr int ML_THREADS = 256;
__global__ __launch_bounds__(ML_THREADS) void k_multi_logml(MultiArgs p) {
  __shared__ double red[ML_THREADS];
  const int f = blockIdx.x, tid = threadIdx.x, N = p.N;
  const bool bad = p.info[f] != 0;
  const double *Lf = p.Lw + (size_t)f * p.lw_stride;
  // sum log L_ii from the factor's diagonal: thread t takes i = t, t + 256, ... in order, then one fixed tree over the 256 sums
  double s = 0.0;
  for (int i = tid; i < N; i += ML_THREADS) s += log(Lf[(size_t)i * p.ld + i]);
  red[tid] = s;
  __syncthreads();
  for (int o = ML_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double sumlog = red[0];
  const double *Zf = p.Zw + (size_t)f * p.z_stride;
  for (int pp = tid; pp < p.P; pp += ML_THREADS) {
    double zz = 0.0;
#pragma unroll 8
    for (int c = 0; c < N; ++c) {
      const double z = Zf[(size_t)c * p.ldz + pp];
      zz = __builtin_fma(z, z, zz);
    }
    p.logml[(size_t)f * p.P + pp] = bad ? __builtin_nan("") : -0.5 * zz - sumlog - 0.5 * N * 1.8378770664093453;   // log 2 pi
  }
  if (bad)
    for (int m = tid; m < p.M; m += ML_THREADS) p.var[(size_t)f * p.M + m] = __builtin_nan("");
}

}  // namespace cgp
