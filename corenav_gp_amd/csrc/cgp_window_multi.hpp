// cgp_window_multi.hpp -- multi-target sliding windows: P target columns share a window's resident factor
// (cgp_window_multi_reserve, cgp_window_push_multi, cgp_window_predict_multi).
//
// Nothing in a window's state depends on the target except z: the factor L, the inputs and the diagonal blocks' inverses serve
// every column, and so do the forecast's V = L^-1 K* and its variance.  The push kernels (cgp_window.hpp) keep z for ONE target
// inside a hand-scheduled sweep and are left exactly as they are: column 0 goes through them, and all P columns are kept in a
// target store from which Z = L^-1 Y is formed when a forecast asks for it, from the factor as it stands (so a forecast after
// cgp_window_set_theta / cgp_window_optimize is right for every column with no further call).
//
//   k_window_targets_store   one workgroup per window, in front of a push's launches: the T x P incoming targets into the store
//                            -- a circular buffer [nwin][P][N], tick t at index t mod N, no compaction: sample i of a window of
//                            n samples, oldest first, is tick `ticks - n + i` -- and column 0 gathered into a contiguous
//                            [nwin][T] block for the push kernels.  The tick count (mod N) is a word of the store's own, kept on
//                            the device, so the device entry needs no host state and does not lean on the windows' state words.
//                            Plain vector stores, no atomics.
//   k_window_multi_z         Z = L^-1 Y per window x chunk of target columns: the WM_Z form of k_window_forecast
//                            (cgp_window_forecast.hpp) -- the forecast's left-looking block step on v_mfma_f64_16x16x4_f64, the
//                            kernel's own code, with the start tile read from the target store instead of evaluated as K*.  Every
//                            finished block goes to the Z scratch in the B-operand order [tile][row][16] (the KEEP form's store);
//                            padded columns and the rows past n of the last block are zeros.  Its tail writes
//                            logml[p] = -1/2 sum_i Z[i,p]^2 - sum_i log L_ii - n/2 log 2 pi, the diagonal read in a fixed order.
//   the WM_MEAN form         the forecast's solve, then the P mean rows as an epilogue (the structure of the GRAD form's second
//                            phase): at that point the solve's accumulators are dead and the chunk's whole V is in LDS.
//                            mean(16 targets x chunk points) = Z^T V per target tile: the operand reads are those of
//                            "A = V^T, B = Z" (the lanes of a k-step read 64 consecutive doubles of Z from the scratch -- L2 hits,
//                            a window's chunks share an XCD -- and the forward pass's conflict-free 64 of V from LDS), taken the
//                            other way round so that a lane group's sixteen results are consecutive test points of one mean row.
//                            The rows are split over the waves of a column tile in fixed ranges (blocks jq, jq + SPLIT, ...), the
//                            partial tiles meet in the forecast's partial-tile area in wave order; only the window's real blocks
//                            are summed.  var is the forecast's own code and arithmetic.
// A column's mean row and logml depend on its own targets, the window and N (which picks the form) only: an MFMA's result
// element is a function of its own operand row and column, every sum runs in a fixed order, there are no atomics.
#pragma once
#include "cgp_window_forecast.hpp"

namespace cgp {

constexpr int WM_MAX_P = 64;

// Z = L^-1 Y: no covariance is evaluated, so one instantiation per form serves every kernel id
template <int NCT, int VW> constexpr auto k_window_multi_z = k_window_forecast<NCT, VW, false, false, false, WM_Z>;

struct TargetStoreArgs {
  const double *Ys;   // [nwin][T][P] the push's targets
  double *ystore;     // [nwin][P][N]
  int *ycount;        // [nwin] ticks stored so far, mod N
  double *y0;         // [nwin][T] column 0, for the push kernels
  int N, P, T;
};

__global__ __launch_bounds__(256) void k_window_targets_store(TargetStoreArgs p) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const int c = p.ycount[w];
  __syncthreads();   // every thread has the count before thread 0 replaces it
  const size_t TP = (size_t)p.T * p.P;
  const double *src = p.Ys + (size_t)w * TP;
  double *dst = p.ystore + (size_t)w * p.P * p.N;
  const int first = p.T > p.N ? p.T - p.N : 0;   // of a push longer than the window only the last N ticks stay (one writer per slot)
  for (size_t idx = tid; idx < TP; idx += 256) {
    const int t = (int)(idx / p.P), col = (int)(idx - (size_t)t * p.P);
    const double v = src[idx];
    if (t >= first) dst[(size_t)col * p.N + (int)(((long long)c + t) % p.N)] = v;
    if (col == 0) p.y0[(size_t)w * p.T + t] = v;
  }
  if (tid == 0) p.ycount[w] = (int)(((long long)c + p.T) % p.N);
}

// target `col` of sample `row` (oldest first) of a window of n samples
__device__ __forceinline__ double window_multi_target(const ForecastArgs &p, int w, int col, int n, int row) {
  int t = p.ycount[w] - n + row;   // in (-N, N)
  t = t < 0 ? t + p.N : t;
  return p.ystore[((size_t)w * p.P + col) * p.N + t];
}

// a failed (NaN) or empty (prior) window, called by the lane of test point / target column `col`
template <int MULTI> __device__ __forceinline__ void window_multi_prior(const ForecastArgs &p, int w, int col, bool bad, double prior_var) {
  const double nan = __builtin_nan("");
  if constexpr (MULTI == WM_Z) {
    if (p.mlogml) p.mlogml[(size_t)w * p.P + col] = bad ? nan : 0.0;
  } else {
    for (int t = 0; t < p.P; ++t) p.mean[((size_t)w * p.P + t) * p.M + col] = bad ? nan : 0.0;
    p.var[(size_t)w * p.M + col] = bad ? nan : prior_var;
  }
}

// logml[p] from the finished solve, called by all 512 threads: sv2 = sum_i Z[i,p]^2 in the tile's solver wave (jq == 0), summed
// as the forecast sums V^2; `writer` names the one lane that stores column `col`.
// sum_i log L_ii: thread t takes the rows t, t + 512, ..., the lanes of a wave meet by six shuffles, the waves in `red` in wave
// order (`red` is free: the loop's last barrier).
__device__ __forceinline__ void window_multi_z_tail(const ForecastArgs &p, double *red, const double *L, int w, int col, bool writer,
                                                    int n, double sv2) {
  if (!p.mlogml) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0;
  for (int i = tid; i < n; i += WF_THREADS) s += log(L[(size_t)i * p.CAP + i]);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (writer) {   // the first lane group of the column's solver wave
    double slog = red[0];
#pragma unroll
    for (int q = 1; q < WF_WAVES; ++q) slog += red[q];
    p.mlogml[(size_t)w * p.P + col] = -0.5 * sv2 - slog - 0.5 * (double)n * 1.8378770664093453;
  }
}

template <int NCT, int VW>
__device__ __forceinline__ void window_multi_mean_tail(const ForecastArgs &p, const double *V, double *red, int w, int ch, int n, int nb) {
  constexpr int SPLIT = WF_WAVES / NCT, MC = NCT * VW;
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = wave % NCT, jq = wave / NCT;
  const int nrow = p.NB * WPB;
  const double *Vt = V + (size_t)ct * nrow * VW;
  const bool vok = VW == 16 || l15 < VW;
  const int col = ch * MC + ct * VW + l15;
  const bool colok = vok && col < p.M;
  for (int tt = 0; tt < p.pt; ++tt) {
    const double *Zt = p.zs + ((size_t)w * p.pt + tt) * nrow * WPB;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    // A = Z^T: lane (l15, lq) holds target l15, row 4 ks + lq of the block; B = V: row 4 ks + lq, test point l15
    for (int blk = jq; blk < nb; blk += SPLIT) {
      const double *za = Zt + (size_t)(blk * WPB + lq) * WPB + l15;
      const double *vb = Vt + (size_t)(blk * WPB + lq) * VW + l15;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double b = vok ? vb[4 * ks * VW] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(za[4 * ks * WPB], b, acc, 0, 0, 0);
      }
    }
    if (jq != 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (jq == 0) {   // register r: target lq + 4 r of the tile, test point l15
#pragma unroll
      for (int q = 1; q < SPLIT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += red[((ct + NCT * q) * 4 + r) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tg = tt * WPB + lq + 4 * r;
        if (colok && tg < p.P) p.mean[((size_t)w * p.P + tg) * p.M + col] = acc[r];
      }
    }
    __syncthreads();   // `red` is rewritten by the next target tile
  }
}

}  // namespace cgp
