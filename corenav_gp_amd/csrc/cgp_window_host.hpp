// cgp_window_host.hpp -- host layer of the sliding windows: the cgp_window_* entry points of include/corenav_gp.h.  The kernels
// are in cgp_window.hpp (push), cgp_window_forecast.hpp, cgp_window_pgrad.hpp, cgp_window_multi.hpp, cgp_window_multi_grad.hpp, cgp_window_adapt.hpp and cgp_window_joint.hpp.  Not a translation unit
// of its own: cgp_engine.hip includes it after cgp_ctx (whose WinBufs ... WinLooGradBufs records hold the windows' device buffers)
// and the helpers it uses (hip_ok / HIP_TRY, grow_pinned, grow_device, pick_stream, cdiv, xcd_grid, ntheta).
#pragma once

namespace {

#ifndef CGP_WIN_PAIRS
#define CGP_WIN_PAIRS 1   // sliding window: steady-state ticks two per pass over the factor (`make variant`: 0 = every tick on its own)
#endif
constexpr bool kWinPairs = CGP_WIN_PAIRS != 0;
constexpr size_t kWinZeroCopyBytes = 16 * 1024;   // cgp_window_push blocks up to this size are read / written in pinned host memory by the kernels
constexpr int kWinPackLds = 72 * 1024;       // pack windows into a workgroup only while two workgroups still fit a CU's LDS ...
#ifndef CGP_WIN_MULTI
#define CGP_WIN_MULTI 4   // steady-state ticks per pass over the factor where the window is long enough (k_window_multi); 0 = pairs only
#endif
constexpr int kWinMulti = CGP_WIN_MULTI > 2 ? CGP_WIN_MULTI : 4;
constexpr bool kWinUseMulti = CGP_WIN_MULTI > 2;
constexpr int kWinMultiMinWindows = 512;
constexpr size_t kWinPairStage = 3 * WPB * 64 * sizeof(double);   // k_window_pairs: the three sweep waves' staged trips (24 KB)
constexpr int kWinPackMinGroups = 512;
constexpr int kWinWideMax = 256;            // single-tick kernel: up to this many windows 512 threads per window       // ... and the chip still gets two workgroups per CU
#ifndef CGP_WIN_CAP_PAD
#define CGP_WIN_CAP_PAD 0   // `make variant`: leading dimension of the windows' slabs beyond 2 N (measured: no effect)
#endif
// the forecast and the refactorisation come in three forms, by the window length alone: the largest N of each
constexpr int kWinClassMaxN[3] = {512, 1024, 2048};

// Which instantiation serves a window: the launches and cgp_window_init's LDS limits both ask here.
// LDS of a k_window_pairs workgroup of wpw windows: the two-ticks-per-pass kernel keeps six window-length vectors per window
// (98 KB at N = 2048), and the sweep waves' staged trips
inline size_t pairs_lds(int N, int wpw) {
  return wpw * (size_t)(6 * ((N + 3) & ~1) + 16 * WPB + 2 * MAXD + 16) * sizeof(double) + kWinPairStage;
}
constexpr int kWinPushLdsMax = 150 * 1024;   // the limit of k_window_pairs and k_window_multi
template <bool MAT> auto pairs_kernel_of(int wpw) {
  return wpw == 4 ? k_window_pairs<4, MAT> : wpw == 2 ? k_window_pairs<2, MAT> : k_window_pairs<1, MAT>;
}
inline auto pairs_kernel(int wpw, bool matern) { return matern ? pairs_kernel_of<true>(wpw) : pairs_kernel_of<false>(wpw); }

// LDS of a k_window_multi workgroup: three vectors per tick of the pass, the ticks' column blocks and the sweep waves' staged trips
inline size_t multi_lds(int N) {
  const int NSm = (N + kWinMulti + 3) & ~1;
  return (size_t)(3 * kWinMulti * NSm + kWinMulti * (8 * WPB + MAXD + 8)) * sizeof(double) + kWinPairStage;
}

// The T ticks of a push are cut into launches: runs of steady-state ticks (full windows, no ring compaction inside) go two per
// pass over the factor (k_window_pairs) or four (k_window_multi), everything else -- filling, the tick that compacts the ring, an
// odd one out -- through the single-tick kernel.  Origin o and size n of the windows are deterministic and identical for every
// window of the context, so the host mirrors them instead of reading them back: they come in as they stand before the push and
// leave as they stand after it.  emit(kind, arg, t0, nt) is called once per launch, in order: kind CGP_PLAN_*, arg the windows per
// workgroup (pairs), the ticks per pass (multi) or the threads per window (ticks), [t0, t0 + nt) the ticks.  cgp_window_push
// launches from it and cgp_debug_window_plan records it: the choices below are made here and nowhere else.
template <class Emit> void window_cut(int nwin, int N, int CAP, int T, int &o, int &n, Emit &&emit) {
  // windows per workgroup of the paired kernel (rows of wave 0 per window: 4 / wpw)
  // measured (tools/r3_winpack.sh, N = 512): 1024 windows 2.20 / 2.65 / 2.03 M ticks/s at 1 / 2 / 4 per workgroup, 512 windows
  // 2.18 / 1.81 / 1.20 -- two per workgroup once that still leaves two workgroups per CU, four never
  int wpw = 1;
  if (nwin % 2 == 0 && pairs_lds(N, 2) <= (size_t)kWinPackLds + 8 * 1024 && nwin / 2 >= kWinPackMinGroups) wpw = 2;
  // threads per window of the single-tick kernel: with no more windows than CUs a workgroup sweeps with seven waves instead of
  // three (1024 threads: 128 VGPRs per lane, the serial wave spills -- 251 us per host tick against 117)
  int wth = nwin <= kWinWideMax ? 512 : 256;
  if constexpr (kAbBuild) {
    const char *e = getenv("CGP_WIN_WPW");
    int v = e ? atoi(e) : 0;
    if ((v == 1 || v == 2 || v == 4) && nwin % v == 0 && pairs_lds(N, v) <= (size_t)kWinPushLdsMax) wpw = v;
    e = getenv("CGP_WIN_THREADS");
    v = e ? atoi(e) : 0;
    if (v == 256 || v == 512) wth = v;
  }
  auto one_tick = [&](int &oo, int &nn) {   // k_window_ticks, one tick
    if (oo + nn >= CAP) oo = 0;
    const bool drop = nn >= N;
    oo = drop ? oo + 1 : oo;
    nn = (drop ? nn - 1 : nn) + 1;
  };
  auto pair_ok = [&](int oo, int nn, int left) { return kWinPairs && N >= 2 * WPB && nn == N && left >= 2 && oo + N + 1 < CAP; };
  const size_t ldsm = multi_lds(N);
  auto multi_ok = [&](int oo, int nn, int left) {
    // (measured, N = 512: 512 windows 3.99 M ticks/s against 3.54 M two per pass, 1 024 windows 3.97 against 3.41; 256 windows 2.92 against 3.38 --
    // one window per workgroup leaves half of a small call's lanes idle: from kWinMultiMinWindows windows)
    return kWinUseMulti && kWinPairs && nwin >= kWinMultiMinWindows && N >= 4 * WPB && ldsm <= 80 * 1024 && nn == N && left >= kWinMulti &&
           oo + N + kWinMulti - 1 < CAP;
  };
  for (int t = 0; t < T;) {
    int nm = 0;
    for (int oo = o; multi_ok(oo, n, T - t - kWinMulti * nm); oo += kWinMulti) ++nm;
    if (nm > 0) {
      emit(CGP_PLAN_MULTI, kWinMulti, t, kWinMulti * nm);
      o += kWinMulti * nm;
      t += kWinMulti * nm;
      continue;
    }
    int np = 0;
    for (int oo = o; pair_ok(oo, n, T - t - 2 * np); oo += 2) ++np;
    if (np > 0) {
      emit(CGP_PLAN_PAIRS, wpw, t, 2 * np);
      o += 2 * np;
      t += 2 * np;
      continue;
    }
    int ns = 0;
    do {
      one_tick(o, n);
      ++ns;
    } while (t + ns < T && !pair_ok(o, n, T - t - ns));
    emit(CGP_PLAN_TICKS, wth, t, ns);
    t += ns;
  }
}

template <bool MAT> auto refactor_kernel_of(int N) {   // accumulators per wave: 4 / 8 / 16
  return N <= kWinClassMaxN[0] ? k_window_refactor<4, MAT> : N <= kWinClassMaxN[1] ? k_window_refactor<8, MAT> : k_window_refactor<16, MAT>;
}
inline auto refactor_kernel(int N, bool matern) { return matern ? refactor_kernel_of<true>(N) : refactor_kernel_of<false>(N); }

struct ForecastForm {
  void (*kernel)(ForecastArgs);
  int mc;           // test points per workgroup (NCT * VW)
  size_t lds = 0;   // of a launch: the chunk's V + the waves' partial tiles
};
// the forecast keeps a chunk's V = L^-1 K* in LDS: 128 KB + the waves' partial tiles in every form (cgp_window_forecast.hpp)
constexpr int kWinForecastLdsMax = 160 * 1024;
template <bool KEEP, bool MAT> ForecastForm forecast_form_of(int N) {
  if (N <= kWinClassMaxN[0]) return {k_window_forecast<2, 16, KEEP, MAT>, 32};
  if (N <= kWinClassMaxN[1]) return {k_window_forecast<1, 16, KEEP, MAT>, 16};
  return {k_window_forecast<1, 8, KEEP, MAT>, 8};
}
// keep: the same solve with V kept for the joint forecast (cgp_window_joint.hpp)
inline ForecastForm forecast_form(int N, bool keep, bool matern) {
  ForecastForm f = keep ? (matern ? forecast_form_of<true, true>(N) : forecast_form_of<true, false>(N))
                        : (matern ? forecast_form_of<false, true>(N) : forecast_form_of<false, false>(N));
  f.lds = ((size_t)cdiv(N, WPB) * WPB * f.mc + WF_WAVES * 256) * sizeof(double);
  return f;
}

// the gradient form of the forecast (cgp_window_pgrad.hpp): the forecast's forms (KEEP = false), chunk widths and LDS
template <bool MAT> ForecastForm pgrad_win_form_of(int N) {
  if (N <= kWinClassMaxN[0]) return {k_window_forecast<2, 16, false, MAT, true>, 32};
  if (N <= kWinClassMaxN[1]) return {k_window_forecast<1, 16, false, MAT, true>, 16};
  return {k_window_forecast<1, 8, false, MAT, true>, 8};
}
inline ForecastForm pgrad_win_form(int N, bool matern) {
  ForecastForm f = matern ? pgrad_win_form_of<true>(N) : pgrad_win_form_of<false>(N);
  f.lds = forecast_form(N, false, matern).lds;
  return f;
}

// the multi-target forms (cgp_window_multi.hpp): the forecast's forms (KEEP = false), chunk widths and LDS.  z = true: Z = L^-1 Y
// (k_window_multi_z: no covariance is evaluated, one instantiation serves every kernel id); else the forecast with P mean rows
template <bool MAT> ForecastForm multi_win_form_of(int N) {
  if (N <= kWinClassMaxN[0]) return {k_window_forecast<2, 16, false, MAT, false, WM_MEAN>, 32};
  if (N <= kWinClassMaxN[1]) return {k_window_forecast<1, 16, false, MAT, false, WM_MEAN>, 16};
  return {k_window_forecast<1, 8, false, MAT, false, WM_MEAN>, 8};
}
inline ForecastForm multi_win_form(int N, bool z, bool matern) {
  ForecastForm f;
  if (z) {
    if (N <= kWinClassMaxN[0]) f = {k_window_multi_z<2, 16>, 32};
    else if (N <= kWinClassMaxN[1]) f = {k_window_multi_z<1, 16>, 16};
    else f = {k_window_multi_z<1, 8>, 8};
  } else {
    f = matern ? multi_win_form_of<true>(N) : multi_win_form_of<false>(N);
  }
  f.lds = forecast_form(N, false, matern).lds;
  return f;
}

// A kernel's view of the resident windows: the fields that do not depend on the call.
ForecastArgs forecast_args(cgp_ctx *c) {
  const WindowArgs &wa = c->win;
  ForecastArgs a{};
  a.L = wa.L; a.z = wa.z; a.xw = wa.xw; a.state = wa.state; a.prep = wa.prep; a.theta = wa.theta;
  a.dinv = c->wb.dinv;
  a.N = wa.N; a.CAP = wa.CAP; a.d = wa.d; a.kernel_id = wa.kernel_id; a.nwin = c->nwin;
  a.NB = cdiv(wa.N, WPB);
  return a;
}
JointArgs joint_args(cgp_ctx *c) {   // with the scratch of cgp_window_joint_reserve
  const WindowArgs &wa = c->win;
  JointArgs j{};
  j.state = wa.state; j.prep = wa.prep; j.theta = wa.theta;
  j.V = c->wj.V;
  j.C = c->wj.C;
  j.jinfo = c->wj.jinfo;
  j.d = wa.d; j.kernel_id = wa.kernel_id; j.nwin = c->nwin;
  j.nrow = cdiv(wa.N, WPB) * WPB;
  return j;
}
AdaptArgs adapt_args(cgp_ctx *c) {
  const WindowArgs &wa = c->win;
  AdaptArgs a{};
  a.L = wa.L; a.z = wa.z; a.xw = wa.xw; a.yw = wa.yw; a.state = wa.state;
  a.prep = const_cast<double *>(wa.prep);
  a.theta = const_cast<double *>(wa.theta);
  a.N = wa.N; a.CAP = wa.CAP; a.d = wa.d; a.kernel_id = wa.kernel_id; a.nwin = c->nwin;
  a.NB = cdiv(wa.N, WPB);
  a.dinv = c->wb.dinv;
  a.alpha = c->wb.grad_scratch;   // alpha | chunk sums | values
  a.gpart = a.alpha + (size_t)c->nwin * a.NB * WPB;
  a.nllv = a.gpart + (size_t)c->nwin * a.NB * GRAD_N;
  // the multi-target objective (null / 0 without its reservations)
  a.zs = c->wm.zs;
  a.am = c->wg.am;
  a.P = c->wm.P;
  a.pt = cdiv(c->wm.P, WPB);
  return a;
}
// k_window_multi_z's view: Z = L^-1 Y of the reservation's P columns into the Z scratch, with the columns' logml to mlogml (or
// null).  The targets take the test points' place: M = P, the chunks are zf's.
ForecastArgs multi_z_args(cgp_ctx *c, const ForecastForm &zf, double *mlogml) {
  ForecastArgs za = forecast_args(c);
  za.ystore = c->wm.ystore; za.ycount = c->wm.ycount; za.zs = c->wm.zs;
  za.P = c->wm.P;
  za.pt = cdiv(c->wm.P, WPB);
  za.M = c->wm.P;
  za.nchunk = cdiv(c->wm.P, zf.mc);
  za.mlogml = mlogml;
  return za;
}

// ---- launches several entry points share.  They enqueue and check nothing: every limit of a call is checked by the call, before
// its first launch, with fits_grid (a plain grid) or the engine's xcd_grid (a grid rounded up to the XCDs) ----------------------
inline bool fits_grid(long long workgroups) { return workgroups <= (1ll << 30); }
inline long long diag_inv_groups(const cgp_ctx *c) { return (long long)cdiv(cdiv(c->win.N, WPB), 4) * c->nwin; }   // four blocks per workgroup
inline long long window_chunks(const cgp_ctx *c) { return (long long)c->nwin * cdiv(c->win.N, WPB); }              // four per workgroup of 256
// the inverses of the factors' diagonal blocks (the kernel reads the windows and writes the inverses only)
void launch_diag_inv(cgp_ctx *c, hipStream_t ws) {
  hipLaunchKernelGGL(k_window_diag_inv, dim3((unsigned)diag_inv_groups(c)), dim3(64), 0, ws, forecast_args(c));
}
// ... and alpha = L^-T z into the gradient's scratch
void launch_alpha(cgp_ctx *c, const AdaptArgs &a, hipStream_t ws) {
  launch_diag_inv(c, ws);
  hipLaunchKernelGGL(k_window_alpha, dim3(c->nwin), dim3(256), (size_t)a.NB * WPB * sizeof(double), ws, a);
}
// ... and the leave-one-out pass with its finish
void launch_loo(cgp_ctx *c, const AdaptArgs &a, const WindowLooOut &out, hipStream_t ws) {
  launch_alpha(c, a, ws);
  hipLaunchKernelGGL(k_window_loo, dim3((unsigned)((window_chunks(c) + 3) / 4)), dim3(256), 0, ws, a, out);
  hipLaunchKernelGGL(k_window_loo_finish, dim3(c->nwin), dim3(64), 0, ws, a, out);
}
// every instantiation a launch can pick gets its LDS limit in cgp_window_init / cgp_window_multi_reserve only: the _device entry
// points make no attribute call (they are captured into graphs)
template <class K> bool lds_limit(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}

// The host entry points stage through one pinned block and its device twin, which live in the context, grown on demand and kept.
// (the pinned block is never smaller than the largest push the kernels access in place: a block that was freed and allocated again
// between two small pushes -- the first pushes of a stream grow -- is what round 6's sweep caught under load, fourteen processes on
// the GPU: about one push in a hundred came back with its outputs untouched, the kernel's stores having gone to the pages of the
// block just freed.  One allocation for the context's lifetime takes the window out of that path.)
bool window_stage(cgp_ctx *c, size_t pinned_bytes, size_t device_bytes, double *&h, double *&d) {
  if (!grow_pinned(c->win_pin, c->win_pin_cap, std::max(pinned_bytes, kWinZeroCopyBytes)) || !grow_device(c->win_dev, c->win_dev_cap, device_bytes))
    return false;
  h = static_cast<double *>(c->win_pin);
  d = static_cast<double *>(c->win_dev);
  return true;
}
// the windows' [nwin][4] state words to hst behind the work of s, and the call's one synchronisation
int window_read_state(cgp_ctx *c, int *hst, hipStream_t s) {
  HIP_TRY(c, hipMemcpyAsync(hst, c->win.state, (size_t)c->nwin * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CGP_OK;
}
// what a push or a forecast returns: the first failing tick of the first failed window, from status words `stride` ints apart --
// word 2 of the state words (stride 4), or the [nwin] copy of it the push kernels write for the host (WindowArgs::info_out)
inline int first_failing_tick(const int *status, size_t W, size_t stride) {
  for (size_t w = 0; w < W; ++w)
    if (status[w * stride] != 0) return status[w * stride];
  return CGP_OK;
}
// what the calls with an [nwin] info array return: w + 1 of the first window whose word is set
inline int first_flagged_window(const int *info, size_t W) {
  for (size_t w = 0; w < W; ++w)
    if (info[w] != 0) return (int)w + 1;
  return CGP_OK;
}

// What the host forms of the forecasts and of the multi-target push share, after their checks: one pinned block [nin doubles of
// inputs | nout of outputs | state words] and its device twin; fill(h) stages the inputs, run(io, stream) is the device form on
// the block at io, of whose outputs the first nback come back.  zero_copy: a block of up to kWinZeroCopyBytes is read and
// written in place by the kernels (no copy command); else one H2D and two D2H (outputs, state words), one synchronisation.
// Returns a negative code, or what first_failing_tick says with the outputs at h + nin for the caller to hand out.
template <class Fill, class Run>
int window_staged_call(cgp_ctx *c, size_t nin, size_t nout, size_t nback, bool zero_copy, double *&h, Fill &&fill, Run &&run) {
  const size_t W = c->nwin, ndbl = nin + nout, bytes = ndbl * 8 + W * 4 * sizeof(int);
  double *d;
  if (!window_stage(c, bytes, ndbl * 8, h, d)) return CGP_ENOMEM;
  int *hst = reinterpret_cast<int *>(h + ndbl);
  fill(h);
  hipStream_t s = c->stream;
  const bool inplace = zero_copy && bytes <= kWinZeroCopyBytes;
  if (!inplace) HIP_TRY(c, hipMemcpyAsync(d, h, nin * 8, hipMemcpyHostToDevice, s));
  int rc = run(inplace ? h : d, s);
  if (rc != CGP_OK) return rc;
  if (!inplace) HIP_TRY(c, hipMemcpyAsync(h + nin, d + nin, nback * 8, hipMemcpyDeviceToHost, s));
  if ((rc = window_read_state(c, hst, s)) != CGP_OK) return rc;
  return first_failing_tick(hst + 2, W, 4);
}

// ---- the windows' buffer records (WinBufs ... WinLooGradBufs, cgp_engine.hip) ---------------------------------------------------
template <class R> void window_release(R &r) {   // a record's buffers freed, its capacity back to none
  r.each([](auto *p) { if (p) (void)hipFree(p); });
  r = R{};
}
// The lifetime rules, here and nowhere else: what goes when `what` goes (a new cgp_window_init, a new reservation, cgp_destroy).
// Every reservation was sized for the windows it was made on, and the multi-target objective's scratch for the reservation's P.
void window_drop(cgp_ctx *c, WinDrop what) {   // (declared in cgp_engine.hip for cgp_destroy)
  const bool all = what == WinDrop::Windows;
  if (all) window_release(c->wb);
  if (all || what == WinDrop::Multi) window_release(c->wm);
  if (all || what == WinDrop::Multi || what == WinDrop::MultiGrad) window_release(c->wg);
  if (all || what == WinDrop::Multi || what == WinDrop::Trend) window_release(c->wt);
  if (all || what == WinDrop::LooGrad) window_release(c->wl);
  if (all || what == WinDrop::Joint) window_release(c->wj);
}
// One buffer of the reservation `what` (a member of its record, null when the call starts): its size, and whether it starts as zeros.
struct WinSlot { void **p; size_t bytes; bool zero; };
template <class T> WinSlot slot(T *&p, size_t bytes, bool zero = false) { return {reinterpret_cast<void **>(&p), bytes, zero}; }
// one hipMalloc per slot; on failure the HIP error is cleared and the reservation is dropped, which frees what it got
template <size_t K> int window_alloc(cgp_ctx *c, WinDrop what, const WinSlot (&slots)[K]) {
  for (const WinSlot &s : slots)
    if (hipMalloc(s.p, s.bytes) != hipSuccess) {
      (void)hipGetLastError();
      *s.p = nullptr;
      window_drop(c, what);
      return CGP_ENOMEM;
    }
  return CGP_OK;
}
// the zero-filled slots' memsets and the synchronisation they need (cgp_window_init on why); on failure the reservation is dropped
template <size_t K> int window_zero(cgp_ctx *c, WinDrop what, const WinSlot (&slots)[K], const char *name) {
  bool ok = true;
  for (const WinSlot &s : slots) ok = ok && (!s.zero || hip_ok(c, hipMemset(*s.p, 0, s.bytes), name));
  if (ok && hip_ok(c, hipDeviceSynchronize(), name)) return CGP_OK;
  window_drop(c, what);
  return CGP_EHIP;
}

}  // namespace

extern "C" int cgp_window_init(cgp_ctx *c, int nwin, int N, int d, int kid, const double *theta, int theta_stride) {
  if (!c || nwin < 1 || N < 2 || N > 2048 || d < 1 || d > CGP_MAX_D || !theta || kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  if (k_is_matern(kid) && c->dtype != CGP_F64) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  if (theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // every instantiation a launch can pick for this kernel id gets its LDS limit (lds_limit on why here)
  const bool mat = k_is_matern(kid);
  for (int wpw : {1, 2, 4})
    if (!lds_limit(pairs_kernel(wpw, mat), kWinPushLdsMax)) return CGP_EHIP;
  if (!lds_limit(k_window_multi<kWinMulti>, kWinPushLdsMax)) return CGP_EHIP;
  for (int n : kWinClassMaxN)
    for (bool keep : {false, true})
      if (!lds_limit(forecast_form(n, keep, mat).kernel, kWinForecastLdsMax)) return CGP_EHIP;
  for (int n : kWinClassMaxN)
    if (!lds_limit(pgrad_win_form(n, mat).kernel, kWinForecastLdsMax)) return CGP_EHIP;
  // the old windows are gone from here on: a failure below must leave the context without windows,
  // not with stale pointers (cgp_window_push checks nwin)
  c->nwin = 0;
  c->win = WindowArgs{};
  window_drop(c, WinDrop::Windows);
  const int CAP = 2 * N + CGP_WIN_CAP_PAD;   // ring capacity = leading dimension of the windows' slabs
  const size_t W = nwin, NB = cdiv(N, WPB);
  WinBufs &b = c->wb;
  // dinv: cgp_window_predict's (allocated here: no allocation between launches of a call); grad_scratch: cgp_window_nll_grad's
  // alpha, per-chunk partial sums and values (cgp_window_adapt.hpp): 28 N / 16 + 1 doubles per window
  const WinSlot slots[] = {slot(b.L, W * CAP * CAP * 8), slot(b.z, W * CAP * 8), slot(b.xw, W * d * CAP * 8), slot(b.yw, W * CAP * 8),
                           slot(b.state, W * 4 * sizeof(int), true), slot(b.prep_theta, W * (PREP_N + MAX_THETA) * 8),
                           slot(b.dinv, W * NB * WPB * WPB * 8), slot(b.grad_scratch, W * (NB * (WPB + GRAD_N) + 1) * 8)};
  if (window_alloc(c, WinDrop::Windows, slots) != CGP_OK) return CGP_ENOMEM;
  WindowArgs wa{};
  wa.L = b.L; wa.z = b.z; wa.xw = b.xw; wa.yw = b.yw; wa.state = b.state;
  double *pt = b.prep_theta;
  wa.prep = pt;
  wa.theta = pt + W * PREP_N;
  wa.N = N;
  wa.CAP = CAP;
  wa.d = d;
  wa.kernel_id = kid;
  std::vector<double> h(W * (PREP_N + MAX_THETA), 0.0);
  for (size_t w = 0; w < W; ++w) {
    const double *th = theta + w * theta_stride;
    double *o = h.data() + w * PREP_N;
    for (int q = 0; q < d; ++q) o[q] = k_is_ard(kid) ? 1.0 / th[1 + q] : 1.0 / th[1];
    o[9] = th[0];
    o[10] = (kid == CGP_KERNEL_RBF_BROWNIAN) ? th[2] : 0.0;
    for (int q = 0; q < nth; ++q) h[W * PREP_N + w * MAX_THETA + q] = th[q];
  }
  // hipMemset of device memory is ASYNCHRONOUS to the host and ordered on the legacy default stream only -- the pushes run on the
  // context's non-blocking stream (or the caller's), which does not wait for it: without the synchronisation below the first
  // push could read the windows' state words before they were zeroed (found by round 6's sweep under load: fourteen processes
  // sharing the GPU -- a memory access fault, or garbage for one window; never seen on an idle GPU, where the fill is over
  // before the first launch is issued).
  if (!hip_ok(c, hipMemcpy(pt, h.data(), h.size() * 8, hipMemcpyHostToDevice), "window theta H2D")) {
    window_drop(c, WinDrop::Windows);
    return CGP_EHIP;
  }
  if (window_zero(c, WinDrop::Windows, slots, "window state memset / synchronise") != CGP_OK) return CGP_EHIP;
  c->win = wa;  // published only when every allocation and copy has succeeded
  c->nwin = nwin;
  c->win_o = c->win_n = 0;
  return CGP_OK;
}

namespace {
int window_push_impl(cgp_ctx *c, int T, const double *dxs, const double *dys, int include_noise, double *dpm, double *dpv, double *dl,
                     int *info_out, hipStream_t ws);
}
extern "C" int cgp_window_push_device(cgp_ctx *c, int T, const double *dxs, const double *dys, int include_noise,
                                      double *dpm, double *dpv, double *dl, void *hip_stream) {
  if (!c || c->nwin < 1 || c->wm.P > 0) return CGP_ESTATE;   // (a single-target push would leave the other columns behind)
  if (T < 1 || !dxs || !dys || !dpm || !dpv || !dl) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  return window_push_impl(c, T, dxs, dys, include_noise, dpm, dpv, dl, nullptr, pick_stream(c, hip_stream));
}
namespace {
// info_out: [nwin] ints the kernels mirror every window's status word into (pinned host memory for the per-tick entry), or null
int window_push_impl(cgp_ctx *c, int T, const double *dxs, const double *dys, int include_noise, double *dpm, double *dpv, double *dl,
                     int *info_out, hipStream_t ws) {
  WindowArgs a = c->win;
  a.info_out = info_out;
  a.xs = dxs;
  a.ys = dys;
  a.pred_mean = dpm;
  a.pred_var = dpv;
  a.logml = dl;
  a.T = T;
  a.include_noise = include_noise;
  const size_t lds1 = (size_t)(3 * a.N + 8 * WPB + MAXD + 8 + 2 * WIN_STG) * sizeof(double);
  if (c->win_o < 0) {   // the mirror was invalidated by a failed push: read the windows' state back (they advance in lock-step)
    int st[4];
    HIP_TRY(c, hipStreamSynchronize(ws));
    HIP_TRY(c, hipMemcpy(st, c->win.state, sizeof(st), hipMemcpyDeviceToHost));
    c->win_o = st[0];
    c->win_n = st[1];
  }
  int o = c->win_o, n = c->win_n;
  const bool matern = k_is_matern(a.kernel_id);
  window_cut(c->nwin, a.N, a.CAP, T, o, n, [&](int kind, int arg, int t0, int nt) {
    a.t0 = t0;
    a.nt = nt;
    if (kind == CGP_PLAN_MULTI) hipLaunchKernelGGL(k_window_multi<kWinMulti>, dim3(c->nwin), dim3(256), multi_lds(a.N), ws, a);
    else if (kind == CGP_PLAN_PAIRS) hipLaunchKernelGGL(pairs_kernel(arg, matern), dim3(c->nwin / arg), dim3(256), pairs_lds(a.N, arg), ws, a);
    else if (arg == 512) hipLaunchKernelGGL(k_window_ticks<512>, dim3(c->nwin), dim3(512), lds1, ws, a);
    else hipLaunchKernelGGL(k_window_ticks<256>, dim3(c->nwin), dim3(256), lds1, ws, a);
  });
  if (!hip_ok(c, hipGetLastError(), "window launches")) {
    c->win_o = c->win_n = -1;   // what reached the device is unknown: the next push re-reads the state
    return CGP_EHIP;
  }
  c->win_o = o;   // committed only once every launch of the push was accepted
  c->win_n = n;
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_push(cgp_ctx *c, int T, const double *xs, const double *ys, int include_noise, double *pm,
                               double *pv, double *logml) {
  if (!c || c->nwin < 1 || c->wm.P > 0) return CGP_ESTATE;
  if (T < 1 || !xs || !ys || !pm || !pv || !logml) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // The per-tick host entry (configs[3] is "streamed per IMU tick": T = 1 is the common call): no allocation and no
  // pageable copy on the path.  One pinned block [xs | ys | pm pv logml | state] and its device twin live in the
  // context; per call: stage in, ONE H2D, the launch, TWO D2H (outputs, window states), one synchronisation.
  const size_t W = c->nwin, nx = W * T * c->win.d, ny = W * T;
  const size_t ndbl = nx + 4 * ny, bytes = ndbl * 8 + W * 4 * sizeof(int);
  double *h, *d;
  if (!window_stage(c, bytes, ndbl * 8, h, d)) return CGP_ENOMEM;
  int *hst = reinterpret_cast<int *>(h + ndbl);
  memcpy(h, xs, nx * 8);
  memcpy(h + nx, ys, ny * 8);
  hipStream_t s = c->stream;
  const bool inplace = bytes <= kWinZeroCopyBytes;
  if (inplace) {
    // A tick or a handful of them (configs[3] is "streamed per IMU tick"): no copy command at all.  The kernels read the
    // samples where they were staged (pinned host memory is device-visible at its host address) and write the tick's
    // outputs and every window's status word back there; one synchronisation.  (Round 4: one H2D, two D2H, 176 us per tick of
    // one N = 512 window, ~30 us of it the three copy commands; the tick itself is 147 us of one workgroup's serial chains.)
    // T = 1 is ONE launch of the single-tick kernel, whose last store is the window's status word (after a system-scope fence): the host
    // polls those words in the pinned block instead of synchronising the stream (a few microseconds of the runtime's wake-up), and
    // falls back to the synchronisation if they do not arrive (which is also where a faulting kernel's error surfaces)
    constexpr int kPending = INT_MIN;
    const bool poll = T == 1;
    for (size_t w = 0; w < W; ++w) hst[w] = poll ? kPending : 0;
    int rc0 = window_push_impl(c, T, h, h + nx, include_noise, h + nx + ny, h + nx + 2 * ny, h + nx + 3 * ny, hst, s);
    if (rc0 != CGP_OK) return rc0;
    bool done = false;
    if (poll) {
      volatile int *v = hst;
      const auto t0 = std::chrono::steady_clock::now();
      for (int spin = 0;; ++spin) {
        size_t w = 0;
        while (w < W && v[w] != kPending) ++w;
        if (w == W) { done = true; break; }
        if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!done) HIP_TRY(c, hipStreamSynchronize(s));
  } else {
    HIP_TRY(c, hipMemcpyAsync(d, h, (nx + ny) * 8, hipMemcpyHostToDevice, s));
    int rc = cgp_window_push_device(c, T, d, d + nx, include_noise, d + nx + ny, d + nx + 2 * ny, d + nx + 3 * ny, s);
    if (rc != CGP_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h + nx + ny, d + nx + ny, 3 * ny * 8, hipMemcpyDeviceToHost, s));
    if ((rc = window_read_state(c, hst, s)) != CGP_OK) return rc;
  }
  memcpy(pm, h + nx + ny, ny * 8);
  memcpy(pv, h + nx + 2 * ny, ny * 8);
  memcpy(logml, h + nx + 3 * ny, ny * 8);
  return inplace ? first_failing_tick(hst, W, 1) : first_failing_tick(hst + 2, W, 4);
}

// ---- forecast from the windows as they stand (cgp_window_forecast.hpp) ----------------------------------------------
extern "C" int cgp_window_predict_device(cgp_ctx *c, int M, const double *dxs, int include_noise, double *dmean, double *dvar,
                                         void *hip_stream) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (M < 1 || !dxs || !dmean || !dvar) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  ForecastArgs a = forecast_args(c);
  a.xs = dxs; a.mean = dmean; a.var = dvar;
  a.M = M; a.include_noise = include_noise;
  // Origin and size are read from the windows' state words on the device (the kernels run after every earlier push of the
  // stream), so the launches are sized by the capacity N and need no host mirror.  The form depends on N alone.
  const ForecastForm form = forecast_form(a.N, false, k_is_matern(a.kernel_id));
  a.nchunk = cdiv(M, form.mc);
  unsigned grid;
  if (xcd_grid((long long)c->nwin * a.nchunk, grid) != CGP_OK || !fits_grid(diag_inv_groups(c))) return CGP_EINVAL;
  launch_diag_inv(c, ws);
  hipLaunchKernelGGL(form.kernel, dim3(grid), dim3(WF_THREADS), form.lds, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window forecast launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_predict(cgp_ctx *c, int M, const double *xs, int include_noise, double *mean, double *var) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (M < 1 || !xs || !mean || !var) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // staged like a push: one pinned block [xs | mean var | state] and its device twin; a small call is read and written in
  // place by the kernels (no copy command), a large one is one H2D and two D2H
  const size_t W = c->nwin, nx = W * M * c->win.d, ny = W * M;
  double *h;
  const int rc = window_staged_call(
      c, nx, 2 * ny, 2 * ny, true, h, [&](double *hx) { memcpy(hx, xs, nx * 8); },
      [&](double *io, hipStream_t s) { return cgp_window_predict_device(c, M, io, include_noise, io + nx, io + nx + ny, s); });
  if (rc < 0) return rc;
  memcpy(mean, h + nx, ny * 8);
  memcpy(var, h + nx + ny, ny * 8);
  return rc;
}

// ---- predictive gradients from the windows as they stand (cgp_window_pgrad.hpp) --------------------------------------
// The forecast's launches with the gradient's alpha between them: diagonal inverses, alpha = L^-T z (cgp_window_nll_grad's
// second launch, into its scratch), then the gradient form of the forecast kernel.
extern "C" int cgp_window_predict_gradients_device(cgp_ctx *c, int M, const double *dxs, int include_noise, double *dmean_out,
                                                   double *dvar_out, double *ddmean, double *ddvar, void *hip_stream) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (M < 1 || !dxs || (!ddmean && !ddvar)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  ForecastArgs a = forecast_args(c);
  a.xs = dxs; a.mean = dmean_out; a.var = dvar_out;
  a.M = M; a.include_noise = include_noise;
  const AdaptArgs ad = adapt_args(c);
  a.alpha = ad.alpha; a.gdmean = ddmean; a.gdvar = ddvar;
  const ForecastForm form = pgrad_win_form(a.N, k_is_matern(a.kernel_id));   // by N alone, as the forecast's
  a.nchunk = cdiv(M, form.mc);
  unsigned grid;
  if (xcd_grid((long long)c->nwin * a.nchunk, grid) != CGP_OK || !fits_grid(diag_inv_groups(c))) return CGP_EINVAL;
  launch_alpha(c, ad, ws);
  hipLaunchKernelGGL(form.kernel, dim3(grid), dim3(WF_THREADS), form.lds, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window gradient forecast launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_predict_gradients(cgp_ctx *c, int M, const double *xs, int include_noise, double *mean, double *var,
                                            double *dmean, double *dvar) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (M < 1 || !xs || (!dmean && !dvar)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // staged as cgp_window_predict: one pinned block [xs | mean var | dmean dvar | state] and its device twin
  const size_t W = c->nwin, nx = W * M * c->win.d, ny = W * M;
  const size_t om = nx, ov = nx + ny, odm = nx + 2 * ny, odv = 2 * nx + 2 * ny;
  double *h;
  const int rc = window_staged_call(c, nx, 2 * ny + 2 * nx, 2 * ny + 2 * nx, true, h, [&](double *hx) { memcpy(hx, xs, nx * 8); },
                                    [&](double *io, hipStream_t s) {
                                      return cgp_window_predict_gradients_device(c, M, io, include_noise, mean ? io + om : nullptr,
                                                                                 var ? io + ov : nullptr, dmean ? io + odm : nullptr,
                                                                                 dvar ? io + odv : nullptr, s);
                                    });
  if (rc < 0) return rc;
  if (mean) memcpy(mean, h + om, ny * 8);
  if (var) memcpy(var, h + ov, ny * 8);
  if (dmean) memcpy(dmean, h + odm, nx * 8);
  if (dvar) memcpy(dvar, h + odv, nx * 8);
  return rc;
}

// ---- multi-target windows: P target columns share the resident factor (cgp_window_multi.hpp) --------------------------
namespace {
// the checks the multi-target calls start with, before anything is enqueued; objective: the calls that need
// cgp_window_multi_grad_reserve's scratch as well
int window_multi_check(const cgp_ctx *c, int P, bool args_ok, bool objective = false) {
  if (!c) return CGP_ESTATE;
  if (c->dtype != CGP_F64) return CGP_EINVAL;
  if (c->nwin < 1 || c->wm.P < 1 || (objective && !c->wg.am)) return CGP_ESTATE;
  if (P != c->wm.P || !args_ok) return CGP_EINVAL;
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_multi_reserve(cgp_ctx *c, int P) {
  if (!c) return CGP_ESTATE;
  if (c->dtype != CGP_F64) return CGP_EINVAL;
  if (c->nwin < 1) return CGP_ESTATE;
  if (P < 1 || P > WM_MAX_P) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // earlier pushes have landed; an earlier reservation's buffers are idle
  const size_t W = c->nwin;
  {   // every window still empty: the store starts at tick 0 with the windows
    std::vector<int> st(W * 4);
    HIP_TRY(c, hipMemcpy(st.data(), c->win.state, st.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
      if (st[w * 4 + 1] != 0 || st[w * 4 + 3] != 0) return CGP_ESTATE;
  }
  // every instantiation a multi-target launch can pick gets its LDS limit (lds_limit on why here)
  const int N = c->win.N;
  const bool mat = k_is_matern(c->win.kernel_id);
  for (int n : kWinClassMaxN)
    for (bool z : {false, true})
      if (!lds_limit(multi_win_form(n, z, mat).kernel, kWinForecastLdsMax)) return CGP_EHIP;
  window_drop(c, WinDrop::Multi);
  const size_t pt = cdiv(P, WPB), nrow = (size_t)cdiv(N, WPB) * WPB, ticks = std::max(N, 256);
  WinMultiBufs &b = c->wm;
  // (the Z scratch starts as zeros: the columns past P of the last target tile are never written and stay so)
  const WinSlot slots[] = {slot(b.ystore, W * P * N * 8, true), slot(b.ycount, W * sizeof(int), true),
                           slot(b.zs, W * pt * nrow * WPB * 8, true), slot(b.y0, W * ticks * 8)};
  if (window_alloc(c, WinDrop::Multi, slots) != CGP_OK) return CGP_ENOMEM;
  if (window_zero(c, WinDrop::Multi, slots, "window multi reserve memsets / synchronise") != CGP_OK) return CGP_EHIP;
  b.P = P;
  b.ticks = ticks;
  return CGP_OK;
}

extern "C" int cgp_window_push_multi_device(cgp_ctx *c, int T, int P, const double *dxs, const double *dYs, int include_noise,
                                            double *dpm, double *dpv, double *dl, void *hip_stream) {
  int rc = window_multi_check(c, P, T >= 1 && dxs && dYs && dpm && dpv && dl);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  if ((size_t)T > c->wm.ticks) {   // a push longer than any before it: the gather block grows (an allocation; the free waits for the device)
    void *nb = nullptr;
    if (hipMalloc(&nb, (size_t)c->nwin * T * 8) != hipSuccess) {
      (void)hipGetLastError();
      return CGP_ENOMEM;
    }
    (void)hipFree(c->wm.y0);
    c->wm.y0 = static_cast<double *>(nb);
    c->wm.ticks = T;
  }
  TargetStoreArgs s{};
  s.Ys = dYs;
  s.ystore = c->wm.ystore;
  s.ycount = c->wm.ycount;
  s.y0 = c->wm.y0;
  s.N = c->win.N; s.P = P; s.T = T;
  hipLaunchKernelGGL(k_window_targets_store, dim3(c->nwin), dim3(256), 0, ws, s);
  return window_push_impl(c, T, dxs, s.y0, include_noise, dpm, dpv, dl, nullptr, ws);
}

extern "C" int cgp_window_push_multi(cgp_ctx *c, int T, int P, const double *xs, const double *Ys, int include_noise, double *pm,
                                     double *pv, double *logml) {
  int rc = window_multi_check(c, P, T >= 1 && xs && Ys && pm && pv && logml);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // staged like a large cgp_window_push: one pinned block [xs | Ys | pm pv logml | state] and its device twin, one H2D, two D2H
  const size_t W = c->nwin, nx = W * T * c->win.d, ny = W * T, nY = ny * P;
  const size_t oo = nx + nY;
  double *h;
  rc = window_staged_call(
      c, oo, 3 * ny, 3 * ny, false, h,
      [&](double *hx) {
        memcpy(hx, xs, nx * 8);
        memcpy(hx + nx, Ys, nY * 8);
      },
      [&](double *io, hipStream_t s) {
        return cgp_window_push_multi_device(c, T, P, io, io + nx, include_noise, io + oo, io + oo + ny, io + oo + 2 * ny, s);
      });
  if (rc < 0) return rc;
  memcpy(pm, h + oo, ny * 8);
  memcpy(pv, h + oo + ny, ny * 8);
  memcpy(logml, h + oo + 2 * ny, ny * 8);
  return rc;
}

// Three launches: the diagonal blocks' inverses, Z = L^-1 Y of the P columns into the scratch (with logml), the forecast whose
// epilogue contracts V with Z.  Sized by the capacity N; origin, size and tick count are read on the device.
extern "C" int cgp_window_predict_multi_device(cgp_ctx *c, int M, int P, const double *dxs, int include_noise, double *dmean,
                                               double *dvar, double *dlogml, void *hip_stream) {
  int rc = window_multi_check(c, P, M >= 1 && dxs && dmean && dvar);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  const bool matern = k_is_matern(c->win.kernel_id);
  const ForecastForm zf = multi_win_form(c->win.N, true, matern), mf = multi_win_form(c->win.N, false, matern);   // by N alone, as the forecast's
  const ForecastArgs za = multi_z_args(c, zf, dlogml);
  ForecastArgs a = za;   // the forecast proper: the test points back in their place, the Z scratch read
  a.mlogml = nullptr;
  a.xs = dxs; a.mean = dmean; a.var = dvar;
  a.M = M; a.include_noise = include_noise;
  a.nchunk = cdiv(M, mf.mc);
  unsigned grid, zgrid;
  if (xcd_grid((long long)c->nwin * a.nchunk, grid) != CGP_OK || xcd_grid((long long)c->nwin * za.nchunk, zgrid) != CGP_OK ||
      !fits_grid(diag_inv_groups(c)))
    return CGP_EINVAL;
  launch_diag_inv(c, ws);
  hipLaunchKernelGGL(zf.kernel, dim3(zgrid), dim3(WF_THREADS), zf.lds, ws, za);
  hipLaunchKernelGGL(mf.kernel, dim3(grid), dim3(WF_THREADS), mf.lds, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window multi-target forecast launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_predict_multi(cgp_ctx *c, int M, int P, const double *xs, int include_noise, double *mean, double *var,
                                        double *logml) {
  int rc = window_multi_check(c, P, M >= 1 && xs && mean && var);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // one pinned block [xs | mean | var | logml | state] and its device twin: one H2D, one D2H of the outputs, the state words
  const size_t W = c->nwin, nx = W * M * c->win.d, nm = W * P * M, nv = W * M, nl = W * P;
  double *h;
  rc = window_staged_call(c, nx, nm + nv + nl, nm + nv + (logml ? nl : 0), false, h, [&](double *hx) { memcpy(hx, xs, nx * 8); },
                          [&](double *io, hipStream_t s) {
                            return cgp_window_predict_multi_device(c, M, P, io, include_noise, io + nx, io + nx + nm,
                                                                   logml ? io + nx + nm + nv : nullptr, s);
                          });
  if (rc < 0) return rc;
  memcpy(mean, h + nx, nm * 8);
  memcpy(var, h + nx + nm, nv * 8);
  if (logml) memcpy(logml, h + nx + nm + nv, nl * 8);
  return rc;
}

// ---- explicit basis functions on the multi-target windows (cgp_trend.hpp): the last q of the P columns are the basis ----------
namespace {
// the checks the two calls start with, before anything is enqueued
int window_trend_check(const cgp_ctx *c, int M, int P, int q, bool args_ok) {
  if (!c) return CGP_ESTATE;
  if (c->dtype != CGP_F64) return CGP_EINVAL;
  if (c->nwin < 1 || c->wm.P < 1 || c->wt.q < 1) return CGP_ESTATE;
  if (P != c->wm.P || q != c->wt.q || M < 1 || !args_ok) return CGP_EINVAL;
  if (M > c->wt.max_m) return CGP_ECAPACITY;
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_trend_reserve(cgp_ctx *c, int q, int max_m) {
  if (!c) return CGP_ESTATE;
  if (c->dtype != CGP_F64) return CGP_EINVAL;
  if (c->nwin < 1 || c->wm.P < 1) return CGP_ESTATE;
  if (q < 1 || q > TR_MAX || q >= c->wm.P || max_m < 1) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // an earlier reservation's buffers are idle
  window_drop(c, WinDrop::Trend);
  const size_t W = c->nwin, P = c->wm.P, ncol = (size_t)cdiv(c->wm.P, TR_MAX) * TR_MAX;
  const WinSlot slots[] = {slot(c->wt.mean0, W * (P * max_m + P) * 8), slot(c->wt.sl, W * (ncol + TR_MAX) * TR_MAX * 8)};
  if (window_alloc(c, WinDrop::Trend, slots) != CGP_OK) return CGP_ENOMEM;
  c->wt.q = q;
  c->wt.max_m = max_m;
  return CGP_OK;
}

// cgp_window_predict_multi_device's three launches over all P columns into the reservation's scratch, then the three trend launches
// (gram over the Z scratch, solve, apply).  Reads the windows and writes the two scratches only.
extern "C" int cgp_window_predict_trend_device(cgp_ctx *c, int M, int P, int q, const double *dxs, const double *dHs, int include_noise,
                                               double *dmean, double *dvar, double *dbeta, double *dlogml, int *dtinfo,
                                               void *hip_stream) {
  int rc = window_trend_check(c, M, P, q, dxs && dHs && dmean && dvar && dbeta && dlogml && dtinfo);
  if (rc != CGP_OK) return rc;
  const size_t W = c->nwin;
  double *mean0 = c->wt.mean0, *logml0 = mean0 + W * P * M;
  if ((rc = cgp_window_predict_multi_device(c, M, P, dxs, include_noise, mean0, dvar, logml0, hip_stream)) != CGP_OK) return rc;
  hipStream_t ws = pick_stream(c, hip_stream);
  TrendArgs a{};
  a.N = c->win.N; a.M = M; a.P = P - q; a.q = q; a.nfit = c->nwin;
  a.ncol = cdiv(P, TR_MAX) * TR_MAX;
  a.S = c->wt.sl;
  a.Linv = a.S + W * a.ncol * TR_MAX;
  a.mean0 = mean0;
  a.logml0 = logml0;
  a.Hs = dHs;
  a.mean = dmean; a.var = dvar; a.beta = dbeta; a.logml = dlogml;
  a.info = c->win.state + 2;
  a.info_stride = 4;
  a.tinfo = dtinfo;
  a.zs = c->wm.zs;
  a.state = c->win.state;
  a.pt = cdiv(P, WPB);
  a.nrow = cdiv(c->win.N, WPB) * WPB;
  hipLaunchKernelGGL(k_trend_gram<true>, dim3(a.ncol / TR_MAX, a.nfit), dim3(TG_WAVES * 64), 0, ws, a);
  hipLaunchKernelGGL(k_trend_solve, dim3(a.nfit), dim3(64), 0, ws, a);
  hipLaunchKernelGGL(k_trend_apply, dim3(cdiv(M, TA_THREADS), cdiv(a.P, TA_PCH), a.nfit), dim3(TA_THREADS), 0, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window trend launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_predict_trend(cgp_ctx *c, int M, int P, int q, const double *xs, const double *Hs, int include_noise,
                                        double *mean, double *var, double *beta, double *logml, int *tinfo) {
  int rc = window_trend_check(c, M, P, q, xs && Hs && mean && var);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // one pinned block [xs | Hs | mean | var | beta | logml | tinfo (as doubles' room) | state] and its device twin
  const size_t W = c->nwin, Pt = P - q, nx = W * M * c->win.d, nh = W * q * M, nm = W * Pt * M, nv = W * M, nb = W * Pt * q, nl = W * Pt,
               nt = (W + 1) / 2, nin = nx + nh;
  double *h;
  rc = window_staged_call(c, nin, nm + nv + nb + nl + nt, nm + nv + nb + nl + nt, false, h,
                          [&](double *hx) {
                            memcpy(hx, xs, nx * 8);
                            memcpy(hx + nx, Hs, nh * 8);
                          },
                          [&](double *io, hipStream_t s) {
                            double *o = io + nin;
                            return cgp_window_predict_trend_device(c, M, P, q, io, io + nx, include_noise, o, o + nm, o + nm + nv,
                                                                   o + nm + nv + nb, reinterpret_cast<int *>(o + nm + nv + nb + nl), s);
                          });
  if (rc < 0) return rc;
  const double *o = h + nin;
  memcpy(mean, o, nm * 8);
  memcpy(var, o + nm, nv * 8);
  if (beta) memcpy(beta, o + nm + nv, nb * 8);
  if (logml) memcpy(logml, o + nm + nv + nb, nl * 8);
  if (tinfo) memcpy(tinfo, o + nm + nv + nb + nl, W * sizeof(int));
  return rc;
}

// ---- joint forecast: full posterior covariance and sample paths (cgp_window_joint.hpp) -------------------------------
extern "C" int cgp_window_joint_reserve(cgp_ctx *c, int max_m) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (max_m < 1 || max_m > 1024) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // an earlier joint forecast may still read the buffers that go
  window_drop(c, WinDrop::Joint);
  const size_t W = c->nwin, mpad = (size_t)cdiv(max_m, WPB) * WPB, nrow = (size_t)cdiv(c->win.N, WPB) * WPB;
  WinJointBufs &b = c->wj;
  const WinSlot slots[] = {slot(b.V, W * nrow * mpad * 8), slot(b.C, W * mpad * mpad * 8), slot(b.mean_var, 2 * W * (size_t)max_m * 8),
                           slot(b.jinfo, W * sizeof(int))};
  if (window_alloc(c, WinDrop::Joint, slots) != CGP_OK) return CGP_ENOMEM;
  b.max_m = max_m;
  return CGP_OK;
}

namespace {
// The super-tile grid of a joint covariance launch (k_window_joint_cov, k_joint_cov) over nunit windows or fits: fills the args'
// grid fields and returns the number of workgroups, a multiple of WF_XCDS, or 0 when it would pass 2^30.
unsigned joint_cov_grid(int M, int nunit, int &mt, int &nsup, int &npair, int &per_unit) {
  mt = cdiv(M, WPB);
  nsup = cdiv(mt, WJ_ST);
  npair = nsup * (nsup + 1) / 2;
  per_unit = cdiv(npair, WJ_WAVES);
  unsigned grid;
  return xcd_grid((long long)nunit * per_unit, grid) == CGP_OK ? grid : 0u;
}
// C C^T = scratch matrix + jitter I in place, then out = mean + C xi, for the nunit windows or fits whose buffers, M, mt and S j
// names: the tail of every sampling route.  CGP_EINVAL (nothing enqueued) when the paths' grid would pass 2^30.
int joint_chol_paths_launch(JointArgs &j, int nunit, hipStream_t s) {
  const long long per = ((long long)j.mt * cdiv(j.S, WPB) + WJ_WAVES - 1) / WJ_WAVES;   // one wave per 16 x 16 tile of the paths
  if (!fits_grid(per * nunit)) return CGP_EINVAL;
  j.per_win = (int)per;
  if (j.mt <= 4 * WA_WAVES) hipLaunchKernelGGL(k_window_joint_chol<4>, dim3(nunit), dim3(WA_THREADS), 0, s, j);
  else hipLaunchKernelGGL(k_window_joint_chol<8>, dim3(nunit), dim3(WA_THREADS), 0, s, j);
  hipLaunchKernelGGL(k_window_joint_paths, dim3((unsigned)(j.per_win * nunit)), dim3(WJ_THREADS), 0, s, j);
  return CGP_OK;
}
// the checks every window joint call starts with: windows and reservation, the arguments, the reservation's capacity
int window_joint_check(const cgp_ctx *c, int M, bool args_ok) {
  if (!c || c->nwin < 1 || c->wj.max_m < 1) return CGP_ESTATE;
  if (M < 1 || !args_ok) return CGP_EINVAL;
  if (M > c->wj.max_m) return CGP_ECAPACITY;
  return CGP_OK;
}

// the launches both entry points share: diagonal inverses, the solve with V kept (mean to dmean, variance to the scratch), and
// the contraction -- into the caller's dcov, or (dcov == nullptr) into the scratch matrix for the factorisation
int window_joint_launch(cgp_ctx *c, int M, const double *dxs, int include_noise, double *dmean, double *dcov, JointArgs &j, hipStream_t ws) {
  ForecastArgs a = forecast_args(c);
  a.xs = dxs; a.mean = dmean;
  a.var = c->wj.mean_var + (size_t)c->nwin * c->wj.max_m;
  a.M = M; a.include_noise = include_noise;
  a.vkeep = c->wj.V;
  a.mt = cdiv(M, WPB);
  const ForecastForm form = forecast_form(a.N, true, k_is_matern(a.kernel_id));   // the forecast's forms, by N alone
  a.nchunk = cdiv(M, form.mc);
  j = joint_args(c);
  j.xs = dxs; j.mean = dmean; j.var = a.var; j.cov = dcov;
  j.M = M;
  const unsigned jgrid = joint_cov_grid(M, c->nwin, j.mt, j.nsup, j.npair, j.per_win);
  unsigned grid;
  if (xcd_grid((long long)c->nwin * a.nchunk, grid) != CGP_OK || jgrid == 0 || !fits_grid(diag_inv_groups(c))) return CGP_EINVAL;
  launch_diag_inv(c, ws);
  hipLaunchKernelGGL(form.kernel, dim3(grid), dim3(WF_THREADS), form.lds, ws, a);
  if (dcov) hipLaunchKernelGGL(k_window_joint_cov<false>, dim3(jgrid), dim3(WJ_THREADS), 0, ws, j);
  else hipLaunchKernelGGL(k_window_joint_cov<true>, dim3(jgrid), dim3(WJ_THREADS), 0, ws, j);
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_predict_cov_device(cgp_ctx *c, int M, const double *dxs, int include_noise, double *dmean, double *dcov,
                                             void *hip_stream) {
  int rc = window_joint_check(c, M, dxs && dmean && dcov);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  JointArgs j;
  rc = window_joint_launch(c, M, dxs, include_noise, dmean, dcov, j, pick_stream(c, hip_stream));
  if (rc != CGP_OK) return rc;
  if (!hip_ok(c, hipGetLastError(), "window joint covariance launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_sample_device(cgp_ctx *c, int M, const double *dxs, int S, const double *dxi, int include_noise,
                                        double jitter_rel, double *dout, int *dinfo, void *hip_stream) {
  int rc = window_joint_check(c, M, S >= 1 && dxs && dxi && dout && jitter_rel >= 0.0);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  JointArgs j;
  rc = window_joint_launch(c, M, dxs, include_noise, c->wj.mean_var, nullptr, j, ws);
  if (rc != CGP_OK) return rc;
  j.xi = dxi; j.out = dout; j.S = S; j.info = dinfo; j.jitter_rel = jitter_rel;
  if ((rc = joint_chol_paths_launch(j, c->nwin, ws)) != CGP_OK) return rc;
  if (!hip_ok(c, hipGetLastError(), "window sample launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_predict_cov(cgp_ctx *c, int M, const double *xs, int include_noise, double *mean, double *cov) {
  int rc = window_joint_check(c, M, xs && mean && cov);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // device block [xs | mean | cov]; the copies are ordered on the context's stream with the launches
  const size_t W = c->nwin, nx = W * M * c->win.d, ny = W * M, nc = W * M * M;
  double *h, *d;
  if (!window_stage(c, W * 4 * sizeof(int), (nx + ny + nc) * 8, h, d)) return CGP_ENOMEM;
  int *hst = reinterpret_cast<int *>(h);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(d, xs, nx * 8, hipMemcpyHostToDevice, s));
  rc = cgp_window_predict_cov_device(c, M, d, include_noise, d + nx, d + nx + ny, s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(mean, d + nx, ny * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(cov, d + nx + ny, nc * 8, hipMemcpyDeviceToHost, s));
  if ((rc = window_read_state(c, hst, s)) != CGP_OK) return rc;
  return first_failing_tick(hst + 2, W, 4);
}

extern "C" int cgp_window_sample(cgp_ctx *c, int M, const double *xs, int S, const double *xi, int include_noise, double jitter_rel,
                                 double *out, int *info) {
  int rc = window_joint_check(c, M, S >= 1 && xs && xi && out && jitter_rel >= 0.0);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // device block [xs | xi | out | info]
  const size_t W = c->nwin, nx = W * M * c->win.d, np = W * (size_t)S * M, ni = (W + 1) / 2;
  double *h, *d;
  if (!window_stage(c, W * sizeof(int), (nx + 2 * np + ni) * 8, h, d)) return CGP_ENOMEM;
  int *hi = reinterpret_cast<int *>(h);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(d, xs, nx * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(d + nx, xi, np * 8, hipMemcpyHostToDevice, s));
  rc = cgp_window_sample_device(c, M, d, S, d + nx, include_noise, jitter_rel, d + nx + np, reinterpret_cast<int *>(d + nx + 2 * np), s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, d + nx + np, np * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(hi, d + nx + 2 * np, W * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (info) memcpy(info, hi, W * sizeof(int));
  return first_flagged_window(hi, W);
}

extern "C" int cgp_window_state(cgp_ctx *c, int w, int *n, int *info) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (w < 0 || w >= c->nwin) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  int st[4];
  HIP_TRY(c, hipMemcpy(st, c->win.state + w * 4, sizeof(st), hipMemcpyDeviceToHost));
  if (n) *n = st[1];
  if (info) *info = st[2];
  return CGP_OK;
}

extern "C" int cgp_debug_window_plan(cgp_ctx *c, int T, int *out, int cap) {
  if (!c || c->nwin < 1 || c->win_o < 0) return CGP_ESTATE;   // (an invalidated mirror is re-read by the next push, not here)
  if (T < 1 || cap < 0 || (cap > 0 && !out)) return CGP_EINVAL;
  int o = c->win_o, n = c->win_n, count = 0;
  window_cut(c->nwin, c->win.N, c->win.CAP, T, o, n, [&](int kind, int arg, int t0, int nt) {
    if (count < cap) {
      const int rec[4] = {kind, arg, t0, nt};
      memcpy(out + 4 * count, rec, sizeof(rec));
    }
    ++count;
  });
  return count;
}

// ---- hyper-parameters of the resident windows replaced / re-estimated in place (cgp_window_adapt.hpp) -----------------
extern "C" int cgp_window_set_theta_device(cgp_ctx *c, const double *dtheta, int theta_stride, const unsigned char *dselect,
                                           double *dlogml, int *dinfo, void *hip_stream) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (!dtheta || theta_stride < ntheta(c->win.kernel_id, c->win.d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  AdaptArgs a = adapt_args(c);
  a.new_theta = dtheta; a.theta_stride = theta_stride; a.select = dselect; a.logml = dlogml; a.info = dinfo;
  // origin and size come from the windows' state words; the form (accumulators per wave) depends on N alone
  hipLaunchKernelGGL(refactor_kernel(a.N, k_is_matern(a.kernel_id)), dim3(c->nwin), dim3(WA_THREADS), 0, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window refactor launch")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_set_theta(cgp_ctx *c, const double *theta, int theta_stride, const unsigned char *select, double *logml,
                                    int *info) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  const int nth = ntheta(c->win.kernel_id, c->win.d);
  if (!theta || theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  // one pinned block [theta | logml | info | select] and its device twin: one H2D, the launch, one D2H, one synchronisation
  const size_t W = c->nwin, nt = W * nth, ni = (W + 1) / 2, ns = (W + 7) / 8, ndbl = nt + W + ni + ns;
  double *h, *d;
  if (!window_stage(c, ndbl * 8, ndbl * 8, h, d)) return CGP_ENOMEM;
  for (size_t w = 0; w < W; ++w) memcpy(h + w * nth, theta + w * theta_stride, nth * sizeof(double));
  unsigned char *hs = reinterpret_cast<unsigned char *>(h + nt + W + ni);
  for (size_t w = 0; w < W; ++w) hs[w] = select ? (select[w] ? 1 : 0) : 1;
  int *hi = reinterpret_cast<int *>(h + nt + W);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemsetAsync(d + nt, 0, (W + ni) * 8, s));   // unselected windows report logML 0, info 0
  HIP_TRY(c, hipMemcpyAsync(d, h, nt * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(d + nt + W + ni, hs, ns * 8, hipMemcpyHostToDevice, s));
  int rc = cgp_window_set_theta_device(c, d, nth, reinterpret_cast<unsigned char *>(d + nt + W + ni), d + nt, reinterpret_cast<int *>(d + nt + W), s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(h + nt, d + nt, (W + ni) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (logml) memcpy(logml, h + nt, W * sizeof(double));
  if (info) memcpy(info, hi, W * sizeof(int));
  return first_flagged_window(hi, W);
}

extern "C" int cgp_window_nll_grad_device(cgp_ctx *c, double *dnll, double *dgrad, int grad_stride, void *hip_stream) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (!dnll || !dgrad || grad_stride < ntheta(c->win.kernel_id, c->win.d)) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  AdaptArgs a = adapt_args(c);
  a.nll = dnll; a.grad = dgrad; a.grad_stride = grad_stride;
  const long long chunks = window_chunks(c);
  if (!fits_grid(chunks)) return CGP_EINVAL;
  launch_alpha(c, a, ws);
  hipLaunchKernelGGL(k_window_kinv_grad, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, ws, a);
  hipLaunchKernelGGL(k_window_grad_finish, dim3((unsigned)cdiv(c->nwin, 64)), dim3(64), 0, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

namespace {
// The host form of the three objectives (cgp_window_nll_grad, _multi_nll_grad, _loo_nll_grad), after the call's own checks: one
// device block [value | grad | nextra more doubles] and its pinned twin, `eval(dvalue, dgrad, grad_stride, dextra, stream)` -- the
// objective's device form; dextra is null when the caller passed no `extra` --, one D2H, one synchronisation, the gradient
// scattered by grad_stride.
template <class Eval>
int window_objective_host(cgp_ctx *c, double *value, double *grad, int grad_stride, double *extra, size_t nextra, Eval &&eval) {
  HIP_TRY(c, hipSetDevice(c->device));
  const int nth = ntheta(c->win.kernel_id, c->win.d);
  const size_t W = c->nwin, ndbl = W * (1 + nth) + nextra;
  double *h, *d;
  if (!window_stage(c, ndbl * 8, ndbl * 8, h, d)) return CGP_ENOMEM;
  hipStream_t s = c->stream;
  int rc = eval(d, d + W, nth, extra ? d + W * (1 + nth) : nullptr, s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(h, d, ndbl * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  memcpy(value, h, W * sizeof(double));
  for (size_t w = 0; w < W; ++w) memcpy(grad + w * grad_stride, h + W + w * nth, nth * sizeof(double));
  if (extra) memcpy(extra, h + W * (1 + nth), nextra * sizeof(double));
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_nll_grad(cgp_ctx *c, double *nll, double *grad, int grad_stride) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (!nll || !grad || grad_stride < ntheta(c->win.kernel_id, c->win.d)) return CGP_EINVAL;
  return window_objective_host(c, nll, grad, grad_stride, nullptr, 0, [&](double *dnll, double *dgrad, int stride, double *, hipStream_t s) {
    return cgp_window_nll_grad_device(c, dnll, dgrad, stride, s);
  });
}

// Leave-one-out cross-validation of the windows as they stand (cgp_window_loo.hpp): the gradient's first two launches, then the
// forward half of its substitution and the finish.  Alpha and the chunks' partial sums live where the gradient keeps alpha and
// its partial sums (WinBufs::grad_scratch: one double per chunk against the gradient's GRAD_N).
extern "C" int cgp_window_loo_device(cgp_ctx *c, double *dloo_mean, double *dloo_var, double *dloo_lpd, double *dlpd_sum,
                                     void *hip_stream) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (!dloo_mean && !dloo_var && !dloo_lpd && !dlpd_sum) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  const AdaptArgs a = adapt_args(c);
  const WindowLooOut out{dloo_mean, dloo_var, dloo_lpd, dlpd_sum, a.gpart};
  if (!fits_grid(window_chunks(c))) return CGP_EINVAL;
  launch_loo(c, a, out, ws);
  if (!hip_ok(c, hipGetLastError(), "window LOO launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_loo(cgp_ctx *c, double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  if (!loo_mean && !loo_var && !loo_lpd && !lpd_sum) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t W = c->nwin, WN = W * c->win.N, ndbl = 3 * WN + W;
  double *h, *d;
  if (!window_stage(c, ndbl * 8, ndbl * 8, h, d)) return CGP_ENOMEM;
  hipStream_t s = c->stream;
  int rc = cgp_window_loo_device(c, loo_mean ? d : nullptr, loo_var ? d + WN : nullptr, loo_lpd ? d + 2 * WN : nullptr,
                                 lpd_sum ? d + 3 * WN : nullptr, s);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(h, d, ndbl * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (loo_mean) memcpy(loo_mean, h, WN * sizeof(double));
  if (loo_var) memcpy(loo_var, h + WN, WN * sizeof(double));
  if (loo_lpd) memcpy(loo_lpd, h + 2 * WN, WN * sizeof(double));
  if (lpd_sum) memcpy(lpd_sum, h + 3 * WN, W * sizeof(double));
  return CGP_OK;
}

// m.optimize() on the resident windows: the batched L-BFGS driver of cgp_optimize_batch (one batched evaluation per round, every
// window its own stepper and line search) with set_theta + nll_grad on the windows themselves as the evaluation.
// The loop is written once: `eval(dnll, dgrad, grad_stride, stream)` enqueues the evaluation of every window where it stands --
// cgp_window_nll_grad_device (cgp_window_optimize) or the summed objective of the P columns (cgp_window_optimize_multi).
namespace {
template <class Eval>
int window_optimize_impl(cgp_ctx *c, int max_evals, const unsigned char *select, double *theta_out, int theta_stride,
                         double *logml_out, int *n_evals, Eval &&eval) {
  const int nth = ntheta(c->win.kernel_id, c->win.d);
  if (theta_out && theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t W = c->nwin;
  std::vector<double> cur(W * MAX_THETA);
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipMemcpy(cur.data(), c->win.theta, cur.size() * sizeof(double), hipMemcpyDeviceToHost));
  auto sel = [&](size_t w) { return !select || select[w] != 0; };
  for (size_t w = 0; w < W; ++w)
    for (int i = 0; i < nth; ++i)
      if (sel(w) && !(cur[w * MAX_THETA + i] > 0.0)) return CGP_EINVAL;
  // staging: [theta | nll | grad | logml | info | select], pinned and on the device
  const size_t nt = W * nth, ni = (W + 1) / 2, ns = (W + 7) / 8, ndbl = 2 * nt + 2 * W + ni + ns;
  double *h, *d;
  if (!window_stage(c, ndbl * 8, ndbl * 8, h, d)) return CGP_ENOMEM;
  double *hth = h, *hnll = h + nt, *hgrad = hnll + W, *hlm = hgrad + nt;
  int *hinfo = reinterpret_cast<int *>(hlm + W);
  unsigned char *hsel = reinterpret_cast<unsigned char *>(hlm + W + ni);
  const size_t o_nll = nt, o_grad = nt + W, o_lm = 2 * nt + W, o_info = o_lm + W, o_sel = o_info + ni;
  auto set_theta = [&]() -> int {    // the windows marked in hsel take hth
    HIP_TRY(c, hipMemcpyAsync(d, hth, nt * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_sel, hsel, ns * 8, hipMemcpyHostToDevice, s));
    return cgp_window_set_theta_device(c, d, nth, reinterpret_cast<unsigned char *>(d + o_sel), d + o_lm, reinterpret_cast<int *>(d + o_info), s);
  };
  // one round: the active windows take their trial theta and are evaluated where they stand; the others stay deselected, with
  // the theta they have.  A trial point that is not positive definite is infeasible (no jitter ladder).
  auto round = [&](const double *th, const char *active, double *f, double *g, char *feasible) -> int {
    memcpy(hth, th, nt * sizeof(double));
    for (size_t w = 0; w < W; ++w) hsel[w] = active[w] ? 1 : 0;
    int rc = set_theta();
    if (rc != CGP_OK) return rc;
    rc = eval(d + o_nll, d + o_grad, nth, s);
    if (rc != CGP_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(hnll, d + o_nll, (2 * W + nt + ni) * 8, hipMemcpyDeviceToHost, s));   // nll | grad | logml | info
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t w = 0; w < W; ++w) feasible[w] = hinfo[w] == 0 && std::isfinite(hnll[w]);
    memcpy(f, hnll, W * sizeof(double));
    memcpy(g, hgrad, nt * sizeof(double));
    return CGP_OK;
  };
  corenav::LbfgsBatchResult res;
  int rc = corenav::lbfgs_minimize_logexp_batch((int)W, nth, cur.data(), MAX_THETA, select, max_evals, round, res);
  if (rc != CGP_OK) return rc;
  // a window whose last trial was not its best point gets the best theta's factor back
  bool again = false;
  for (size_t w = 0; w < W; ++w) {
    hsel[w] = sel(w) && !res.last_is_best[w];
    again = again || hsel[w];
    for (int i = 0; i < nth; ++i) hth[w * nth + i] = std::max(res.theta[w * nth + i], 1e-300);
  }
  if (again) {
    rc = set_theta();
    if (rc != CGP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  for (size_t w = 0; w < W; ++w) {
    if (!sel(w)) continue;
    if (theta_out) memcpy(theta_out + w * theta_stride, hth + w * nth, nth * sizeof(double));
    if (logml_out) logml_out[w] = -res.f[w];
    if (n_evals) n_evals[w] = res.evals[w];
  }
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_window_optimize(cgp_ctx *c, int max_evals, const unsigned char *select, double *theta_out, int theta_stride,
                                   double *logml_out, int *n_evals) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  return window_optimize_impl(c, max_evals, select, theta_out, theta_stride, logml_out, n_evals,
                              [&](double *dnll, double *dgrad, int stride, hipStream_t s) {
                                return cgp_window_nll_grad_device(c, dnll, dgrad, stride, s);
                              });
}

// ---- multi-target windows: value, gradient and optimiser of the P columns' summed logML (cgp_window_multi_grad.hpp) ----
extern "C" int cgp_window_multi_grad_reserve(cgp_ctx *c) {
  if (!c) return CGP_ESTATE;
  if (c->dtype != CGP_F64) return CGP_EINVAL;
  if (c->nwin < 1 || c->wm.P < 1) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // an earlier reservation's buffers are idle
  window_drop(c, WinDrop::MultiGrad);
  const size_t W = c->nwin, P = c->wm.P, pt = cdiv(c->wm.P, WPB), nrow = (size_t)cdiv(c->win.N, WPB) * WPB;
  const WinSlot slots[] = {slot(c->wg.am, W * pt * nrow * WPB * 8, true), slot(c->wg.colval, W * P * 8, true)};
  if (window_alloc(c, WinDrop::MultiGrad, slots) != CGP_OK) return CGP_ENOMEM;
  return window_zero(c, WinDrop::MultiGrad, slots, "window multi grad reserve memsets / synchronise");
}

// Five launches: the diagonal blocks' inverses, Z = L^-1 Y with the columns' logml (cgp_window_predict_multi's second launch), A =
// L^-T Z, the contraction with dK/dtheta, the finish.  Sized by the capacity N; origin, size and tick count are read on the device.
extern "C" int cgp_window_multi_nll_grad_device(cgp_ctx *c, int P, double *dnll, double *dgrad, int grad_stride, double *dlogml,
                                                void *hip_stream) {
  int rc = window_multi_check(c, P, c && dnll && dgrad && grad_stride >= ntheta(c->win.kernel_id, c->win.d), true);
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  AdaptArgs a = adapt_args(c);
  a.nll = dnll; a.grad = dgrad; a.grad_stride = grad_stride;
  double *lm = dlogml ? dlogml : c->wg.colval;   // the value is read from it by the finish
  a.mlogml = lm;
  const ForecastForm zf = multi_win_form(a.N, true, k_is_matern(a.kernel_id));   // by N alone
  const ForecastArgs za = multi_z_args(c, zf, lm);   // cgp_window_predict_multi_device's second launch
  const long long chunks = window_chunks(c), tiles = (long long)c->nwin * a.pt;
  unsigned zgrid;
  if (!fits_grid(chunks) || xcd_grid((long long)c->nwin * za.nchunk, zgrid) != CGP_OK || !fits_grid(tiles)) return CGP_EINVAL;
  launch_diag_inv(c, ws);
  hipLaunchKernelGGL(zf.kernel, dim3(zgrid), dim3(WF_THREADS), zf.lds, ws, za);
  hipLaunchKernelGGL(k_window_multi_alpha, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, ws, a);
  hipLaunchKernelGGL(k_window_multi_kinv_grad, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, ws, a);
  hipLaunchKernelGGL(k_window_multi_grad_finish, dim3((unsigned)cdiv(c->nwin, 64)), dim3(64), 0, ws, a);
  if (!hip_ok(c, hipGetLastError(), "window multi-target gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_multi_nll_grad(cgp_ctx *c, int P, double *nll, double *grad, int grad_stride, double *logml) {
  int rc = window_multi_check(c, P, c && nll && grad && grad_stride >= ntheta(c->win.kernel_id, c->win.d), true);
  if (rc != CGP_OK) return rc;
  return window_objective_host(c, nll, grad, grad_stride, logml, logml ? (size_t)c->nwin * P : 0,   // [nll | grad | logml], the last only when asked for
                               [&](double *dnll, double *dgrad, int stride, double *dlogml, hipStream_t s) {
                                 return cgp_window_multi_nll_grad_device(c, P, dnll, dgrad, stride, dlogml, s);
                               });
}

// cgp_window_optimize with the summed objective: the same driver and the same round, the evaluation above in cgp_window_nll_grad_device's place.
extern "C" int cgp_window_optimize_multi(cgp_ctx *c, int P, int max_evals, const unsigned char *select, double *theta_out,
                                         int theta_stride, double *logml_sum_out, int *n_evals) {
  int rc = window_multi_check(c, P, true, true);
  if (rc != CGP_OK) return rc;
  return window_optimize_impl(c, max_evals, select, theta_out, theta_stride, logml_sum_out, n_evals,
                              [&](double *dnll, double *dgrad, int stride, hipStream_t s) {
                                return cgp_window_multi_nll_grad_device(c, P, dnll, dgrad, stride, nullptr, s);
                              });
}

// ---- leave-one-out objective of the resident windows: value, gradient and optimiser (cgp_window_loo_grad.hpp) ----------
namespace {
// the reservation's second block, in doubles: loo_var [W][N] | k_window_loo's chunk sums [W][NB] | lpd_sum [W] | c, b, beta
// [3][W][NP] | k_window_loo_grad's pair sums [W][npair][GRAD_N]
struct WindowLooGradPlan {
  size_t NP, nsup, npair, o_part, o_sum, o_c, o_b, o_beta, o_gpart, ndbl;
};
WindowLooGradPlan window_loo_grad_plan(const cgp_ctx *c) {
  WindowLooGradPlan q{};
  const size_t W = c->nwin, N = c->win.N, NB = cdiv(c->win.N, WPB);
  q.nsup = cdiv(c->win.N, WJ_ST * WPB);
  q.NP = q.nsup * WJ_ST * WPB;
  q.npair = q.nsup * (q.nsup + 1) / 2;
  q.o_part = W * N;
  q.o_sum = q.o_part + W * NB;
  q.o_c = q.o_sum + W;
  q.o_b = q.o_c + W * q.NP;
  q.o_beta = q.o_b + W * q.NP;
  q.o_gpart = q.o_beta + W * q.NP;
  q.ndbl = q.o_gpart + W * q.npair * GRAD_N;
  return q;
}
// the checks the objective's calls start with, before anything is enqueued
int window_loo_grad_check(const cgp_ctx *c, bool args_ok) {
  if (!c || c->nwin < 1 || !c->wl.kinv) return CGP_ESTATE;
  return args_ok ? CGP_OK : CGP_EINVAL;
}
}  // namespace

extern "C" int cgp_window_loo_grad_reserve(cgp_ctx *c) {
  if (!c || c->nwin < 1) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // an earlier reservation's buffers are idle
  window_drop(c, WinDrop::LooGrad);
  const WindowLooGradPlan q = window_loo_grad_plan(c);
  // no memset of Ky^-1: every reader masks what the call itself did not write (cgp_window_loo_grad.hpp)
  const WinSlot slots[] = {slot(c->wl.kinv, (size_t)c->nwin * q.NP * q.NP * 8), slot(c->wl.blk, q.ndbl * 8, true)};
  if (window_alloc(c, WinDrop::LooGrad, slots) != CGP_OK) return CGP_ENOMEM;
  return window_zero(c, WinDrop::LooGrad, slots, "window LOO gradient reserve memset / synchronise");
}

// Nine launches: cgp_window_loo_device's four as they stand (loo_var and lpd_sum into the reservation), then c and b, Ky^-1,
// beta, the product with its contraction, the finish.  Sized by the capacity N; origin, size and failure word are read on the device.
extern "C" int cgp_window_loo_nll_grad_device(cgp_ctx *c, double *dnlpd, double *dgrad, int grad_stride, double *dlogml,
                                              void *hip_stream) {
  int rc = window_loo_grad_check(c, c && c->nwin >= 1 && dnlpd && dgrad && grad_stride >= ntheta(c->win.kernel_id, c->win.d));
  if (rc != CGP_OK) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t ws = pick_stream(c, hip_stream);
  AdaptArgs a = adapt_args(c);
  a.grad = dgrad; a.grad_stride = grad_stride;
  const WindowLooGradPlan q = window_loo_grad_plan(c);
  double *blk = c->wl.blk;
  const WindowLooOut out{nullptr, blk, nullptr, blk + q.o_sum, blk + q.o_part};
  WindowLooGradArgs g{};
  g.kinv = c->wl.kinv;
  g.var = blk; g.lsum = blk + q.o_sum;
  g.cv = blk + q.o_c; g.bv = blk + q.o_b; g.beta = blk + q.o_beta; g.part = blk + q.o_gpart;
  g.nlpd = dnlpd; g.logml = dlogml;
  g.NP = (int)q.NP; g.npair = (int)q.npair; g.per_win = cdiv((int)q.npair, WJ_WAVES);
  const long long chunks = window_chunks(c);
  unsigned ggrid;
  if (!fits_grid(chunks) || xcd_grid((long long)c->nwin * g.per_win, ggrid) != CGP_OK || c->nwin > 65535) return CGP_EINVAL;   // (nwin is a grid.y below)
  launch_loo(c, a, out, ws);
  hipLaunchKernelGGL(k_window_loo_prep, dim3((unsigned)cdiv(g.NP, 256), c->nwin), dim3(256), 0, ws, a, g);
  hipLaunchKernelGGL(k_window_loo_kinv, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, ws, a, g);
  hipLaunchKernelGGL(k_window_loo_beta, dim3((unsigned)(g.NP / WLG_EB), c->nwin), dim3(WLG_WAVES * 64), 0, ws, a, g);
  hipLaunchKernelGGL(k_window_loo_grad, dim3(ggrid), dim3(WJ_THREADS), 0, ws, a, g);
  hipLaunchKernelGGL(k_window_loo_grad_finish, dim3((unsigned)cdiv(c->nwin, 64)), dim3(64), 0, ws, a, g);
  if (!hip_ok(c, hipGetLastError(), "window LOO gradient launches")) return CGP_EHIP;
  return CGP_OK;
}

extern "C" int cgp_window_loo_nll_grad(cgp_ctx *c, double *nlpd, double *grad, int grad_stride, double *logml) {
  int rc = window_loo_grad_check(c, c && c->nwin >= 1 && nlpd && grad && grad_stride >= ntheta(c->win.kernel_id, c->win.d));
  if (rc != CGP_OK) return rc;
  return window_objective_host(c, nlpd, grad, grad_stride, logml, c->nwin,   // [nlpd | grad | logml], the last staged whether asked for or not
                               [&](double *dnlpd, double *dgrad, int stride, double *dlogml, hipStream_t s) {
                                 return cgp_window_loo_nll_grad_device(c, dnlpd, dgrad, stride, dlogml, s);
                               });
}

// cgp_window_optimize with the leave-one-out objective: the same driver and the same round, the evaluation above in
// cgp_window_nll_grad_device's place; the driver's -f at the returned theta is lpd_sum.
extern "C" int cgp_window_optimize_loo(cgp_ctx *c, int max_evals, const unsigned char *select, double *theta_out, int theta_stride,
                                       double *lpd_sum_out, int *n_evals) {
  int rc = window_loo_grad_check(c, true);
  if (rc != CGP_OK) return rc;
  return window_optimize_impl(c, max_evals, select, theta_out, theta_stride, lpd_sum_out, n_evals,
                              [&](double *dnlpd, double *dgrad, int stride, hipStream_t s) {
                                return cgp_window_loo_nll_grad_device(c, dnlpd, dgrad, stride, nullptr, s);
                              });
}
