// cgp_sched_host.hpp -- host side of the fit schedules: every batch or single fit goes through run() below.  Which schedule a
// call takes is decided once, by sched_plan (cgp_sched_plan.hpp, plain host code with the measured crossovers); here are the
// launch helpers, the call's prologue and one enqueue function per schedule: enqueue_latency (k_tile_sk + k_trmm_sk),
// enqueue_launches (throughput / mid-size launches with their stream groups and the extra-row stream) and, in the measurement
// library, enqueue_one_launch (k_sched) and enqueue_look_ahead (two streams).  Each takes the plan and re-derives nothing it holds.
// Not a translation unit of its own: cgp_engine.hip includes it after cgp_ctx, tune_groups, the flop counts and group_view.
#pragma once

namespace {

static_assert(cgp_ctx::kMaxStreams == kSchedMaxGroups, "a call's stream groups are the context's worker streams");

struct Launcher {
  cgp_ctx *c;
  hipStream_t s;
  int pending = -1;
  void begin(int kernel, double flops, int step = -1) {
    if (!c->prof) return;
    if (c->prof_step >= 0 && !(kernel == 0 && step == c->prof_step)) return;  // one update launch per schedule
    ProfRec r{kernel, get_event(c), get_event(c), flops};
    (void)hipEventRecord(r.a, s);
    c->recs.push_back(r);
    pending = (int)c->recs.size() - 1;
  }
  void end() {
    if (!c->prof || pending < 0) return;
    (void)hipEventRecord(c->recs[pending].b, s);
    pending = -1;
  }
};

inline size_t alpha_lds_bytes(int NT) { return (size_t)(NT * TS + TS) * sizeof(double); }
template <typename T> constexpr int upd_lds_bytes() { return 4 * KT * LDST * (int)sizeof(T); }
template <typename T> constexpr int panel_lds_bytes() {   // + z of one block column; fp32 with the bf16 planes: planes + Gram inputs + z
  return (kF32Bf16x6 && sizeof(T) == 4) ? (bx_z_offset<false>() + TS) * 4 : upd_lds_bytes<T>() + TS * (int)sizeof(T);
}
static_assert(panel_lds_bytes<float>() >= WIMG * 4 && panel_lds_bytes<float>() >= upd_lds_bytes<float>() + TS * 4,
              "the panel kernels stage W_k's image (and k_rows64 its chunk buffers) over the loop's LDS");
template <typename T> constexpr int paneldiag_lds_bytes() { return std::max(panel_lds_bytes<T>(), diag_lds_elems<T>() * (int)sizeof(T)); }
// mid-size build: fp32 factors the diagonal tile in the fat form (potf2_tile), see mid_fat
template <typename T> constexpr int paneldiag_mid_lds_bytes() {
  return mid_fat<T, true>() ? std::max(paneldiag_lds_bytes<T>(), potf2_lds_elems<T>() * (int)sizeof(T)) : paneldiag_lds_bytes<T>();
}
static_assert(!kF32Bf16x6 || (bx_z_offset<true>() + TS) * 4 <= paneldiag_mid_lds_bytes<float>(), "mid-size build: the two plane buffers do not fit its LDS");
// the deep loop's chunk ring + z of one block column must fit what the mid-size build's launches carry
static_assert(deep_ring<float, true>() * KT * LDST * 4 + TS * 4 <= paneldiag_mid_lds_bytes<float>() &&
              deep_ring<double, true>() * KT * LDST * 8 + TS * 8 <= paneldiag_mid_lds_bytes<double>(), "mid-size build: ring does not fit its LDS");
template <typename T> constexpr int potf2_lds_bytes() {
  return (TS * LDP + 8 * DB * DB + 4 * DB * DB) * (int)sizeof(T) + 16;
}

#ifndef CGP_F32_FULL_DEEP
#define CGP_F32_FULL_DEEP 0   // `make variant` A/B: the deep-prefetch fp32 loops at full batch too (measured slower: 128 -> 168 VGPRs)
#endif
// hipFuncSetAttribute applies to the CURRENT device's function object: called from cgp_create after
// hipSetDevice, once per (device, dtype).
// (two contexts may be created from two threads at once: the per-device "done" marks are guarded by a mutex)
template <typename T> int set_lds_attrs(int device) {
  static bool done[64] = {false};
  std::lock_guard<std::mutex> lk(g_attr_mutex);
  if (device >= 0 && device < 64 && done[device]) return 0;
  const int upd = upd_lds_bytes<T>(), tile = potf2_lds_bytes<T>();
  auto set = [](const void *fn, int bytes) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess; };
  bool ok = true;
  ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, false>), panel_lds_bytes<T>());
  ok = ok && set(reinterpret_cast<const void *>(&k_grad<T>), upd);
  if constexpr (sizeof(T) == 8) {   // the Matern instantiations (fp64 only)
    ok = ok && set(reinterpret_cast<const void *>(&k_grad<T, 1>), upd);
    ok = ok && set(reinterpret_cast<const void *>(&k_grad<T, 2>), upd);
    ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, false, true, false, true>), panel_lds_bytes<T>());
    ok = ok && set(reinterpret_cast<const void *>(&k_tile_sk<T, true>), tile);
    ok = ok && set(reinterpret_cast<const void *>(&k_diag_lean<T, false, true>), paneldiag_lds_bytes<T>());
    ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, true, true, false, true>), paneldiag_lds_bytes<T>());
    ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, true, true, true, true>), paneldiag_mid_lds_bytes<T>());
#ifdef CGP_AB
    ok = ok && set(reinterpret_cast<const void *>(&k_diag<T, true>), tile);
#endif
  }
  ok = ok && set(reinterpret_cast<const void *>(&k_tile_sk<T>), tile);
  ok = ok && set(reinterpret_cast<const void *>(&k_trmm_sk<T>), upd);
  ok = ok && set(reinterpret_cast<const void *>(&k_diag_lean<T>), paneldiag_lds_bytes<T>());
  ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, true>), paneldiag_lds_bytes<T>());
  ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, true, true, true>), paneldiag_mid_lds_bytes<T>());
#ifdef CGP_AB
  ok = ok && set(reinterpret_cast<const void *>(&k_sched<T>), paneldiag_mid_lds_bytes<T>());
#endif
  if constexpr (sizeof(T) == 4) ok = ok && set(reinterpret_cast<const void *>(&k_refine_solve<float>), 160 * 1024);
  if constexpr (sizeof(T) == 4) ok = ok && set(reinterpret_cast<const void *>(&k_refine_gated<float>), 160 * 1024);
  if constexpr (mid_fat<T, true>()) ok = ok && set(reinterpret_cast<const void *>(&k_diag_lean<T, true>), paneldiag_mid_lds_bytes<T>());
  if constexpr (CGP_F32_FULL_DEEP && sizeof(T) == 4) ok = ok && set(reinterpret_cast<const void *>(&k_panel<T, true, true, false>), paneldiag_lds_bytes<T>());
#ifdef CGP_AB
  ok = ok && set(reinterpret_cast<const void *>(&k_diag<T>), tile);
#endif
  if (!ok) return -1;
  if (device >= 0 && device < 64) done[device] = true;
  return 0;
}

// The process's SchedSwitches (cgp_sched_plan.hpp), read from the environment once
const SchedSwitches &sched_switches() {
  static const SchedSwitches sw = [] {
    SchedSwitches w;
    // CGP_SCHED=throughput is honoured by every build: the tests use it to run the throughput schedule
    // on a handful of fits.
    const char *e = getenv("CGP_SCHED");
    const std::string sch = e ? e : "";
    w.no_latency = sch == "throughput";
#ifdef CGP_AB
    w.no_latency = w.no_latency || sch == "overlap" || sch == "splitdiag";
    w.split_diag = sch == "splitdiag";
    w.fused_diag = sch == "fuseddiag";
    w.no_latency = w.no_latency || w.fused_diag;
    w.overlap = sch == "overlap";
    w.one_launch = sch == "onelaunch";   // as measured it does not beat the launches
    const char *dg = getenv("CGP_DIAG");
    w.fat_diag = dg && std::string(dg) == "fat";
    const char *ac = getenv("CGP_ACC");
    w.acc_off = ac && std::string(ac) == "off";
    const char *tk = getenv("CGP_SK_TRMM");
    w.sk_fused_trmm = tk && std::string(tk) == "fused";
#endif
    return w;
  }();
  return sw;
}

// A launch of a kernel that builds Gram tiles: a Matern fit (fp64 contexts only, check_shape) runs the kernel's MAT = true
// instantiation, every other kernel id the instantiation it ran before the Matern kernels existed.
#define CGP_LAUNCH_GRAM(T, A, KERN, KERN_MAT, ...)                    \
  do {                                                                \
    bool cgp_matern_ = false;                                         \
    if constexpr (sizeof(T) == 8) {                                   \
      if (k_is_matern((A).kernel_id)) {                               \
        hipLaunchKernelGGL(KERN_MAT, __VA_ARGS__);                    \
        cgp_matern_ = true;                                           \
      }                                                               \
    }                                                                 \
    if (!cgp_matern_) hipLaunchKernelGGL(KERN, __VA_ARGS__);          \
  } while (0)

// k_panel<T, true> has two builds: the full-batch one, and the one for calls that leave CUs underfilled (kinds C /
// image-A compiled in; fp32: deep-prefetch loops)
template <typename T> void launch_panel_diag(bool mid, dim3 grid, hipStream_t s, const FitArgs &a, int k) {
  if (mid) {
    CGP_LAUNCH_GRAM(T, a, (k_panel<T, true, true, true>), (k_panel<T, true, true, true, true>), grid, dim3(256), paneldiag_mid_lds_bytes<T>(), s, a, k);
    return;
  }
  if constexpr (CGP_F32_FULL_DEEP && sizeof(T) == 4) hipLaunchKernelGGL((k_panel<T, true, true, false>), grid, dim3(256), paneldiag_lds_bytes<T>(), s, a, k);
  else CGP_LAUNCH_GRAM(T, a, (k_panel<T, true>), (k_panel<T, true, true, false, true>), grid, dim3(256), paneldiag_lds_bytes<T>(), s, a, k);
}

// The panel tiles of block step k without a diagonal tile: the split-diagonal and look-ahead schedules, predict after fit
template <typename T> void launch_panel(dim3 grid, hipStream_t s, const FitArgs &a, int k) {
  CGP_LAUNCH_GRAM(T, a, (k_panel<T, false>), (k_panel<T, false, true, false, true>), grid, dim3(256), panel_lds_bytes<T>(), s, a, k);
}

// The extra-row tiles of block step k alone (rows_from_extra), in the loop flavour of the mid-size build
template <typename T> void launch_panel_rows(dim3 grid, hipStream_t s, const FitArgs &a, int k) {
  CGP_LAUNCH_GRAM(T, a, (k_panel<T, false, true, false>), (k_panel<T, false, true, false, true>), grid, dim3(256), panel_lds_bytes<T>(), s, a, k);
}

template <typename T> void launch_diag(const FitArgs &a, int nfits, int k, bool fat, hipStream_t s, bool mid = false) {
  if constexpr (mid_fat<T, true>()) {
    if (mid) {
      hipLaunchKernelGGL((k_diag_lean<T, true>), dim3(nfits), dim3(256), paneldiag_mid_lds_bytes<T>(), s, a, k);
      return;
    }
  }
#ifdef CGP_AB
  if (fat) {
    CGP_LAUNCH_GRAM(T, a, (k_diag<T>), (k_diag<T, true>), dim3(nfits), dim3(256), potf2_lds_bytes<T>(), s, a, k);
    return;
  }
#endif
  (void)fat;
  CGP_LAUNCH_GRAM(T, a, (k_diag_lean<T>), (k_diag_lean<T, false, true>), dim3(nfits), dim3(256), paneldiag_lds_bytes<T>(), s, a, k);
}

// Refinement of an fp32 fit (cgp_refine.hpp; refine_steps in cgp_sched_plan.hpp says how many steps a call takes): under the
// default setting every fit of a window of at most three input dimensions takes them, beyond only the fits k_finalize marks
constexpr int kRefineAutoMaxD = 3;
inline bool refine_gated(const cgp_ctx *c, const FitArgs &a) { return c->refine < 0 && a.d > kRefineAutoMaxD; }
template <bool MEAN> void launch_refine_gemv(int rows, int nfits, hipStream_t s, const FitArgs &a, const RefineArgs &q) {
  const dim3 grid(cdiv(rows, RF_ROWS), nfits);
  if (a.kernel_id == K_RBF_BROWNIAN) hipLaunchKernelGGL((k_refine_gemv<float, 1, true, MEAN>), grid, dim3(256), 0, s, a, q);
  else if (a.d == 1) hipLaunchKernelGGL((k_refine_gemv<float, 1, false, MEAN>), grid, dim3(256), 0, s, a, q);
  else if (a.d == 2) hipLaunchKernelGGL((k_refine_gemv<float, 2, false, MEAN>), grid, dim3(256), 0, s, a, q);
  else if (a.d == 3) hipLaunchKernelGGL((k_refine_gemv<float, 3, false, MEAN>), grid, dim3(256), 0, s, a, q);
  else hipLaunchKernelGGL((k_refine_gemv<float, 0, false, MEAN>), grid, dim3(256), 0, s, a, q);
}
// The launches that follow k_finalize of `nfits` fits starting at fit g0 of the call: alpha_0 = L^-T z in double (in place of
// k_alpha), `steps` correction steps (solve = false: alpha of the last fit call is already in dref_a -- predict after fit),
// then the mean of the M test points.
inline void launch_refine(cgp_ctx *c, const FitArgs &a, int nfits, int g0, hipStream_t s, int steps, bool solve, bool alpha_for_all) {
  const RefineArgs q{c->dref_r + (size_t)g0 * c->alpha_stride, c->dref_a + (size_t)g0 * c->alpha_stride, c->alpha_stride, a.rflag};
  if (solve && q.flag && !alpha_for_all && a.NT <= kRefineGatedMaxNT) {
    // d > 3 under the default setting: k_finalize marked the dense fits, almost always none -- one launch, not four
    hipLaunchKernelGGL(k_refine_gated<float>, dim3(nfits), dim3(RS_THREADS), refine_gated_lds_bytes(a.NT), s, a, q, steps, a.M > 0 ? 1 : 0);
    return;
  }
  if (solve) {
    const size_t lds = refine_solve_lds_bytes(a.NT);
    RefineArgs q0 = q;
    if (alpha_for_all) q0.flag = nullptr;   // the caller asked for alpha (cgp_get_alpha): alpha_0 of every fit, marked or not
    hipLaunchKernelGGL(k_refine_solve<float>, dim3(nfits), dim3(RS_THREADS), lds, s, a, q0, 0);
    for (int st = 0; st < steps; ++st) {
      launch_refine_gemv<false>(a.N, nfits, s, a, q);
      hipLaunchKernelGGL(k_refine_solve<float>, dim3(nfits), dim3(RS_THREADS), lds, s, a, q, 1);
    }
  }
  if (a.M > 0) launch_refine_gemv<true>(a.M, nfits, s, a, q);
}
inline double refine_flops(const FitArgs &a, int nfits, int steps, bool solve) {   // covariance entries at (3 d + 20) flops + the two passes over the factor
  const double ent = (solve ? (double)steps * a.N * a.N : 0.0) + (double)a.M * a.N;
  return nfits * (ent * (3.0 * a.d + 20.0) + (solve ? (steps + 0.5) * 2.0 * a.N * a.N : 0.0));
}

// The launches that end the schedule of the `nfits` fits from fit g0 of the call (a: their view), on L's stream and each bracketed
// by L: k_finalize with TM test points per workgroup, k_alpha when the caller wants alpha, the fp32 refinement -- as the plan says
template <typename T, int TM>
void launch_epilogue(cgp_ctx *c, Launcher &L, const FitArgs &a, const SchedPlan &p, int nfits, int g0) {
  L.begin(3, nfits * (4.0 * a.M * a.N + 2.0 * a.N));
  hipLaunchKernelGGL((k_finalize<T, TM>), dim3(cdiv(a.M, TM) + 1, nfits), dim3(256), 0, L.s, a, p.in_rows ? 1 : 0);
  L.end();
  if (p.want_alpha) {
    L.begin(4, nfits * (double)a.N * a.N);
    hipLaunchKernelGGL(k_alpha<T>, dim3(nfits), dim3(256), alpha_lds_bytes(a.NT), L.s, a);
    L.end();
  }
  if (p.rsteps > 0) {
    L.begin(4, refine_flops(a, nfits, p.rsteps, p.rsolve));
    launch_refine(c, a, nfits, g0, L.s, p.rsteps, p.rsolve, p.ralpha_all);
    L.end();
  }
}

// One call on its way through a schedule: the plan, and what the prologue makes of it -- per stream group g of the plan's G the
// view ga[g] of its p.gb[g] fits, its stream gs[g] and the Launcher that brackets its launches under cgp_profile_enable
struct SchedCall {
  cgp_ctx *c;
  hipStream_t s;   // the caller's stream
  FitArgs a;       // the whole call
  int batch;
  SchedPlan p;
  FitArgs ga[kSchedMaxGroups];
  hipStream_t gs[kSchedMaxGroups];
  Launcher L[kSchedMaxGroups];
};

// What a call reads of the context and its arguments to decide its schedule (the measurement library's environment is run_schedule's to add)
template <typename T> SchedIn sched_in(const cgp_ctx *c, const FitArgs &a, int batch, bool in_rows, bool want_alpha) {
  SchedIn in;
  in.esz = (int)sizeof(T);
  in.batch = batch;
  in.NT = a.NT;
  in.ET = a.ET;
  in.M = a.M;
  in.xid = a.xid != 0;
  in.matern = k_is_matern(a.kernel_id);
  in.in_rows = in_rows;
  in.want_alpha = want_alpha;
  in.prof = c->prof;
  in.nstreams = c->nstreams;
  in.lat_cap = c->lat.lat_cap;
  in.mid_cap = c->mid_cap;
  in.lat_units = c->lat.lat_units;
  in.lat_img_fits = c->lat.lat_img_fits;
  in.lat_images_fit = lat_images(a.NT - 1) <= LAT_IMG_MAX;
  in.refine = c->refine;
  in.refined = c->refined;
  in.refine_bufs = c->dtype == CGP_F32 && c->dref_a;
  in.refine_max_nt = kRefineMaxNT;
  in.sw = sched_switches();
  return in;
}

// What every schedule starts with.  The batch is cut into the plan's contiguous groups, one worker stream each, forked from /
// joined to the caller's stream `s` with events.  tune: the stream-group tuner's step for this call (its first event goes
// on the caller's stream ahead of everything).
template <typename T> int sched_prologue(SchedCall &q, const TuneStep &tune) {
  cgp_ctx *c = q.c;
  const SchedPlan &p = q.p;
  FitArgs &a = q.a;
  a.rows_from_extra = p.in_rows ? 0 : 1;
  if constexpr (sizeof(T) == 4) a.rflag = p.rsteps > 0 && refine_gated(c, a) ? c->dref_flag : nullptr;
  if (tune.ev0) HIP_TRY(c, hipEventRecord(tune.ev0, q.s));
  for (int g = 0, g0 = 0; g < p.G; g0 += p.gb[g], ++g) {
    q.ga[g] = group_view<T>(a, g0);
    // group 0 stays on the caller's stream, the others go to worker streams: the workers live in another priority pool
    // (cgp_create), so they never share a hardware queue with the caller's stream -- two WORKER streams may share one
    // (the pool has few queues and every context creates eight streams: a 64-fit call as two groups on two workers ran
    // 1.37 instead of 0.92 ms whenever other contexts existed in the process)
    q.gs[g] = g == 0 ? q.s : c->wstream[g - 1];
    q.L[g] = Launcher{c, q.gs[g]};
  }
  hipLaunchKernelGGL(k_prep, dim3(cdiv(q.batch, 64)), dim3(64), 0, q.s, a, q.batch, c->dprep, p.in_rows ? 1 : 0,
                     (p.latency && p.in_rows) ? c->lat.dwready : nullptr);
  if (p.G > 1) {
    HIP_TRY(c, hipEventRecord(c->ev_fork, q.s));
    for (int g = 0; g < p.G; ++g)
      if (q.gs[g] != q.s) HIP_TRY(c, hipStreamWaitEvent(q.gs[g], c->ev_fork, 0));
  }
  if (p.use_acc) {   // (sched_plan has what the running sums are)
    const size_t half = (size_t)q.batch * a.M;
    for (int g = 0, g0 = 0; g < p.G; g0 += p.gb[g], ++g) {
      q.ga[g].macc = c->dmacc + (size_t)g0 * a.M;
      q.ga[g].vacc = c->dmacc + half + (size_t)g0 * a.M;
    }
  }
  return CGP_OK;
}

// Latency schedule for a handful of fits (k_tile_sk): the diagonal tile and
// the panel tiles of a step in one launch, inner dimension split over up to SK_MAX workgroups.
template <typename T> int enqueue_latency(SchedCall &q) {
  cgp_ctx *c = q.c;
  const FitArgs &a = q.ga[0];
  const bool in_rows = q.p.in_rows, split_trmm = q.p.split_trmm;
  const int batch = q.batch, upd_lds = upd_lds_bytes<T>(), tile_lds = potf2_lds_bytes<T>();
  Launcher &L = q.L[0];
  // tile slots per fit of THIS call (slab and tickets are indexed with it; the tickets are zero between launches whatever the stride)
  const int call_slots = a.NT + a.ET + 1;
  SplitArgs sa{c->lat.dpart, c->lat.dticket, call_slots, 1, in_rows ? 1 : 0, c->lat.dwready, c->lat.dlatimg, split_trmm ? 0 : 1};
  for (int k = 0; k < a.NT; ++k) {
    const int tiles = (in_rows ? a.NT - k - 1 : 0) + a.ET;
    const int nslots = tiles + (in_rows ? 1 : 0);
    // >= 8 chunks of 16 columns per range; a function of k only, so a fit's result does not
    // depend on how many fits share the call (the partial sums are added in range order)
    const int sk = std::max(1, std::min(SK_MAX, k));
    sa.sk = sk;
    L.begin(0, panel_flops(a.N, a.M, a.d, k, in_rows, batch) + (in_rows ? diag_flops(a.N, a.d, k, batch) : 0.0), k);
    // z also carries the pre-update workgroups of the NEXT diagonal tile (1 + images of tile k + 1)
    const int gz = in_rows ? std::max(sk, 1 + (k + 1 < a.NT ? lat_images(k + 1) : 0)) : sk;
    CGP_LAUNCH_GRAM(T, a, (k_tile_sk<T>), (k_tile_sk<T, true>), dim3(nslots, batch, gz), dim3(256), in_rows ? tile_lds : upd_lds, q.s, a, sa, k);
    L.end();
    if (split_trmm) {
      L.begin(2, trsm_flops(a.N, a.M, k, in_rows, batch));
      hipLaunchKernelGGL(k_trmm_sk<T>, dim3(tiles * TRMM_SPLIT, batch), dim3(64 * TRMM_WAVES), upd_lds, q.s, a, k);
      L.end();
    }
  }
  launch_epilogue<T, 8>(c, L, a, q.p, batch, 0);
  HIP_TRY(c, hipGetLastError());
  return CGP_OK;
}

#ifdef CGP_AB
// A mid-size fit call as ONE persistent launch (k_sched, cgp_kernels_fused.hpp): the tile programs of the NT + 1 launches
// become tasks of a list ordered by block step; per-fit progress counters replace the launch boundaries.  Bitwise the
// launches' results; measured slower than them (round 4), so it exists in the -DCGP_AB library only.
// The task list of a (fits, NT, ET) shape, kept in the context until another shape comes, and the grid that runs it.
template <typename T> int sched_task_list(cgp_ctx *c, int batch, int NT, int ET, int lag, hipStream_t s) {
  OneLaunchBufs &ol = c->ol;
  if (ol.key[0] == batch && ol.key[1] == NT && ol.key[2] == ET) return CGP_OK;
  std::vector<int4> tasks;
  auto put = [&](int kind, int k, int b, int rt) { tasks.push_back(make_int4(kind, k, b, rt)); };
  // Order: by block step; inside a step the chain first (A, then the pre-updates C and B), then the matrix rows' tiles (the
  // next step's chain reads them), and only then the EXTRA rows' tiles of the step BEFORE -- they feed nothing but their own
  // next block column, so they lag one step behind and fill in beside the chain.  CGP_SCHED_LAG=0: no lag (measurement).
  auto extra = [&](int k) {
    for (int e = 0; e < ET; ++e)
      for (int b = 0; b < batch; ++b) put(SCHED_T, k, b, NT + e);
  };
  for (int k = 0; k < NT; ++k) {
    if (k + 1 < NT) for (int b = 0; b < batch; ++b) put(SCHED_A, k, b, k + 1);
    if (k + 2 < NT) for (int b = 0; b < batch; ++b) put(SCHED_C, k, b, k + 2);
    if (k + 2 < NT && k >= 1) for (int b = 0; b < batch; ++b) put(SCHED_B, k, b, k + 2);
    for (int rt = k + 2; rt < NT; ++rt)
      for (int b = 0; b < batch; ++b) put(SCHED_T, k, b, rt);
    if (k - lag >= 0) extra(k - lag);
  }
  for (int k = std::max(0, NT - lag); k < NT; ++k) extra(k);
  if (!grow_device(ol.tasks, ol.tasks_cap, tasks.size() * sizeof(int4))) return CGP_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(ol.tasks, tasks.data(), tasks.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipStreamSynchronize(s));   // `tasks` is a local (once per shape)
  ol.ntasks = (int)tasks.size();
  ol.key[0] = batch;
  ol.key[1] = NT;
  ol.key[2] = ET;
  int occ = 0;
  HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_sched<T>, 256, paneldiag_mid_lds_bytes<T>()));
  ol.grid = std::max(1, std::min(ol.ntasks, std::max(1, occ) * std::max(1, c->n_cu)));
  return CGP_OK;
}
template <typename T> int run_sched(cgp_ctx *c, FitArgs a, int batch, int lag, hipStream_t s) {
  OneLaunchBufs &ol = c->ol;
  int rc = sched_task_list<T>(c, batch, a.NT, a.ET, lag, s);
  if (rc != CGP_OK) return rc;
  const int pstride = c->NTmax + c->ETmax, fstride = c->NTmax + 2;
  const size_t nflag = 2 + (size_t)batch * (pstride + 1 + 2 * fstride);
  const size_t img_bytes = (size_t)batch * c->NTmax * DPART * sizeof(T);
  if (!grow_device(ol.flags, ol.flags_cap, nflag * sizeof(int)) || !grow_device(ol.bimg, ol.bimg_cap, img_bytes) ||
      !grow_device(ol.cimg, ol.cimg_cap, img_bytes))
    return CGP_ENOMEM;
  HIP_TRY(c, hipMemsetAsync(ol.flags, 0, nflag * sizeof(int), s));
  int *fl = static_cast<int *>(ol.flags);
  SchedArgs sq{};
  sq.tasks = static_cast<const int4 *>(ol.tasks);
  sq.ntasks = ol.ntasks;
  sq.head = fl;
  sq.abort = fl + 1;
  sq.prog = fl + 2;
  sq.prog_stride = pstride;
  sq.wdone = sq.prog + (size_t)batch * pstride;
  sq.bflag = sq.wdone + batch;
  sq.cflag = sq.bflag + (size_t)batch * fstride;
  sq.flag_stride = fstride;
  a.dpart = ol.bimg;
  a.pimg = ol.cimg;
  a.img_slots = c->NTmax;
  a.diag_slots = 0;
  a.diag_stride = 0;
  hipLaunchKernelGGL(k_sched<T>, dim3(ol.grid), dim3(256), paneldiag_mid_lds_bytes<T>(), s, a, sq);
  return CGP_OK;
}
// (the whole call is group 0's view with all the fits: a call the tuner cut in two runs as one launch all the same)
template <typename T> int enqueue_one_launch(SchedCall &q) {
  launch_diag<T>(q.ga[0], q.batch, 0, q.p.fat_diag, q.s, true);   // diagonal tile 0: nothing to run beside it yet
  int rc = run_sched<T>(q.c, q.ga[0], q.batch, q.p.sched_lag, q.s);
  if (rc != CGP_OK) return rc;
  launch_epilogue<T, 64>(q.c, q.L[0], q.ga[0], q.p, q.batch, 0);
  HIP_TRY(q.c, hipGetLastError());
  return CGP_OK;
}

// Look-ahead schedule on two streams: the panel launch of step k is cut into P1 = the tile right
// below the diagonal (the only one the next diagonal tile needs) and P2 = all the others, and
//     sA:  P1(k) -> diag(k+1)            sB:  P2(k)
// run concurrently; events carry the cross dependencies.  Measured: no gain.
// sA = the context's HIGH-priority stream (the chain P1 -> diag must be dispatched ahead of the bulk P2 queued on the
// caller's stream; round 1-3 ran both on equal-priority worker streams, which may even have shared a hardware queue)
template <typename T> int enqueue_look_ahead(SchedCall &q) {
  cgp_ctx *c = q.c;
  hipStream_t s = q.s, sA = c->hstream, sB = s;
  auto ev = [&](int i) { return c->ev_look[i]; };
  HIP_TRY(c, hipEventRecord(c->ev_fork, s));
  HIP_TRY(c, hipStreamWaitEvent(sA, c->ev_fork, 0));
  FitArgs a1 = q.ga[0], a2 = q.ga[0];
  a1.tile_off = 0;
  a2.tile_off = 1;
  const int B = q.p.gb[0], NT = q.a.NT;
  launch_diag<T>(q.ga[0], B, 0, q.p.fat_diag, sA);
  HIP_TRY(c, hipEventRecord(ev(0), sA));                         // evD[0]
  for (int k = 0; k < NT; ++k) {
    const int nin = NT - k - 1;                                  // in-matrix tiles below the diagonal
    const bool has_p1 = nin >= 1;
    const int n2 = (has_p1 ? nin - 1 : 0) + q.a.ET;              // P2: everything but the first tile
    if (has_p1) {
      if (k > 0) HIP_TRY(c, hipStreamWaitEvent(sA, ev(3 * (k - 1) + 2), 0));  // P2(k-1)
      launch_panel<T>(dim3(1, B), sA, a1, k);
      HIP_TRY(c, hipEventRecord(ev(3 * k + 1), sA));             // evP1[k]
    }
    HIP_TRY(c, hipStreamWaitEvent(sB, ev(3 * k), 0));            // diag(k)
    if (k > 0 && NT - k >= 1) HIP_TRY(c, hipStreamWaitEvent(sB, ev(3 * (k - 1) + 1), 0));  // P1(k-1)
    launch_panel<T>(dim3(n2, B), sB, has_p1 ? a2 : a1, k);
    HIP_TRY(c, hipEventRecord(ev(3 * k + 2), sB));               // evP2[k]
    if (k + 1 < NT) {
      if (!has_p1 && k > 0) HIP_TRY(c, hipStreamWaitEvent(sA, ev(3 * (k - 1) + 2), 0));
      launch_diag<T>(q.ga[0], B, k + 1, q.p.fat_diag, sA);
      HIP_TRY(c, hipEventRecord(ev(3 * (k + 1)), sA));           // evD[k+1]
    }
  }
  HIP_TRY(c, hipStreamWaitEvent(sA, ev(3 * (NT - 1) + 2), 0));
  Launcher LA{c, sA};
  launch_epilogue<T, 64>(c, LA, q.ga[0], q.p, B, 0);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev_join[0], sA));
  HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join[0], 0));
  return CGP_OK;
}
#endif

// The extra-row launch E(k) of group g on the second stream (plan: xsplit; sched_plan has the timeline and the measurements)
template <typename T> int launch_step_extra_rows(SchedCall &q, Launcher &LE, int g, int k) {
  cgp_ctx *c = q.c;
  const FitArgs &a = q.a;
  const int nfits = q.p.gb[g];
  // E(k) needs W_k and the row panel k: diag(0) for k = 0, else everything up to A(k - 1), the last thing queued on s
  HIP_TRY(c, hipEventRecord(c->ev_look[k], q.gs[g]));
  HIP_TRY(c, hipStreamWaitEvent(LE.s, c->ev_look[k], 0));
  FitArgs ae = q.ga[g];
  ae.rows_from_extra = 1;
  LE.begin(0, panel_flops(a.N, a.M, a.d, k, false, nfits), k);
  if constexpr (sizeof(T) == 8) launch_panel_rows<T>(dim3(a.ET, nfits), LE.s, ae, k);
  else hipLaunchKernelGGL(k_rows64<T>, dim3(cdiv(a.M + 1, HR), nfits), dim3(256), panel_lds_bytes<T>(), LE.s, ae, k);
  LE.end();
  return CGP_OK;
}

// The fused panel launch of block step k of group g: the matrix rows' tiles (gx_t of them, with the extra rows' unless they are
// on the second stream), diagonal tile k + 1 finished in it (kind A) and tile k + 2 pre-updated (kind B; mid-size build: kind C
// pre-updates the next launch's kind-A tile, which then starts from that image)
template <typename T> void launch_step_panel_diag(SchedCall &q, int g, int k, int gx_t) {
  const FitArgs &a = q.a;
  const bool mid = q.p.mid;
  const int nfits = q.p.gb[g];
  const bool hasA = k + 1 < a.NT, hasB = k + 2 < a.NT && k >= 1;
  const bool hasC = mid && k + 2 < a.NT, imgA = mid && hasA && k >= 1;  // launch k - 1 had a kind C iff k + 1 < NT
  FitArgs ak = q.ga[g];
  ak.diag_slots = (hasA ? 1 : 0) | (hasB ? 2 : 0) | (hasC ? 4 : 0) | (imgA ? 8 : 0);
  ak.diag_stride = sizeof(T) == 8 || mid ? 2 : (CGP_F32_FULL_DEEP ? 3 : F32_FULL_OCC);  // workgroups per CU of k_panel<T, true> (LDS / VGPR bound)
  const int gx = gx_t + (hasB ? 1 : 0) + (hasC ? 1 : 0);  // gx_t already counts row tile k + 1 (kind A)
  // algorithmic flops of THIS launch: kind C does the part of tile (k + 2, k + 1) that kind A of launch k + 1 no longer does
  double fl = panel_flops(a.N, a.M, a.d, k, true, nfits) + (hasA ? diag_flops(a.N, a.d, k + 1, nfits) : 0.0);
  if (q.p.xsplit) fl -= panel_flops(a.N, a.M, a.d, k, false, nfits);
  auto tile_part = [&](int kc, int ncols) {  // Gram + `ncols` inner columns of one 128-row tile of block column kc, all fits
    const double w = std::min(TS, a.N - kc * TS), rows = std::min(TS, a.N - (kc + 1) * TS);
    return nfits * rows * w * (2.0 * ncols + (3.0 * a.d + 2.0));
  };
  if (imgA) fl -= tile_part(k, (k - 1) * TS);
  if (hasC) fl += tile_part(k + 1, k * TS);
  if (gx < 1) return;  // (mid-size call, last block step: the extra rows are all that is left)
  q.L[g].begin(0, fl, k);
  launch_panel_diag<T>(mid, dim3(gx, nfits), q.gs[g], ak, k);
  q.L[g].end();
}

// Fit launches: the diagonal tile k + 1 is finished inside the panel launch of step k and tile k + 2 is
// pre-updated there (k_panel<T, true>, diag_next), so only tile 0 has a launch of its own: NT + 1
// launches per fit schedule instead of 2 NT, and no launch in which one workgroup per fit factors a tile
// while the rest of the chip waits.  -DCGP_AB, CGP_SCHED=splitdiag: one k_diag_lean launch per step.
// Measured (same box, alternating libraries): fp32 N = 1024 +2.6 % fits/s, fp64 N = 2048 -0.7 % -- in fp64
// the diagonal launches are already MFMA-bound in their syrk part and two workgroups per CU leave the
// finisher's factorisation chain nothing to hide behind -- so at the bench batch fp64 keeps one k_diag_lean
// launch per step (CGP_SCHED=fuseddiag in a -DCGP_AB build selects the fused form there too).
// fp64: a diagonal launch is one workgroup per fit on a latency chain whose length does not depend on the
// batch (3.3 ms per N = 2048 schedule), so below FUSED64_BELOW fits per call the fused form wins there too
// (batch 32 +26 %, 64 +15 %, 128 +6 %, 256 +0.2 %, 512 -0.7 %).
// The launches are issued step-interleaved over the stream groups so every stream always has work queued.
template <typename T> int enqueue_launches(SchedCall &q) {
  cgp_ctx *c = q.c;
  const FitArgs &a = q.a;
  const SchedPlan &p = q.p;
  Launcher LE{c, c->wstream[0]};   // the extra rows' stream
  for (int k = 0; k < a.NT; ++k) {
    const int gx_t = (p.in_rows ? a.NT - k - 1 : 0) + (p.xsplit ? 0 : a.ET);
    for (int g = 0; g < p.G; ++g) {
      if (p.in_rows && (p.split_diag || k == 0)) {
        q.L[g].begin(1, diag_flops(a.N, a.d, k, p.gb[g]));
        launch_diag<T>(q.ga[g], p.gb[g], k, p.fat_diag, q.gs[g], p.mid && !p.split_diag);
        q.L[g].end();
      }
      if (p.xsplit) {
        int rc = launch_step_extra_rows<T>(q, LE, g, k);
        if (rc != CGP_OK) return rc;
      }
      if (p.split_diag) {
        q.L[g].begin(0, panel_flops(a.N, a.M, a.d, k, p.in_rows, p.gb[g]), k);
        launch_panel<T>(dim3(gx_t, p.gb[g]), q.gs[g], q.ga[g], k);
        q.L[g].end();
      } else launch_step_panel_diag<T>(q, g, k, gx_t);
    }
  }
  if (p.xsplit) {  // join: k_finalize reads the extra rows
    HIP_TRY(c, hipEventRecord(c->ev_join[0], LE.s));
    HIP_TRY(c, hipStreamWaitEvent(q.gs[0], c->ev_join[0], 0));
  }
  for (int g = 0, g0 = 0; g < p.G; g0 += p.gb[g], ++g) launch_epilogue<T, 64>(c, q.L[g], q.ga[g], p, p.gb[g], g0);
  HIP_TRY(c, hipGetLastError());
  for (int g = 0; g < p.G; ++g) {
    if (q.gs[g] == q.s) continue;   // ran on the caller's stream itself
    hipEvent_t ej = c->ev_join[(g + 1) % cgp_ctx::kMaxStreams];   // ([0] is the extra rows' join)
    HIP_TRY(c, hipEventRecord(ej, q.gs[g]));
    HIP_TRY(c, hipStreamWaitEvent(q.s, ej, 0));
  }
  return CGP_OK;
}

// Enqueue the whole schedule for `batch` fits: decide (sched_plan; an fp32 call of 56 ... 96 fits asks the stream-group tuner
// and decides again with its answer), start (sched_prologue), and hand the call to its schedule's enqueue function.
// in_rows = false: predict after fit (only the extra row tiles).
template <typename T>
int run_schedule(cgp_ctx *c, const FitArgs &a, int batch, bool in_rows, bool want_alpha, hipStream_t s) {
  SchedIn in = sched_in<T>(c, a, batch, in_rows, want_alpha);
  if constexpr (kAbBuild) {   // measurement: integer overrides from the environment (cgp_sched_plan.hpp says what each moves)
    auto env = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : kNoOverride; };
    static const int x32env = env("CGP_XSPLIT32"), lagenv = env("CGP_SCHED_LAG");
    in.lat_fits_env = env("CGP_LAT_FITS");
    in.mid_fits_env = env("CGP_MID_FITS");
    in.group0_env = env("CGP_GROUP0");
    in.xsplit32_env = x32env;
    in.sched_lag_env = lagenv;
  }
  SchedCall q{c, s, a, batch, sched_plan(in)};
  TuneStep tune;
  if (q.p.tune_eligible) {
    tune = tune_groups(c, batch, a.NT, s);
    in.tuned_groups = tune.groups;
    q.p = sched_plan(in);
  }
  if (in_rows || want_alpha) c->refined = q.p.rsolve;
  int rc = sched_prologue<T>(q, tune);
  if (rc != CGP_OK) return rc;
  switch (q.p.sched) {
    case Sched::Latency: return enqueue_latency<T>(q);
#ifdef CGP_AB
    case Sched::OneLaunch: return enqueue_one_launch<T>(q);
    case Sched::LookAhead: return enqueue_look_ahead<T>(q);
#endif
    default: break;
  }
  rc = enqueue_launches<T>(q);
  if (rc != CGP_OK) return rc;
  if (tune.ev1) HIP_TRY(c, hipEventRecord(tune.ev1, s));
  if (tune.entry) ++tune.entry->state;
  return CGP_OK;
}

int run(cgp_ctx *c, const FitArgs &a, int batch, bool in_rows, bool want_alpha, hipStream_t s) {
  return c->dtype == CGP_F64 ? run_schedule<double>(c, a, batch, in_rows, want_alpha, s)
                             : run_schedule<float>(c, a, batch, in_rows, want_alpha, s);
}

}  // namespace
