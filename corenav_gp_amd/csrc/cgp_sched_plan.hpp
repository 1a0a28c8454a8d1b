// cgp_sched_plan.hpp -- which schedule a fit call takes, decided once per call as plain host code: the measured crossovers, the
// record of what the decision reads (SchedIn), the decision (SchedPlan) and the one function that makes it (sched_plan).
// No HIP header and nothing of the kernels: the two kernel constants the decision needs arrive as SchedIn members, so a
// stand-alone C++ program can print the table (tests/sched_plan_table.cpp, tests/test_sched_plan_cpu.py).
// The enqueue functions of cgp_sched_host.hpp take the plan and re-derive nothing it holds.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>

namespace cgp {

#ifdef CGP_AB
constexpr bool kAbBuild = true;
#else
constexpr bool kAbBuild = false;
#endif

// Batches up to this size take the latency schedule: the measured crossover against the (mid-size) throughput
// schedule (tools/lat_crossover.sh, round 3: N = 2048 fp64 8 fits 1.87 vs 2.64 ms, 12 fits 2.72 vs 2.66; N = 1024 fp32
// 20 fits 0.641 vs 0.672 ms, 24 fits 0.769 vs 0.712) is 11 fits in fp64 and 20 in fp32 (16 / 24 before the mid-size form).
constexpr int LAT_FITS_F64 = 11, LAT_FITS_F32 = 20;
// The shorter the window, the larger the call the latency schedule still wins (tools/lat_crossover.sh by window length, end of
// round 3, ms per call latency vs throughput).  fp64: N = 256 32 fits 0.171 vs 0.240, 48 fits 0.225 vs 0.245; N = 512 28 fits 0.417 vs
// 0.422 (no extra-row split), 32 fits 0.464 vs 0.456; N = 768 20 fits 0.607 vs 0.657, 24 fits 0.681 vs 0.681; N = 1024 16 fits 0.835 vs
// 0.920, 20 fits 1.010 vs 0.954; N = 1536 12 fits 1.487 vs 1.635, 16 fits 1.926 vs 1.682; N = 2048 11 (above).  fp32: N = 256 32 fits
// 0.124 vs 0.133, 48 fits 0.154 vs 0.138; N = 512 24 fits 0.261 vs 0.272, 28 fits 0.290 vs 0.276; N = 768 20 fits 0.412 vs 0.414; N = 1024
// 20 (above).  The slabs are sized for LAT_FITS_SHORT fits.
// (Round 4, tools/check_crossovers.py: fp64 N = 256 33 fits 0.168 latency vs 0.205 throughput -- the limit of 32 was the slab's,
// not the crossover's; with round 3's 48 fits 0.225 vs 0.245 the fp64 limit for one and two block steps is 48.)
constexpr int LAT_FITS_SHORT = 32, LAT_FITS_SHORT64 = 48;
inline int lat_fits_by_steps(bool f64, int NT) {
  if (NT <= 2) return f64 ? LAT_FITS_SHORT64 : LAT_FITS_SHORT;
  if (f64) return NT <= 4 ? 28 : NT <= 6 ? 22 : NT <= 8 ? 18 : NT <= 12 ? 13 : LAT_FITS_F64;
  return NT <= 4 ? 24 : LAT_FITS_F32;
}
constexpr int FUSED64_BELOW = 512;                // fp64 throughput schedule: diagonal tiles inside the panel launches below this batch
// Calls too small to fill the chip (a launch then lasts as long as its longest workgroup chain): the next launch's
// kind-A tile is pre-updated by a kind-C workgroup (k_panel), and fp32 takes the deep-prefetch loops (DEEP).
// Measured crossover (tools/r3_mid2.sh, same box, CGP_MID_FITS either side): fp32 N = 1024: 32 fits +14 %, 48 +13 %,
// 64 +9 %, 96 +2 %, 128 -4 %; fp64 N = 2048: 24 fits +18 %, 32 +11 %, 48 +4 %, 64 -2 %.
constexpr int MID_FITS_F64 = 48, MID_FITS_F32 = 96;
#ifndef CGP_NO_EXTRA_SPLIT
#define CGP_NO_EXTRA_SPLIT 0   // `make variant` A/B: mid-size calls keep the extra rows inside the factorisation launches
#endif
constexpr bool kNoExtraSplit = CGP_NO_EXTRA_SPLIT != 0;
#ifndef CGP_LAT_MIN_NT
#define CGP_LAT_MIN_NT 1   // block steps from which a handful of fits takes the latency schedule (3 until the end of round 3: `make variant` A/B)
#endif
// fp64 mid-size calls put their extra rows on a second stream when there is enough of them: fits x block steps >= this
// (tools/r3_xs_n.sh, same box, with / without, ms per call: N = 2048 28 fits 3.77 / 3.70, 36 fits 4.25 / 4.45, 48 fits 5.01 / 5.70;
// N = 1536 36 fits 2.37 / 2.38, 48 fits 2.71 / 3.01; N = 1024 36 fits 1.27 / 1.17, 48 fits 1.29 / 1.31; N = 512 28 fits 0.52 / 0.42)
constexpr int XSPLIT64_WORK = 480;
#ifndef CGP_XSPLIT32_FITS
#define CGP_XSPLIT32_FITS 0    // fp32 mid-size calls from this many fits: extra rows on the second stream as 64-row tiles (k_rows64); 0 = never.
                               // Measured (round 5, ms per call without / with): 24 fits 0.629 / 0.647, 32 0.686 / 0.777, 48 0.770 / 0.791, 64 0.994 / 0.954,
                               // 96 1.282 / 1.270 -- bitwise the one-stream results, but two stream GROUPS (0.895 at 64 fits) beat it: not taken
#endif
constexpr int XSPLIT32_FITS = CGP_XSPLIT32_FITS;
constexpr int MID_FITS_ALLOC = kAbBuild ? 512 : (MID_FITS_F64 > MID_FITS_F32 ? MID_FITS_F64 : MID_FITS_F32);
constexpr int LAT_FITS_ALLOC = kAbBuild ? 64 : LAT_FITS_SHORT64;  // slabs are sized for min(this, max_batch) fits
// An integer override of the measurement library that its environment does not set (SchedIn: lat_fits_env ... group0_env)
constexpr int kNoOverride = INT_MIN;
// fp64 by window length (tools/r3_mid_n2.sh, end of round 3, with the extra-row split by work; mid-size form off / on, ms per call):
// N = 2048 64 fits 7.26 / 6.87, 96 fits 9.80 / 9.67; N = 1536 96 fits 5.14 / 4.95; N = 1024 96 fits 2.22 / 2.10; N = 768 64 fits 1.06 /
// 1.01, 80 fits 1.16 / 1.16, 96 fits 1.27 / 1.28; N = 512 96 fits 0.645 / 0.663 -- up to 96 fits from eight block steps, 64 from six.
inline int mid_fits(bool f64, int NT, int env) {     // ablation build: CGP_MID_FITS (env) moves the crossover (measurement)
  if (kAbBuild && env != kNoOverride) return std::max(0, std::min(env, MID_FITS_ALLOC));
  if (f64) return NT >= 8 ? MID_FITS_F32 : NT >= 6 ? 64 : MID_FITS_F64;
  return MID_FITS_F32;
}
inline int lat_fits(bool f64, int NT, int env) {     // ablation build: CGP_LAT_FITS (env) moves the crossover (measurement)
  if (kAbBuild && env != kNoOverride) return std::max(0, std::min(env, LAT_FITS_ALLOC));
  return lat_fits_by_steps(f64, NT);
}

// A/B switches of the schedule.  The shipped library has ONE schedule pair (throughput: k_diag_lean +
// k_panel with running predictive sums; latency: k_tile_sk + k_trmm_sk for <= LAT_FITS_F64 / LAT_FITS_F32 fits); the
// alternatives measured in DESIGN.md (one diagonal launch per step, two-stream overlap,
// fat diagonal, finalize without accumulators, fused trmm) exist only in a -DCGP_AB build, where the
// environment selects them once per process (sched_switches, cgp_sched_host.hpp).
struct SchedSwitches {
  bool no_latency = false, split_diag = false, fused_diag = false, overlap = false, fat_diag = false, acc_off = false,
       sk_fused_trmm = false;
  bool one_launch = false;   // CGP_SCHED=onelaunch: a mid-size call as one persistent launch (k_sched)
};

constexpr int kSchedMaxGroups = 8;   // stream groups of a call: the context's worker streams (cgp_ctx::kMaxStreams)

// What the decision reads: the call, the context's state and capacities, the switches
struct SchedIn {
  int esz = 8;                          // element size: 8 = fp64, 4 = fp32
  int batch = 1, NT = 1, ET = 1, M = 0;   // fits, block steps, extra-row tiles (ET = ceil((M + 1) / 128) >= 1 always), test points
  bool xid = false, matern = false;     // FitArgs::xid (the extra rows are an identity: gradient-mode calls), a Matern kernel id
  bool in_rows = true;                  // false: predict after fit (only the extra row tiles)
  bool want_alpha = false;
  bool prof = false;                    // cgp_profile_enable
  int nstreams = 0;                     // cgp_set_streams
  int lat_cap = 0, mid_cap = 0;         // the context's capacities (cgp_create_ex)
  size_t lat_units = 0;
  int lat_img_fits = 0;
  bool lat_images_fit = true;           // lat_images(NT - 1) <= LAT_IMG_MAX: the diagonal tile's pre-update images hold this window (N <= 2560)
  int refine = -1;                      // cgp_set_refine
  bool refined = false;                 // dref_a holds the refined alpha of the last fit call
  bool refine_bufs = false;             // the context has the refinement's buffers (fp32 contexts)
  int refine_max_nt = 0;                // kRefineMaxNT: block steps the refinement kernels' LDS holds
  SchedSwitches sw;
  // measurement library only, read from the environment by the caller: CGP_LAT_FITS, CGP_MID_FITS, CGP_XSPLIT32, CGP_GROUP0, CGP_SCHED_LAG
  int lat_fits_env = kNoOverride, mid_fits_env = kNoOverride, xsplit32_env = kNoOverride, group0_env = kNoOverride, sched_lag_env = kNoOverride;
  int tuned_groups = 0;                 // the stream-group tuner's answer (tune_groups) once SchedPlan::tune_eligible asked for it; 0: not asked
};

enum class Sched { Latency, OneLaunch, LookAhead, Launches };

struct SchedPlan {
  Sched sched = Sched::Launches;
  bool latency = false;      // the call is in the latency schedule's range (k_prep then resets the published block steps)
  bool mid = false;          // the mid-size build of the launches (kinds C / image-A; fp32: deep-prefetch loops)
  bool split_diag = false;   // one diagonal launch per block step
  bool xsplit = false;       // the extra rows on the second stream
  bool use_acc = false;      // running predictive sums inside k_panel
  bool split_trmm = true;    // latency schedule: k_trmm_sk launches of their own
  bool fat_diag = false;     // measurement: the diagonal launches in the fat form (k_diag)
  int sched_lag = 1;         // one-launch schedule: block steps the extra rows' tasks lag behind the chain (CGP_SCHED_LAG)
  bool tune_eligible = false;   // the caller asks tune_groups and decides again with SchedIn::tuned_groups
  int G = 1;                 // stream groups, and the fits of each
  int gb[kSchedMaxGroups] = {0};
  // how the schedule ends: k_alpha or not, refinement steps (0: none), with a solve for alpha_0 or on the alpha the fit call
  // left, alpha of every fit or of the marked
  bool in_rows = true, want_alpha = false;
  int rsteps = 0;
  bool rsolve = false, ralpha_all = false;
};

// Refinement of an fp32 fit (cgp_refine.hpp): how many steps this call takes, and whether every fit takes them or only the
// ones k_finalize marks as dense (FitArgs::rflag, RF_RHO).  -1 (the default) = one step; every fit of a window of at most three
// input dimensions (measured, 40 fits of N = 1000, mean error against the oracle without / with: d = 1 1.0e-3 / 6e-7, d = 2
// 7e-4 / 1.5e-7, d = 3 3.1e-4 with a worst fit at 1.1e-3 / 1e-7), the marked fits beyond (d = 4: two windows of 43 000 fuzz cases
// at 1.1 and 1.3e-3, rho = 21; d = 6: 7e-5, worst 1.8e-4, rho 3 ... 8): BASELINE configs[2] (d = 6, rho 3 ... 11.5) pays one
// launch whose workgroups return at once (k_refine_gated).
static inline int refine_steps(const SchedIn &in) {
  if (in.esz != 4 || !in.refine_bufs || in.xid || in.NT > in.refine_max_nt) return 0;
  // one step contracts the mean's error by ~1e-3 on most windows (N = 1536 / 2048 / 3000, d = 1, a lone fit: 2.4e-3 / 8.8e-4 / 2.4e-3 ->
  // 1.8e-6 / 6.0e-6 / 1.9e-6) but by as little as 2e-2 on some -- 6.7e-3 -> 1.4e-4 -> 2.6e-6 at N = 4 500; in batched calls of N = 1 100
  // the sweep found single fits at 3 ... 7e-5 after one step (six in ~3 000 refined cases) -- so windows of more than 1 024 samples
  // take two (the contract for a refined mean is 5e-5: include/corenav_gp.h)
  if (in.refine < 0) return in.NT > 8 ? 2 : 1;
  return std::min(in.refine, 3);
}

// The schedule of one call.  In the order it is decided: how the call ends (refinement), latency or not, mid-size or not, the
// stream groups, diagonal form, extra-row split, predictive sums, and last which of the four schedules enqueues it.
// (static: the library exports nothing of it)
static inline SchedPlan sched_plan(const SchedIn &in) {
  const SchedSwitches &sw = in.sw;
  const bool f64 = in.esz == 8, in_rows = in.in_rows;
  const int batch = in.batch, NT = in.NT;
  SchedPlan p;
  // fp32: alpha and the mean refined against a double-precision residual (cgp_refine.hpp).  A fit call computes alpha for it;
  // a predict-after-fit call (in_rows = false) reuses the alpha the fit call left in dref_a.
  p.rsteps = refine_steps(in);
  p.rsolve = p.rsteps > 0 && (in_rows || in.want_alpha);
  if (p.rsteps > 0 && !p.rsolve && !in.refined) p.rsteps = 0;
  p.ralpha_all = p.rsolve && in.want_alpha;
  p.in_rows = in_rows;
  p.want_alpha = in.want_alpha && !p.rsolve;   // alpha_0 comes from k_refine_solve (double precision, dref_a): no k_alpha launch
  const bool auto_groups = in.nstreams == 0;
  int G = auto_groups ? 1 : std::max(1, std::min(std::min(in.nstreams, kSchedMaxGroups), batch));
  // latency schedule: a handful of fits, windows long enough for splitting to pay and short enough for the
  // diagonal tile's pre-update images (N <= 2560); anything else takes the throughput schedule
  // (the slab / image capacities are part of the predicate: a call they cannot hold -- only reachable with the measurement
  // build's CGP_LAT_FITS override -- takes the mid-size or throughput schedule instead of failing after k_prep was queued)
  const int latf = lat_fits(f64, NT, in.lat_fits_env);
  const bool latency = !sw.no_latency && batch <= std::min(latf, in.lat_cap) && NT >= CGP_LAT_MIN_NT && in.lat_images_fit &&
                       (size_t)batch * (NT + in.ET + 1) <= in.lat_units && (NT < 3 || batch <= in.lat_img_fits);
  const bool mid = batch <= std::min(mid_fits(f64, NT, in.mid_fits_env), in.mid_cap);  // the whole call (the images are indexed by fit)
  // A latency-schedule call is one chain; an fp64 mid-size call has its own concurrency (factorisation || extra rows, below).
  // An fp32 mid-size call honours cgp_set_streams: cut into groups on worker streams, the chain-bound early launches of
  // one group run beside the others' (64 x N=1024: 0.99 -> 0.92 ms per call at two groups) -- as long as every group stays
  // above the latency schedule's range (a group that small would switch schedule: four groups of 16 measured 1.50 ms).
  // Two groups, from 56 fits (measured, ms per call at 1 / 2 / 3 groups: 48 fits 0.77 / 0.83 / 0.83, 64 fits 0.99 / 0.92 / 1.48,
  // 96 fits 1.24 / 1.17 / 1.66).
  // Since round 5 the engine takes that split by itself (cgp_set_streams(0), the default): every caller of a 56 ... 96-fit fp32
  // call -- cgp_sweep_*, a plain C host -- gets the 0.90 ms, not only a caller that knew to ask; cgp_set_streams(1) keeps one group.
  if (latency || (mid && f64)) G = 1;
  if (mid && !f64 && (G > 1 || auto_groups)) {
    G = batch >= 56 && batch / 2 > latf ? 2 : 1;
    if (G == 2 && auto_groups && in_rows && !in.prof) {   // the default does not assume that two groups run side by side: it measures
      p.tune_eligible = true;
      if (in.tuned_groups > 0) G = in.tuned_groups;
    }
  }
  if (in.prof || !in_rows) G = 1;  // per-kernel timing wants isolated launches
  const bool fused64 = sw.fused_diag || batch < FUSED64_BELOW;
  const bool split_diag = sw.split_diag || !in_rows || (f64 && !fused64);
  // Mid-size calls: the extra rows (test points and y: M + 1 of them against N - 128 (k + 1) matrix rows, i.e. most of
  // the update work) do not feed the factorisation, only their own next block column.  They get launches of their own on
  // a second stream -- E(k), after the launch that finished diagonal tile k -- so the chain-bound factorisation launches
  // A(k) (few workgroups, long chains) run beside the MFMA-bound extra-row launches instead of in lock-step with them:
  //     s :  diag(0)  A(0)  A(1)  A(2) ...            A(k): matrix tiles of step k + kinds A / B / C
  //     sE:           E(0)  E(1)  E(2) ...            E(k) waits for A(k - 1) (W_k, row panel k) and follows E(k - 1)
  // Measured (tools/r3_xsplit.sh, same box, variant without the split): fp64 N = 2048 48 fits 5.58 -> 4.99 ms, 32 fits 4.03 ->
  // 3.92, 24 fits 3.48 -> 3.51, 12 fits 2.62 -> 3.45 (the call is one chain then: nothing to run beside it); fp32 N = 1024
  // 64 fits 0.99 -> 1.01, 32 fits 0.69 -> 0.76: its launches last as long as kind A's chain at every k, so the extra rows'
  // last launches only queue up behind it, and two contexts overlap worse (0.76 -> 0.96 ms per call).  fp64 from 28 fits.
  // (not under cgp_profile_enable: per-launch events of two concurrent streams would overlap in time and their sum overstate the kernel)
  // fp32: the extra rows go to the second stream as 64-row tiles (k_rows64) from XSPLIT32_FITS fits per call
  int x32 = XSPLIT32_FITS;
  if (kAbBuild && in.xsplit32_env >= 0) x32 = in.xsplit32_env;   // measurement: CGP_XSPLIT32=<min fits> moves the threshold (0: never)
  const bool xsplit_on = f64 ? batch * NT >= XSPLIT64_WORK : (x32 > 0 && batch >= x32);
  p.xsplit = mid && !latency && xsplit_on && in_rows && !split_diag && G == 1 && in.ET > 0 && !kNoExtraSplit && !in.prof;
  p.latency = latency;
  p.mid = mid;
  p.split_diag = split_diag;
  p.G = G;
  for (int g = 0; g < G; ++g) {
    p.gb[g] = batch / G + (g < batch % G ? 1 : 0);
    // measurement: CGP_GROUP0 = fits of group 0 of two (uneven halves run out of step with each other)
    if (kAbBuild && G == 2 && in.group0_env > 0 && in.group0_env < batch) p.gb[g] = g == 0 ? in.group0_env : batch - in.group0_env;
  }
  // throughput schedule: the predictive sums V z and |V|^2 accumulate inside k_panel (block column
  // k - 1 while it streams through the row fragments of step k); k_finalize then only adds the last
  // block column instead of reading all of V.
  // (No memset of the sums: block step 1 -- the first that has a finished block column behind it -- WRITES them, later steps add;
  // the two fill launches were 10 us at the head of every call.  A window of one block step has nothing to accumulate.)
  p.use_acc = !latency && !sw.acc_off && in.M > 0 && !in.xid && NT >= 2;
  p.split_trmm = !sw.sk_fused_trmm;
  p.fat_diag = sw.fat_diag;
  if (kAbBuild && in.sched_lag_env != kNoOverride) p.sched_lag = in.sched_lag_env;
  // which schedule enqueues the call.  The measurement library's two alternatives come first, as they always did: the one-launch
  // form takes mid-size fit calls only, the two-stream look-ahead any one-group fit call of two block steps or more
  if (mid && !latency && in_rows && !in.prof && NT >= 2 && sw.one_launch && !in.matern && !sw.split_diag && !sw.overlap) p.sched = Sched::OneLaunch;
  else if (kAbBuild && sw.overlap && in_rows && G == 1 && !in.prof && NT >= 2) p.sched = Sched::LookAhead;
  else if (latency) p.sched = Sched::Latency;
  else p.sched = Sched::Launches;
  return p;
}

}  // namespace cgp
