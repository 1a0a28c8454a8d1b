// cgp_engine.hip -- context, launch schedule and the C ABI of include/corenav_gp.h.
// Host side of the slip-GP hot path; the arithmetic is in cgp_kernels.hpp (HIP, gfx950 only).
// There is no CPU fallback anywhere in this file: without a usable device cgp_create returns NULL.
#include "../../include/corenav_gp.h"
#include "cgp_kernels.hpp"
#include "cgp_kernels_fused.hpp"
#include "cgp_window.hpp"
#include "cgp_window_forecast.hpp"
#include "cgp_window_adapt.hpp"
#include "cgp_window_loo.hpp"
#include "cgp_window_loo_grad.hpp"
#include "cgp_window_joint.hpp"
#include "cgp_window_pgrad.hpp"
#include "cgp_window_multi.hpp"
#include "cgp_window_multi_grad.hpp"
#include "cgp_joint.hpp"
#include "cgp_multi.hpp"
#include "cgp_multi_grad.hpp"
#include "cgp_trend.hpp"
#include "cgp_sparse.hpp"
#include "cgp_sparse_grad.hpp"
#include "cgp_pgrad.hpp"
#include "cgp_lookahead.hpp"
#include "cgp_small.hpp"
#include "cgp_loo.hpp"
#include "cgp_loo_grad.hpp"
#include "cgp_refine.hpp"
#include "cgp_sched_plan.hpp"
#include "gp_predictor_core.hpp"
#include "gp_predictor.h"
#include "lbfgs.hpp"
#include "slip_recorder.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace cgp;

static_assert(CGP_MAX_D == MAXD, "header / kernel MAXD mismatch");
static_assert(CGP_DEBUG_SLOTS == DBG_SLOTS, "header / kernel debug slot mismatch");
static_assert(CGP_MAX_THETA == MAX_THETA, "header / kernel MAX_THETA mismatch");
static_assert(CGP_SMALL_OUT == SM_OUT, "header / kernel short-window record mismatch");

namespace {

struct ProfRec {
  int kernel;
  hipEvent_t a, b;
  double flops;
};

// What a feature's cgp_*_reserve leaves in the context: the device scratch its kernels work in, sized for up to max_batch fits x
// max_dim test points or targets (0: nothing reserved), and the staging block of its host calls, grown on demand and kept
// (scratch_free / scratch_check / scratch_reserve below)
struct Scratch {
  void *buf = nullptr;
  int max_batch = 0, max_dim = 0;
  void *stage = nullptr;
  size_t stage_cap = 0;
};

// The fit schedules' own device buffers (cgp_sched_host.hpp), each() naming the pointers once for cgp_destroy.
struct LatBufs {   // latency schedule, allocated by cgp_create_ex:
  void *dpart = nullptr;     // partial tiles [lat_units][SK_MAX][128*128]
  int *dticket = nullptr;    // arrival tickets [lat_cap][sk_slots]
  int *dwready = nullptr;    // published block steps [lat_cap]
  void *dlatimg = nullptr;   // pre-updated diagonal tiles [lat_img_fits][2][LAT_IMG_MAX][DPART]
  int lat_cap = 0;           // fits the latency slabs are sized for: min(LAT_FITS_ALLOC, max_batch)
  size_t lat_units = 0;      // fits x tile slots the partial-tile slab holds
  int lat_img_fits = 0;      // fits the pre-update image buffer holds (only windows of >= 3 block steps use it)
  int sk_slots = 0;          // tile slots per fit of the longest window: NTmax + ETmax + 1
  size_t part_bytes(size_t esz) const { return lat_units * SK_MAX * TS * TS * esz; }
  size_t img_bytes(size_t esz) const { return (size_t)lat_img_fits * 2 * LAT_IMG_MAX * DPART * esz; }
  template <class F> void each(F &&f) { f(dpart); f(dticket); f(dwready); f(dlatimg); }
};
struct OneLaunchBufs {   // one-launch schedule of a mid-size call (k_sched), grown on demand: task list of the last (fits, NT, ET) shape,
  void *tasks = nullptr, *flags = nullptr, *bimg = nullptr, *cimg = nullptr;   // flag words, one image slot per tile index
  size_t tasks_cap = 0, flags_cap = 0, bimg_cap = 0, cimg_cap = 0;
  int key[3] = {0, 0, 0}, ntasks = 0, grid = 0;
  template <class F> void each(F &&f) { f(tasks); f(flags); f(bimg); f(cimg); }
};

// The sliding windows' device buffers: one record per reservation, one hipMalloc per member, the reservation's capacity beside
// them.  each() names the members once, for window_release; which record goes with which is window_drop's to say (cgp_window_host.hpp).
struct WinBufs {   // cgp_window_init: factors [nwin][CAP][CAP], z = L^-1 y [nwin][CAP], inputs [nwin][d][CAP], targets [nwin][CAP],
  double *L = nullptr, *z = nullptr, *xw = nullptr, *yw = nullptr;
  int *state = nullptr;            // state words [nwin][4],
  double *prep_theta = nullptr;    // prep [nwin][PREP_N] | theta [nwin][MAX_THETA],
  double *dinv = nullptr;          // k_window_diag_inv's inverses of the factors' 16 x 16 diagonal blocks [nwin][NB][256],
  double *grad_scratch = nullptr;  // alpha [nwin][NB * 16] | chunk sums [nwin][NB][GRAD_N] | values [nwin] (adapt_args carves it)
  template <class F> void each(F &&f) { f(L); f(z); f(xw); f(yw); f(state); f(prep_theta); f(dinv); f(grad_scratch); }
};
struct WinJointBufs {   // cgp_window_joint_reserve: V kept [nwin][mt][NB * 16][16], the matrix / its factor [nwin][(mt * 16)^2],
  double *V = nullptr, *C = nullptr, *mean_var = nullptr;   // mean | variance [2][nwin][max_m],
  int *jinfo = nullptr;                                     // failure words [nwin]
  int max_m = 0;                                            // test points the reservation holds; 0 = none
  template <class F> void each(F &&f) { f(V); f(C); f(mean_var); f(jinfo); }
};
struct WinMultiBufs {   // cgp_window_multi_reserve: the target store [nwin][P][N], its tick counts [nwin], the Z scratch
  double *ystore = nullptr;   // [nwin][ceil(P / 16)][NB * 16][16], and column 0 of a push gathered for the push kernels
  int *ycount = nullptr;      // [nwin][ticks], which regrows on its own (cgp_window_push_multi_device)
  double *zs = nullptr, *y0 = nullptr;
  int P = 0;          // the reservation's P; 0 = none
  size_t ticks = 0;   // ticks per push the gather block holds
  template <class F> void each(F &&f) { f(ystore); f(ycount); f(zs); f(y0); }
};
struct WinMultiGradBufs {   // cgp_window_multi_grad_reserve: the A scratch [nwin][ceil(P / 16)][NB * 16][16] (null = none) and the
  double *am = nullptr, *colval = nullptr;   // per-column values [nwin][P] a call without a logml buffer writes
  template <class F> void each(F &&f) { f(am); f(colval); }
};
struct WinTrendBufs {   // cgp_window_trend_reserve: the contraction of all P columns [nwin][P][max_m] | their evidence [nwin][P],
  double *mean0 = nullptr, *sl = nullptr;   // and S [nwin][P up to 16][16] | L_A^-1 [nwin][16][16] (cgp_trend.hpp)
  int q = 0, max_m = 0;                     // the reservation's basis columns and test points; 0 = none
  template <class F> void each(F &&f) { f(mean0); f(sl); }
};
struct WinLooGradBufs {   // cgp_window_loo_grad_reserve: Ky^-1 of every window [nwin][NP][NP], NP = N rounded up to 64 (null = none),
  double *kinv = nullptr, *blk = nullptr;   // and one block of per-sample vectors, partial sums and per-window values (WindowLooGradPlan)
  template <class F> void each(F &&f) { f(kinv); f(blk); }
};

}  // namespace

struct cgp_ctx {
  int device = 0, dtype = CGP_F64;
  int max_n = 0, max_m = 0, max_d = 0, max_batch = 0;
  int NTmax = 0, ETmax = 0, ld = 0;
  size_t esz = 8;
  hipStream_t stream = nullptr;
  // worker streams: a batch is cut into groups whose schedules run concurrently, so the
  // one-workgroup-per-fit potf2 launches of one group overlap the MFMA launches of the others
  static constexpr int kMaxStreams = 8;
  hipStream_t wstream[kMaxStreams] = {nullptr};
  hipStream_t hstream = nullptr;   // highest stream priority: for a latency chain that must be dispatched AHEAD of bulk work on the caller's stream
  hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams] = {nullptr};
  // Two stream groups or one for an fp32 call of 56 ... 96 fits?  Decided per caller stream by timing one call each way (run_schedule).
  struct GroupTune {
    hipStream_t stream = nullptr;
    int batch = 0, NT = 0;     // the entry is for calls of this many fits and block steps on `stream`
    int state = -1;            // -1 free, else eligible calls seen on this stream so far (kTuneDecide and beyond: decided)
    int groups = 2;
    float ms[2] = {0.f, 0.f};
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t mon[2] = {nullptr, nullptr};   // after the decision: one call in a while bracketed, read later with hipEventQuery
    bool mon_pending = false;
    int slow = 0;                              // consecutive monitored calls well above what the chosen form measured
    int retune = 24;                           // decided calls until the two forms are measured again: 24, 48, ... kRetune
    unsigned long long used = 0;
  } tune[4];
  unsigned long long tune_clock = 0;
  hipEvent_t ev_look[3 * 64] = {nullptr};  // look-ahead schedule: diag / P1 / P2 completion per step
  int nstreams = 0;   // cgp_set_streams: 0 = the engine decides (two groups for fp32 calls of 56 ... 96 fits, else one); n >= 1 = as told
  // device buffers
  void *Lw = nullptr, *Winv = nullptr, *dX = nullptr, *dXs = nullptr, *dy = nullptr;
  void *Lp = nullptr;   // fp32: the panel tiles of a mid-size call as bf16 planes [mid_cap][3][lw_stride] (cgp_kernels_fused.hpp, bx6p_loop)
  void *dmean = nullptr, *dvar = nullptr, *dalpha = nullptr;
  // fp32 contexts: mixed-precision refinement of alpha and the predictive mean (cgp_refine.hpp, cgp_set_refine)
  double *dref_r = nullptr, *dref_a = nullptr;   // [max_batch][alpha_stride] residual, alpha in double precision
  int *dref_flag = nullptr;                      // [max_batch] fits k_finalize marked as dense (d > 3 under the default setting)
  int refine = -1;        // -1: the engine decides (one step: every fit at d <= 3, the dense ones beyond), 0: never, 1..3: that many steps for every call
  bool refined = false;   // dref_a holds the refined alpha of the fits of the last fit call (cgp_predict / cgp_get_alpha use it)
  double *dtheta = nullptr, *djitter = nullptr, *dlogml = nullptr, *dprep = nullptr;
  long long *ddbg = nullptr;
  double *dgpart = nullptr;
  LatBufs lat;             // latency schedule: its slabs and their capacities
  double *dmacc = nullptr;  // [max_batch][2][max_m] running predictive sums (throughput schedule, fp64)
  void *ddiagimg = nullptr;  // [max_batch][2][DPART] pre-updated diagonal tiles (throughput schedule, diag_next)
  void *dpanimg = nullptr;   // [min(max_batch, mid cap)][2][DPART] pre-updated kind-A panel tiles (k_panel kind C)
  int mid_cap = 0;
  OneLaunchBufs ol;   // one-launch schedule of a mid-size call (k_sched, measurement library)
  int n_cu = 0;
  // cgp_fit_predict_batch staging, grown on demand and kept: pinned host buffers (hipHostMalloc) so the
  // H2D / D2H copies are real asynchronous DMA, and a raw fp64 device buffer the pack kernels read
  void *pin_in = nullptr, *pin_out = nullptr, *draw = nullptr;
  size_t pin_in_cap = 0, pin_out_cap = 0, draw_cap = 0;
  double *la_buf = nullptr;  // cgp_predict_stop_batch staging, grown on demand
  int *la_ibuf = nullptr;
  size_t la_nd = 0, la_ni = 0;
  // sliding windows (cgp_window_*)
  WindowArgs win{};
  int nwin = 0;
  int win_o = 0, win_n = 0;   // origin / size of the windows (they advance in lock-step), mirrored on the host to cut a push into launches
  // their buffers and the four reservations' (the records above name every member and its shape).  Lifetimes, as window_drop
  // states them: the windows go -> every reservation goes; the multi-target reservation goes -> its objective's and its trend's scratch go;
  // the joint forecast's and the leave-one-out objective's scratch go alone.
  WinBufs wb;            // cgp_window_init (win points into it)
  WinJointBufs wj;       // joint forecast: cgp_window_joint_reserve
  WinMultiBufs wm;       // multi-target windows: cgp_window_multi_reserve
  WinMultiGradBufs wg;   // their summed objective: cgp_window_multi_grad_reserve
  WinTrendBufs wt;       // explicit basis functions on the multi-target windows: cgp_window_trend_reserve
  WinLooGradBufs wl;     // leave-one-out objective: cgp_window_loo_grad_reserve
  // joint forecast after batch / single fits (cgp_joint_reserve): the posterior covariance or its factor [max_batch][(mt * 16)^2],
  // then the factorisations' failure words [max_batch]; staging of the host sampling calls [xi | out]
  Scratch fj;
  // multi-target fits (cgp_multi_reserve): Z = L^-1 Y of up to max_batch fits x max_dim targets, [fit][NT 128][P padded to 128];
  // staging of the host call [Y | mean | logml]
  Scratch mz;
  int mz_form = 0;   // cgp_multi_set_form: 0 = the engine picks the solve's tile height, 64 / 128 = as told (tests)
  // explicit basis functions after the multi-target fits (cgp_trend_reserve): per fit the contraction and the evidence of the
  // max_dim + 16 packed columns, S = G^T [Z | G] and L_A^-1 (cgp_trend_host.hpp, trend_layout); staging of the host call
  // [Y | H | Hs | mean | beta | logml | tinfo]
  Scratch tr;
  int tr_max_m = 0;
  // sparse (inducing-point) fits (cgp_sparse_reserve): all the scratch of the sparse calls, for up to max_batch fits of max_dim
  // inducing inputs and sp_max_n samples (cgp_sparse_host.hpp, sparse_layout); staging of the host call
  Scratch sp;
  int sp_max_n = 0, sp_max_m = 0;
  // the sparse fits' objective (cgp_sparse_grad_reserve): A, T and G_uu of up to max_batch fits of max_dim inducing inputs and the
  // partial sums of sg_max_n samples (cgp_sparse_grad_host.hpp, sparse_grad_layout); staging of the host calls
  Scratch sg;
  int sg_max_n = 0;
  // several target columns on one sparse fit (cgp_sparse_multi_reserve): what up to max_dim columns add to the sparse scratch of up
  // to max_batch fits of sm_max_ind inducing inputs and sm_max_n samples (cgp_sparse_multi_host.hpp, sparse_multi_layout); staging
  // of the host call
  Scratch sm;
  int sm_max_n = 0, sm_max_ind = 0;
  // the objective of several target columns on one sparse fit (cgp_sparse_multi_grad_reserve): the operand image of That where the
  // targets add a tile row and the columns' bounds, for up to max_batch fits of mg_max_ind inducing inputs and max_dim columns
  // (cgp_sparse_multi_grad_host.hpp, sparse_multi_grad_layout); staging of the host calls
  Scratch mg;
  int mg_max_ind = 0;
  // multi-target objective (cgp_multi_grad_reserve): A = Ky^-1 Y of up to max_batch fits x max_dim targets, [fit][P padded to 16][NT 128],
  // then (max_batch, max_dim) logml; staging of the host calls [Y | nll | grad | logml]
  Scratch ma;
  // predictive gradients (cgp_pgrad_reserve): B^T = (Ky^-1 K*)^T and alpha of up to max_batch fits x max_dim test points,
  // [fit][NT 128][M + 1 padded to 128]; the host calls' outputs [dmean | dvar]
  Scratch pg;
  // leave-one-out objective (cgp_loo_grad_reserve): S = Ky^-1 diag(sqrt c) of up to max_batch fits, [fit][NTmax 128][NTmax 128], then
  // four vectors per fit, lpd_sum and logml (max_dim is 1); staging of the host calls [nlpd | grad | logml]
  Scratch lg;
  // cgp_window_push staging, grown on demand and kept: one pinned host block and one device block per direction
  void *win_pin = nullptr, *win_dev = nullptr;
  size_t win_pin_cap = 0, win_dev_cap = 0;
  // gradient-mode evaluations (cgp_nll_grad / cgp_optimize*): theta + jitter out, partial sums + logML + info back, one pinned block
  void *opt_pin = nullptr;
  size_t opt_pin_cap = 0;
  int *dinfo = nullptr;
  double *dsmall = nullptr;   // [max_batch][SM_OUT] results of the one-launch short-window kernel (k_small, fp64 contexts)
  unsigned short *dsmdeal = nullptr;   // k_small's helper work lists (sm_build_deal) of every NB <= SM_MAX_NB, at smdeal_off[NB]
  int *dsmdone = nullptr;              // k_small_predict's count of finished workgroups (the node callback polls a pinned word the last one writes)
  int small_seq = 0;
  size_t smdeal_off[SM_MAX_NB + 1] = {0};
  std::vector<char> xs_stage;     // cgp_predict's test points in the device layout: the source of an asynchronous copy, kept until the next call
  std::vector<double> lazy_win;   // [X (N, d) | y] of the window a short-window kernel evaluated in place (ensure_fitted uploads it)
  int pending_tab = 0;               // tick-grid table size cgp_fit_predict_batch found for the batch it is about to submit (0: none)
  bool last_small_dev = false;       // ... or window 0's record of the last batched fit + predict launch, still in dsmall
  double last_small[SM_OUT] = {0};   // the last single-window short-window record (the kernels write it to pinned host memory)
  size_t lw_stride = 0, winv_stride = 0, alpha_stride = 0;
  // state of the last single fit (cgp_fit -> cgp_predict)
  bool have_fit = false;
  bool lazy_fit = false;      // the window, theta and jitter of the last short-window evaluation are on the device but the factor
                              // panel is not: cgp_predict / cgp_get_alpha / cgp_get_factor run the fit schedule first (ensure_fitted)
  double f_meandiag_x = 0.0;  // mean |x| of that window's first input (GPy jitchol's mean(diag) for the Brownian factor)
  int fN = 0, fd = 0, fkernel = 0;
  double ftheta[CGP_MAX_THETA] = {0};
  double fjitter = 0.0;
  // profiling
  bool prof = false;
  int prof_step = -1;  // >= 0: only the update launch of this block step is bracketed (cgp_profile_enable(2 + k))
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  double prof_ms[CGP_PROF_KERNELS] = {0}, prof_flops[CGP_PROF_KERNELS] = {0};
  long long prof_n[CGP_PROF_KERNELS] = {0};
  std::string err;
};

namespace {

// cgp_ctx::GroupTune's state machine: two stream groups or one for this eligible call (fp32, mid-size, 56 ... 96 fits, the
// engine decides) of `batch` fits and NT block steps on the caller's stream s.
// Whether the two groups really run side by side depends on how the runtime mapped the caller's stream and the worker
// stream onto its few hardware queues -- the process's history, which nothing reports: the same 64-fit call took 0.89 ms
// on the legacy stream and 1.28 ms (the two groups in order: worse than one group's 0.98) on a fresh torch stream or on a
// context created later in the process (tools/sweep_probe.py, stream_probe.py; a probe with spin kernels did not predict
// it, both groups on the context's own streams was no better, and a single timed call does not show it: it is a
// steady-state effect of calls issued back to back).  So the default does not assume: per caller stream, after two
// warm-up calls, four eligible calls run as two groups and four as one, each run bracketed by events on the caller's
// stream, and from then on the faster form is used.  Results are bitwise the same either way.
// Every kRetune calls the two runs are repeated (a caller that first synchronises after every call and later issues calls
// back to back sees the other behaviour: sweep_probe.py's 1.24 ms): 8 calls in 264, half of them at the slower setting.
// The measurement never blocks the caller and never touches a stream that is being captured: the decision is read with
// hipEventQuery (until the last timed call has finished the call keeps two groups and asks again next time), an entry is
// keyed by (stream, fits, block steps) -- a caller that mixes shapes on one stream gets one decision per shape --, a pair
// of spans that differ by more than 4 x is the caller's own host gaps, not the schedules (discarded, measured again), and
// while the stream is capturing (cgp_set_streams documents fixing the form for graphs; this keeps the default safe) the
// call takes the form already decided, or two groups, without recording or reading any timing event.
struct TuneStep {
  int groups = 2;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // events to record on the caller's stream before / after this call
  cgp_ctx::GroupTune *entry = nullptr;       // non-null: this call belongs to the tuning runs (++entry->state once it is enqueued)
};
TuneStep tune_groups(cgp_ctx *c, int batch, int NT, hipStream_t s) {
  int G = 2;
  cgp_ctx::GroupTune *tune = nullptr;
  hipEvent_t tune_ev0 = nullptr, tune_ev1 = nullptr;
  constexpr int kWarm = 2, kRun = 4, kTuneDecide = kWarm + 2 * kRun, kRetune = 256;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
  if (capturing) (void)hipGetLastError();
  cgp_ctx::GroupTune *t = nullptr, *lru = &c->tune[0];
  for (auto &e : c->tune) {
    if (e.state >= 0 && e.stream == s && e.batch == batch && e.NT == NT) t = &e;
    if (e.used < lru->used) lru = &e;
  }
  if (!t && !capturing) {
    t = lru;
    t->stream = s;
    t->batch = batch;
    t->NT = NT;
    t->state = 0;
    t->groups = 2;
    for (auto &e : t->e)
      if (!e && hipEventCreate(&e) != hipSuccess) {   // no events: keep the two groups, never measure
        (void)hipGetLastError();
        t->state = kTuneDecide + 1;
      }
    for (auto &e : t->mon)
      if (!e && hipEventCreate(&e) != hipSuccess) (void)hipGetLastError();   // (no monitor then)
    t->mon_pending = false;
    t->slow = 0;
    t->retune = 24;
  }
  if (capturing) {
    G = t && t->state > kTuneDecide ? t->groups : 2;
    t = nullptr;
  }
  if (t) {
    t->used = ++c->tune_clock;
    // (the first decisions are re-checked early: a context's first calls run while the part is still coming out of idle -- both forms
    // then measure alike, 4.70 / 4.72 ms per four calls where warm they are 4.5 / 2.9 -- and the decision is a coin toss)
    if (t->state > kTuneDecide + t->retune) {
      t->state = kWarm;
      t->retune = std::min(2 * t->retune, kRetune);
    }
    if (t->state == kTuneDecide) {
      float m2 = 0.f, m1 = 0.f;
      const hipError_t qe = hipEventQuery(t->e[3]);
      if (qe == hipSuccess && hipEventElapsedTime(&m2, t->e[0], t->e[1]) == hipSuccess &&
          hipEventElapsedTime(&m1, t->e[2], t->e[3]) == hipSuccess) {
        t->ms[0] = m2;
        t->ms[1] = m1;
        if (m2 > 4.f * m1 || m1 > 4.f * m2) t->state = kWarm - 1;   // host gaps, not schedules: measure again
        else t->groups = m2 <= m1 ? 2 : 1;
        ++t->state;
        static const bool trace = getenv("CGP_TUNE_TRACE") != nullptr;   // development aid: what was measured and decided
        if (trace) fprintf(stderr, "cgp tune: ctx %p stream %p fits %d NT %d: two groups %.3f ms, one group %.3f ms per %d calls -> %s\n", (void *)c, (void *)s,
                           batch, NT, m2, m1, kRun, t->state == kWarm ? "measure again" : (t->groups == 2 ? "two groups" : "one group"));
      } else {
        (void)hipGetLastError();   // not ready (or a failed query): nothing sticks, two groups for this call, ask again
        if (qe != hipErrorNotReady) t->state = kTuneDecide + 1;
      }
    }
    if (t->state == kTuneDecide) {
      G = 2;
    } else if (t->state > kTuneDecide) {
      G = t->groups;
      ++t->state;
      // The stream -> hardware-queue mapping the decision rests on can change under a long-lived caller (other contexts and
      // streams come and go): one call in a while is bracketed by two events that a LATER call reads without blocking; three
      // such calls in a row at more than 1.3 x what the chosen form measured send the entry back to measuring.
      if (t->mon[0] && t->mon[1]) {
        if (t->mon_pending) {
          const hipError_t qm = hipEventQuery(t->mon[1]);
          if (qm == hipSuccess) {
            float ms1 = 0.f;
            const float base = t->ms[t->groups == 2 ? 0 : 1] / (float)kRun;
            if (hipEventElapsedTime(&ms1, t->mon[0], t->mon[1]) == hipSuccess && base > 0.f) t->slow = ms1 > 1.3f * base ? t->slow + 1 : 0;
            t->mon_pending = false;
            if (t->slow >= 3) {
              t->slow = 0;
              t->state = kWarm;
              static const bool trace2 = getenv("CGP_TUNE_TRACE") != nullptr;
              if (trace2) fprintf(stderr, "cgp tune: ctx %p stream %p: three monitored calls above 1.3 x %.3f ms (last %.3f): measuring again\n", (void *)c, (void *)s, base, ms1);
            }
          } else (void)hipGetLastError();
        } else if ((t->state & 7) == 0) {
          tune_ev0 = t->mon[0];
          tune_ev1 = t->mon[1];
          t->mon_pending = true;
        }
      }
    } else {
      G = t->state < kWarm + kRun ? 2 : 1;
      tune = t;
      if (t->state == kWarm) tune_ev0 = t->e[0];
      if (t->state == kWarm + kRun - 1) tune_ev1 = t->e[1];
      if (t->state == kWarm + kRun) tune_ev0 = t->e[2];
      if (t->state == kTuneDecide - 1) tune_ev1 = t->e[3];
    }
  }
  return TuneStep{G, tune_ev0, tune_ev1, tune};
}

int ensure_fitted(cgp_ctx *c);   // below, with the short-window paths
bool small_batch_predict_ok(const cgp_ctx *c, int batch, int N, int d, int M);
int tick_table_entries_batch(int kid, int d, int batch, const double *X, int N, const double *Xs, int M);
struct SmallRaw;
struct SmallDev {   // a batch resident in the caller's device buffers (cgp_fit_predict_batch_device): no ladder, jitter as given
  const double *X, *y, *Xs, *theta, *jitter;
  double *logml;
  int *info;
};
int small_predict_launch(cgp_ctx *c, int batch, int N, int d, int M, int kid, int include_noise, double *dmean, double *dvar, double *dout,
                         hipStream_t s, const SmallRaw *raw = nullptr, const SmallDev *dev = nullptr, int tab_n = 0, int *done_flag = nullptr,
                         int done_seq = 0);
int node_callback_small(cgp_ctx *c, const double *time_array, const double *slip_array, int n, int kid, double *theta, int max_evals,
                        double *mean, double *sigma, int cap, int *m_out);
bool grow_pinned(void *&p, size_t &cap, size_t bytes);
bool grow_device(void *&p, size_t &cap, size_t bytes);
enum class WinDrop { Windows, Multi, MultiGrad, Trend, Joint, LooGrad };
void window_drop(cgp_ctx *c, WinDrop what);   // cgp_window_host.hpp: frees what goes with `what`
// What a batch entry point with more than mean / variance to compute (joint, multi-target, predictive-gradient calls) enqueues on s
// for the `nfit` fits whose panels are slabs slab, slab + 1, ... into the slots slot, slot + 1, ... of its own arrays, while the
// fits' V rows are still in the panel.  Each entry point builds its own, next to the arrays (fit_predict_batch_host calls it):
// a function pointer and the closure it is called with, which the entry point keeps alive (nothing allocated, nothing exported).
struct PostFit {
  int (*fn)(const void *closure, int slab, int slot, int nfit, hipStream_t s);
  const void *closure;
  int operator()(int slab, int slot, int nfit, hipStream_t s) const { return fn(closure, slab, slot, nfit, s); }
};
template <typename F> PostFit post_fit(const F &f) {
  return PostFit{[](const void *p, int slab, int slot, int nfit, hipStream_t s) { return (*static_cast<const F *>(p))(slab, slot, nfit, s); }, &f};
}

inline int ntheta(int kid, int d) { return k_ntheta(kid, d); }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// A one-dimensional grid of `work` workgroups dealt to the XCDs in turn: rounded up to a multiple of WF_XCDS
inline int xcd_grid(long long work, unsigned &grid) {
  if (work > (1ll << 30)) return CGP_EINVAL;
  grid = (unsigned)(cdiv((int)work, WF_XCDS) * WF_XCDS);
  return CGP_OK;
}

bool hip_ok(cgp_ctx *c, hipError_t e, const char *what) {
  if (e == hipSuccess) return true;
  if (c) c->err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}
#define HIP_TRY(ctx, expr)                                   \
  do {                                                       \
    if (!hip_ok((ctx), (expr), #expr)) return CGP_EHIP;      \
  } while (0)

void scratch_free(Scratch &r) {
  if (r.buf) (void)hipFree(r.buf);
  if (r.stage) (void)hipFree(r.stage);
  r = Scratch{};
}
// after the call's own dtype / count checks: is there a reservation, and does it hold `batch` fits x `dim`
int scratch_check(const Scratch &r, int batch, int dim) {
  if (r.max_dim < 1) return CGP_ESTATE;
  if (batch > r.max_batch || dim > r.max_dim) return CGP_ECAPACITY;
  return CGP_OK;
}
// after the caller's own range checks: the old reservation goes, `bytes` of scratch come
int scratch_reserve(cgp_ctx *c, Scratch &r, int max_batch, int max_dim, size_t bytes) {
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());   // an earlier call may still use the scratch that goes
  scratch_free(r);
  if (hipMalloc(&r.buf, bytes) != hipSuccess) {
    (void)hipGetLastError();
    r.buf = nullptr;
    return CGP_ENOMEM;
  }
  r.max_batch = max_batch;
  r.max_dim = max_dim;
  return CGP_OK;
}

hipEvent_t get_event(cgp_ctx *c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

constexpr size_t kOptPinIn = CGP_MAX_THETA + 8;   // doubles at the head of the gradient-mode pinned block: theta, jitter
std::mutex g_attr_mutex;   // guards the per-device "done" marks of set_lds_attrs (cgp_sched_host.hpp) and set_small_attr
constexpr size_t kLdsPerWorkgroup = 160 * 1024;   // gfx950
// k_small<BROWN, DMAX>: the reference's kernel, and SE kernels compiled for d <= 1 / 3 / 8 (the smallest that fits is launched)
template <typename F> int for_each_small_kernel(F &&f) {
  int rc = f(reinterpret_cast<const void *>(&k_small<true, 1>));
  if (rc == 0) rc = f(reinterpret_cast<const void *>(&k_small<false, 1>));
  if (rc == 0) rc = f(reinterpret_cast<const void *>(&k_small<false, 3>));
  if (rc == 0) rc = f(reinterpret_cast<const void *>(&k_small<false, 8>));
  return rc;
}
inline size_t small_predict_lds(int NB, int d) { return ((small_lds_bytes(NB, d) + 15) & ~(size_t)15) + small_predict_lds_extra(NB, d); }
int set_small_attr(int device) {
  static bool done[64] = {false};
  std::lock_guard<std::mutex> lk(g_attr_mutex);
  if (device >= 0 && device < 64 && done[device]) return 0;
  const int rc = for_each_small_kernel([](const void *fn) {
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerWorkgroup) == hipSuccess ? 0 : -1;
  });
  if (rc != 0) return -1;
  const void *pk[] = {reinterpret_cast<const void *>(&k_small_predict<true, 1>), reinterpret_cast<const void *>(&k_small_predict<false, 1>),
                      reinterpret_cast<const void *>(&k_small_predict<false, 3>), reinterpret_cast<const void *>(&k_small_predict<false, 8>)};
  for (const void *fn : pk)
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerWorkgroup) != hipSuccess) return -1;
  if (device >= 0 && device < 64) done[device] = true;
  return 0;
}

// Algorithmic flops of the update launches of block step k (DESIGN.md "Kernels"): lower-trapezoid
// entries of block column k times a 2*(k*128)-flop inner product, plus (3d+2) per Gram entry.
double trsm_flops(int N, int M, int k, bool in_rows, int batch) {
  const double w = std::min(TS, N - k * TS);
  const double rows = (in_rows ? std::max(0, N - (k + 1) * TS) : 0) + (M + 1);
  return batch * rows * w * w;  // w^2/2 multiply-adds per row
}

// Fused schedule: k_panel = off-diagonal + extra rows of block column k (update + Gram + in-register
// trmm); k_diag = the diagonal tile (update + Gram + potf2 + inverse).
double panel_flops(int N, int M, int d, int k, bool in_rows, int batch) {
  const double w = std::min(TS, N - k * TS);
  const double rows = (in_rows ? std::max(0, N - (k + 1) * TS) : 0) + (M + 1);
  return batch * (rows * w * 2.0 * (double)(k * TS) + rows * w * w + (3.0 * d + 2.0) * (rows - 1) * w);
}
double diag_flops(int N, int d, int k, int batch) {
  const double w = std::min(TS, N - k * TS);
  const double tri = w * (w + 1) / 2.0;
  return batch * (tri * 2.0 * (double)(k * TS) + (3.0 * d + 2.0) * tri + w * w * w / 3.0 + w * w * w / 3.0);
}

// Offsets every per-fit pointer of `a` by g0 fits (group view of a batch).
template <typename T> FitArgs group_view(const FitArgs &a, int g0) {
  FitArgs v = a;
  auto adv = [](const void *p, size_t elems) -> const void * {
    return p ? static_cast<const void *>(static_cast<const T *>(p) + elems) : nullptr;
  };
  v.Lw = const_cast<void *>(adv(a.Lw, (size_t)g0 * a.lw_stride));
  v.Winv = const_cast<void *>(adv(a.Winv, (size_t)g0 * a.winv_stride));
  v.Lp = a.Lp ? static_cast<void *>(static_cast<unsigned short *>(a.Lp) + (size_t)g0 * a.lp_stride) : nullptr;
  v.dpart = const_cast<void *>(adv(a.dpart, (size_t)g0 * 2 * DPART));
  v.pimg = const_cast<void *>(adv(a.pimg, (size_t)g0 * 2 * DPART));
  v.X = adv(a.X, (size_t)g0 * a.d * a.N);
  v.Xs = adv(a.Xs, (size_t)g0 * a.d * a.M);
  v.y = adv(a.y, (size_t)g0 * a.N);
  v.mean = const_cast<void *>(adv(a.mean, (size_t)g0 * a.M));
  v.var = const_cast<void *>(adv(a.var, (size_t)g0 * a.M));
  v.alpha = const_cast<void *>(adv(a.alpha, (size_t)g0 * a.alpha_stride));
  v.theta = a.theta + (size_t)g0 * MAX_THETA;
  v.jitter = a.jitter ? a.jitter + g0 : nullptr;
  v.prep = a.prep ? a.prep + (size_t)g0 * PREP_N : nullptr;
  v.logml = a.logml ? a.logml + g0 : nullptr;
  v.info = a.info ? a.info + g0 : nullptr;
  v.rflag = a.rflag ? a.rflag + g0 : nullptr;
  return v;
}

}  // namespace

// the fit schedules: the launch helpers, one enqueue function per schedule, run_schedule / run
#include "cgp_sched_host.hpp"

namespace {

FitArgs base_args(cgp_ctx *c, int N, int d, int M, int kid, int include_noise) {
  FitArgs a{};
  a.Lw = c->Lw;
  a.lw_stride = c->lw_stride;
  a.ld = c->ld;
  a.Winv = c->Winv;
  a.winv_stride = c->winv_stride;
  a.Lp = c->Lp;
  a.lp_stride = 3 * c->lw_stride;
  a.alpha = c->dalpha;
  a.alpha_stride = c->alpha_stride;
  a.prep = c->dprep;
  a.dpart = c->ddiagimg;
  a.pimg = c->dpanimg;
  a.dbgbuf = c->ddbg;
  a.N = N;
  a.d = d;
  a.M = M;
  a.NT = cdiv(N, TS);
  a.ET = cdiv(M + 1, TS);
  // the tile loops read up to four chunks (64 columns) past block column k - 1 of a panel without a branch (bx6_iter): every block
  // step k < NT of a call stays inside the NTmax x 128 columns of the fit's slab
  static_assert(4 * KT <= TS, "the unconditional look-ahead of the tile loops stays inside the next block column");
  a.kernel_id = kid;
  a.include_noise = include_noise;
#ifdef CGP_ABLATION
  static const int dbg_env = [] { const char *e = getenv("CGP_DBG"); return e ? atoi(e) : 0; }();
  a.dbg = dbg_env;  // timing ablations: results are wrong on purpose, cgp_build_flags() reports the build
#endif
  return a;
}
// the nine arrays of a call (every pointer: its first fit), in the device dtype where void
inline void set_call_arrays(FitArgs &a, const void *X, const void *y, const void *Xs, const double *theta, const double *jitter, void *mean,
                            void *var, double *logml, int *info) {
  a.X = X;
  a.Xs = Xs;
  a.y = y;
  a.theta = theta;
  a.jitter = jitter;
  a.mean = mean;
  a.var = var;
  a.logml = logml;
  a.info = info;
}
// ... of a call on the context's own copies (the single fit of cgp_fit, slot 0)
inline void set_ctx_arrays(cgp_ctx *c, FitArgs &a) {
  set_call_arrays(a, c->dX, c->dy, c->dXs, c->dtheta, c->djitter, c->dmean, c->dvar, c->dlogml, c->dinfo);
}

int check_shape(const cgp_ctx *c, int batch, int N, int d, int M, int kid) {
  if (!c) return CGP_EINVAL;
  if (batch < 1 || N < 1 || d < 1 || M < 0) return CGP_EINVAL;
  if (kid < 0 || kid > CGP_KERNEL_MATERN52_ARD) return CGP_EINVAL;
  if (kid == CGP_KERNEL_RBF_BROWNIAN && d != 1) return CGP_EINVAL;
  if (k_is_matern(kid) && c->dtype != CGP_F64) return CGP_EINVAL;   // the Matern kernels are fp64 paths (corenav_gp.h)
  if (batch > c->max_batch || N > c->max_n || M > c->max_m || d > c->max_d) return CGP_ECAPACITY;
  return CGP_OK;
}

// hip_stream argument of the device entry points: NULL is the legacy default stream itself (what
// torch.cuda.current_stream().cuda_stream is for the default stream), so the work is ordered with the
// caller's other default-stream work; CGP_STREAM_CTX selects the context's private stream.
inline hipStream_t pick_stream(cgp_ctx *c, void *hip_stream) {
  return hip_stream == CGP_STREAM_CTX ? c->stream : (hipStream_t)hip_stream;
}

// Pinned staging blocks that kernels also access IN PLACE (the one-launch short-window paths, the per-tick window push) must not be
// freed and allocated again between two such launches (see cgp_window_push: stores lost under load): a block starts at 64 KB -- more
// than any in-place use needs -- and grows geometrically, so the in-place paths never see a second allocation and the DMA-staged
// ones (cgp_fit_predict_batch's megabytes) see few.
bool grow_pinned(void *&p, size_t &cap, size_t bytes) {
  if (bytes <= cap) return true;
  bytes = std::max({bytes, (size_t)64 * 1024, 2 * cap});
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    p = nullptr;
    return false;
  }
  cap = bytes;
  return true;
}
bool grow_device(void *&p, size_t &cap, size_t bytes) {
  if (bytes <= cap) return true;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    p = nullptr;
    return false;
  }
  cap = bytes;
  return true;
}

// (n, d) row-major fp64  ->  SoA [d][n] in the device dtype, staged in `tmp`
void pack_soa(const double *src, int n, int d, int dtype, std::vector<char> &tmp, size_t off_elems) {
  if (dtype == CGP_F64) {
    double *o = reinterpret_cast<double *>(tmp.data()) + off_elems;
    for (int q = 0; q < d; ++q)
      for (int i = 0; i < n; ++i) o[(size_t)q * n + i] = src[(size_t)i * d + q];
  } else {
    float *o = reinterpret_cast<float *>(tmp.data()) + off_elems;
    for (int q = 0; q < d; ++q)
      for (int i = 0; i < n; ++i) o[(size_t)q * n + i] = (float)src[(size_t)i * d + q];
  }
}
void pack_vec(const double *src, size_t n, int dtype, std::vector<char> &tmp, size_t off_elems) {
  if (dtype == CGP_F64) memcpy(reinterpret_cast<double *>(tmp.data()) + off_elems, src, n * sizeof(double));
  else {
    float *o = reinterpret_cast<float *>(tmp.data()) + off_elems;
    for (size_t i = 0; i < n; ++i) o[i] = (float)src[i];
  }
}
void unpack_vec(const std::vector<char> &tmp, size_t off_elems, size_t n, int dtype, double *dst) {
  if (dtype == CGP_F64) memcpy(dst, reinterpret_cast<const double *>(tmp.data()) + off_elems, n * sizeof(double));
  else {
    const float *o = reinterpret_cast<const float *>(tmp.data()) + off_elems;
    for (size_t i = 0; i < n; ++i) dst[i] = (double)o[i];
  }
}

// mean of diag(Ky) for GPy's jitter policy (jitchol: jitter = diagA.mean() * 1e-6)
double mean_diag(int kid, const double *theta, int d, const double *X, int N) {
  const double noise = theta[ntheta(kid, d) - 1] + 1e-8;
  if (kid != CGP_KERNEL_RBF_BROWNIAN) return theta[0] + noise;
  double s = 0;
  for (int i = 0; i < N; ++i) s += std::fabs(X[i]);
  return theta[0] * theta[2] * s / N + noise;
}

int upload_theta(cgp_ctx *c, const double *theta, int theta_stride, int nth, int batch, hipStream_t s,
                 std::vector<double> &stage) {
  stage.assign((size_t)batch * CGP_MAX_THETA, 0.0);
  for (int b = 0; b < batch; ++b)
    for (int q = 0; q < nth; ++q) stage[(size_t)b * CGP_MAX_THETA + q] = theta[(size_t)b * theta_stride + q];
  HIP_TRY(c, hipMemcpyAsync(c->dtheta, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice, s));
  return CGP_OK;
}

// The windows of a batch -> slots 0 .. batch - 1 of c->dX (SoA, device dtype) and, unless y is null, c->dy
int upload_batch_xy(cgp_ctx *c, int batch, int N, int d, const double *X, const double *y, hipStream_t s) {
  std::vector<char> hx((size_t)batch * d * N * c->esz), hy(y ? (size_t)batch * N * c->esz : 0);
  for (int b = 0; b < batch; ++b) {
    pack_soa(X + (size_t)b * N * d, N, d, c->dtype, hx, (size_t)b * d * N);
    if (y) pack_vec(y + (size_t)b * N, N, c->dtype, hy, (size_t)b * N);
  }
  HIP_TRY(c, hipMemcpyAsync(c->dX, hx.data(), hx.size(), hipMemcpyHostToDevice, s));          // pageable sources: staged by the
  if (y) HIP_TRY(c, hipMemcpyAsync(c->dy, hy.data(), hy.size(), hipMemcpyHostToDevice, s));   // runtime before the calls return
  return CGP_OK;
}

// FitArgs of a gradient-mode factorisation (xid = 1, M = N: the "test rows" are the identity, Xs is unused, and the extra block of
// the factor panel ends up holding Wt = (L^-1)^T) with the context's mean / var / gpart; the caller sets y, theta, jitter, logml, info
FitArgs grad_mode_args(cgp_ctx *c, int N, int d, int kid, const void *dX) {
  FitArgs a = base_args(c, N, d, /*M=*/N, kid, 0);
  a.xid = 1;
  a.X = dX;
  a.Xs = dX;
  a.mean = c->dmean;
  a.var = c->dvar;
  a.gpart = c->dgpart;
  return a;
}

// GPy's jitchol policy for the fits of a batched call that failed (hinfo[b] != 0, not marked in skip), one fit at a time (rare
// path): jitter = mean(diag Ky) 1e-6 10^k, k = 0..4, goes to c->djitter[b], resubmit(b) queues the fit again on s, and its info
// word is read back from c->dinfo[b].  jit_last[b]: the last jitter fit b was tried with (0: it never failed).
template <typename F>
int jitter_ladder(cgp_ctx *c, int batch, int N, int d, int kid, const double *theta, int theta_stride, const double *X, int *hinfo,
                  const std::vector<char> *skip, double *jit_last, hipStream_t s, F &&resubmit) {
  for (int b = 0; b < batch; ++b) {
    jit_last[b] = 0.0;
    if (hinfo[b] == 0 || (skip && (*skip)[b])) continue;
    double jit = mean_diag(kid, theta + (size_t)b * theta_stride, d, X + (size_t)b * N * d, N) * 1e-6;
    for (int attempt = 0; attempt < 5 && hinfo[b] != 0; ++attempt, jit *= 10.0) {
      HIP_TRY(c, hipMemcpyAsync(c->djitter + b, &jit, sizeof(double), hipMemcpyHostToDevice, s));
      const int rc = resubmit(b);
      if (rc != CGP_OK) return rc;
      HIP_TRY(c, hipMemcpyAsync(&hinfo[b], c->dinfo + b, sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipStreamSynchronize(s));
      jit_last[b] = jit;
    }
  }
  return CGP_OK;
}

}  // namespace

extern "C" {

int cgp_abi_version(void) { return CGP_ABI_VERSION; }

const char *cgp_strerror(int code) {
  switch (code) {
    case CGP_OK: return "ok";
    case CGP_EINVAL: return "invalid argument";
    case CGP_ENOMEM: return "out of device memory";
    case CGP_EHIP: return "HIP runtime error (see cgp_last_error)";
    case CGP_ESTATE: return "no fitted model in this context";
    case CGP_ENODEVICE: return "no usable gfx950 device";
    case CGP_ECAPACITY: return "problem exceeds the context capacity given to cgp_create";
    default: return code > 0 ? "matrix not positive definite after the jitter policy (value = failing pivot)" : "unknown error";
  }
}

const char *cgp_last_error(const cgp_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }
double cgp_last_jitter(const cgp_ctx *ctx) { return ctx ? ctx->fjitter : 0.0; }

cgp_ctx *cgp_create(int device, int max_n, int max_m, int max_d, int max_batch, int dtype) {
  return cgp_create_ex(device, max_n, max_m, max_d, max_batch, dtype, nullptr);
}

cgp_ctx *cgp_create_ex(int device, int max_n, int max_m, int max_d, int max_batch, int dtype, int *status) {
  auto fail = [status](int code) -> cgp_ctx * {
    if (status) *status = code;
    return nullptr;
  };
  if (status) *status = CGP_OK;
  if (max_n < 1 || max_m < 0 || max_d < 1 || max_d > CGP_MAX_D || max_batch < 1) return fail(CGP_EINVAL);
  if (dtype != CGP_F64 && dtype != CGP_F32) return fail(CGP_EINVAL);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(CGP_ENODEVICE);
  if (hipSetDevice(device) != hipSuccess) return fail(CGP_ENODEVICE);
  // the code object holds gfx950 kernels only (MFMA f64 16x16x4, 64-bit DPP row_newbcast, 16-byte LDS-DMA)
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(CGP_ENODEVICE);
  if ((dtype == CGP_F64 ? set_lds_attrs<double>(device) : set_lds_attrs<float>(device)) != 0) return fail(CGP_EHIP);
  (void)hipGetLastError();   // a clean slate: what the allocations below leave behind tells out-of-memory from anything else
  cgp_ctx *c = new cgp_ctx();
  c->n_cu = prop.multiProcessorCount;
  c->device = device;
  c->dtype = dtype;
  c->esz = dtype == CGP_F64 ? 8 : 4;
  c->max_n = max_n;
  c->max_m = max_m;
  c->max_d = max_d;
  c->max_batch = max_batch;
  c->NTmax = cdiv(max_n, TS);
  c->ETmax = cdiv(max_m + 1, TS);
  c->ld = (c->NTmax + c->ETmax) * TS;
  c->lw_stride = (size_t)c->ld * c->NTmax * TS;
  c->winv_stride = (size_t)c->NTmax * WIMG;
  c->alpha_stride = (size_t)c->NTmax * TS;
  const size_t B = max_batch;
  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
  // Worker streams carry launches that must run BESIDE the caller's stream (the extra-row launches E(k) of a mid-size
  // call, the groups of cgp_set_streams).  The runtime multiplexes HIP streams onto a few hardware queues per priority
  // level, and two streams that land on one queue run in order: a 64-fit fp64 call took 8.34 instead of 6.87 ms whenever
  // its worker stream shared the legacy default stream's queue -- which depended on how many streams the process had used
  // before (tools/ctx_placement.py, profiles/r04_ctx_placement.txt: one throw-away stream created in between restored
  // 6.89 ms; memory placement played no part).  Queues are pooled per priority, so the workers are created at the LOWEST
  // priority: they never share a queue with a normal-priority caller stream, and the chain-bound factorisation launches
  // on the caller's stream are dispatched ahead of the extra rows that fill in beside them.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  for (int i = 0; i < cgp_ctx::kMaxStreams; ++i) {
    ok = ok && hipStreamCreateWithPriority(&c->wstream[i], hipStreamNonBlocking, prio_least) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) == hipSuccess;
  }
  ok = ok && hipStreamCreateWithPriority(&c->hstream, hipStreamNonBlocking, prio_greatest) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
  for (auto &e : c->ev_look) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMalloc(&c->Lw, B * c->lw_stride * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->Winv, B * c->winv_stride * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dX, B * max_d * max_n * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dXs, B * max_d * (size_t)std::max(max_m, 1) * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dy, B * max_n * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dmean, B * (size_t)std::max(max_m, 1) * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dvar, B * (size_t)std::max(max_m, 1) * c->esz) == hipSuccess;
  ok = ok && hipMalloc(&c->dalpha, B * c->alpha_stride * c->esz) == hipSuccess;
  if (dtype == CGP_F32) {
    ok = ok && hipMalloc((void **)&c->dref_r, B * c->alpha_stride * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void **)&c->dref_a, B * c->alpha_stride * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void **)&c->dref_flag, B * sizeof(int)) == hipSuccess;
    ok = ok && hipMemset(c->dref_flag, 0, B * sizeof(int)) == hipSuccess;
  }
  ok = ok && hipMalloc((void **)&c->dtheta, B * CGP_MAX_THETA * sizeof(double)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->djitter, B * sizeof(double)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->dgpart, (B * c->NTmax * (c->NTmax + 1) / 2 * GRAD_N + 2) * sizeof(double)) == hipSuccess;  // + logML, info of a single evaluation
  LatBufs &lat = c->lat;
  lat.sk_slots = c->NTmax + c->ETmax + 1;
  lat.lat_cap = std::min(LAT_FITS_ALLOC, max_batch);
  // partial-tile slab: the latency schedule takes MORE fits the fewer block steps a window has (lat_fits_by_steps), and a
  // call of NT block steps uses NT + ET + 1 tile slots per fit, so the slab is sized for the largest fits x slots product over
  // the block-step counts this context can see (a max_n = 2048 fp64 context: 11 fits x 22 slots, not 32 x 22) and a call
  // indexes it with its OWN slot count (SplitArgs::slots)
  for (int nt = 1; nt <= c->NTmax; ++nt) {
    const int fits = std::min(lat.lat_cap, kAbBuild ? LAT_FITS_ALLOC : lat_fits_by_steps(dtype == CGP_F64, nt));
    lat.lat_units = std::max(lat.lat_units, (size_t)fits * (nt + c->ETmax + 1));
  }
  ok = ok && hipMalloc(&lat.dpart, lat.part_bytes(c->esz)) == hipSuccess;
  ok = ok && hipMalloc((void **)&lat.dticket, sizeof(int) * lat.lat_cap * lat.sk_slots) == hipSuccess;
  ok = ok && hipMemset(lat.dticket, 0, sizeof(int) * lat.lat_cap * lat.sk_slots) == hipSuccess;
  ok = ok && hipMalloc((void **)&lat.dwready, sizeof(int) * lat.lat_cap) == hipSuccess;
  // pre-update images exist from three block steps on (lat_images): sized for the most fits the latency schedule takes there
  int img_fits = 1;
  for (int nt = 3; nt <= std::max(3, c->NTmax); ++nt)
    img_fits = std::max(img_fits, std::min(lat.lat_cap, kAbBuild ? LAT_FITS_ALLOC : lat_fits_by_steps(dtype == CGP_F64, nt)));
  lat.lat_img_fits = c->NTmax >= 3 ? img_fits : 1;
  ok = ok && hipMalloc(&lat.dlatimg, lat.img_bytes(c->esz)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->dmacc, sizeof(double) * 2 * B * std::max(c->max_m, 1)) == hipSuccess;
  ok = ok && hipMalloc(&c->ddiagimg, B * 2 * DPART * c->esz) == hipSuccess;
  c->mid_cap = std::min(MID_FITS_ALLOC, max_batch);
  ok = ok && hipMalloc(&c->dpanimg, (size_t)c->mid_cap * 2 * DPART * c->esz) == hipSuccess;
  if (dtype == CGP_F32 && kMidPlanes) ok = ok && hipMalloc(&c->Lp, (size_t)c->mid_cap * 3 * c->lw_stride * sizeof(unsigned short)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->ddbg, DBG_SLOTS * sizeof(long long)) == hipSuccess;
  ok = ok && hipMemset(c->ddbg, 0, DBG_SLOTS * sizeof(long long)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->dprep, B * PREP_N * sizeof(double)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->dlogml, B * sizeof(double)) == hipSuccess;
  ok = ok && hipMalloc((void **)&c->dinfo, B * sizeof(int)) == hipSuccess;
  if (dtype == CGP_F64) {
    ok = ok && hipMalloc((void **)&c->dsmall, B * SM_OUT * sizeof(double)) == hipSuccess;
    {
      std::vector<unsigned short> tab;
      for (int NB = 1; NB <= SM_MAX_NB; ++NB) {
        c->smdeal_off[NB] = tab.size();
        tab.resize(tab.size() + small_table_elems(NB), 0);
        for (int jb = 0; jb < NB; ++jb) ok = sm_build_deal(tab.data() + c->smdeal_off[NB], NB, jb) && ok;   // false: the deal outgrew sm_eval's lists
        sm_build_rowmap(tab.data() + c->smdeal_off[NB] + (size_t)NB * SM_NH * SM_DEAL, NB);
      }
      ok = ok && hipMalloc((void **)&c->dsmdeal, tab.size() * sizeof(unsigned short)) == hipSuccess;
      ok = ok && hipMemcpy(c->dsmdeal, tab.data(), tab.size() * sizeof(unsigned short), hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && hipMalloc((void **)&c->dsmdone, sizeof(int)) == hipSuccess && hipMemset(c->dsmdone, 0, sizeof(int)) == hipSuccess;
    }
    ok = ok && set_small_attr(device) == 0;
  }
  // the fills above (tickets, debug slots, refinement flags) are asynchronous to the host and ordered on the legacy default stream;
  // the context's work runs on non-blocking streams that do not wait for it (see cgp_window_init)
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    const hipError_t e = hipGetLastError();
    cgp_destroy(c);
    return fail(e == hipErrorOutOfMemory ? CGP_ENOMEM : CGP_EHIP);
  }
  return c;
}

void cgp_destroy(cgp_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto &r : c->recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  void *bufs[] = {c->Lw, c->Winv, c->dX, c->dXs, c->dy, c->dmean, c->dvar, c->dalpha, c->dtheta, c->djitter, c->dlogml, c->dinfo, c->dprep, c->ddbg, c->dgpart, c->la_buf, c->la_ibuf, c->dmacc, c->ddiagimg, c->dpanimg, c->dsmall, c->dsmdeal, c->dsmdone, c->dref_r, c->dref_a, c->dref_flag, c->Lp};
  for (void *p : bufs)
    if (p) (void)hipFree(p);
  auto drop = [](auto *p) {
    if (p) (void)hipFree(p);
  };
  c->lat.each(drop);
  c->ol.each(drop);
  for (int i = 0; i < cgp_ctx::kMaxStreams; ++i) {
    if (c->wstream[i]) {
      (void)hipStreamSynchronize(c->wstream[i]);
      (void)hipStreamDestroy(c->wstream[i]);
    }
    if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
  }
  if (c->hstream) {
    (void)hipStreamSynchronize(c->hstream);
    (void)hipStreamDestroy(c->hstream);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (auto &t : c->tune) {
    for (auto e : t.e)
      if (e) (void)hipEventDestroy(e);
    for (auto e : t.mon)
      if (e) (void)hipEventDestroy(e);
  }
  for (auto e : c->ev_look)
    if (e) (void)hipEventDestroy(e);
  window_drop(c, WinDrop::Windows);
  for (Scratch *r : {&c->fj, &c->mz, &c->tr, &c->sp, &c->sg, &c->sm, &c->mg, &c->ma, &c->pg, &c->lg}) scratch_free(*r);
  if (c->win_pin) (void)hipHostFree(c->win_pin);
  if (c->opt_pin) (void)hipHostFree(c->opt_pin);
  if (c->win_dev) (void)hipFree(c->win_dev);
  if (c->pin_in) (void)hipHostFree(c->pin_in);
  if (c->pin_out) (void)hipHostFree(c->pin_out);
  if (c->draw) (void)hipFree(c->draw);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int cgp_debug_read(cgp_ctx *c, long long out[CGP_DEBUG_SLOTS]) {
  if (!c || !out) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(out, c->ddbg, DBG_SLOTS * sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemset(c->ddbg, 0, DBG_SLOTS * sizeof(long long)));  // the sums restart
  HIP_TRY(c, hipDeviceSynchronize());                                 // (the fill is asynchronous to the host: see cgp_window_init)
  return CGP_OK;
}

int cgp_debug_buffers(cgp_ctx *c, unsigned long long out[2 * CGP_DEBUG_BUFFERS]) {
  if (!c || !out) return CGP_EINVAL;
  const size_t B = c->max_batch;
  const void *p[CGP_DEBUG_BUFFERS] = {c->Lw, c->Winv, c->ddiagimg, c->dpanimg, c->dX, c->dmacc, c->lat.dpart, c->lat.dlatimg};
  const size_t n[CGP_DEBUG_BUFFERS] = {B * c->lw_stride * c->esz,
                                       B * c->winv_stride * c->esz,
                                       B * 2 * DPART * c->esz,
                                       (size_t)c->mid_cap * 2 * DPART * c->esz,
                                       B * c->max_d * c->max_n * c->esz,
                                       sizeof(double) * 2 * B * std::max(c->max_m, 1),
                                       c->lat.part_bytes(c->esz),
                                       c->lat.img_bytes(c->esz)};
  for (int i = 0; i < CGP_DEBUG_BUFFERS; ++i) {
    out[2 * i] = (unsigned long long)(uintptr_t)p[i];
    out[2 * i + 1] = n[i];
  }
  return CGP_OK;
}

int cgp_debug_small(cgp_ctx *c, double out[CGP_SMALL_OUT]) {
  if (!c || !out) return CGP_EINVAL;
  if (!c->dsmall) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->last_small_dev) {
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(out, c->dsmall, SM_OUT * sizeof(double), hipMemcpyDeviceToHost));
  } else memcpy(out, c->last_small, SM_OUT * sizeof(double));
  return CGP_OK;
}

int cgp_build_flags(void) {
  int f = 0;
#ifdef CGP_ABLATION
  f |= CGP_BUILD_ABLATION;
#endif
#ifdef CGP_AB
  f |= CGP_BUILD_AB;
#endif
  if (!kF32Bf16x6) f |= CGP_BUILD_F32_NATIVE;
  return f;
}

int cgp_synchronize(cgp_ctx *c) {
  if (!c) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CGP_OK;
}

int cgp_set_streams(cgp_ctx *c, int n) {
  if (!c || n < 0 || n > cgp_ctx::kMaxStreams) return CGP_EINVAL;
  c->nstreams = n;
  return CGP_OK;
}

int cgp_set_refine(cgp_ctx *c, int steps) {
  if (!c || steps < -1 || steps > 3) return CGP_EINVAL;
  c->refine = steps;
  return CGP_OK;
}

int cgp_profile_enable(cgp_ctx *c, int on) {
  if (!c) return CGP_EINVAL;
  c->prof = on != 0;
  c->prof_step = on >= 2 ? on - 2 : -1;
  return CGP_OK;
}

int cgp_profile_read(cgp_ctx *c, double ms[CGP_PROF_KERNELS], double flops[CGP_PROF_KERNELS],
                     long long launches[CGP_PROF_KERNELS]) {
  if (!c) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &r : c->recs) {
    HIP_TRY(c, hipEventSynchronize(r.b));
    float t = 0;
    HIP_TRY(c, hipEventElapsedTime(&t, r.a, r.b));
    static const bool dump = getenv("CGP_PROF_DUMP") != nullptr;
    if (dump) fprintf(stderr, "cgp prof: kernel %d  %.4f ms\n", r.kernel, t);
    c->prof_ms[r.kernel] += t;
    c->prof_flops[r.kernel] += r.flops;
    c->prof_n[r.kernel] += 1;
    c->pool.push_back(r.a);
    c->pool.push_back(r.b);
  }
  c->recs.clear();
  for (int i = 0; i < CGP_PROF_KERNELS; ++i) {
    if (ms) ms[i] = c->prof_ms[i];
    if (flops) flops[i] = c->prof_flops[i];
    if (launches) launches[i] = c->prof_n[i];
    c->prof_ms[i] = c->prof_flops[i] = 0;
    c->prof_n[i] = 0;
  }
  return CGP_OK;
}

// tiled_only: the joint entry points (cgp_joint_host.hpp) keep every shape on the tiled schedules -- the contraction reads V^T from
// the factor panel, which the one-launch short-window kernel never writes.  Among the tiled
// schedules the call takes the one the marginal call of its size takes: mean and variance are bitwise that call's
static int fit_predict_device(cgp_ctx *c, int batch, int N, int d, int M, int kid, const void *dX, const void *dy, const void *dXs,
                              const double *dtheta, const double *djitter, int include_noise, void *dmean, void *dvar, double *dlogml,
                              int *dinfo, void *hip_stream, bool tiled_only) {
  int rc = check_shape(c, batch, N, d, M, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dy || !dtheta || !dlogml || !dinfo || (M > 0 && (!dXs || !dmean || !dvar))) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  FitArgs a = base_args(c, N, d, M, kid, include_noise);
  set_call_arrays(a, dX, dy, dXs, dtheta, djitter, dmean, dvar, dlogml, dinfo);
  c->have_fit = false;
  c->lazy_fit = false;
  if (!tiled_only && !k_is_matern(kid) && small_batch_predict_ok(c, batch, N, d, M)) {   // short windows: fit + predictions of the whole batch in ONE launch, factors in LDS
    const SmallDev dev{static_cast<const double *>(dX), static_cast<const double *>(dy), static_cast<const double *>(dXs), dtheta, djitter, dlogml, dinfo};
    const int tab = c->pending_tab;   // only the host-buffer entry point knows whether the inputs are tick counts
    c->pending_tab = 0;
    return small_predict_launch(c, batch, N, d, M, kid, include_noise, static_cast<double *>(dmean), static_cast<double *>(dvar), c->dsmall,
                                pick_stream(c, hip_stream), nullptr, &dev, tab);
  }
  return run(c, a, batch, true, false, pick_stream(c, hip_stream));
}

int cgp_fit_predict_batch_device(cgp_ctx *c, int batch, int N, int d, int M, int kid, const void *dX,
                                 const void *dy, const void *dXs, const double *dtheta, const double *djitter,
                                 int include_noise, void *dmean, void *dvar, double *dlogml, int *dinfo,
                                 void *hip_stream) {
  return fit_predict_device(c, batch, N, d, M, kid, dX, dy, dXs, dtheta, djitter, include_noise, dmean, dvar, dlogml, dinfo, hip_stream,
                            false);
}

// post: what a joint, multi-target or predictive-gradient call (cgp_joint_host.hpp, cgp_multi_host.hpp, cgp_pgrad_host.hpp; fp64)
// does with every fit's V rows while they are still in the panel: for the whole batch before the ladder's first retry, for a
// retried fit -- which runs as a call of one fit, in slab 0 -- right after its retry.  Such a call reads the factor panel, so it
// keeps the tiled schedules for every shape, and its mean / var may be NULL (the device copies stay in the context).
static int fit_predict_batch_host(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *X, const double *y,
                                  const double *Xs, const double *theta, int theta_stride, int include_noise,
                                  double *mean, double *var, double *logml, int *info, const PostFit *post) {
  const bool reads_panel = post != nullptr;
  int rc = check_shape(c, batch, N, d, M, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta || (M > 0 && (!Xs || (!reads_panel && (!mean || !var))))) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  if (theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t esz = c->esz;
  const bool trace = kAbBuild && getenv("CGP_TRACE_E2E");
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t_start = now(), t_last = t_start;
  auto lap = [&](const char *what) {
    if (!trace) return;
    auto t = now();
    fprintf(stderr, "[e2e] %-18s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  // Host side of the boundary (gp_slip_node.py:19-25 "list -> (n, 1) fp64"): the caller's row-major fp64
  // arrays go through ONE pinned staging block and ONE H2D DMA; the (n, d) -> SoA [d][n] transposition
  // and the fp64 -> device dtype conversion run on the device (k_pack_soa), not on a host core.
  const size_t B = batch, nX = B * N * d, ny = B * N, nXs = B * (size_t)M * d, nTh = B * CGP_MAX_THETA;
  const size_t in_bytes = (nX + ny + nXs + nTh) * sizeof(double);
  const size_t out_elems = 2 * B * (size_t)M;                    // mean, var in the device dtype
  const size_t out_bytes = out_elems * esz + B * sizeof(double) + B * sizeof(int);
  if (!grow_pinned(c->pin_in, c->pin_in_cap, in_bytes) || !grow_pinned(c->pin_out, c->pin_out_cap, out_bytes) ||
      !grow_device(c->draw, c->draw_cap, in_bytes))
    return CGP_ENOMEM;
  double *hin = static_cast<double *>(c->pin_in);
  double *hth = hin + nX + ny + nXs;
  for (size_t b = 0; b < B; ++b)
    for (int q = 0; q < CGP_MAX_THETA; ++q) hth[b * CGP_MAX_THETA + q] = q < nth ? theta[b * theta_stride + q] : 0.0;
  const double *draw = static_cast<const double *>(c->draw);
  // Staging copy (pageable -> pinned) is the longest host step of a large call (66 MB for the headline batch:
  // 6.6 ms on one core against 1.3 ms of DMA): ranges of fits are copied by up to 4 threads and each range's
  // DMA is queued as soon as it is staged, so the copy engine works while the later ranges are still copied.
  const int nthr = in_bytes > (4u << 20) ? (int)std::min<size_t>({4, B, std::max(1u, std::thread::hardware_concurrency())}) : 1;
  auto stage = [&](size_t b0, size_t b1) {
    memcpy(hin + b0 * N * d, X + b0 * N * d, (b1 - b0) * N * d * sizeof(double));
    memcpy(hin + nX + b0 * N, y + b0 * N, (b1 - b0) * N * sizeof(double));
    if (nXs) memcpy(hin + nX + ny + b0 * M * d, Xs + b0 * (size_t)M * d, (b1 - b0) * (size_t)M * d * sizeof(double));
  };
  auto dma = [&](size_t b0, size_t b1) -> hipError_t {
    char *dd = static_cast<char *>(c->draw);
    auto one = [&](size_t off, size_t cnt) {
      return cnt ? hipMemcpyAsync(dd + off * sizeof(double), hin + off, cnt * sizeof(double), hipMemcpyHostToDevice, s) : hipSuccess;
    };
    hipError_t e = one(b0 * N * d, (b1 - b0) * N * d);
    if (e == hipSuccess) e = one(nX + b0 * N, (b1 - b0) * N);
    if (e == hipSuccess) e = one(nX + ny + b0 * M * d, (b1 - b0) * (size_t)M * d);
    return e;
  };
  if (nthr == 1) {
    // a small call: the whole staged block [X | y | Xs | theta] in ONE DMA, unpacked by ONE launch
    stage(0, B);
    HIP_TRY(c, hipMemcpyAsync(c->draw, hin, in_bytes, hipMemcpyHostToDevice, s));
    lap("stage + queue DMA");
    const dim3 grid(std::min(64, cdiv(std::max(N, M) * d, 256)), batch);
    if (c->dtype == CGP_F64)
      hipLaunchKernelGGL(k_pack_call<double>, grid, dim3(256), 0, s, draw, static_cast<double *>(c->dX), static_cast<double *>(c->dy),
                         static_cast<double *>(c->dXs), c->dtheta, c->djitter, batch, N, d, M);
    else
      hipLaunchKernelGGL(k_pack_call<float>, grid, dim3(256), 0, s, draw, static_cast<float *>(c->dX), static_cast<float *>(c->dy),
                         static_cast<float *>(c->dXs), c->dtheta, c->djitter, batch, N, d, M);
  } else {
    std::vector<std::thread> th;
    auto lo = [&](int w) { return B * w / nthr; };
    for (int w = 1; w < nthr; ++w) th.emplace_back(stage, lo(w), lo(w + 1));
    stage(0, lo(1));
    hipError_t e = dma(0, lo(1));
    for (int w = 1; w < nthr; ++w) {
      th[w - 1].join();
      if (e == hipSuccess) e = dma(lo(w), lo(w + 1));
    }
    HIP_TRY(c, e);
    lap("stage + queue DMA");
    HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(c->draw) + (nX + ny + nXs) * sizeof(double), hth, nTh * sizeof(double),
                              hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->dtheta, draw + nX + ny + nXs, nTh * sizeof(double), hipMemcpyDeviceToDevice, s));
    auto pack = [&](const double *src, void *dst, int n, int dd) {
      const dim3 grid(std::min(64, cdiv(n * dd, 256)), batch);
      if (c->dtype == CGP_F64) hipLaunchKernelGGL(k_pack_soa<double>, grid, dim3(256), 0, s, src, static_cast<double *>(dst), n, dd);
      else hipLaunchKernelGGL(k_pack_soa<float>, grid, dim3(256), 0, s, src, static_cast<float *>(dst), n, dd);
    };
    pack(draw, c->dX, N, d);
    pack(draw + nX, c->dy, N, 1);
    if (M > 0) pack(draw + nX + ny, c->dXs, M, d);
    HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  }
  // (the scan that establishes "tick counts" is 1.5 ns per input on the host: 0.3 ms for 256 windows with their 599 test points,
  // more than the launch it would shorten by a tenth -- ensembles beyond 20 k inputs take the direct evaluation)
  const int tick_tab = !reads_panel && small_batch_predict_ok(c, batch, N, d, M) && (size_t)batch * (N + M) <= 20000
                           ? tick_table_entries_batch(kid, d, batch, X, N, Xs, M) : 0;
  c->pending_tab = tick_tab;
  rc = fit_predict_device(c, batch, N, d, M, kid, c->dX, c->dy, c->dXs, c->dtheta, c->djitter,
                          include_noise, c->dmean, c->dvar, c->dlogml, c->dinfo, CGP_STREAM_CTX, /*tiled_only=*/reads_panel);
  c->pending_tab = 0;
  if (rc != CGP_OK) return rc;
  if (post && (rc = (*post)(0, 0, batch, s)) != CGP_OK) return rc;
  char *hout = static_cast<char *>(c->pin_out);
  double *hl = reinterpret_cast<double *>(hout + out_elems * esz);
  int *hinfo = reinterpret_cast<int *>(hl + B);
  lap("queue schedule");
  // results are requested together with the status: one synchronisation per call unless a fit needs the jitter ladder
  auto queue_results = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    if (M > 0) {
      e = hipMemcpyAsync(hout, c->dmean, B * M * esz, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(hout + B * M * esz, c->dvar, B * M * esz, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hl, c->dlogml, sizeof(double) * batch, hipMemcpyDeviceToHost, s);
    return e;
  };
  HIP_TRY(c, hipMemcpyAsync(hinfo, c->dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, queue_results());
  HIP_TRY(c, hipStreamSynchronize(s));
  lap("device done (info + results)");
  // the fits that failed climb the jitter ladder, re-submitted into the same device slots
  const bool retried = std::any_of(hinfo, hinfo + batch, [](int v) { return v != 0; });
  std::vector<double> hjit(batch, 0.0);
  rc = jitter_ladder(c, batch, N, d, kid, theta, theta_stride, X, hinfo, nullptr, hjit.data(), s, [&](int b) {
    c->pending_tab = tick_tab;
    int r = fit_predict_device(
        c, 1, N, d, M, kid, (char *)c->dX + (size_t)b * d * N * esz, (char *)c->dy + (size_t)b * N * esz,
        (char *)c->dXs + (size_t)b * d * M * esz, c->dtheta + (size_t)b * CGP_MAX_THETA, c->djitter + b,
        include_noise, (char *)c->dmean + (size_t)b * M * esz, (char *)c->dvar + (size_t)b * M * esz,
        c->dlogml + b, c->dinfo + b, CGP_STREAM_CTX, /*tiled_only=*/reads_panel);
    if (r == CGP_OK && post) r = (*post)(0, b, 1, s);
    return r;
  });
  if (rc != CGP_OK) return rc;
  c->fjitter = hinfo[0] == 0 ? hjit[0] : 0.0;   // only a fit that factored reports a jitter (cgp_last_jitter; as the gradient-mode and short-window paths)
  if (retried) {
    HIP_TRY(c, queue_results());
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  lap("D2H");
  if (M > 0) {
    if (c->dtype == CGP_F64) {
      if (mean) memcpy(mean, hout, B * M * sizeof(double));
      if (var) memcpy(var, hout + B * M * esz, B * M * sizeof(double));
    } else {
      const float *fm = reinterpret_cast<const float *>(hout), *fv = fm + B * M;
      for (size_t i = 0; i < B * M; ++i) {
        mean[i] = (double)fm[i];
        var[i] = (double)fv[i];
      }
    }
  }
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    if (logml) logml[b] = hl[b];
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  lap("copy out");
  return first;
}

int cgp_fit_predict_batch(cgp_ctx *c, int batch, int N, int d, int M, int kid, const double *X, const double *y,
                          const double *Xs, const double *theta, int theta_stride, int include_noise,
                          double *mean, double *var, double *logml, int *info) {
  return fit_predict_batch_host(c, batch, N, d, M, kid, X, y, Xs, theta, theta_stride, include_noise, mean, var, logml, info, nullptr);
}

int cgp_fit(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta, double *logml) {
  int rc = check_shape(c, 1, N, d, 0, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  int info = 0;
  double l = 0;
  rc = cgp_fit_predict_batch(c, 1, N, d, 0, kid, X, y, nullptr, theta, nth, 0, nullptr, nullptr, &l, &info);
  if (rc < 0) return rc;
  c->have_fit = (info == 0);
  c->fN = N;
  c->fd = d;
  c->fkernel = kid;
  memcpy(c->ftheta, theta, sizeof(double) * nth);
  if (logml) *logml = l;
  return info;
}

// the extra rows of M test points against the resident factor of the last single fit, on the context's stream: V^T into slab 0,
// mean / variance into dmean / dvar (cgp_predict; the single-fit joint calls of cgp_joint_host.hpp contract V^T after it)
static int predict_enqueue(cgp_ctx *c, const double *Xs, int M, int include_noise) {
  if (!c->have_fit) return CGP_ESTATE;
  if (M > c->max_m) return CGP_ECAPACITY;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int fr = ensure_fitted(c)) return fr;
  hipStream_t s = c->stream;
  const size_t esz = c->esz;
  HIP_TRY(c, hipStreamSynchronize(s));   // (an earlier call's copy has read the staging vector)
  std::vector<char> &hxs = c->xs_stage;
  hxs.resize((size_t)c->fd * M * esz);
  pack_soa(Xs, M, c->fd, c->dtype, hxs, 0);
  HIP_TRY(c, hipMemcpyAsync(c->dXs, hxs.data(), hxs.size(), hipMemcpyHostToDevice, s));
  FitArgs a = base_args(c, c->fN, c->fd, M, c->fkernel, include_noise);
  set_ctx_arrays(c, a);
  return run(c, a, 1, false, false, s);
}

int cgp_predict(cgp_ctx *c, const double *Xs, int M, int include_noise, double *mean, double *var) {
  if (!c || !Xs || !mean || !var || M < 1) return CGP_EINVAL;
  int rc = predict_enqueue(c, Xs, M, include_noise);
  if (rc != CGP_OK) return rc;
  hipStream_t s = c->stream;
  const size_t esz = c->esz;
  std::vector<char> hm((size_t)M * esz), hv((size_t)M * esz);
  HIP_TRY(c, hipMemcpyAsync(hm.data(), c->dmean, hm.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(hv.data(), c->dvar, hv.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  unpack_vec(hm, 0, M, c->dtype, mean);
  unpack_vec(hv, 0, M, c->dtype, var);
  return CGP_OK;
}

int cgp_get_alpha(cgp_ctx *c, double *alpha) {
  if (!c || !alpha) return CGP_EINVAL;
  if (!c->have_fit) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int fr = ensure_fitted(c)) return fr;
  hipStream_t s = c->stream;
  // z is the y row of the factor panel; it sits at extra row index M of the LAST run.  Re-run the
  // y row alone (M = 0) so its position is known, then back-substitute.
  FitArgs a = base_args(c, c->fN, c->fd, 0, c->fkernel, 0);
  set_ctx_arrays(c, a);
  int rc = run(c, a, 1, false, true, s);
  if (rc != CGP_OK) return rc;
  if (c->dtype == CGP_F32 && c->refined) {   // the refined alpha is kept in double precision (cgp_refine.hpp)
    HIP_TRY(c, hipMemcpyAsync(alpha, c->dref_a, (size_t)c->fN * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return CGP_OK;
  }
  std::vector<char> h((size_t)c->fN * c->esz);
  HIP_TRY(c, hipMemcpyAsync(h.data(), c->dalpha, h.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  unpack_vec(h, 0, c->fN, c->dtype, alpha);
  return CGP_OK;
}

int cgp_get_factor(cgp_ctx *c, double *L) {
  if (!c || !L) return CGP_EINVAL;
  if (!c->have_fit) return CGP_ESTATE;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int fr = ensure_fitted(c)) return fr;
  const int N = c->fN;
  std::vector<char> h((size_t)N * N * c->esz);
  // columns 0..N-1, rows 0..N-1 of the column-major panel -> dense (N x N) column-major staging
  HIP_TRY(c, hipMemcpy2DAsync(h.data(), (size_t)N * c->esz, c->Lw, (size_t)c->ld * c->esz, (size_t)N * c->esz, N,
                              hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double v = 0;
      if (j <= i) v = c->dtype == CGP_F64 ? reinterpret_cast<double *>(h.data())[(size_t)j * N + i]
                                          : (double)reinterpret_cast<float *>(h.data())[(size_t)j * N + i];
      L[(size_t)i * N + j] = v;
    }
  return CGP_OK;
}

int cgp_slip_node_callback(cgp_ctx *c, const double *time_array, const double *slip_array, int n, int kid,
                           const double *theta, double *mean, double *sigma, int cap, int *m_out) {
  if (!c || !time_array || !slip_array || !theta || !mean || !sigma || n < 2 || cap < 0) return CGP_EINVAL;
  // gp_slip_node.py:27-29  per = 0.9 ; x_train = X[:int(per*len(X))]
  const int ntr = (int)(0.9 * (double)n);
  if (ntr < 1) return CGP_EINVAL;
  // gp_slip_node.py:45  X_ = np.arange(X.min(), X.max() + 600, 1)
  double xmin = time_array[0], xmax = time_array[0];
  for (int i = 1; i < n; ++i) {
    xmin = std::min(xmin, time_array[i]);
    xmax = std::max(xmax, time_array[i]);
  }
  const long long glen = (long long)std::ceil((xmax + 600.0 - xmin) / 1.0);
  // gp_slip_node.py:59-61  means[len(X):]  (index slice)
  const long long mo = std::max(0LL, glen - n);
  if (m_out) *m_out = (int)mo;
  const int M = (int)std::min<long long>(mo, cap);
  if (M == 0) return CGP_OK;
  {   // a short fp64 window (the reference's 149-tick GP_Input is one): fit and predictions in one launch
    double th[CGP_MAX_THETA];
    std::copy(theta, theta + ntheta(kid, 1), th);
    const int rs = node_callback_small(c, time_array, slip_array, n, kid, th, 0, mean, sigma, cap, m_out);
    if (rs != CGP_ESTATE) return rs;
  }
  std::vector<double> xs(M), var(M);
  for (int m = 0; m < M; ++m) xs[m] = xmin + (double)(n + m);
  // GPRegression(...) and the m.predict loop (gp_slip_node.py:35,45-49) in ONE factorisation pass: the
  // prediction points ride as extra rows (one schedule, one host round trip instead of two)
  double logml = 0.0;
  int info = 0;
  int rc = cgp_fit_predict_batch(c, 1, ntr, 1, M, kid, time_array, slip_array, xs.data(), theta, ntheta(kid, 1), 1, mean,
                                 var.data(), &logml, &info);
  if (rc != CGP_OK) return rc;
  if (info != 0) return info;  // not positive definite even with GPy's jitter ladder (LinAlgError there)
  for (int m = 0; m < M; ++m) sigma[m] = 2.0 * std::sqrt(var[m]);  // gp_slip_node.py:61
  return CGP_OK;
}

int cgp_llh_to_enu(double lat, double lon, double h, const double init_llh[3], const double init_ecef[3], double enu[3]) {
  if (!init_llh || !init_ecef || !enu) return CGP_EINVAL;
  corenav::llh_to_enu(lat, lon, h, init_llh, init_ecef, enu);
  return CGP_OK;
}

int cgp_predict_stop(const double *mean, const double *sigma, int M, const double *P, const double *Q,
                     const double *STM, const double *Hvec, const double pos_llh[3], double arrival_time, double now,
                     double threshold, int h_bug_compatible, const double init_llh[3], const double init_ecef[3],
                     int *fired, double *stop_cmd, int *i_out, double *xy_err) {
  if (!mean || !sigma || M < 0 || !P || !Q || !STM || !Hvec || !pos_llh || !init_llh || !init_ecef) return CGP_EINVAL;
  corenav::StopPrediction r = corenav::predict_stop(mean, sigma, M, P, Q, STM, Hvec, pos_llh, arrival_time, now,
                                                    threshold, h_bug_compatible != 0, init_llh, init_ecef);
  if (fired) *fired = r.fired ? 1 : 0;
  if (stop_cmd) *stop_cmd = r.stop_cmd;
  if (i_out) *i_out = r.i;
  if (xy_err) *xy_err = r.xy_err;
  return CGP_OK;
}

int cgp_gppredictor_callback(const double *mean, const double *sigma, int M, const double *P, const double *Q,
                             const double *STM, const double *Hvec, const double pos_llh[3], double arrival_time,
                             double now, int h_bug_compatible, int *published, double *stop_cmd) {
  if (!mean || !sigma || M < 0 || !P || !Q || !STM || !Hvec || !pos_llh) return CGP_EINVAL;
  corenav::NodeHandle nh;
  int clock_reads = 0, npub = 0;
  double last = 0.0;
  nh.now = [&]() { return clock_reads++ == 0 ? arrival_time : now; };
  nh.call_set_stopping = [&](corenav_pod::core_nav::SetStopping &srv) {
    std::copy(P, P + 225, srv.response.PvecData.begin());
    std::copy(Q, Q + 225, srv.response.QvecData.begin());
    std::copy(STM, STM + 225, srv.response.STMvecData.begin());
    std::copy(Hvec, Hvec + 60, srv.response.HvecData.begin());
    srv.response.PosData.x = pos_llh[0];
    srv.response.PosData.y = pos_llh[1];
    srv.response.PosData.z = pos_llh[2];
    return srv.request.stopping;
  };
  nh.publish_stop_cmd = [&](const corenav_pod::std_msgs::Float64 &m) {
    ++npub;
    last = m.data;
  };
  GpPredictor node(nh);
  node.h_bug_compatible = h_bug_compatible != 0;
  auto msg = std::make_shared<corenav_pod::core_nav::GP_Output>();
  msg->mean.assign(mean, mean + M);
  msg->sigma.assign(sigma, sigma + M);
  node.GPCallBack(msg);
  if (published) *published = npub;
  if (stop_cmd) *stop_cmd = last;
  return CGP_OK;
}

}  // extern "C"

namespace {
// One gradient-mode evaluation on the device for the window already uploaded to slot 0.
// k_grad of the fit's kernel: the Matern pair has instantiations of its own (fp64; check_shape refuses them in fp32 contexts)
template <typename T> void launch_grad(const FitArgs &a, int npairs, int batch, hipStream_t s) {
  if constexpr (sizeof(T) == 8) {
    if (a.kernel_id == K_MATERN32_ARD) {
      hipLaunchKernelGGL((k_grad<T, 1>), dim3(npairs, batch), dim3(256), upd_lds_bytes<T>(), s, a, npairs);
      return;
    }
    if (a.kernel_id == K_MATERN52_ARD) {
      hipLaunchKernelGGL((k_grad<T, 2>), dim3(npairs, batch), dim3(256), upd_lds_bytes<T>(), s, a, npairs);
      return;
    }
  }
  hipLaunchKernelGGL(k_grad<T>, dim3(npairs, batch), dim3(256), upd_lds_bytes<T>(), s, a, npairs);
}

template <typename T>
int grad_eval(cgp_ctx *c, int N, int d, int kid, double *logml, double sums[GRAD_N], int *info) {
  hipStream_t s = c->stream;
  FitArgs a = grad_mode_args(c, N, d, kid, c->dX);
  a.y = c->dy;
  a.theta = c->dtheta;
  a.jitter = c->djitter;
  // logML and info of this one window live right behind its partial sums: [sums | logml | info] comes back in ONE copy,
  // into the pinned block (a real asynchronous copy, no pageable staging)
  const int npairs = a.NT * (a.NT + 1) / 2;
  const size_t npart = (size_t)npairs * GRAD_N;
  a.logml = c->dgpart + npart;
  a.info = reinterpret_cast<int *>(c->dgpart + npart + 1);
  int rc = run(c, a, 1, true, true, s);
  if (rc != CGP_OK) return rc;
  launch_grad<T>(a, npairs, 1, s);
  HIP_TRY(c, hipGetLastError());
  if (!grow_pinned(c->opt_pin, c->opt_pin_cap, (kOptPinIn + npart + 2) * sizeof(double))) return CGP_ENOMEM;
  double *part = static_cast<double *>(c->opt_pin) + kOptPinIn, *hl = part + npart;
  int *hi = reinterpret_cast<int *>(hl + 1);
  HIP_TRY(c, hipMemcpyAsync(part, c->dgpart, (npart + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  *logml = *hl;
  *info = *hi;
  for (int i = 0; i < GRAD_N; ++i) sums[i] = 0.0;
  for (int pz = 0; pz < npairs; ++pz)  // fixed order: deterministic
    for (int i = 0; i < GRAD_N; ++i) sums[i] += part[(size_t)pz * GRAD_N + i];
  return CGP_OK;
}

// The window of a gradient-mode evaluation -> slot 0 (once per cgp_nll_grad call, once per cgp_optimize run)
int upload_window(cgp_ctx *c, const double *X, const double *y, int N, int d, hipStream_t s) {
  std::vector<char> hx((size_t)d * N * c->esz), hy((size_t)N * c->esz);
  pack_soa(X, N, d, c->dtype, hx, 0);
  pack_vec(y, N, c->dtype, hy, 0);
  HIP_TRY(c, hipMemcpyAsync(c->dX, hx.data(), hx.size(), hipMemcpyHostToDevice, s));   // pageable source: staged by the
  HIP_TRY(c, hipMemcpyAsync(c->dy, hy.data(), hy.size(), hipMemcpyHostToDevice, s));   // runtime before the call returns
  return CGP_OK;
}

// -logML and its gradient at theta for the window in slot 0 (upload_window); X only feeds the jitter ladder's mean diagonal
int nll_grad_resident(cgp_ctx *c, const double *X, int N, int d, int kid, const double *theta, double *nll, double *grad) {
  const int nth = ntheta(kid, d);
  hipStream_t s = c->stream;
  // the whole block -- [theta | jitter | partial sums, logML, info] -- before any copy is queued: grad_eval must never
  // reallocate it under a copy in flight (hipHostFree would have to synchronise the device)
  const size_t nt_ = cdiv(N, TS), need = kOptPinIn + std::max<size_t>(64, nt_ * (nt_ + 1) / 2 * GRAD_N + 2);
  if (!grow_pinned(c->opt_pin, c->opt_pin_cap, need * sizeof(double))) return CGP_ENOMEM;
  double *hin = static_cast<double *>(c->opt_pin);   // [theta (CGP_MAX_THETA) | jitter]
  double jit = 0.0, logml = 0.0, sums[GRAD_N];
  int info = 0, rc = CGP_OK;
  for (int attempt = 0; attempt <= 5; ++attempt) {  // GPy jitchol policy
    hin = static_cast<double *>(c->opt_pin);
    for (int q = 0; q < CGP_MAX_THETA; ++q) hin[q] = q < nth ? theta[q] : 0.0;
    hin[CGP_MAX_THETA] = jit;
    HIP_TRY(c, hipMemcpyAsync(c->dtheta, hin, sizeof(double) * CGP_MAX_THETA, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->djitter, hin + CGP_MAX_THETA, sizeof(double), hipMemcpyHostToDevice, s));
    rc = c->dtype == CGP_F64 ? grad_eval<double>(c, N, d, kid, &logml, sums, &info)
                             : grad_eval<float>(c, N, d, kid, &logml, sums, &info);
    if (rc != CGP_OK) return rc;
    if (info == 0) break;
    jit = (attempt == 0) ? mean_diag(kid, theta, d, X, N) * 1e-6 : jit * 10.0;
  }
  c->fjitter = (info == 0) ? jit : 0.0;
  c->have_fit = (info == 0);
  c->fN = N;
  c->fd = d;
  c->fkernel = kid;
  memcpy(c->ftheta, theta, sizeof(double) * nth);
  if (info != 0) return info;
  *nll = -logml;
  grad_from_sums(kid, d, theta, sums, grad);   // dlogML/dtheta = 0.5 * sum_ij w_ij dK_ij/dtheta -> gradient of the NEGATIVE log likelihood
  return CGP_OK;
}
}  // namespace


// ---- short windows (N <= SM_MAX_N, fp64): one launch per evaluation / per whole optimisation (cgp_small.hpp) -------------
namespace {
bool small_enabled() {   // CGP_SMALL=off: the large-window machinery for every size (A/B, and the tests that cover it at small N)
  static const bool off = [] {
    const char *e = getenv("CGP_SMALL");
    return e && std::string(e) == "off";
  }();
  return !off;
}
inline bool small_ok(const cgp_ctx *c, int N) { return c->dtype == CGP_F64 && N <= SM_MAX_N && c->dsmall && small_enabled(); }
// k_small / k_small_predict hold the squared-exponential and Brownian forms only: a Matern call of any length takes the tiled
// schedules and the host optimiser over device gradients (which form runs stays a function of (kernel, N, d, M) alone)
inline bool small_ok(const cgp_ctx *c, int N, int kid) { return !k_is_matern(kid) && small_ok(c, N); }

// Tick-grid table of the short-window kernels (SmallArgs::tab_n): entries needed when every input is integer-valued and small
// enough for r^2 to be exact, 0 otherwise.  ad hoc off-switch for A/B and the bitwise test: CGP_TICKTAB=off.
int tick_table_entries(int kid, int d, const double *X, int N, const double *Xs, int M) {
  static const bool off = [] {
    const char *e = getenv("CGP_TICKTAB");
    return e && std::string(e) == "off";
  }();
  if (off || kid != CGP_KERNEL_RBF_BROWNIAN || d != 1) return 0;
  double lo = X[0], hi = X[0];
  auto scan = [&](const double *v, int n) {   // branch-free body (vectorises): this runs in front of launches that take 50 us
    double l = lo, h = hi;
    int bad = 0;
    for (int i = 0; i < n; ++i) {
      const double x = v[i];
      const double c = x < -67108864.0 ? -67108864.0 : (x > 67108864.0 ? 67108864.0 : x);   // NaN falls through as itself
      bad |= (double)(int)c != x;
      l = x < l ? x : l;
      h = x > h ? x : h;
    }
    lo = l;
    hi = h;
    return bad == 0;
  };
  if (!scan(X, N) || (Xs && !scan(Xs, M))) return 0;
  const double spread = hi - lo;
  return spread < (double)SM_TAB_MAX ? (int)spread + 1 : 0;
}

// ... of a batch of windows (and their test points): the largest of the windows' tables, 0 as soon as one window is off the grid
int tick_table_entries_batch(int kid, int d, int batch, const double *X, int N, const double *Xs, int M) {
  int n = 0;
  for (int b = 0; b < batch; ++b) {
    const int nb = tick_table_entries(kid, d, X + (size_t)b * N * d, N, Xs ? Xs + (size_t)b * M * d : nullptr, M);
    if (nb == 0) return 0;
    n = std::max(n, nb);
  }
  return n;
}

double mean_abs_first(const double *X, int N, int d) {
  double s = 0;
  for (int i = 0; i < N; ++i) s += std::fabs(X[(size_t)i * d]);
  return s / N;
}
double mean_diag_from(int kid, const double *theta, int d, double meanabs) {   // mean_diag with the window's mean |x| precomputed
  const double noise = theta[ntheta(kid, d) - 1] + 1e-8;
  return kid == CGP_KERNEL_RBF_BROWNIAN ? theta[0] * theta[2] * meanabs + noise : theta[0] + noise;
}

// ONE window (X (N, d) row-major, y, theta) and optionally M test points staged in the pinned block [X | y | Xs | theta],
// which the short-window kernels read in place: no copy command and no unpack launch in front of them (8 KB over the
// host link inside a launch costs less than either)
struct SmallRaw {
  const double *X, *y, *Xs;
  double *theta;
};
int small_stage_window(cgp_ctx *c, const double *X, const double *y, int N, int d, const double *Xs, int M, const double *theta, int nth,
                       SmallRaw &r) {
  const size_t nX = (size_t)N * d, nXs = (size_t)M * d, in_bytes = (nX + N + nXs + CGP_MAX_THETA) * sizeof(double);
  if (!grow_pinned(c->pin_in, c->pin_in_cap, in_bytes)) return CGP_ENOMEM;
  double *hin = static_cast<double *>(c->pin_in);
  memcpy(hin, X, nX * sizeof(double));
  memcpy(hin + nX, y, (size_t)N * sizeof(double));
  if (Xs) memcpy(hin + nX + N, Xs, nXs * sizeof(double));
  for (int q = 0; q < CGP_MAX_THETA; ++q) hin[nX + N + nXs + q] = q < nth ? theta[q] : 0.0;
  r = SmallRaw{hin, hin + nX, hin + nX + N, hin + nX + N + nXs};
  return CGP_OK;
}

int small_launch(cgp_ctx *c, int batch, int N, int d, int kid, int mode, int max_evals, hipStream_t s, double *out = nullptr,
                 const SmallRaw *raw = nullptr, int tab_n = 0) {
  SmallArgs a{};
  a.tab_n = tab_n;
  a.X = raw ? raw->X : static_cast<const double *>(c->dX);
  a.y = raw ? raw->y : static_cast<const double *>(c->dy);
  a.theta = raw ? raw->theta : c->dtheta;
  a.x_sq = raw ? 1 : N;
  a.x_sr = raw ? d : 1;
  a.out = out ? out : c->dsmall;
  a.deal = c->dsmdeal + c->smdeal_off[cdiv(N, DB)];
  a.N = N;
  a.d = d;
  a.kernel_id = kid;
  a.nth = ntheta(kid, d);
  a.mode = mode;
  a.max_evals = max_evals > 0 ? max_evals : 1000;
  a.pgtol = 1e-5;   // scipy fmin_l_bfgs_b as paramz calls it: pgtol 1e-5, factr 1e7
  a.factr = 1e7;
  const size_t lds = ((small_lds_bytes(cdiv(N, DB), d) + 15) & ~(size_t)15) + (size_t)tab_n * sizeof(double);
  if (kid == CGP_KERNEL_RBF_BROWNIAN) hipLaunchKernelGGL((k_small<true, 1>), dim3(batch), dim3(SM_THREADS), lds, s, a);
  else if (d <= 1) hipLaunchKernelGGL((k_small<false, 1>), dim3(batch), dim3(SM_THREADS), lds, s, a);
  else if (d <= 3) hipLaunchKernelGGL((k_small<false, 3>), dim3(batch), dim3(SM_THREADS), lds, s, a);
  else hipLaunchKernelGGL((k_small<false, 8>), dim3(batch), dim3(SM_THREADS), lds, s, a);
  HIP_TRY(c, hipGetLastError());
  return CGP_OK;
}

// fit at the theta slots + prediction of M test points per window in ONE launch (k_small_predict); `parts` workgroups per window
inline bool small_predict_ok(const cgp_ctx *c, int N, int d, int M) {
  return small_ok(c, N) && M > 0 && small_predict_lds(cdiv(N, DB), d) <= kLdsPerWorkgroup;
}
bool small_batch_predict_ok(const cgp_ctx *c, int batch, int N, int d, int M) {
  static const bool off = [] {
    const char *e = kAbBuild ? getenv("CGP_SMALLPRED") : nullptr;
    return e && std::string(e) == "off";
  }();
  return !off && batch <= c->max_batch && small_predict_ok(c, N, d, M);
}
int small_predict_launch(cgp_ctx *c, int batch, int N, int d, int M, int kid, int include_noise, double *dmean, double *dvar, double *dout,
                         hipStream_t s, const SmallRaw *raw, const SmallDev *dev, int tab_n, int *done_flag, int done_seq) {
  SmallArgs a{};
  a.ladder = 1;
  a.done_flag = (done_flag && c->dsmdone) ? done_flag : nullptr;
  a.done_count = c->dsmdone;
  a.done_seq = done_seq;
  a.X = raw ? raw->X : static_cast<const double *>(c->dX);
  a.y = raw ? raw->y : static_cast<const double *>(c->dy);
  a.theta = raw ? raw->theta : c->dtheta;
  a.x_sq = raw ? 1 : N;
  a.x_sr = raw ? d : 1;
  a.xs_sq = raw ? 1 : M;
  a.xs_sr = raw ? d : 1;
  a.out = dout;
  a.deal = c->dsmdeal + c->smdeal_off[cdiv(N, DB)];
  a.N = N;
  a.d = d;
  a.kernel_id = kid;
  a.nth = ntheta(kid, d);
  a.Xs = raw ? raw->Xs : static_cast<const double *>(c->dXs);
  if (dev) {
    a.X = dev->X, a.y = dev->y, a.Xs = dev->Xs, a.theta = const_cast<double *>(dev->theta);
    a.jitter = dev->jitter, a.logml = dev->logml, a.info = dev->info, a.ladder = 0;
  }
  a.mean = dmean;
  a.var = dvar;
  a.M = M;
  a.include_noise = include_noise;
  const int nchunk = cdiv(M, DB);
  // every workgroup repeats its window's fit (one workgroup per CU: the factor fills the LDS), so: as many parts as keep the
  // launch to ONE round of workgroups -- a lone window: a chunk of 16 test points each; >= n_cu windows: one workgroup each
  a.parts = std::max(1, std::min(nchunk, std::max(c->n_cu, 1) / batch));
  a.parts = cdiv(nchunk, cdiv(nchunk, a.parts));   // no part without a chunk (8 windows x 38 chunks: 19 parts of two, not 32)
  size_t lds = small_predict_lds(cdiv(N, DB), d);
  if (lds + (size_t)tab_n * sizeof(double) > kLdsPerWorkgroup) tab_n = 0;   // no room beside the factor and the K* chunk: direct evaluation
  a.tab_n = tab_n;
  lds += (size_t)tab_n * sizeof(double);
  c->last_small_dev = dout == c->dsmall;
  const dim3 grid(batch * a.parts), block(SM_THREADS);
  if (kid == CGP_KERNEL_RBF_BROWNIAN) hipLaunchKernelGGL((k_small_predict<true, 1>), grid, block, lds, s, a);
  else if (d <= 1) hipLaunchKernelGGL((k_small_predict<false, 1>), grid, block, lds, s, a);
  else if (d <= 3) hipLaunchKernelGGL((k_small_predict<false, 3>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((k_small_predict<false, 8>), grid, block, lds, s, a);
  HIP_TRY(c, hipGetLastError());
  return CGP_OK;
}

// the single-window record: the kernel writes it to the pinned block (behind its input part); one synchronisation
double *small_record_slot(cgp_ctx *c) {
  if (!grow_pinned(c->opt_pin, c->opt_pin_cap, (kOptPinIn + 64 + SM_OUT) * sizeof(double))) return nullptr;
  return static_cast<double *>(c->opt_pin) + kOptPinIn;
}
int small_read_one(cgp_ctx *c, const double *slot, double out[SM_OUT], hipStream_t s) {
  HIP_TRY(c, hipStreamSynchronize(s));
  memcpy(out, slot, SM_OUT * sizeof(double));
  memcpy(c->last_small, slot, SM_OUT * sizeof(double));
  c->last_small_dev = false;
  return CGP_OK;
}

void small_mark_fitted(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta, double jitter, bool ok) {
  c->have_fit = ok;
  c->lazy_fit = ok;
  if (ok) {
    c->lazy_win.resize((size_t)N * d + N);
    memcpy(c->lazy_win.data(), X, (size_t)N * d * sizeof(double));
    memcpy(c->lazy_win.data() + (size_t)N * d, y, (size_t)N * sizeof(double));
  }
  c->f_meandiag_x = mean_abs_first(X, N, d);
  c->fjitter = ok ? jitter : 0.0;
  c->fN = N;
  c->fd = d;
  c->fkernel = kid;
  memcpy(c->ftheta, theta, sizeof(double) * ntheta(kid, d));
}

// cgp_predict / cgp_get_alpha / cgp_get_factor after a short-window evaluation: the window, theta (and the jitter the
// evaluation needed) are on the device, the factor panel is not -- run the fit schedule once, GPy's jitter ladder around it
int ensure_fitted(cgp_ctx *c) {
  if (!c->lazy_fit) return CGP_OK;
  // nothing counts as fitted until the schedule below has succeeded: an early return (upload, copy, launch error) must not
  // leave have_fit set over a factor panel that was never built for this window
  c->lazy_fit = false;
  c->have_fit = false;
  hipStream_t s = c->stream;
  {   // the window was evaluated where the caller's copy was staged: bring it (and theta) to slot 0 now
    int rc = upload_window(c, c->lazy_win.data(), c->lazy_win.data() + (size_t)c->fN * c->fd, c->fN, c->fd, s);
    if (rc != CGP_OK) return rc;
    double th[CGP_MAX_THETA] = {0};
    std::copy(c->ftheta, c->ftheta + ntheta(c->fkernel, c->fd), th);
    HIP_TRY(c, hipMemcpyAsync(c->dtheta, th, sizeof th, hipMemcpyHostToDevice, s));   // pageable source: staged before the call returns
  }
  FitArgs a = base_args(c, c->fN, c->fd, 0, c->fkernel, 0);
  set_ctx_arrays(c, a);
  double jit = c->fjitter;
  int info = 0;
  // GPy's jitchol: one attempt without jitter, then five rungs mean(diag) 1e-6 10^r.  The short-window kernel may already
  // have climbed to rung `rung` (its jitter is kept bit for bit); the refit continues from there and never passes rung 5.
  const double base = mean_diag_from(c->fkernel, c->ftheta, c->fd, c->f_meandiag_x) * 1e-6;
  int rung = jit > 0.0 && base > 0.0 ? 1 + (int)std::lround(std::log10(jit / base)) : 0;
  for (; rung <= 5; ++rung) {
    HIP_TRY(c, hipMemcpyAsync(c->djitter, &jit, sizeof(double), hipMemcpyHostToDevice, s));
    int rc = run(c, a, 1, true, false, s);
    if (rc != CGP_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(&info, c->dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (info == 0) break;
    jit = jit == 0.0 ? base : jit * 10.0;
  }
  c->have_fit = info == 0;
  c->fjitter = info == 0 ? jit : 0.0;
  return info;
}

int small_nll_grad(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta, double *nll, double *grad) {
  hipStream_t s = c->stream;
  const int nth = ntheta(kid, d);
  double *slot = small_record_slot(c);
  if (!slot) return CGP_ENOMEM;
  SmallRaw raw;
  int rc = small_stage_window(c, X, y, N, d, nullptr, 0, theta, nth, raw);
  if (rc == CGP_OK) rc = small_launch(c, 1, N, d, kid, SM_MODE_EVAL, 1, s, slot, &raw, tick_table_entries(kid, d, X, N, nullptr, 0));
  double out[SM_OUT];
  if (rc == CGP_OK) rc = small_read_one(c, slot, out, s);
  if (rc != CGP_OK) return rc;
  const int info = (int)out[SMO_INFO];
  small_mark_fitted(c, X, y, N, d, kid, theta, out[SMO_JITTER], info == 0);
  if (info != 0) return info;
  *nll = -out[SMO_LOGML];
  for (int i = 0; i < nth; ++i) grad[i] = out[SMO_GRAD + i];
  return CGP_OK;
}

// m.optimize() of ONE short window: stage, one launch (the L-BFGS loop runs on the device), one copy back
int small_optimize(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, double *theta, int max_evals, double *logml,
                   int *n_evals) {
  hipStream_t s = c->stream;
  const int nth = ntheta(kid, d);
  for (int i = 0; i < nth; ++i)
    if (!(theta[i] > 0.0)) return CGP_EINVAL;
  double *slot = small_record_slot(c);
  if (!slot) return CGP_ENOMEM;
  SmallRaw raw;
  int rc = small_stage_window(c, X, y, N, d, nullptr, 0, theta, nth, raw);
  if (rc == CGP_OK) rc = small_launch(c, 1, N, d, kid, SM_MODE_OPT, max_evals, s, slot, &raw, tick_table_entries(kid, d, X, N, nullptr, 0));
  double out[SM_OUT];
  if (rc == CGP_OK) rc = small_read_one(c, slot, out, s);
  if (rc != CGP_OK) return rc;
  if (out[SMO_INFO] != 0.0) {   // the start itself is not positive definite even with the jitter ladder
    c->have_fit = false;
    return 1;
  }
  for (int i = 0; i < nth; ++i) theta[i] = out[SMO_THETA + i];
  small_mark_fitted(c, X, y, N, d, kid, theta, 0.0, true);
  if (logml) *logml = out[SMO_LOGML];
  if (n_evals) *n_evals = (int)out[SMO_EVALS];
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_nll_grad(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta,
                            double *nll, double *grad) {
  int rc = check_shape(c, 1, N, d, N, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta || !nll || !grad) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  if (small_ok(c, N, kid)) return small_nll_grad(c, X, y, N, d, kid, theta, nll, grad);
  c->lazy_fit = false;
  rc = upload_window(c, X, y, N, d, c->stream);
  if (rc != CGP_OK) return rc;
  return nll_grad_resident(c, X, N, d, kid, theta, nll, grad);
}

extern "C" int cgp_optimize(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, double *theta,
                            int max_evals, double *logml, int *n_evals) {
  int rc = check_shape(c, 1, N, d, N, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  std::vector<double> x(nth), th(nth), g(nth);   // x: the Logexp image of theta
  for (int i = 0; i < nth; ++i) {
    if (!(theta[i] > 0.0)) return CGP_EINVAL;
    x[i] = corenav::logexp_x(theta[i]);
  }
  int hard_error = CGP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (small_ok(c, N, kid)) return small_optimize(c, X, y, N, d, kid, theta, max_evals, logml, n_evals);
  c->lazy_fit = false;
  rc = upload_window(c, X, y, N, d, c->stream);   // the window does not change between evaluations: only theta travels
  if (rc != CGP_OK) return rc;
  auto fg = [&](const std::vector<double> &xx, std::vector<double> &gx) -> double {
    for (int i = 0; i < nth; ++i) th[i] = corenav::logexp_theta_eval(xx[i]);
    double nll = 0.0;
    const int r = nll_grad_resident(c, X, N, d, kid, th.data(), &nll, g.data());
    if (r < 0) hard_error = r;
    if (r != 0) return INFINITY;  // not PD even with jitter: infeasible point
    for (int i = 0; i < nth; ++i) gx[i] = g[i] * corenav::logexp_dtheta_dx(xx[i], th[i]);
    return nll;
  };
  corenav::LbfgsResult res = corenav::lbfgs_minimize(fg, x, max_evals > 0 ? max_evals : 1000);
  if (hard_error != CGP_OK) return hard_error;
  for (int i = 0; i < nth; ++i) theta[i] = corenav::logexp_theta(x[i]);
  // leave the context fitted at the optimum
  double nll = 0.0;
  rc = nll_grad_resident(c, X, N, d, kid, theta, &nll, g.data());
  if (rc != CGP_OK) return rc;
  if (logml) *logml = -nll;
  if (n_evals) *n_evals = res.evals + 1;
  return CGP_OK;
}


namespace {
// The reference node's whole callback (gp_slip_node.py:16-63) for a short window in ONE host round trip: stage the window,
// the prediction ticks and theta (one H2D), then queue  unpack -> [k_small: m.optimize() on the device, optimum left in the
// context's theta slot] -> k_small_predict (fit at that slot with GPy's jitter ladder + the predictions) -> one D2H, and
// synchronise once.  max_evals == 0: fixed theta.  CGP_ESTATE: not a short fp64 window -- the caller's general path.
int node_callback_small(cgp_ctx *c, const double *time_array, const double *slip_array, int n, int kid, double *theta, int max_evals,
                        double *mean, double *sigma, int cap, int *m_out) {
  const int ntr = (int)(0.9 * (double)n);  // gp_slip_node.py:27-29
  if (ntr < 1 || !small_ok(c, ntr, kid) || check_shape(c, 1, ntr, 1, ntr, kid) != CGP_OK) return CGP_ESTATE;
  const int nth = ntheta(kid, 1);
  for (int i = 0; i < nth; ++i)
    if (!(theta[i] > 0.0)) return max_evals > 0 ? CGP_EINVAL : CGP_ESTATE;
  double xmin = time_array[0], xmax = time_array[0];   // gp_slip_node.py:45  X_ = np.arange(X.min(), X.max() + 600, 1)
  for (int i = 1; i < n; ++i) {
    xmin = std::min(xmin, time_array[i]);
    xmax = std::max(xmax, time_array[i]);
  }
  const long long glen = (long long)std::ceil((xmax + 600.0 - xmin) / 1.0);
  const long long mo = std::max(0LL, glen - n);         // gp_slip_node.py:59-61  means[len(X):]
  const int M = (int)std::min<long long>(mo, cap);
  if (M == 0 || M > c->max_m || !small_predict_ok(c, ntr, 1, M)) return CGP_ESTATE;
  if (m_out) *m_out = (int)mo;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t nout = 2 * (size_t)M + 2 * SM_OUT, out_bytes = (nout + 1) * sizeof(double);   // mean, var, the two kernels' records, the completion word
  if (!grow_pinned(c->pin_in, c->pin_in_cap, (2 * (size_t)ntr + M + CGP_MAX_THETA) * sizeof(double)) ||
      !grow_pinned(c->pin_out, c->pin_out_cap, out_bytes))
    return CGP_ENOMEM;
  // no copy commands and no unpack launch: the kernels read the pinned block in place and write their results (10 KB) to
  // pinned host memory, visible when the stream has drained
  SmallRaw raw;
  int rc = small_stage_window(c, time_array, slip_array, ntr, 1, nullptr, 0, theta, nth, raw);
  if (rc != CGP_OK) return rc;
  {   // the prediction ticks behind y, theta behind them
    double *hin = static_cast<double *>(c->pin_in), *xs = hin + 2 * (size_t)ntr;
    for (int m = 0; m < M; ++m) xs[m] = xmin + (double)(n + m);
    for (int q = 0; q < CGP_MAX_THETA; ++q) xs[M + q] = q < nth ? theta[q] : 0.0;
    raw.Xs = xs;
    raw.theta = xs + M;
  }
  double *hout = static_cast<double *>(c->pin_out);
  double *rec = hout + 2 * (size_t)M, *opt = rec + SM_OUT;
  if (max_evals > 0) {   // leaves the optimum in raw.theta, where the next launch reads it
    rc = small_launch(c, 1, ntr, 1, kid, SM_MODE_OPT, max_evals, s, opt, &raw, tick_table_entries(kid, 1, time_array, ntr, nullptr, 0));
    if (rc != CGP_OK) return rc;
  }
  // the last workgroup of the prediction launch stores the call's sequence number to a word of the pinned block (behind a system-scope
  // fence): the host polls it instead of synchronising the stream, and falls back to the synchronisation after 2 ms (a long
  // optimisation, a faulting kernel)
  volatile int *flag = reinterpret_cast<volatile int *>(hout + nout);
  const int seq = (c->small_seq = c->small_seq % 1000000 + 1);
  *flag = 0;
  rc = small_predict_launch(c, 1, ntr, 1, M, kid, 1, hout, hout + M, rec, s, &raw, nullptr, tick_table_entries(kid, 1, time_array, ntr, raw.Xs, M),
                            const_cast<int *>(reinterpret_cast<volatile int *>(flag)), seq);
  if (rc != CGP_OK) return rc;
  bool done = false;
  if (c->dsmdone) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
      if (*flag == seq) { done = true; break; }
      if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  if (!done) HIP_TRY(c, hipStreamSynchronize(s));
  memcpy(c->last_small, max_evals > 0 ? opt : rec, SM_OUT * sizeof(double));
  if (max_evals > 0) {
    if (opt[SMO_INFO] != 0.0) {   // the start values themselves are not positive definite even with the jitter ladder
      c->have_fit = false;
      c->lazy_fit = false;
      return 1;
    }
    for (int i = 0; i < nth; ++i) theta[i] = opt[SMO_THETA + i];
  }
  const int info = (int)rec[SMO_INFO];
  small_mark_fitted(c, time_array, slip_array, ntr, 1, kid, theta, rec[SMO_JITTER], info == 0);
  if (info != 0) return info;  // not positive definite even with GPy's jitter ladder (LinAlgError there)
  memcpy(mean, hout, (size_t)M * sizeof(double));
  for (int m = 0; m < M; ++m) sigma[m] = 2.0 * std::sqrt(hout[M + m]);   // gp_slip_node.py:61
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_slip_node_callback_opt(cgp_ctx *c, const double *time_array, const double *slip_array, int n,
                                          int kid, double *theta, int max_evals, double *mean, double *sigma, int cap,
                                          int *m_out) {
  if (!c || !time_array || !slip_array || !theta || n < 2) return CGP_EINVAL;
  if (max_evals > 0 && mean && sigma && cap >= 0) {
    const int rc = node_callback_small(c, time_array, slip_array, n, kid, theta, max_evals, mean, sigma, cap, m_out);
    if (rc != CGP_ESTATE) return rc;   // CGP_ESTATE: not a short fp64 window -- the two-call path below
  }
  if (max_evals > 0) {
    const int ntr = (int)(0.9 * (double)n);  // gp_slip_node.py:27-29
    int rc = cgp_optimize(c, time_array, slip_array, ntr, 1, kid, theta, max_evals, nullptr, nullptr);  // :36
    if (rc != CGP_OK) return rc;
  }
  return cgp_slip_node_callback(c, time_array, slip_array, n, kid, theta, mean, sigma, cap, m_out);
}

// the sliding windows' host layer: cgp_window_init ... cgp_window_optimize
#include "cgp_window_host.hpp"
// joint forecast after batch / single fits: cgp_joint_reserve ... cgp_sample
#include "cgp_joint_host.hpp"
// multi-target fits: cgp_multi_reserve ... cgp_fit_predict_multi_batch_device
#include "cgp_multi_host.hpp"
// explicit basis functions (trend) after the multi-target fits: cgp_trend_reserve ... cgp_fit_predict_trend_batch_device
#include "cgp_trend_host.hpp"
// sparse (inducing-point) fits: cgp_sparse_reserve ... cgp_fit_predict_sparse_batch_device
#include "cgp_sparse_host.hpp"

struct cgp_recorder {
  corenav::SlipWindowRecorder r;
};
extern "C" cgp_recorder *cgp_recorder_create(void) { return new cgp_recorder(); }
extern "C" void cgp_recorder_destroy(cgp_recorder *rec) { delete rec; }
extern "C" int cgp_recorder_update(cgp_recorder *rec, const double wv[4], double vlin, double cmd_x, double *slip_out,
                                   double *time_out, double *slipwin_out, int cap, int *n_out) {
  if (!rec || !wv) return CGP_EINVAL;
  const bool pub = rec->r.Update(wv[0], wv[1], wv[2], wv[3], vlin, cmd_x);
  if (slip_out) *slip_out = rec->r.slip;
  if (pub) {
    const int n = (int)rec->r.time_array.size();
    if (n_out) *n_out = n;
    for (int i = 0; i < std::min(n, cap); ++i) {
      if (time_out) time_out[i] = rec->r.time_array[i];
      if (slipwin_out) slipwin_out[i] = rec->r.slip_array[i];
    }
    if (n > cap && (time_out || slipwin_out)) return CGP_ECAPACITY;  // *n_out = the size the window needs
  }
  return pub ? 1 : 0;
}
extern "C" void cgp_recorder_stop_cmd(cgp_recorder *rec, double cmd_stop) {
  if (rec) rec->r.stopCallback(cmd_stop);
}
extern "C" void cgp_recorder_cmd(cgp_recorder *rec, double cmd_x) {
  if (rec) rec->r.CmdCallBack(cmd_x);
}
extern "C" void cgp_recorder_state(const cgp_recorder *rec, double st[8]) {
  if (!rec || !st) return;
  const auto &r = rec->r;
  st[0] = r.odomUptCount; st[1] = r.startRecording; st[2] = r.stopRecording; st[3] = r.gp_flag;
  st[4] = r.first_driving_flag; st[5] = r.new_stop_data_arrived_; st[6] = r.skipped_windows; st[7] = r.cmd_stop_;
}

extern "C" int cgp_predict_stop_batch(cgp_ctx *c, int ntraj, int M, const double *mean, const double *sigma,
                                      const double *P, const double *Q, const double *STM, const double *Hvec,
                                      const double *pos, const double *arrival, const double *now, double threshold,
                                      int h_bug, const double init_llh[3], const double init_ecef[3], int *fired,
                                      double *stop_cmd, int *i_out, double *xy_err) {
  if (!c || ntraj < 1 || M < 0 || !mean || !sigma || !P || !Q || !STM || !Hvec || !pos || !arrival || !now ||
      !init_llh || !init_ecef || !fired || !stop_cmd || !i_out || !xy_err)
    return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t T = ntraj;
  const size_t nd = T * (2 * (size_t)M + 3 * 225 + 60 + 3 + 4 + 2 + 2);  // doubles in (incl. 4 trig values), 2 double outputs
  // staging buffers live in the context and only grow (the replay loop calls this once per tick group)
  if (nd > c->la_nd) {
    if (c->la_buf) (void)hipFree(c->la_buf);
    c->la_buf = nullptr;
    c->la_nd = 0;
    if (hipMalloc((void **)&c->la_buf, nd * sizeof(double)) != hipSuccess) return CGP_ENOMEM;
    c->la_nd = nd;
  }
  if (T * 2 > c->la_ni) {
    if (c->la_ibuf) (void)hipFree(c->la_ibuf);
    c->la_ibuf = nullptr;
    c->la_ni = 0;
    if (hipMalloc((void **)&c->la_ibuf, T * 2 * sizeof(int)) != hipSuccess) return CGP_ENOMEM;
    c->la_ni = T * 2;
  }
  double *buf = c->la_buf;
  int *ibuf = c->la_ibuf;
  hipStream_t s = c->stream;
  double *d = buf;
  LookaheadArgs a{};
  auto put = [&](const double *src, size_t n) {
    double *dst = d;
    (void)hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, s);
    d += n;
    return dst;
  };
  a.mean = put(mean, T * M);
  a.sigma = put(sigma, T * M);
  a.P = put(P, T * 225);
  a.Q = put(Q, T * 225);
  a.STM = put(STM, T * 225);
  a.Hvec = put(Hvec, T * 60);
  a.pos = put(pos, T * 3);
  // sines / cosines of the base positions and of the ENU origin on the host: libm's large-argument
  // paths would otherwise set the kernel's register and scratch footprint
  std::vector<double> trig(T * 4);
  for (size_t t = 0; t < T; ++t) {
    trig[4 * t + 0] = std::sin(pos[3 * t]);
    trig[4 * t + 1] = std::cos(pos[3 * t]);
    trig[4 * t + 2] = std::sin(pos[3 * t + 1]);
    trig[4 * t + 3] = std::cos(pos[3 * t + 1]);
  }
  a.trig = put(trig.data(), T * 4);
  a.origin_trig[0] = std::sin(init_llh[0]);
  a.origin_trig[1] = std::cos(init_llh[0]);
  a.origin_trig[2] = std::sin(init_llh[1]);
  a.origin_trig[3] = std::cos(init_llh[1]);
  a.arrival = put(arrival, T);
  a.now = put(now, T);
  a.stop_cmd = d;
  a.xy_err = d + T;
  a.fired = ibuf;
  a.i_out = ibuf + T;
  a.ntraj = ntraj;
  a.M = M;
  a.h_bug_compatible = h_bug;
  a.threshold = threshold;
  for (int i = 0; i < 3; ++i) {
    a.init_llh[i] = init_llh[i];
    a.init_ecef[i] = init_ecef[i];
  }
  hipLaunchKernelGGL(k_lookahead, dim3(cdiv(ntraj, LA_WAVES)), dim3(64 * LA_WAVES),
                     (size_t)LA_WAVES * LA_PER_WAVE * sizeof(double), s, a);
  int rc = CGP_OK;
  if (!hip_ok(c, hipGetLastError(), "k_lookahead")) rc = CGP_EHIP;
  std::vector<int> hi(T * 2);
  if (rc == CGP_OK && !hip_ok(c, hipMemcpyAsync(stop_cmd, a.stop_cmd, T * 8, hipMemcpyDeviceToHost, s), "D2H")) rc = CGP_EHIP;
  if (rc == CGP_OK && !hip_ok(c, hipMemcpyAsync(xy_err, a.xy_err, T * 8, hipMemcpyDeviceToHost, s), "D2H")) rc = CGP_EHIP;
  if (rc == CGP_OK && !hip_ok(c, hipMemcpyAsync(hi.data(), ibuf, T * 2 * sizeof(int), hipMemcpyDeviceToHost, s), "D2H")) rc = CGP_EHIP;
  if (!hip_ok(c, hipStreamSynchronize(s), "sync")) rc = CGP_EHIP;
  if (rc != CGP_OK) return rc;
  for (size_t i = 0; i < T; ++i) {
    fired[i] = hi[i];
    i_out[i] = hi[T + i];
  }
  return CGP_OK;
}

extern "C" int cgp_selftest_lbfgs(double *x, int n, int max_evals, double *f_out) {
  if (!x || n < 2 || n > 16) return CGP_EINVAL;
  std::vector<double> xv(x, x + n);
  auto fg = [n](const std::vector<double> &v, std::vector<double> &g) {
    double f = 0.0;
    for (int i = 0; i < n; ++i) g[i] = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
      const double a = v[i + 1] - v[i] * v[i], b = 1.0 - v[i];
      f += 100.0 * a * a + b * b;
      g[i] += -400.0 * a * v[i] - 2.0 * b;
      g[i + 1] += 200.0 * a;
    }
    return f;
  };
  corenav::LbfgsResult r = corenav::lbfgs_minimize(fg, xv, max_evals > 0 ? max_evals : 1000, 1e-8, 10.0);
  for (int i = 0; i < n; ++i) x[i] = xv[i];
  if (f_out) *f_out = r.f;
  return r.status == 3 ? -1 : r.evals;
}

extern "C" int cgp_lbfgs_minimize(cgp_objective_fn fn, void *user, double *x, int n, int max_evals, double pgtol, double factr,
                                  double *f_out, int *n_evals, int *n_iters, int *status) {
  if (!fn || !x || n < 1 || n > corenav::LB_N) return CGP_EINVAL;
  std::vector<double> xv(x, x + n);
  auto fg = [&](const std::vector<double> &v, std::vector<double> &g) { return fn(v.data(), g.data(), n, user); };
  corenav::LbfgsResult r = corenav::lbfgs_minimize(fg, xv, max_evals > 0 ? max_evals : 1000, pgtol, factr);
  for (int i = 0; i < n; ++i) x[i] = xv[i];
  if (f_out) *f_out = r.f;
  if (n_evals) *n_evals = r.evals;
  if (n_iters) *n_iters = r.iters;
  if (status) *status = r.status;
  return CGP_OK;
}

namespace {
// Gradient-mode evaluation of `batch` windows already uploaded to slots 0..batch-1 (theta in dtheta).
template <typename T>
int grad_eval_batch(cgp_ctx *c, int batch, int N, int d, int kid, std::vector<double> &logml, std::vector<double> &sums,
                    std::vector<int> &info) {
  hipStream_t s = c->stream;
  FitArgs a = grad_mode_args(c, N, d, kid, c->dX);
  a.y = c->dy;
  a.theta = c->dtheta;
  a.jitter = c->djitter;  // per window; zero unless the jitter ladder of cgp_optimize_batch is climbing
  a.logml = c->dlogml;
  a.info = c->dinfo;
  int rc = run(c, a, batch, true, true, s);
  if (rc != CGP_OK) return rc;
  const int npairs = a.NT * (a.NT + 1) / 2;
  launch_grad<T>(a, npairs, batch, s);
  HIP_TRY(c, hipGetLastError());
  std::vector<double> part((size_t)batch * npairs * GRAD_N);
  logml.resize(batch);
  info.resize(batch);
  HIP_TRY(c, hipMemcpyAsync(part.data(), c->dgpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(logml.data(), c->dlogml, sizeof(double) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(info.data(), c->dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  sums.assign((size_t)batch * GRAD_N, 0.0);
  for (int b = 0; b < batch; ++b)
    for (int pz = 0; pz < npairs; ++pz)
      for (int i = 0; i < GRAD_N; ++i) sums[(size_t)b * GRAD_N + i] += part[((size_t)b * npairs + pz) * GRAD_N + i];
  return CGP_OK;
}
}  // namespace

extern "C" int cgp_optimize_batch(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y,
                                  double *theta, int theta_stride, int max_evals, double *logml_out, int *n_evals) {
  int rc = check_shape(c, batch, N, d, N, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta) return CGP_EINVAL;
  const int nth = ntheta(kid, d);
  if (theta_stride < nth) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if ((rc = upload_batch_xy(c, batch, N, d, X, y, s)) != CGP_OK) return rc;
  c->lazy_fit = false;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < nth; ++i)
      if (!(theta[(size_t)b * theta_stride + i] > 0.0)) return CGP_EINVAL;
  if (small_ok(c, N, kid)) {
    // short windows: ONE launch, one workgroup per window, each running its own L-BFGS loop on the device (cgp_small.hpp)
    std::vector<double> hth;
    rc = upload_theta(c, theta, theta_stride, nth, batch, s, hth);
    if (rc == CGP_OK) rc = small_launch(c, batch, N, d, kid, SM_MODE_OPT, max_evals, s, nullptr, nullptr, tick_table_entries_batch(kid, d, batch, X, N, nullptr, 0));
    c->last_small_dev = true;
    if (rc != CGP_OK) return rc;
    std::vector<double> out((size_t)batch * SM_OUT);
    HIP_TRY(c, hipMemcpyAsync(out.data(), c->dsmall, out.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->have_fit = false;
    for (int b = 0; b < batch; ++b) {
      const double *ob = out.data() + (size_t)b * SM_OUT;
      for (int i = 0; i < nth; ++i) theta[(size_t)b * theta_stride + i] = ob[SMO_THETA + i];
      if (logml_out) logml_out[b] = ob[SMO_LOGML];
      if (n_evals) n_evals[b] = (int)ob[SMO_EVALS];
    }
    return CGP_OK;
  }
  std::vector<double> hth, lml, sums, jit(batch, 0.0), lml2, sums2;
  std::vector<int> info, info2;
  c->have_fit = false;
  auto eval = [&](std::vector<double> &l, std::vector<double> &sm, std::vector<int> &inf) {
    return c->dtype == CGP_F64 ? grad_eval_batch<double>(c, batch, N, d, kid, l, sm, inf)
                               : grad_eval_batch<float>(c, batch, N, d, kid, l, sm, inf);
  };
  // one round of the optimiser: every window is evaluated (a finished one at its best point), only active ones climb the ladder
  auto round = [&](const double *th, const char *active, double *f, double *g, char *feasible) -> int {
    int rc = upload_theta(c, th, nth, nth, batch, s, hth);
    if (rc != CGP_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
    rc = eval(lml, sums, info);
    if (rc != CGP_OK) return rc;
    // GPy jitchol inside m.optimize(): a trial point whose matrix is not positive definite is retried
    // with jitter mean(diag) 1e-6 10^k, k = 0..4.  Only the windows that failed climb the ladder (the
    // others keep jitter 0 and their first results); the re-evaluation is one more batched schedule.
    for (int attempt = 0; attempt < 5; ++attempt) {
      bool any_bad = false;
      for (int b = 0; b < batch; ++b) {
        if (!active[b] || info[b] == 0) continue;
        any_bad = true;
        jit[b] = attempt == 0 ? mean_diag(kid, th + (size_t)b * nth, d, X + (size_t)b * N * d, N) * 1e-6 : jit[b] * 10.0;
      }
      if (!any_bad) break;
      HIP_TRY(c, hipMemcpyAsync(c->djitter, jit.data(), sizeof(double) * batch, hipMemcpyHostToDevice, s));
      rc = eval(lml2, sums2, info2);
      if (rc != CGP_OK) return rc;
      for (int b = 0; b < batch; ++b) {
        if (!active[b] || info[b] == 0) continue;
        info[b] = info2[b];
        lml[b] = lml2[b];
        std::copy(sums2.begin() + (size_t)b * GRAD_N, sums2.begin() + (size_t)(b + 1) * GRAD_N, sums.begin() + (size_t)b * GRAD_N);
      }
    }
    std::fill(jit.begin(), jit.end(), 0.0);
    for (int b = 0; b < batch; ++b) {
      if (!active[b]) continue;
      feasible[b] = info[b] == 0;
      if (!feasible[b]) continue;
      grad_from_sums(kid, d, th + (size_t)b * nth, sums.data() + (size_t)b * GRAD_N, g + (size_t)b * nth);
      f[b] = -lml[b];
    }
    return CGP_OK;
  };
  corenav::LbfgsBatchResult res;
  if ((rc = corenav::lbfgs_minimize_logexp_batch(batch, nth, theta, theta_stride, nullptr, max_evals, round, res)) != CGP_OK) return rc;
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < nth; ++i) theta[(size_t)b * theta_stride + i] = res.theta[(size_t)b * nth + i];
    if (logml_out) logml_out[b] = -res.f[b];
    if (n_evals) n_evals[b] = res.evals[b];
  }
  return CGP_OK;
}

// ---- leave-one-out cross-validation from the factor (cgp_loo.hpp; fp64 contexts) -------------------------------------------
namespace {
struct LooOut {   // device pointers at the first fit of the call; each may be null
  double *mean, *var, *lpd, *sum;
};

// Gradient-mode factorisation of `nfit` fits into slabs 0 .. nfit - 1 (grad_eval_batch's arguments: xid = 1, M = N, the tiled
// schedules for every shape), then k_loo on Wt and alpha instead of k_grad, then the per-fit sums.  All on s, nothing allocated,
// nothing synchronised.  dvar is free once k_finalize has run: it holds loo_lpd for k_loo_sum when the caller wants no loo_lpd.
int loo_enqueue(cgp_ctx *c, int nfit, int N, int d, int kid, const double *dX, const double *dy, const double *dtheta,
                const double *djitter, const LooOut &o, double *dlogml, int *dinfo, hipStream_t s) {
  FitArgs a = grad_mode_args(c, N, d, kid, dX);
  a.y = dy;
  a.theta = dtheta;
  a.jitter = djitter;
  a.logml = dlogml;
  a.info = dinfo;
  int rc = run(c, a, nfit, true, true, s);
  if (rc != CGP_OK) return rc;
  double *lpd = o.lpd ? o.lpd : static_cast<double *>(c->dvar);
  hipLaunchKernelGGL(k_loo, dim3(cdiv(N, LOO_EB), nfit), dim3(LOO_WAVES * 64), 0, s, a, o.mean, o.var, lpd);
  if (o.sum) hipLaunchKernelGGL(k_loo_sum, dim3(nfit), dim3(64), 0, s, lpd, dinfo, N, o.sum);
  HIP_TRY(c, hipGetLastError());
  return CGP_OK;
}

// Host buffers: the windows to slots 0 .. batch - 1 (cgp_optimize_batch's upload), one batched call, then GPy's jitter ladder
// for the fits that failed, one fit at a time in slab 0 (cgp_fit_predict_batch's policy); LOO of a retried fit is computed on the
// Ky that finally factored.  jit_out (batch) receives the jitter each fit ended with.
int loo_batch_host(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y, const double *theta,
                   int theta_stride, double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum, double *logml, int *info,
                   double *jit_out) {
  const int nth = ntheta(kid, d);
  hipStream_t s = c->stream;
  const size_t B = batch, BN = B * N;
  c->have_fit = false;
  c->lazy_fit = false;
  if (!grow_device(c->draw, c->draw_cap, (3 * BN + B) * sizeof(double))) return CGP_ENOMEM;
  double *dout = static_cast<double *>(c->draw);
  const LooOut o{loo_mean ? dout : nullptr, loo_var ? dout + BN : nullptr, loo_lpd ? dout + 2 * BN : nullptr,
                 lpd_sum ? dout + 3 * BN : nullptr};
  int rc = upload_batch_xy(c, batch, N, d, X, y, s);
  if (rc != CGP_OK) return rc;
  std::vector<double> hth;
  if ((rc = upload_theta(c, theta, theta_stride, nth, batch, s, hth)) != CGP_OK) return rc;
  HIP_TRY(c, hipMemsetAsync(c->djitter, 0, sizeof(double) * batch, s));
  const double *dX = static_cast<const double *>(c->dX), *dy = static_cast<const double *>(c->dy);
  rc = loo_enqueue(c, batch, N, d, kid, dX, dy, c->dtheta, c->djitter, o, c->dlogml, c->dinfo, s);
  if (rc != CGP_OK) return rc;
  std::vector<int> hinfo(batch);
  HIP_TRY(c, hipMemcpyAsync(hinfo.data(), c->dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  rc = jitter_ladder(c, batch, N, d, kid, theta, theta_stride, X, hinfo.data(), nullptr, jit_out, s, [&](int b) {
    const size_t off = (size_t)b * N;
    const LooOut ob{o.mean ? o.mean + off : nullptr, o.var ? o.var + off : nullptr, o.lpd ? o.lpd + off : nullptr,
                    o.sum ? o.sum + b : nullptr};
    return loo_enqueue(c, 1, N, d, kid, dX + off * d, dy + off, c->dtheta + (size_t)b * CGP_MAX_THETA, c->djitter + b, ob,
                       c->dlogml + b, c->dinfo + b, s);
  });
  if (rc != CGP_OK) return rc;
  for (int b = 0; b < batch; ++b)
    if (hinfo[b] != 0) jit_out[b] = 0.0;   // only a fit that factored reports a jitter
  if (loo_mean) HIP_TRY(c, hipMemcpyAsync(loo_mean, o.mean, BN * sizeof(double), hipMemcpyDeviceToHost, s));
  if (loo_var) HIP_TRY(c, hipMemcpyAsync(loo_var, o.var, BN * sizeof(double), hipMemcpyDeviceToHost, s));
  if (loo_lpd) HIP_TRY(c, hipMemcpyAsync(loo_lpd, o.lpd, BN * sizeof(double), hipMemcpyDeviceToHost, s));
  if (lpd_sum) HIP_TRY(c, hipMemcpyAsync(lpd_sum, o.sum, B * sizeof(double), hipMemcpyDeviceToHost, s));
  if (logml) HIP_TRY(c, hipMemcpyAsync(logml, c->dlogml, B * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  int first = 0;
  for (int b = 0; b < batch; ++b) {
    if (info) info[b] = hinfo[b];
    if (first == 0 && hinfo[b] != 0) first = hinfo[b];
  }
  return first;
}

int loo_check(const cgp_ctx *c, int batch, int N, int d, int kid) {
  if (!c || c->dtype != CGP_F64) return CGP_EINVAL;   // alpha_i / kd_i cancels against y_i: not promised in single precision
  return check_shape(c, batch, N, d, N, kid);
}
}  // namespace

extern "C" int cgp_loo_batch_device(cgp_ctx *c, int batch, int N, int d, int kid, const double *dX, const double *dy,
                                    const double *dtheta, const double *djitter, double *dloo_mean, double *dloo_var,
                                    double *dloo_lpd, double *dlpd_sum, double *dlogml, int *dinfo, void *hip_stream) {
  int rc = loo_check(c, batch, N, d, kid);
  if (rc != CGP_OK) return rc;
  if (!dX || !dy || !dtheta || !dlogml || !dinfo) return CGP_EINVAL;
  if (!dloo_mean && !dloo_var && !dloo_lpd && !dlpd_sum) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->have_fit = false;
  c->lazy_fit = false;
  return loo_enqueue(c, batch, N, d, kid, dX, dy, dtheta, djitter, LooOut{dloo_mean, dloo_var, dloo_lpd, dlpd_sum}, dlogml, dinfo,
                     pick_stream(c, hip_stream));
}

extern "C" int cgp_loo_batch(cgp_ctx *c, int batch, int N, int d, int kid, const double *X, const double *y, const double *theta,
                             int theta_stride, double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum, double *logml,
                             int *info) {
  int rc = loo_check(c, batch, N, d, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta || theta_stride < ntheta(kid, d)) return CGP_EINVAL;
  if (!loo_mean && !loo_var && !loo_lpd && !lpd_sum) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<double> jit(batch);
  return loo_batch_host(c, batch, N, d, kid, X, y, theta, theta_stride, loo_mean, loo_var, loo_lpd, lpd_sum, logml, info, jit.data());
}

extern "C" int cgp_loo(cgp_ctx *c, const double *X, const double *y, int N, int d, int kid, const double *theta, double *loo_mean,
                       double *loo_var, double *loo_lpd, double *lpd_sum) {
  int rc = loo_check(c, 1, N, d, kid);
  if (rc != CGP_OK) return rc;
  if (!X || !y || !theta) return CGP_EINVAL;
  if (!loo_mean && !loo_var && !loo_lpd && !lpd_sum) return CGP_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const int nth = ntheta(kid, d);
  int info = 0;
  double jit = 0.0;
  rc = loo_batch_host(c, 1, N, d, kid, X, y, theta, nth, loo_mean, loo_var, loo_lpd, lpd_sum, nullptr, &info, &jit);
  if (rc < 0) return rc;
  // the factor panel of slab 0, alpha, the window, theta and the jitter are resident: fitted, as after cgp_nll_grad
  c->fjitter = jit;
  c->have_fit = (info == 0);
  c->fN = N;
  c->fd = d;
  c->fkernel = kid;
  memcpy(c->ftheta, theta, sizeof(double) * nth);
  return info;
}

// multi-target objective: cgp_multi_grad_reserve ... cgp_optimize_multi_batch
#include "cgp_multi_grad_host.hpp"
// leave-one-out objective: cgp_loo_grad_reserve ... cgp_optimize_loo_batch
#include "cgp_loo_grad_host.hpp"
#include "cgp_pgrad_host.hpp"
// the sparse fits' objective: cgp_sparse_grad_reserve ... cgp_optimize_sparse_batch
#include "cgp_sparse_grad_host.hpp"

// sparse fits with several target columns: cgp_sparse_multi_reserve ... cgp_fit_predict_sparse_multi_batch_device
#include "cgp_sparse_multi_host.hpp"

// the objective of sparse fits with several target columns: cgp_sparse_multi_grad_reserve ... cgp_optimize_sparse_multi_batch
#include "cgp_sparse_multi_grad_host.hpp"
