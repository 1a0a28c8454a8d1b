/* corenav_gp.h -- C ABI of the MI355X-native slip-GP engine (libcorenav_gp.so).
 *
 * The reference has no C ABI on this path: its operator boundary is the ROS message pair
 * core_nav/GP_Input -> core_nav/GP_Output (core_navigation/msg/GP_Input.msg:1-3,
 * core_navigation/msg/GP_Output.msg:1-3) produced by core_navigation/script/gp_slip_node.py and
 * consumed by gp_predictor/src/gp_predictor.cpp.  The entry points below are what a binding for
 * that path has to call; each one names the reference lines it replaces.  INTEGRATION.md shows the
 * ctypes stub for gp_slip_node.py and the C++ call for gp_predictor.
 *
 * Conventions: plain C, no exceptions cross the boundary, caller owns every host pointer, the
 * library owns device memory inside the context.  A context is NOT thread-safe: one context per
 * host thread / HIP stream.  Return value: 0 ok, < 0 argument/runtime error (cgp_strerror), > 0 a
 * LAPACK-style `info` = 1-based index of the first non-positive pivot after the GPy jitter policy
 * (mean(diag)*1e-6*10^k, k = 0..4) is exhausted.
 */
#ifndef CORENAV_GP_H_
#define CORENAV_GP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cgp_ctx cgp_ctx;

/* kernel ids; theta layouts (all fp64, natural -- not log -- parameters):
 *   SE_ISO        [sigma_f^2, ell, sigma_n^2]
 *   SE_ARD        [sigma_f^2, ell_1 .. ell_d, sigma_n^2]
 *   RBF_BROWNIAN  [sigma_rbf^2, ell, sigma_brownian^2, sigma_n^2]   d == 1
 *   MATERN32_ARD, MATERN52_ARD   the layout of SE_ARD: [sigma_f^2, ell_1 .. ell_d, sigma_n^2]
 * RBF_BROWNIAN is `GPy.kern.RBF(1) * GPy.kern.Brownian(1)` of gp_slip_node.py:31.  The Matern pair (ids appended: no existing value
 * moved, the ABI revision stays 3; a library built before them answers CGP_EINVAL) is what that one line becomes with the
 * alternatives listed under it, `GPy.kern.Matern32(1)` / `GPy.kern.Matern52(1)` (gp_slip_node.py:32-34) at d = 1, with one
 * length-scale per input dimension beyond:
 *   r^2 = sum_q ((x_q - x'_q) / ell_q)^2
 *   MATERN32: k = sigma_f^2 (1 + sqrt(3) r) exp(-sqrt(3) r)
 *   MATERN52: k = sigma_f^2 (1 + sqrt(5) r + 5/3 r^2) exp(-sqrt(5) r)            k(x, x) = sigma_f^2 for both
 * They are CGP_F64 kernels: every entry point of a CGP_F32 context returns CGP_EINVAL for them before anything is enqueued (the
 * context stays usable).  In fp64 contexts every entry point takes them, the sliding windows included.  The one-launch
 * short-window kernels (below) hold the squared-exponential and Brownian forms only: a Matern call of ANY length runs the tiled
 * schedules, and its optimisation the host L-BFGS over device gradients -- the route windows of more than 160 samples take. */
enum {
  CGP_KERNEL_SE_ISO = 0, CGP_KERNEL_SE_ARD = 1, CGP_KERNEL_RBF_BROWNIAN = 2, CGP_KERNEL_MATERN32_ARD = 3,
  CGP_KERNEL_MATERN52_ARD = 4
};
enum { CGP_F64 = 0, CGP_F32 = 1 };
enum {
  CGP_OK = 0, CGP_EINVAL = -1, CGP_ENOMEM = -2, CGP_EHIP = -3, CGP_ESTATE = -4, CGP_ENODEVICE = -5,
  CGP_ECAPACITY = -6
};
#define CGP_MAX_D 8
#define CGP_MAX_THETA (CGP_MAX_D + 2)
/* `hip_stream` arguments take a hipStream_t.  NULL is the legacy default stream itself (the value
 * torch.cuda.current_stream().cuda_stream has for the default stream): the enqueued work is ordered
 * after the caller's earlier default-stream work (e.g. the kernels that produced dX) and before its
 * later work.  CGP_STREAM_CTX selects the context's private non-blocking stream; the caller then
 * orders it against its own streams with events or cgp_synchronize. */
#define CGP_STREAM_CTX ((void *)(size_t)-1)

/* ---- lifetime ------------------------------------------------------------------------------- */
/* Allocates every device buffer for up to `max_batch` simultaneous fits of at most max_n training
 * points, max_m test points, max_d input dimensions.  dtype = CGP_F64 | CGP_F32 is the arithmetic
 * type of the device path; host buffers are always fp64 (the messages are float64[]).
 * CGP_F64 is the reference's arithmetic and meets 1e-6 against it on every kernel.  CGP_F32 is for the SE kernels on
 * standardised inputs (BASELINE configs[2], 1e-3).  Its contract, checked by tests/fuzz/fuzz_parity.py (one bar, no second class):
 *   - predictive mean: refined against a double-precision residual (cgp_set_refine below; by default every window of d <= 3
 *     input dimensions and, beyond, every fit whose factor shows a dense window) -- 5e-5 of the oracle or better where it is
 *     refined (typically 1e-6), 1e-3 where it is not;
 *   - variance and logML come from the single-precision factor: max(1e-3, 10 x the error of spotrf / strtrs on the same
 *     window) -- the second term only matters for windows that are ill-conditioned in single precision (dense
 *     one-dimensional inputs), where no single-precision factorisation holds 1e-3;
 *   - the reference's RBF x Brownian kernel on raw tick counts (cond(Ky) ~ 1e6, prior variance 1000 x the posterior one) is an
 *     fp64 path, as in the reference: in CGP_F32 its mean is refined like any d = 1 window, its variance is held to
 *     max(3e-3, 30 x that LAPACK error) only (its banded factor meets the bf16 matrix cores' truncating sums: a bias of
 *     +1.6e-3 +- 5e-4 at a thousand samples, one sweep window at 3.29e-3).  Use CGP_F64 for that kernel.
 *   - the Matern kernels are not part of the fp32 contract at all: CGP_EINVAL from every entry point (see the kernel ids above).
 * Returns NULL on failure (device index out of range, device is not gfx950 -- the architecture name
 * is checked: the code object holds gfx950 kernels only -- or out of memory): no CPU fallback. */
cgp_ctx *cgp_create(int device, int max_n, int max_m, int max_d, int max_batch, int dtype);
/* The same, telling WHY it failed: *status (may be NULL) = CGP_OK, CGP_EINVAL (an argument out of range), CGP_ENODEVICE
 * (device index out of range or not a gfx950 part), CGP_ENOMEM (a device allocation failed: the context is sized by
 * max_batch x max_n^2) or CGP_EHIP (any other runtime failure). */
cgp_ctx *cgp_create_ex(int device, int max_n, int max_m, int max_d, int max_batch, int dtype, int *status);
void cgp_destroy(cgp_ctx *ctx);
const char *cgp_strerror(int code);
/* Text of the last HIP error seen by this context ("" if none). */
const char *cgp_last_error(const cgp_ctx *ctx);
/* ABI revision of the library that is loaded; compare with CGP_ABI_VERSION of the header a client was built
 * against.  2: cgp_debug_read writes CGP_DEBUG_SLOTS = 512 slots (version 1: 64), and a NULL `hip_stream` is the legacy
 * default stream (version 1: the context's private stream, now CGP_STREAM_CTX).  3 (this header): cgp_set_streams accepts 0
 * (the engine decides; the default, was one group) and cgp_create_ex, cgp_lbfgs_minimize, cgp_sweep_fit_predict_device,
 * cgp_sweep_synchronize, cgp_sweep_context, cgp_set_refine exist; fp32 windows of d <= 3 get a refined mean by default.
 * Revision 3 libraries built after the sliding-window forecast was added also export cgp_window_predict and
 * cgp_window_predict_device (symbols added only: no signature, struct or default moved); probe with dlsym.  The same holds
 * for cgp_window_set_theta, cgp_window_set_theta_device, cgp_window_nll_grad, cgp_window_nll_grad_device and
 * cgp_window_optimize (hyper-parameters of the resident windows replaced / re-estimated in place): revision 3, symbols added only;
 * and for cgp_window_joint_reserve, cgp_window_predict_cov, cgp_window_predict_cov_device, cgp_window_sample and
 * cgp_window_sample_device (the joint forecast: full posterior covariance and sample paths).  Revision 3 libraries built after the
 * Matern kernels were added accept CGP_KERNEL_MATERN32_ARD and CGP_KERNEL_MATERN52_ARD in fp64 contexts (values added only: an
 * earlier library answers CGP_EINVAL for them; probe with cgp_fit on a two-sample window).  cgp_window_predict_gradients and
 * cgp_window_predict_gradients_device (predictive gradients from the resident windows): revision 3, symbols added only.
 * cgp_window_multi_reserve, cgp_window_push_multi, cgp_window_push_multi_device, cgp_window_predict_multi and
 * cgp_window_predict_multi_device (multi-target sliding windows): revision 3, symbols added only.  The same holds for
 * cgp_window_multi_grad_reserve, cgp_window_multi_nll_grad, cgp_window_multi_nll_grad_device and cgp_window_optimize_multi (the
 * multi-target windows' summed objective and its optimiser), and for cgp_window_loo_grad_reserve, cgp_window_loo_nll_grad,
 * cgp_window_loo_nll_grad_device and cgp_window_optimize_loo (the windows' leave-one-out objective and its optimiser). */
#define CGP_ABI_VERSION 3
int cgp_abi_version(void);
/* How the library was built: 0 for the shipped library.  CGP_BUILD_ABLATION (-DCGP_ABLATION): env
 * CGP_DBG is read and can skip parts of the arithmetic for timing ablations -- outputs are WRONG by
 * design, bench.py refuses to report such a build as a measurement.  CGP_BUILD_AB (-DCGP_AB): the
 * alternative schedules of DESIGN.md section 13 are compiled in and selectable by environment.
 * CGP_BUILD_F32_NATIVE (-DCGP_F32_BF16X6=0): the fp32 tile loops use the fp32-input MFMA instead of the shipped form (every
 * fp32 product as six bf16 products on the bf16 matrix cores, same fp32 rounding level: DESIGN.md section 4). */
enum { CGP_BUILD_ABLATION = 1, CGP_BUILD_AB = 2, CGP_BUILD_F32_NATIVE = 4 };
int cgp_build_flags(void);
/* Blocks until everything enqueued on the context's private stream has finished. */
int cgp_synchronize(cgp_ctx *ctx);

/* ---- single window, host buffers -------------------------------------------------------------
 * cgp_fit replaces `GPy.models.GPRegression(x_train, y_train, kernel)` + the exact-inference pass
 * inside it (gp_slip_node.py:35; Gram build, +(sigma_n^2 + 1e-8) I, jitchol, dpotrs, log marginal
 * likelihood) at the fixed hyper-parameters `theta`.  X is (N, d) row-major, y is (N).
 * logml may be NULL. */
int cgp_fit(cgp_ctx *ctx, const double *X, const double *y, int N, int d, int kernel_id,
            const double *theta, double *logml);
/* cgp_predict replaces the `m.predict(np.array([[x]]))` loop (gp_slip_node.py:45-49) for all M
 * test points at once.  Xs is (M, d) row-major.  var is the latent variance clipped at 1e-15 and,
 * when include_noise != 0, plus sigma_n^2 (GPy predict(include_likelihood=True)).  Needs a prior
 * successful cgp_fit on this context. */
int cgp_predict(cgp_ctx *ctx, const double *Xs, int M, int include_noise, double *mean, double *var);
/* alpha = Ky^-1 y of the last fit (GPy `woodbury_vector`, dpotrs).  alpha has N entries. */
int cgp_get_alpha(cgp_ctx *ctx, double *alpha);
/* Lower Cholesky factor of the last fit, (N, N) row-major, upper triangle zero (GPy `LW`). */
int cgp_get_factor(cgp_ctx *ctx, double *L);
/* Jitter that was added to the diagonal for the last fit to succeed (0 if none).  Only a fit that factored reports a jitter:
 * after a fit that returned a positive status (the ladder ran out) this is 0, not the last rung that was tried. */
double cgp_last_jitter(const cgp_ctx *ctx);

/* ---- hyper-parameter optimisation (the reference's `m.optimize()`, gp_slip_node.py:36) ----------
 * cgp_nll_grad: value and gradient of the NEGATIVE log marginal likelihood at theta (natural
 * parameters, same layout as cgp_fit).  GPy's ExactGaussianInference: dL/dK = 0.5 (alpha alpha^T -
 * Ky^-1) contracted with dK/dtheta; Ky^-1 is formed on the device as a syrk of L^-1.  Needs a
 * context created with max_m >= N.  grad has ntheta entries.  Leaves the context fitted at theta. */
int cgp_nll_grad(cgp_ctx *ctx, const double *X, const double *y, int N, int d, int kernel_id,
                 const double *theta, double *nll, double *grad);
/* cgp_optimize: minimises the negative log marginal likelihood over the Logexp-transformed
 * parameters theta = log(1 + exp(x)) (GPy's default positivity constraint) with L-BFGS, starting from
 * theta_inout (GPy starts every parameter at 1.0), at most max_evals objective evaluations (GPy:
 * 1000).  Writes the optimum to theta_inout, its log marginal likelihood to *logml, the number of
 * evaluations to *n_evals, and leaves the context fitted at the optimum (cgp_predict may follow).
 * *n_evals: windows of at most 160 samples (one-launch device optimiser) report the optimiser's own evaluations (what
 * scipy reports as nfev for the same run); longer windows, and Matern windows of any length (host optimiser over device
 * gradients: which form runs is a function of (kernel, N, d, M) only), report those + 1,
 * the refit at the optimum that leaves the factor panel resident.  The optimiser is scipy's L-BFGS-B without bounds
 * (csrc/lbfgs_core.hpp): same line search, same stopping tests, same trajectory to rounding. */
int cgp_optimize(cgp_ctx *ctx, const double *X, const double *y, int N, int d, int kernel_id,
                 double *theta_inout, int max_evals, double *logml, int *n_evals);

/* cgp_optimize_batch: the same optimisation for `batch` windows of identical shape at once.  Every
 * L-BFGS round evaluates value + gradient of ALL windows in one batched device schedule (each window
 * keeps its own line-search / history state on the host); a window whose matrix is not positive
 * definite at a trial point is re-evaluated with GPy's jitter ladder (mean(diag) 1e-6 10^k, k = 0..4,
 * the windows that failed only), exactly as jitchol does inside m.optimize(); a point that still
 * fails is infeasible (+inf) for the line search.
 * X (batch, N, d), y (batch, N), theta_inout (batch, theta_stride); logml / n_evals (batch) may be
 * NULL.  Needs max_batch >= batch and max_m >= N.  Follow with cgp_fit_predict_batch at the optima. */
int cgp_optimize_batch(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *X, const double *y,
                       double *theta_inout, int theta_stride, int max_evals, double *logml, int *n_evals);

/* Host-only self-test of the L-BFGS used by cgp_optimize: minimises the n-dimensional Rosenbrock
 * function from x0 (n <= 16); writes the minimiser, returns the number of evaluations (< 0 on
 * failure).  Lets the optimiser be tested without a GPU. */
int cgp_selftest_lbfgs(double *x_inout, int n, int max_evals, double *f_out);

/* Host-only: the optimiser state machine of cgp_optimize / cgp_optimize_batch (and, lane-parallel, of the one-launch
 * short-window kernel) driven on a caller-supplied objective -- the role scipy.optimize.fmin_l_bfgs_b plays under
 * m.optimize() (gp_slip_node.py:36).  fn(x, grad, n, user) returns f and writes the gradient; a non-finite f marks an
 * infeasible point.  x_inout (n <= 16) holds the start and receives the best point.  pgtol / factr as in scipy (GPy:
 * 1e-5, 1e7).  Returns 0, or CGP_EINVAL; *status: 0 gradient test, 1 function-decrease test, 2 max_evals, 3 line search
 * failed.  Lets tests compare the optimiser with scipy on the oracle's objective without a GPU. */
typedef double (*cgp_objective_fn)(const double *x, double *grad, int n, void *user);
int cgp_lbfgs_minimize(cgp_objective_fn fn, void *user, double *x_inout, int n, int max_evals, double pgtol, double factr,
                       double *f_out, int *n_evals, int *n_iters, int *status);

/* ---- leave-one-out cross-validation from the factor (fp64 contexts) ------------------------------------
 * How well a fitted model explains its own samples, one sample at a time: GPy's inference_method.LOO(kern, X, Y, likelihood,
 * posterior), i.e. Rasmussen & Williams eq. 5.10-5.12, in closed form from what an exact fit already has:
 *     Ky = K + (sigma_n^2 + 1e-8 [+ jitter]) I,   alpha = Ky^-1 y,   kd_i = [Ky^-1]_ii
 *     loo_var_i  = 1 / kd_i                 predictive variance of the NOISY y_i given all other samples
 *     loo_mean_i = y_i - alpha_i / kd_i
 *     loo_lpd_i  = -0.5 log(2 pi loo_var_i) - 0.5 (y_i - loo_mean_i)^2 / loo_var_i
 *     lpd_sum    = sum_i loo_lpd_i          the LOO pseudo-likelihood; higher is better
 * lpd_sum is the second opinion beside logML when kernels are compared; a strongly negative loo_lpd_i marks an outlier sample.
 * The fit is a gradient-mode factorisation (cgp_nll_grad's: needs max_m >= N) on the tiled schedules for EVERY shape -- windows
 * of at most 160 samples included, the one-launch short-window kernel leaves no L^-1 behind -- after which kd is one pass over
 * (L^-1)^T: N^2 / 2 doubles per fit, no syrk.  All five kernel ids.
 * Precision: CGP_F64 contexts only; a CGP_F32 context gets CGP_EINVAL before anything is enqueued and stays usable (alpha_i /
 * kd_i is a cancellation against y_i that single precision does not promise; the joint forecast is fp64-only for the same reason).
 * Shape errors are the gradient calls': CGP_EINVAL / CGP_ECAPACITY as for cgp_nll_grad / cgp_optimize_batch of the same shape.
 * loo_mean, loo_var, loo_lpd and lpd_sum may each be NULL; with all four NULL the call returns CGP_EINVAL.
 * Determinism: a fit's outputs depend on its own data and on the schedule its call size selects, never on its slot or its
 * neighbours; no atomics, lpd_sum is added in a fixed order.
 *
 * cgp_loo: one window, arguments as cgp_nll_grad; loo_mean / loo_var / loo_lpd (N), *lpd_sum.  GPy's jitter ladder as cgp_nll_grad
 * runs it; LOO is computed on the Ky that finally factored, the jitter included in loo_var (cgp_last_jitter reports it).  Returns
 * 0, or the fit's positive status with NaN in every output.  Leaves the context fitted at theta: cgp_predict may follow.
 * Bitwise cgp_loo_batch of that one fit. */
int cgp_loo(cgp_ctx *ctx, const double *X, const double *y, int N, int d, int kernel_id, const double *theta,
            double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum);
/* cgp_loo_batch: `batch` windows of identical shape, host buffers: X (batch, N, d), y (batch, N), theta (batch, theta_stride);
 * loo_mean / loo_var / loo_lpd (batch, N), lpd_sum / logml / info (batch; logml and info may be NULL).  The jitter ladder runs per
 * fit exactly as in cgp_fit_predict_batch (the fits that failed only, one at a time, mean(diag) 1e-6 10^k, k = 0..4).  A fit whose
 * info stays non-zero gets NaN in all of its outputs, lpd_sum included; its neighbours are unaffected.  Returns 0 if every fit
 * succeeded, else the first non-zero per-fit status (the convention of cgp_fit_predict_batch).  Blocks. */
int cgp_loo_batch(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *X, const double *y,
                  const double *theta, int theta_stride,
                  double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum, double *logml, int *info);
/* Device-resident variant, fp64 buffers in cgp_fit_predict_batch_device's layout: dX (batch, d, N), dy (batch, N), dtheta (batch,
 * CGP_MAX_THETA), djitter (batch) or NULL; dloo_mean / dloo_var / dloo_lpd (batch, N), dlpd_sum (batch), each or NULL; dlogml
 * (batch) and dinfo (batch) int32 are required.  The fit schedule and two more launches on hip_stream (NULL = legacy default
 * stream, CGP_STREAM_CTX = the context's own): no allocation, no synchronisation, no ladder -- read dinfo and re-submit the failed
 * fits with djitter set.  A fit with dinfo != 0 gets NaN. */
int cgp_loo_batch_device(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *dX, const double *dy,
                         const double *dtheta, const double *djitter,
                         double *dloo_mean, double *dloo_var, double *dloo_lpd, double *dlpd_sum,
                         double *dlogml, int *dinfo, void *hip_stream);

/* ---- the leave-one-out objective: value, gradient and optimiser (Rasmussen & Williams 5.4.2) -----
 * theta chosen by the second opinion: the objective MINIMISED is nlpd = -lpd_sum, bitwise cgp_loo_batch's lpd_sum negated (for
 * the same number of fits in the call; it comes from the same kernels).  With alpha, kd as above and
 *     c_i = 1/2 (1 / kd_i + alpha_i^2 / kd_i^2)        b_i = alpha_i / kd_i        beta = Ky^-1 b
 *     d lpd_sum / dK = -Ky^-1 diag(c) Ky^-1 + 1/2 (beta alpha^T + alpha beta^T)
 * contracted with dK / dtheta exactly as cgp_nll_grad contracts 1/2 (alpha alpha^T - Ky^-1): the gradient is with respect to the
 * natural parameters, the noise sees dK / dsigma_n^2 = I, the jitter is a constant of the evaluation.
 * Cost per fit: the gradient-mode factorisation (5 N^3 / 6), Ky^-1 materialised once (N^3 / 3) and the symmetric product
 * Ky^-1 diag(c) Ky^-1 on the lower tile pairs (N^3), all on the fp64 matrix cores: about 1.9 x a cgp_nll_grad evaluation, against
 * 2 ntheta evaluations of cgp_loo_batch for central differences.
 * Scratch: cgp_loo_grad_reserve(ctx, max_batch) takes max_batch x (the context's max_n rounded up to 128)^2 doubles (+ four vectors
 * of that length per fit).  1 <= max_batch <= the context's, else CGP_EINVAL; CGP_ENOMEM leaves no reservation and a usable
 * context; calling it again replaces the reservation.  Blocks.  cgp_destroy frees it.
 * Status of the calls below, before anything is enqueued: CGP_F32 context: CGP_EINVAL; no reservation: CGP_ESTATE; batch beyond it:
 * CGP_ECAPACITY; then cgp_loo_batch's shape rules (max_m >= N among them); a NULL required pointer, theta_stride or grad_stride
 * < ntheta, and for the optimiser a theta <= 0: CGP_EINVAL.  A failed call leaves the context usable.  All five kernel ids; every
 * shape takes the tiled schedules, as cgp_loo does.
 * Determinism: run to run bitwise; a fit's nlpd and gradient depend on its own data and on the schedule its call size selects,
 * never on its slot or its neighbours; no atomics; host, device and graph-replay forms are bitwise equal. */
int cgp_loo_grad_reserve(cgp_ctx *ctx, int max_batch);
/* cgp_loo_nll_grad: one window, arguments as cgp_nll_grad; *nlpd and grad (ntheta).  The jitter ladder as cgp_loo runs it.  Returns
 * 0, or the fit's positive status with NaN in both outputs.  Bitwise cgp_loo_nll_grad_batch of that one fit.  Leaves the context
 * fitted at theta: cgp_predict may follow. */
int cgp_loo_nll_grad(cgp_ctx *ctx, const double *X, const double *y, int N, int d, int kernel_id,
                     const double *theta, double *nlpd, double *grad);
/* cgp_loo_nll_grad_batch: host buffers in cgp_loo_batch's layouts; nlpd (batch), grad (batch, grad_stride), logml (batch) or NULL,
 * info (batch) or NULL.  The jitter ladder per fit exactly as cgp_loo_batch runs it.  A fit whose info stays non-zero has NaN in
 * nlpd and in its gradient; its neighbours are unaffected.  Returns a negative error, else 0 or the first non-zero per-fit status.
 * Blocks. */
int cgp_loo_nll_grad_batch(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *X, const double *y,
                           const double *theta, int theta_stride, double *nlpd, double *grad, int grad_stride,
                           double *logml, int *info);
/* Device-resident variant, buffers as cgp_loo_batch_device: dnlpd (batch), dgrad (batch, grad_stride; entries from ntheta on are
 * not written), dlogml (batch) or NULL, dinfo (batch) int32 (required).  cgp_loo_batch_device's launches plus five on hip_stream:
 * no allocation, no synchronisation, no ladder (capturable into a hipGraph) -- read dinfo and re-submit the failed fits with
 * djitter set.  A fit with dinfo != 0 gets NaN. */
int cgp_loo_nll_grad_batch_device(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *dX, const double *dy,
                                  const double *dtheta, const double *djitter, double *dnlpd, double *dgrad, int grad_stride,
                                  double *dlogml, int *dinfo, void *hip_stream);
/* cgp_optimize_loo_batch: cgp_optimize_batch's host L-BFGS (Logexp transform, pgtol 1e-5, factr 1e7, the jitter ladder per trial
 * point, +inf for a point that stays infeasible) over the evaluation above: each fit's theta (batch, theta_stride) is replaced by
 * its optimum.  lpd_sum, logml (batch: both objectives at the returned theta, from one more evaluation that n_evals does not count)
 * and n_evals (batch) may be NULL.  max_evals <= 0: 1000.  Follow it with cgp_fit_predict_batch at the optima.  Blocks. */
int cgp_optimize_loo_batch(cgp_ctx *ctx, int batch, int N, int d, int kernel_id, const double *X, const double *y,
                           double *theta_inout, int theta_stride, int max_evals,
                           double *lpd_sum, double *logml, int *n_evals);

/* ---- the node callback in one call -------------------------------------------------------------
 * Everything gp_slip_node.py:16-63 computes between "GP Input Arrived" and pub.publish(), at fixed
 * theta: first int(0.9 n) samples train (:27-29), grid arange(min, max + 600, 1) (:45), output
 * mean = means[n:], sigma = 2 sqrt(var[n:]) (:59-61).  Writes at most `cap` entries; *m_out gets
 * the number of entries the reference would publish.  cgp_slip_node_callback_opt additionally runs
 * cgp_optimize on the training window first (max_evals <= 0: fixed theta), returning theta. */
int cgp_slip_node_callback_opt(cgp_ctx *ctx, const double *time_array, const double *slip_array, int n,
                               int kernel_id, double *theta_inout, int max_evals, double *mean,
                               double *sigma, int cap, int *m_out);
int cgp_slip_node_callback(cgp_ctx *ctx, const double *time_array, const double *slip_array, int n,
                           int kernel_id, const double *theta, double *mean, double *sigma, int cap,
                           int *m_out);

/* ---- batch of independent windows, host buffers ------------------------------------------------
 * `batch` fits of identical shape (one per Monte-Carlo trajectory / terrain segment).
 * X (batch, N, d), y (batch, N), Xs (batch, M, d), theta (batch, theta_stride) row-major; outputs
 * mean/var (batch, M), logml (batch), info (batch; per-fit status as the return-value convention).
 * Returns 0 if every fit succeeded, else the first non-zero per-fit status.
 * Short fp64 windows (N <= 144 for any d, N <= 160 at d <= 2; M > 0) run as ONE launch with the factor in LDS
 * (csrc/cgp_small.hpp: k_small_predict), the same form the node callbacks take; longer ones on the tiled schedules.  Which
 * form runs depends on (N, d, M) only, never on `batch` or the slot; cgp_fit + cgp_predict of the same window (always the
 * tiled schedules: the factor stays resident for cgp_get_factor) agree with it to rounding, not bitwise. */
int cgp_fit_predict_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                          const double *X, const double *y, const double *Xs, const double *theta,
                          int theta_stride, int include_noise, double *mean, double *var,
                          double *logml, int *info);

/* ---- batch, device-resident buffers (the measured path) ---------------------------------------
 * All pointers are DEVICE pointers in the context's dtype (fp64 or fp32), SoA per fit:
 *   dX (batch, d, N), dy (batch, N), dXs (batch, d, M), dtheta (batch, CGP_MAX_THETA) fp64,
 *   djitter (batch) fp64 or NULL, dmean/dvar (batch, M), dlogml (batch) fp64, dinfo (batch) int32.
 * Work is enqueued on `hip_stream` (see CGP_STREAM_CTX above: NULL = the legacy default stream,
 * CGP_STREAM_CTX = the context's own stream) and the call returns without synchronising.  No jitter retry happens here: read dinfo and re-submit the failed
 * fits with djitter set (cgp_fit_predict_batch does exactly that).
 *
 * Extents of caller buffers -- this call and EVERY `*_device` entry point of this header (the joint, multi-target, leave-one-out,
 * sweep and window forms).  The kernels work in padded shapes (128-row tiles, 16-column panels, M rounded up to 16); the caller's
 * arrays are exactly the shapes stated with each call, and the contract is:
 *   - the alignment of the element type suffices (8 bytes for fp64, 4 for fp32 / int32, 1 for dselect): a slice of a larger
 *     array is a valid argument;
 *   - nothing outside the documented extents is written, the gap columns [ntheta, stride) of a strided array and the entries of
 *     unselected windows included; inputs are never written;
 *   - no output depends on memory outside the documented extents (a padded lane never reads the caller's memory into a result);
 *   - every documented element of every output that is passed is written by every call that returns 0, for every fit / window
 *     whose status word is 0; the rows of a failed fit or window hold NaN where its section promises NaN, its status word is
 *     always written, and what its remaining rows hold (dmean / dvar / dlogml of cgp_fit_predict_batch_device and the sweep, the
 *     ticks of a push on a failed window) is unspecified -- but it stays inside those rows.
 * tests/test_gpu_device_extents.py holds every entry point to it on guard-band allocations. */
int cgp_fit_predict_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                                 const void *dX, const void *dy, const void *dXs, const double *dtheta,
                                 const double *djitter, int include_noise, void *dmean, void *dvar,
                                 double *dlogml, int *dinfo, void *hip_stream);

/* ---- joint forecast after batch / single fits: full posterior covariance and sample paths ----------
 * The calls above answer with the marginals.  The reference's model also offers the JOINT posterior at its test points --
 * m.predict(Xnew, full_cov=True) and m.posterior_samples_f(Xnew, size) -- which a Monte-Carlo trajectory ensemble needs: one
 * realisation of the whole slip curve per member, correlated from tick to tick.  After a tiled fit the factor panel holds
 * V^T = (L^-1 K*)^T beside L, so the covariance is one more pass over resident rows, no second solve:
 *   cov = K(Xs, Xs) - V^T V        N M^2 flops per fit (lower triangle) on the fp64 matrix cores
 * CGP_F64 contexts only: every entry point of this section returns CGP_EINVAL in a CGP_F32 context before anything is enqueued
 * (a covariance formed by cancellation in single precision is not something to promise).  All five kernel ids.  Every shape
 * takes the tiled schedules here (the one-launch short-window kernel leaves no V^T behind), so for N <= 144 / 160 mean and
 * diag(cov) agree with cgp_fit_predict_batch to rounding; beyond, they are bitwise its mean / var: among the tiled schedules a
 * joint call takes the one the marginal call of its size takes, and adds launches after it.  A fit's covariance and paths are a
 * function of its own data and of that schedule only: never of its slot or its neighbours, and of the size of the call exactly as
 * far as mean / var are -- bitwise the same among the mid-size and fused schedules (a lone fit of N > 2560 up to 511 fits), to
 * rounding (1e-9) against a call small enough for the latency schedule, which sums a tile's inner dimension in ranges.
 *
 * cgp_joint_reserve: scratch for the posterior covariance / its factor of up to max_batch fits at up to max_m test points:
 * max_batch x mpad^2 doubles, mpad = max_m rounded up to 16 (512 x 599: 1.5 GB -- the caller decides).  1 <= max_batch <= the
 * context's, 1 <= max_m <= min(the context's max_m, 1024), else CGP_EINVAL; CGP_ENOMEM leaves no reservation; calling it again
 * replaces the reservation.  Blocks (it synchronises the device).  Without a reservation the calls below return CGP_ESTATE, for
 * a batch or an M beyond it CGP_ECAPACITY; M < 1 and NULL pointers are CGP_EINVAL. */
int cgp_joint_reserve(cgp_ctx *ctx, int max_batch, int max_m);
/* cgp_fit_predict_cov_batch: arguments, status words, jitter ladder and return value as cgp_fit_predict_batch, with
 * cov (batch, M, M) row-major in place of var.  Both triangles are written and exactly equal.  mean and diag(cov) are the fit's
 * own mean / var: the diagonal is clipped at 1e-15 and include_noise != 0 adds sigma_n^2 to the DIAGONAL only (GPy's
 * predict(full_cov=True, include_likelihood=True)).  A fit whose info stays non-zero has NaN in all of its covariance; the
 * other fits of the call are unaffected.  Blocks. */
int cgp_fit_predict_cov_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                              const double *X, const double *y, const double *Xs, const double *theta,
                              int theta_stride, int include_noise, double *mean, double *cov,
                              double *logml, int *info);
/* Device-resident variant: pointers as cgp_fit_predict_batch_device (fp64), dcov (batch, M, M) in place of dvar (the variance
 * stays in the context).  The fit schedule plus one launch, enqueued on hip_stream; no allocation, no synchronisation, no
 * jitter ladder (capturable into a hipGraph).  A fit with dinfo != 0 has NaN in all of its covariance. */
int cgp_fit_predict_cov_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                                     const double *dX, const double *dy, const double *dXs, const double *dtheta,
                                     const double *djitter, int include_noise, double *dmean, double *dcov,
                                     double *dlogml, int *dinfo, void *hip_stream);
/* cgp_fit_sample_batch: the fits of cgp_fit_predict_cov_batch and S sample paths of each, out (batch, S, M) = mean + C xi,
 * where C is the lower Cholesky factor of
 *   A = cov_latent (+ sigma_n^2 I when include_noise)  +  jitter_rel * mean(diag(cov_latent (+ sigma_n^2 I))) * I
 * and xi (batch, S, M) are standard normals SUPPLIED BY THE CALLER: the library holds no random state.  Definition, argument
 * rules and failure rule are cgp_window_sample's: jitter_rel >= 0 (pass 1e-6 unless you know better), no ladder on THIS
 * factorisation -- a fit whose A is not positive definite gets NaN paths and sinfo[b] = the 1-based failing pivot (a fit whose
 * info != 0 reports pivot 1); the fits themselves run the jitter ladder as cgp_fit_predict_batch does.  logml, info, sinfo may be
 * NULL.  The dense covariance is never written to the caller.  Returns a negative error, else 0 or the 1-based index of the
 * first fit whose paths are NaN.  Blocks. */
int cgp_fit_sample_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                         const double *X, const double *y, const double *Xs, const double *theta,
                         int theta_stride, int include_noise, int S, const double *xi, double jitter_rel,
                         double *out, double *logml, int *info, int *sinfo);
/* Device-resident variant: the fit schedule plus three launches on hip_stream, no allocation, no synchronisation (capturable
 * into a hipGraph); dxi / dout (batch, S, M), dsinfo (batch ints) may be NULL.  Mean and variance stay in the context. */
int cgp_fit_sample_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                                const double *dX, const double *dy, const double *dXs, const double *dtheta,
                                const double *djitter, int include_noise, int S, const double *dxi, double jitter_rel,
                                double *dout, double *dlogml, int *dinfo, int *dsinfo, void *hip_stream);
/* After cgp_fit / cgp_optimize, the literal m.predict(Xs, full_cov=True) and m.posterior_samples_f(Xs, S): Xs (M, d),
 * mean (M), cov (M, M), xi / out (S, M); mean and diag(cov) are bitwise cgp_predict's.  The resident fit is not modified.
 * cgp_sample returns 0 or 1 (info: the failing pivot, may be NULL); CGP_ESTATE also without a successful fit.  Block. */
int cgp_predict_cov(cgp_ctx *ctx, const double *Xs, int M, int include_noise, double *mean, double *cov);
int cgp_sample(cgp_ctx *ctx, const double *Xs, int M, int S, const double *xi, int include_noise, double jitter_rel,
               double *out, int *info);

/* ---- predictive gradients after batch / single fits: d mean / d x*, d var / d x* ----------------------
 * The reference's model also offers m.predictive_gradients(Xnew): the derivative of the predictive mean and of the predictive
 * variance with respect to the test inputs -- for the d = 1 slip series the slip rate and the rate at which the confidence band
 * opens along the horizon, for the multi-input windows the sensitivity of predicted slip to each input.  With
 * Ky = K(X, X) + (sigma_n^2 + 1e-8 + jitter) I = L L^T, alpha = Ky^-1 y and B = Ky^-1 K(X, Xs) (N x M):
 *   dmean[m][q] =                     sum_i dk(x*_m, x_i)/dx*_q alpha_i
 *   dvar [m][q] = dk(x*_m, x*_m)/dx*_q - 2 sum_i dk(x*_m, x_i)/dx*_q B[i][m]
 * dmean / dvar are (batch, M, d) row-major.  include_noise adds a constant and does not enter; neither does the variance's clip
 * at 1e-15: the gradient is that of the unclipped expression.  Kernel derivatives, r^2 = sum_q ((x*_q - x_iq) / ell_q)^2 and
 * g = -2 dk/dr^2: ids 0 / 1 / 3 / 4 have dk/dx*_q = g (x_iq - x*_q) / ell_q^2 with g = k (squared exponentials),
 * 3 sigma_f^2 e^-s (Matern 3/2), (5/3) sigma_f^2 (1 + s) e^-s (Matern 5/2) -- finite at r = 0, no quotient by r -- and
 * d k(x*, x*) / dx* = 0.  Id 2 (RBF x Brownian, d = 1), R = sigma_r^2 exp(-(x* - x_i)^2 / 2 ell^2), W = sigma_b^2 min(|x*|, |x_i|) for
 * equal signs, else 0:
 *   dk/dx* = R W (x_i - x*) / ell^2 + R sigma_b^2 sign(x*) [|x*| < |x_i| and equal signs],   d k(x*, x*) / dx* = sigma_r^2 sigma_b^2 sign(x*)
 * with sign(0) = 0 and the bracket 0 at a tie |x*| = |x_i| (test points on the tick grid inside a window hit one).
 * After a tiled fit the factor panel holds V^T = (L^-1 K*)^T and z^T = (L^-1 y)^T beside L; B^T and alpha are ONE backward
 * triangular solve with M + 1 right-hand sides against the tiled factor, N^2 (M + 1) flops per fit on the fp64 matrix cores, and
 * the two sums one pass of N M evaluations of g.  CGP_F64 contexts only: every entry point of this section returns CGP_EINVAL in
 * a CGP_F32 context before anything is enqueued.  All five kernel ids.  Every shape takes the tiled schedules here (the one-launch
 * short-window kernel leaves no V^T behind), and among them the one the marginal call of its size takes: for N > 160
 * mean / var / logml / info are bitwise cgp_fit_predict_batch[_device]'s.  A fit's gradients are a function of its own data and
 * of that schedule only, never of its slot or its neighbours.
 *
 * cgp_pgrad_reserve: scratch for B^T and alpha of up to max_batch fits at up to max_m test points, one slab per fit in the
 * factor panel's layout: max_batch x (the context's max_n rounded up to 128) x (max_m + 1 rounded up to 128) doubles (N = 2048,
 * M = 599: 10.5 MB per fit, 5.4 GB for 512 fits -- the caller decides).  1 <= max_batch <= the context's, 1 <= max_m <= the
 * context's max_m, else CGP_EINVAL; CGP_ENOMEM leaves no reservation; calling it again replaces the reservation.  Blocks (it
 * synchronises the device).  Without a reservation the calls below return CGP_ESTATE, for a batch or an M beyond it
 * CGP_ECAPACITY; M < 1 and NULL pointers are CGP_EINVAL. */
int cgp_pgrad_reserve(cgp_ctx *ctx, int max_batch, int max_m);
/* cgp_fit_predict_grad_batch: arguments, status words, jitter ladder and return value as cgp_fit_predict_batch, plus
 * dmean / dvar (batch, M, d); either may be NULL, not both.  A fit whose info stays non-zero has NaN in all of its gradients;
 * the other fits of the call are unaffected.  A fit the ladder repaired has the gradients of its final jitter.  Blocks. */
int cgp_fit_predict_grad_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                               const double *X, const double *y, const double *Xs, const double *theta,
                               int theta_stride, int include_noise, double *mean, double *var,
                               double *logml, int *info, double *dmean, double *dvar);
/* Device-resident variant: pointers as cgp_fit_predict_batch_device (fp64), plus ddmean / ddvar (batch, M, d), either may be
 * NULL, not both.  The fit schedule plus two launches, enqueued on hip_stream; no allocation, no synchronisation, no jitter
 * ladder (capturable into a hipGraph).  A fit with dinfo != 0 has NaN in all of its gradients. */
int cgp_fit_predict_grad_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int kernel_id,
                                      const double *dX, const double *dy, const double *dXs, const double *dtheta,
                                      const double *djitter, int include_noise, double *dmean, double *dvar,
                                      double *dlogml, int *dinfo, double *ddmean, double *ddvar, void *hip_stream);
/* After cgp_fit / cgp_optimize, the literal m.predictive_gradients(Xs): Xs (M, d), dmean / dvar (M, d), either may be NULL, not
 * both; mean / var (M), each may be NULL, are bitwise cgp_predict's with include_noise = 0.  The extra rows are computed against
 * the resident factor as cgp_predict does; the resident fit is not modified.  CGP_ESTATE also without a successful fit.  Blocks. */
int cgp_predict_gradients(cgp_ctx *ctx, const double *Xs, int M, double *mean, double *var, double *dmean, double *dvar);

/* ---- multi-target fits: P target columns share one factor ------------------------------------------
 * The model the engine restates is GPy.models.GPRegression(X, Y, kernel) with Y (N, P): P independent outputs that share the
 * inputs, the kernel and the hyper-parameters -- a Monte-Carlo ensemble on a common tick grid, the four wheels' slip series on one
 * time base.  There is ONE factorisation, ONE predictive variance and one log marginal likelihood term per column.  Per fit, with
 * Ky = K + (sigma_n^2 + 1e-8 [+ jitter]) I = L L^T:
 *   Z = L^-1 Y  (N x P)          V = L^-1 K(X, Xs)
 *   mean[p, m] = sum_i V[i, m] Z[i, p]
 *   var[m]     = max(k(xs_m, xs_m) - sum_i V[i, m]^2, 1e-15) (+ sigma_n^2 when include_noise)      the fit's own variance
 *   logml[p]   = -1/2 sum_i Z[i, p]^2 - sum_i log L_ii - N/2 log 2 pi
 * sum_i log L_ii is read from the factor's diagonal in a fixed order (not recovered from the fit's own logML by subtraction);
 * sum_p logml[p] is GPy's objective -P/2 log|Ky| - 1/2 tr(Y^T Ky^-1 Y) - N P / 2 log 2 pi.  Against P separate fits the call runs
 * the fit once and adds N^2 P flops for Z and 2 N M P for the means, on the fp64 matrix cores, from what a tiled fit leaves
 * resident (L, the images of L(k,k)^-1, V^T).  CGP_F64 contexts only: every entry point of this section returns CGP_EINVAL in a
 * CGP_F32 context before anything is enqueued, and the context stays usable.  All five kernel ids.  Every shape takes the tiled
 * schedules (the one-launch short-window kernel leaves no factor behind); among them a call takes the one cgp_fit_predict_batch
 * takes for its number of fits.
 *
 * Layouts.  Host: X (batch, N, d), Y (batch, P, N) -- each target of a fit contiguous over its N samples -- Xs (batch, M, d),
 * theta (batch, theta_stride).  Outputs: mean (batch, P, M), var (batch, M) (shared by the P targets of a fit), logml (batch, P),
 * info (batch).  Device variant: dX / dXs / dtheta / djitter as cgp_fit_predict_batch_device (SoA (batch, d, N) / (batch, d, M),
 * (batch, CGP_MAX_THETA), (batch) or NULL), dY (batch, P, N), outputs as above.
 *
 * Determinism.  A column's mean row and logml are a function of its own data and of the schedule the call's number of fits
 * selects: never of its position p, of P, of the other columns, of the fit's slot or of neighbouring fits.  Permuting the columns
 * of Y permutes mean and logml bitwise; the first columns of a wide call are bitwise the same columns run alone.  No atomics; every
 * sum runs in a fixed order over the REAL N samples (padding is not summed).  var is bitwise what cgp_fit_predict_cov_batch
 * reports as diag(cov) for the same fit in a call of the same number of fits: the unchanged schedule's own variance.  Between two
 * schedules (a call small enough for the latency schedule against a larger one) results agree to rounding, 1e-9.
 *
 * cgp_multi_reserve: scratch for Z of up to max_batch fits with up to max_p targets: max_batch x (the context's max_n rounded up
 * to 128) x (max_p rounded up to 128) doubles.  1 <= max_batch <= the context's, 1 <= max_p <= 4096, else CGP_EINVAL; CGP_ENOMEM
 * leaves no reservation; calling it again replaces the reservation.  Blocks (it synchronises the device).  cgp_destroy frees it.
 *
 * Status of the two calls: without a reservation CGP_ESTATE; a batch or a P beyond it CGP_ECAPACITY; P < 1, M < 1, a NULL
 * required pointer or theta_stride < ntheta CGP_EINVAL; shape errors otherwise as cgp_fit_predict_batch (CGP_EINVAL /
 * CGP_ECAPACITY).  A fit whose info stays non-zero has NaN in all P of its means, in its var and in its P logml entries; its
 * neighbours are unaffected.
 *
 * Cost.  The solve is one launch with one workgroup per (fit, 64 or 128 targets) that walks all of N itself (about N^2 flops per
 * target at one SIMD's rate), so its length does not shrink with P: 1.2 ms at N = 2048 whether P is 1 or 512.  Below P ~ 16 on
 * a lone fit of N = 2048, M = 599, replicating X through cgp_fit_predict_batch_device is as fast or faster (measured: P = 8 0.79 x,
 * P = 16 1.23 x, P = 512 17 x the replicate route; 64 fits x P = 8: 5.2 x; DESIGN.md section 9d has the table).
 *
 * Not provided: multi-target leave-one-out or joint covariance, and a cgp_sweep_* form.  (The hyper-parameters of a
 * multi-target model: the next section; multi-target sliding windows: the section after cgp_window_predict_gradients.) */
int cgp_multi_reserve(cgp_ctx *ctx, int max_batch, int max_p);
/* cgp_fit_predict_multi_batch: blocks; GPy's jitter ladder per fit exactly as cgp_fit_predict_batch runs it (a failed fit is
 * retried as a call of one fit; its targets are solved and contracted right after its retry, the whole batch's before the first
 * retry).  logml and info may be NULL.  Returns a negative error, else 0 or the first non-zero per-fit status. */
int cgp_fit_predict_multi_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int kernel_id,
                                const double *X, const double *Y, const double *Xs, const double *theta,
                                int theta_stride, int include_noise, double *mean, double *var, double *logml,
                                int *info);
/* Device-resident variant: the fit schedule plus four launches on hip_stream; no allocation, no synchronisation, no jitter
 * ladder (capturable into a hipGraph).  dlogml and dinfo are required.  The underlying fit runs on each fit's column 0, gathered
 * into a buffer of the context; its own mean / logML are by-products and are not returned. */
int cgp_fit_predict_multi_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int kernel_id,
                                       const double *dX, const double *dY, const double *dXs, const double *dtheta,
                                       const double *djitter, int include_noise, double *dmean, double *dvar,
                                       double *dlogml, int *dinfo, void *hip_stream);
/* Test hook: rows = 64 / 128 forces the tile height of the solve launch, 0 gives the choice back to the engine (it picks from
 * (batch, P) only).  The two forms agree bitwise per element; anything else is CGP_EINVAL. */
int cgp_multi_set_form(cgp_ctx *ctx, int rows);

/* ---- explicit basis functions (a trend) after the multi-target fits ----------------------------------------
 * Every model above has a zero prior mean: a forecast a few length-scales past the last sample returns to 0.  This section fits
 * f(x) = g(x) + h(x)^T beta, g the zero-mean GP and beta the coefficients of q basis functions the CALLER evaluates (a constant, a
 * linear term, a commanded-speed regressor), integrated out under a vague prior (Rasmussen & Williams 2.7, eqs. 2.41, 2.42, 2.45).
 * Per fit, with Ky = K + (sigma_n^2 + 1e-8 [+ jitter]) I = L L^T, Y (N x P) the targets, H (N x q) the basis at the samples, Hs
 * (M x q) the basis at the test points:
 *   Z = L^-1 Y        G = L^-1 H        V = L^-1 K(X, Xs)
 *   A = G^T G (q x q) = L_A L_A^T      B = G^T Z (q x P)      beta[:, p] = A^-1 B[:, p]
 *   R = Hs^T - G^T V   (q x M)
 *   mean[p, m] = sum_i V[i, m] Z[i, p] + sum_r R[r, m] beta[r, p]
 *   var[m]     = max(k(xs_m, xs_m) - sum_i V[i, m]^2, 1e-15) (+ sigma_n^2 when include_noise) + |L_A^-1 R[:, m]|^2
 *   logml[p]   = -1/2 sum_i Z[i, p]^2 + 1/2 B[:, p]^T beta[:, p] - sum_i log L_ii - sum_r log (L_A)_rr - (N - q)/2 log 2 pi
 * The first term of var (with its noise term) is the fit's own variance, by the same code and to the same bits as
 * cgp_fit_predict_multi_batch's var; the last term is the price of not knowing beta and is >= 0.
 *
 * Rank rule.  A is factored by an unpivoted Cholesky in index order.  Pivot r fails when it is not > 1e-10 A[r][r], A[r][r] the
 * entry before elimination; NaN and negative pivots fail the same test.  Then tinfo of that fit takes the 1-based r, all of its
 * trend outputs (mean, var, beta, logml) are NaN and its neighbours are untouched.  q <= N is not required: the rule answers.  A fit
 * whose own info is non-zero has NaN outputs and tinfo = 0.
 *
 * How it runs.  [Y | H] are packed as P + q columns of the multi-target machinery (column 0 = target 0, so the fit schedule sees
 * what it sees in cgp_fit_predict_multi_batch): L^-1 H and G^T V come out of the multi-target solve and contraction on q more
 * columns.  Three more launches follow: S = G^T [Z | G] on the fp64 matrix cores, the q x q factorisation with beta and the
 * evidence terms (one wave per fit), and the correction of mean and var.  CGP_F64 contexts only: CGP_EINVAL in a CGP_F32 context
 * before anything is enqueued.  All five kernel ids.
 *
 * Layouts.  X, Y, Xs, theta, mean, var, logml, info as in the multi-target section; H (batch, q, N) and Hs (batch, q, M), laid out
 * like Y (each basis function contiguous over the samples / the test points); beta (batch, P, q); tinfo (batch).  Device variant:
 * dX / dXs / dtheta / djitter as cgp_fit_predict_batch_device.
 *
 * Determinism.  A column's mean row, beta row and logml are a function of its own data, of the basis and of the schedule the
 * call's number of fits selects: never of p, P, the other target columns, the fit's slot or the neighbours.  Permuting the target
 * columns permutes mean, beta and logml bitwise; the first columns of a wide call are bitwise the same columns run alone.  No
 * atomics; every sum runs in a fixed order over the REAL N samples.  Host form, device form and a replayed graph agree bitwise.  A
 * trend call leaves a following multi-target call bitwise what it is without it.  Between two schedules results agree to 1e-9.
 *
 * cgp_trend_reserve: scratch for the contraction and the evidence of the packed columns, S and L_A^-1: about max_batch x (max_p +
 * 16) x (max_m + 17) doubles.  It needs a cgp_multi_reserve that covers (max_batch, max_p + CGP_MAX_TREND), else CGP_ESTATE.  1 <=
 * max_batch <= the context's, 1 <= max_p <= 4096 - 16, 1 <= max_m <= the context's, else CGP_EINVAL; CGP_ENOMEM leaves no
 * reservation; calling it again replaces the reservation.  Blocks.  cgp_destroy frees it.
 *
 * Status of the two calls, in this order: CGP_EINVAL in a CGP_F32 context, for M < 1, P < 1 or q outside 1 .. CGP_MAX_TREND;
 * without a trend reservation CGP_ESTATE; batch, P or M beyond it CGP_ECAPACITY; a multi-target reservation that no longer
 * covers (batch, P + q) CGP_ESTATE / CGP_ECAPACITY; a NULL required pointer or theta_stride < ntheta CGP_EINVAL; shape errors
 * otherwise as cgp_fit_predict_batch.
 *
 * Not provided: theta-gradients and an optimiser of the trend evidence; joint covariance, leave-one-out and predictive gradients
 * with a trend; a single-fit form; fp32 contexts; a cgp_sweep_* form. */
#define CGP_MAX_TREND 16
int cgp_trend_reserve(cgp_ctx *ctx, int max_batch, int max_p, int max_m);
/* cgp_fit_predict_trend_batch: blocks; the jitter ladder per fit exactly as cgp_fit_predict_multi_batch runs it (a retried fit's
 * trend is computed right after its retry, into its own slot).  beta, logml, info and tinfo may be NULL.  Returns a negative
 * error, else 0 or the first non-zero per-fit info (a failed rank rule is reported in tinfo only). */
int cgp_fit_predict_trend_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int q, int kernel_id,
                                const double *X, const double *Y, const double *H, const double *Xs, const double *Hs,
                                const double *theta, int theta_stride, int include_noise,
                                double *mean, double *var, double *beta, double *logml, int *info, int *tinfo);
/* Device-resident variant: cgp_fit_predict_multi_batch_device's launches (with a pack of its own) plus three; no allocation, no
 * synchronisation, no jitter ladder (capturable into a hipGraph).  Every output pointer is required.  The extent contract at
 * cgp_fit_predict_batch_device applies. */
int cgp_fit_predict_trend_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int q, int kernel_id,
                                       const double *dX, const double *dY, const double *dH, const double *dXs,
                                       const double *dHs, const double *dtheta, const double *djitter, int include_noise,
                                       double *dmean, double *dvar, double *dbeta, double *dlogml, int *dinfo, int *dtinfo,
                                       void *hip_stream);

/* ---- sparse (inducing-point) fits: the collapsed variational bound and its forecast ---------------------------
 * Every fit above is a dense Cholesky of an N x N Gram matrix, sized by the context's max_n.  This section is the model of the family
 * that is not: GPy.models.SparseGPRegression -- m inducing inputs Z, the collapsed variational bound of Titsias (2009), GPy's
 * VarDTC -- at N m^2 + m^3 flops with no N x N object anywhere, so a whole recorded history can be fed instead of a window.  N is
 * bounded by the sparse reservation alone, NOT by the context's max_n.  Per fit, with X (N x d), y (N), Z (m x d), Xs (M x d):
 *   sigma2 = sigma_n^2 + 1e-8 (the dense path's diagonal)            eps = 1e-8 + the fit's jitter
 *   K_uu = K(Z, Z) + eps I = L_u L_u^T
 *   Phi = K_uf K_fu (m x m)      b = K_uf y (m)      yty = y^T y      t = sum_i k(x_i, x_i)   (RBF x Brownian: k(x, x) = s_r^2 s_b^2 |x|)
 *   A = L_u^-1 Phi L_u^-T / sigma2      B = I + A = L_B L_B^T      c = L_B^-1 L_u^-1 b / sigma2
 *   logml = -N/2 log 2 pi - N/2 log sigma2 - sum log diag(L_B) - yty / (2 sigma2) + c^T c / 2 - t / (2 sigma2) + tr(A) / 2
 *   V1 = L_u^-1 K(Z, Xs)      V2 = L_B^-1 V1
 *   mean = V2^T c      var = max(k(xs, xs) - colsum(V1^2) + colsum(V2^2), 1e-15) (+ sigma_n^2 when include_noise)
 * `logml` is the BOUND: it is <= the exact log marginal likelihood of the same data and does not decrease when an inducing input
 * is added.  With Z = X it is the exact fit up to eps (4e-6 relative on the bound at N = 200, sigma_n^2 = 1e-3): not a parity
 * statement.  All five kernel ids (RBF x Brownian needs d = 1); CGP_F64 contexts only.
 *
 * info[b]: 0 the fit succeeded; k in 1 .. m the 1-based failing pivot of K_uu; m + k the failing pivot of B.  A failed fit has NaN
 * in mean, var and logml; its neighbours are untouched.  Non-positive pivots are repaired in flight, so nothing faults.
 *
 * Layouts.  Host form: X (batch, N, d), y (batch, N), Z (batch, m, d) -- every fit has inducing inputs of its own --, Xs (batch, M,
 * d), theta (batch, theta_stride), mean / var (batch, M), logml / info (batch).  Device form: fp64 SoA as
 * cgp_fit_predict_batch_device -- dX (batch, d, N), dy (batch, N), dZ (batch, d, m), dXs (batch, d, M), dtheta (batch,
 * CGP_MAX_THETA), djitter (batch) or NULL.  M = 0 gives the bound only: Xs, mean and var may then be NULL.
 *
 * Determinism.  A fit's outputs are a function of its own data and of (N, m, M, d, kernel) only: bitwise independent of the batch
 * size, the slot and the neighbours.  The sum over N is cut into min(ceil(N / cgp_sparse_chunk()), 16) chunks of equal length
 * (rounded up to 16 samples) whose partial sums are added in chunk order; no floating-point atomics.  Host form (for a fit that
 * needed no ladder step), device form and a replayed graph agree bitwise.
 *
 * cgp_sparse_reserve: ALL the scratch of the sparse calls -- the dense schedules' buffers are not used.  With mt = ceil((max_m_ind
 * + 1) / 16), LD = 16 mt and C = min(ceil(max_n / 512), 16) it allocates
 *   8 max_batch (16 + 128 C mt (mt + 1) + 3 LD^2 + 512 mt + 4 LD + 8) bytes
 * (max_n = 65 536, max_m_ind = 256: 6.9 MB per fit; max_m_ind = 512: 25 MB per fit).  1 <= max_batch <= the context's, 1 <= max_n <=
 * 2^24, 1 <= max_m_ind <= 512, max_m >= 0, else CGP_EINVAL; max_n and max_m are independent of the context's.  CGP_ENOMEM leaves no
 * reservation; calling it again replaces the reservation.  Blocks.  cgp_destroy frees it.
 *
 * Status of the two calls, in this order: CGP_EINVAL in a CGP_F32 context, for batch, N, d or m < 1, m > 512, M < 0, an unknown
 * kernel id or RBF x Brownian with d != 1; without a reservation CGP_ESTATE; batch, N, m or M beyond it, d beyond the context's
 * max_d or batch beyond the context's CGP_ECAPACITY; a NULL required pointer or theta_stride < ntheta CGP_EINVAL.  All of these
 * return before anything is enqueued.  N >= 1 with no relation to m required.
 *
 * cgp_profile_*: the launches of a sparse call are recorded under 0 k_sparse_phi (flops = N (m + 1)(m + 2) per fit), 1
 * k_sparse_algebra, 2 k_sparse_reduce, 3 k_sparse_predict, 4 k_sparse_prep.
 *
 * The gradient of the bound in theta and Z and the optimiser over them are the next section's; several target columns on one fit
 * are the section after it (cgp_fit_predict_sparse_multi_batch), their summed bound's gradient and optimiser the one after that
 * (cgp_sparse_multi_nll_grad_batch).  Not provided: FITC; the resident windows; fp32 contexts; a
 * cgp_sweep_* form. */
int cgp_sparse_reserve(cgp_ctx *ctx, int max_batch, int max_n, int max_m_ind, int max_m);
/* Samples of the shortest chunk of the sum over N (512): the split above, for tests that sit on its edges. */
int cgp_sparse_chunk(void);
/* cgp_fit_predict_sparse_batch: host buffers, blocks.  A fit whose K_uu fails climbs the jitter ladder of cgp_fit_predict_batch
 * (the same function: jitter = 1e-6 10^k of mean(diag K(Z, Z)) + sigma_n^2 + 1e-8, k = 0 .. 4), re-submitted alone into its slot;
 * a failing pivot of B is reported as it is.  logml and info may be NULL.  Returns a negative error, else 0 or the first non-zero
 * per-fit info. */
int cgp_fit_predict_sparse_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int m, int kernel_id,
                                 const double *X, const double *y, const double *Z, const double *Xs, const double *theta,
                                 int theta_stride, int include_noise, double *mean, double *var, double *logml, int *info);
/* Device-resident variant: five launches (four when M = 0) in a linear chain on hip_stream (NULL = legacy default stream,
 * CGP_STREAM_CTX = the context's own); no allocation, no synchronisation, no jitter ladder (capturable into a hipGraph with default
 * settings).  dlogml and dinfo are required.  The extent contract at cgp_fit_predict_batch_device applies. */
int cgp_fit_predict_sparse_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int m, int kernel_id,
                                        const double *dX, const double *dy, const double *dZ, const double *dXs,
                                        const double *dtheta, const double *djitter, int include_noise,
                                        double *dmean, double *dvar, double *dlogml, int *dinfo, void *hip_stream);

/* ---- sparse fits: gradient of the bound in theta and Z, and optimiser ------------------------------------
 * SparseGPRegression(...).optimize() chooses theta AND the inducing inputs Z by maximising the bound above.  With the quantities of
 * the sparse section and F the bound:
 *   chat = L_B^-T c      Q = I - B^-1 - chat chat^T      mu = L_u^-T chat
 *   T = L_u^-T Q L_u^-1 / (2 sigma2) = dF/dPhi      G_uu = 1/2 L_u^-T (Q - A) L_u^-1 = dF/dK_uu      R = 2 T K_uf + mu y^T / sigma2 = dF/dK_uf
 *   dF/dtheta_p  = sum_rs G_uu[r,s] dk(z_r,z_s)/dtheta_p + sum_ri R[r,i] dk(z_r,x_i)/dtheta_p - sum_i dk(x_i,x_i)/dtheta_p / (2 sigma2)
 *   dF/dsigma_n2 = (-N + (yty + t) / sigma2 - tr A + m - tr B^-1 - c^T c - chat^T chat) / (2 sigma2)
 *   dF/dz_rq     = sum_i R[r,i] dk(z_r,x_i)/dz_rq + 2 sum_{s != r} G_uu[r,s] dk(z_r,z_s)/dz_rq + G_uu[r,r] dk(z_r,z_r)/dz_rq
 * eps (the 1e-8 and any jitter) is a constant of the evaluation, as in every other gradient call.  RBF x Brownian: the derivative of
 * min(|z|, |x|) in z is taken for |z| < |x| only (the tie convention of the predictive gradients), and d k(z, z) / dz = s_r^2 s_b^2
 * sign z.  Outputs: nll = -F, grad = d nll / d theta in natural parameters (cgp_nll_grad's order), gradZ = d nll / d Z.  The cost
 * on top of the forward chain is a second pass over N of the same N m^2 size (R is never stored) and six m x m block solves.
 *
 * Promises.  nll is bitwise -logml of cgp_fit_predict_sparse_batch_device on the same inputs, for any M: the same launches produce
 * it.  A fit's outputs are a function of its own data and of (N, m, d, kernel, whether gradZ was asked) only: bitwise independent of
 * the batch size, the slot and the neighbours; no floating-point atomics, every sum in a fixed order.  Host form (for a fit that
 * needed no ladder step), device form and a replayed graph agree bitwise.  grad is bitwise the same whether or not gradZ is asked.
 * A gradient call leaves a following cgp_fit_predict_sparse_batch bitwise what it is without it.  info is the sparse section's; a
 * fit whose info is not 0 has NaN in nll, grad and gradZ, and its neighbours are untouched.
 *
 * cgp_sparse_grad_reserve: needs a cgp_sparse_reserve that covers it (max_batch within it), else CGP_ESTATE, and is sized by that
 * reservation's max_n and max_m_ind as they stand at the call: with mt = ceil((max_m_ind + 1) / 16), LD = 16 mt, mr =
 * ceil(max_m_ind / 16) and C = min(ceil(max_n / 512), 16) it allocates
 *   8 max_batch (3 LD^2 + 12 C mr + 8 C LD + 12 mr + 8 LD + 5) bytes
 * (max_n = 65 536, max_m_ind = 512: 7.3 MB per fit).  1 <= max_batch <= the context's, else CGP_EINVAL; CGP_ENOMEM leaves no reservation; calling
 * it again replaces the reservation.  A later cgp_sparse_reserve does not widen it: N and m of a call must fit both.  Blocks.
 *
 * Status of the calls below, in this order: CGP_EINVAL in a CGP_F32 context, for batch, N, d or m < 1, m > 512, an unknown kernel id
 * or RBF x Brownian with d != 1; without either reservation CGP_ESTATE; batch, N or m beyond either, d beyond the context's max_d
 * CGP_ECAPACITY; a NULL required pointer, theta_stride or grad_stride < ntheta CGP_EINVAL; the optimiser also CGP_EINVAL for a theta
 * <= 0.  All of these return before anything is enqueued.
 *
 * cgp_profile_*: CGP_PROF_KERNELS stays 5.  In a gradient call slot 0 is k_sparse_phi, slot 1 both algebra kernels (k_sparse_algebra,
 * k_sparse_grad_algebra), slot 2 k_sparse_reduce + k_sparse_grad_uu + k_sparse_grad_finish, slot 3 k_sparse_grad_panel (the predict
 * kernel never runs at M = 0; flops = 2 N (m + 1) LD per fit), slot 4 k_sparse_prep.
 *
 * Several target columns on one fit: the forward half is the section after this one, the gradient of their summed bound and its
 * optimiser the one after that.  Not provided: FITC; the resident windows; fp32 contexts; a cgp_sweep_* form. */
int cgp_sparse_grad_reserve(cgp_ctx *ctx, int max_batch);
/* Host buffers, blocks; layouts as cgp_fit_predict_sparse_batch, grad (batch, grad_stride), gradZ (batch, m, d) or NULL, info
 * (batch) or NULL.  A fit whose K_uu fails climbs the jitter ladder of cgp_fit_predict_sparse_batch, re-submitted alone into its
 * slot; the gradient is then that of the bound at that jitter.  Returns a negative error, else 0 or the first non-zero info. */
int cgp_sparse_nll_grad_batch(cgp_ctx *ctx, int batch, int N, int d, int m, int kernel_id, const double *X, const double *y,
                              const double *Z, const double *theta, int theta_stride, double *nll, double *grad, int grad_stride,
                              double *gradZ, int *info);
/* Device-resident variant: the forward chain's four launches, then four more, one linear chain on hip_stream; no allocation, no
 * synchronisation, no jitter ladder (capturable into a hipGraph with default settings).  Layouts as
 * cgp_fit_predict_sparse_batch_device; dgradZ (batch, d, m) -- the layout of dZ -- or NULL.  dnll, dgrad and dinfo are required. */
int cgp_sparse_nll_grad_batch_device(cgp_ctx *ctx, int batch, int N, int d, int m, int kernel_id, const double *dX,
                                     const double *dy, const double *dZ, const double *dtheta, const double *djitter,
                                     double *dnll, double *dgrad, int grad_stride, double *dgradZ, int *dinfo, void *hip_stream);
/* L-BFGS (cgp_optimize_batch's: Logexp on theta, pgtol 1e-5, factr 1e7, max_evals <= 0: 1000) on nll from theta_inout and Z_inout
 * (batch, m, d).  optimize_z = 0: over theta with Z fixed; 1: over [theta | Z row-major] jointly, Z unconstrained.  A trial point
 * whose K_uu fails climbs the ladder; one that stays infeasible (K_uu or B) counts as +inf.  X and y are uploaded once, theta and Z
 * per round.  logml (or NULL): the bound at the returned point, from one evaluation more -- bitwise what
 * cgp_fit_predict_sparse_batch returns there when no ladder step was needed; n_evals (or NULL): evaluations of each fit. */
int cgp_optimize_sparse_batch(cgp_ctx *ctx, int batch, int N, int d, int m, int kernel_id, const double *X, const double *y,
                              double *Z_inout, double *theta_inout, int theta_stride, int optimize_z, int max_evals,
                              double *logml, int *n_evals);

/* ---- sparse fits: P target columns share one inducing-point fit ------------------------------------------
 * GPy's SparseGPRegression(X, Y, Z=Z) with Y (N, P) -- four wheels' slip over one recorded history: Phi = K_uf K_fu, both m x m
 * factors and the variance do not depend on the targets, so they are computed ONCE per (X, Z, theta).  With the sparse section's
 * quantities, b, yty and c per column p:
 *   b_p = K_uf y_p      yty_p = y_p^T y_p      c_p = L_B^-1 L_u^-1 b_p / sigma2
 *   logml[p] = -N/2 log 2 pi - N/2 log sigma2 - sum log diag(L_B) - yty_p / (2 sigma2) + c_p^T c_p / 2 - t / (2 sigma2) + tr(A) / 2
 *   mean[p] = V2^T c_p      var = the single-column call's, shared by the P columns
 * logml[p] is what cgp_fit_predict_sparse_batch returns for y = Y[p]; GPy's objective for the model is sum_p logml[p]
 * (cgp_fit_predict_multi_batch's convention).  info is per fit; a failed fit has NaN in all P means, in var and in all P bounds.
 * The targets ride as rows m .. m + P - 1 of the augmented matrix whose row m carries y in a single-column call: K(Z, x_i) is
 * evaluated once and Phi accumulated once whatever P is, and the launches are the single-column call's (which IS this chain at P =
 * 1): five, four at M = 0.  For P <= 16 ceil((m + 1) / 16) - m the augmented matrix has no more 16-row tiles than at P = 1.
 *
 * Layouts.  Host form: as cgp_fit_predict_sparse_batch with Y (batch, P, N), mean (batch, P, M), var (batch, M), logml (batch, P),
 * info (batch).  Device form: cgp_fit_predict_sparse_batch_device's SoA layouts with dY (batch, P, N), dmean (batch, P, M), dvar
 * (batch, M), dlogml (batch, P), dinfo (batch).  M = 0 gives the P bounds only.
 *
 * Promises.
 *  1. The sparse calls above, the gradient and the optimiser are bitwise what they were before this section existed.
 *  2. var and info are bitwise cgp_fit_predict_sparse_batch[_device]'s for the same (X, Z, theta, Xs), for every P.
 *  3. A column's mean row and logml are a function of that column's targets and of the fit's (X, Z, theta, Xs, N, m, M, d, kernel):
 *     bitwise independent of P, of the column's position p and of the other columns (a NaN among another column's targets included),
 *     of the batch size, the slot and the neighbouring fits.  Permuting the columns permutes the outputs; the first columns of a
 *     wide call are the same columns of a narrower call.  No atomics; every sum runs in a fixed order over the real N.
 *  4. A column's mean row and logml are BITWISE cgp_fit_predict_sparse_batch[_device]'s on y = Y[p] (not merely within the 1e-9
 *     that two schedules of the dense multi call keep): every element of the augmented product is its own accumulator chain in
 *     sample order, c_p is solved by the single-column call's per-column arithmetic and the mean by its fma chain.
 *  5. Host form (for a fit that needed no ladder step), device form and a replayed graph agree bitwise.
 *
 * cgp_sparse_multi_reserve: what P columns add to the sparse scratch.  Needs a cgp_sparse_reserve that covers it (max_batch within
 * it), else CGP_ESTATE, and is sized by that reservation's max_n and max_m_ind as they stand at the call: with mt = ceil((max_m_ind
 * + 1) / 16), LD = 16 mt, C = min(ceil(max_n / 512), 16) and k = ceil((max_p - 1) / 16) -- the 16-row tile rows that the targets of
 * a call within it can add -- it allocates
 *   8 max_batch (128 C k (2 mt + k + 1) + 2 max_p LD + max_p) bytes
 * (max_n = 65 536, max_m_ind = 256: max_p = 4 0.61 MB, max_p = 16 0.66 MB, max_p = 64 2.8 MB per fit).  1 <= max_batch <=
 * the context's and 1 <= max_p <= CGP_SPARSE_MAX_P, else CGP_EINVAL; CGP_ENOMEM leaves no reservation; calling it again replaces the
 * reservation.  A later cgp_sparse_reserve does not widen it: batch, N and m of a call must fit both.  Blocks.  cgp_destroy frees it.
 *
 * Status of the two calls, in this order: CGP_EINVAL in a CGP_F32 context, for batch, N, d, P or m < 1, P > CGP_SPARSE_MAX_P, m >
 * 512, M < 0, an unknown kernel id or RBF x Brownian with d != 1; without either reservation CGP_ESTATE; batch, N, m, M or P beyond
 * them, d beyond the context's max_d CGP_ECAPACITY; a NULL required pointer or theta_stride < ntheta CGP_EINVAL.  All of these return
 * before anything is enqueued.
 *
 * cgp_profile_*: the slots of a sparse call (flops of slot 0: N (m + P)(m + P + 1) per fit).
 *
 * The gradient of the summed bound in theta and Z and its optimiser are the next section's.  Not provided: a trend on the sparse
 * fits; FITC; the resident windows; fp32 contexts; a cgp_sweep_* form. */
#define CGP_SPARSE_MAX_P 64
int cgp_sparse_multi_reserve(cgp_ctx *ctx, int max_batch, int max_p);
/* Host buffers, blocks.  A fit whose K_uu fails climbs the jitter ladder of cgp_fit_predict_sparse_batch on K_uu, re-submitted alone
 * into its slot with all its columns; a failing pivot of B is reported as it is.  logml and info may be NULL.  Returns a negative
 * error, else 0 or the first non-zero per-fit info. */
int cgp_fit_predict_sparse_multi_batch(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int m, int kernel_id,
                                       const double *X, const double *Y, const double *Z, const double *Xs, const double *theta,
                                       int theta_stride, int include_noise, double *mean, double *var, double *logml, int *info);
/* Device-resident variant: the single-column call's five launches (four when M = 0) in a linear chain on hip_stream; no allocation,
 * no synchronisation, no jitter ladder (capturable into a hipGraph with default settings).  dlogml and dinfo are required.  The
 * extent contract at cgp_fit_predict_batch_device applies. */
int cgp_fit_predict_sparse_multi_batch_device(cgp_ctx *ctx, int batch, int N, int d, int M, int P, int m, int kernel_id,
                                              const double *dX, const double *dY, const double *dZ, const double *dXs,
                                              const double *dtheta, const double *djitter, int include_noise,
                                              double *dmean, double *dvar, double *dlogml, int *dinfo, void *hip_stream);

/* ---- sparse fits: gradient and optimiser of P target columns' summed bound --------------------------------
 * SparseGPRegression(X, Y, Z=Z).optimize() with Y (N, P): ONE theta and ONE Z per fit maximise F = sum_p logml[p] of the section
 * above.  With its quantities, C = [c_1 ... c_P] (m x P) and Y (P x N):
 *   Chat = L_B^-T C      M = L_u^-T Chat      Q = P (I - B^-1) - Chat Chat^T
 *   T = L_u^-T Q L_u^-1 / (2 sigma2) = dF/dPhi      G_uu = 1/2 L_u^-T (Q - P A) L_u^-1 = dF/dK_uu      R = 2 T K_uf + M Y / sigma2 = dF/dK_uf
 *   dF/dtheta_j  = sum G_uu o dK_uu/dtheta_j + sum R o dK_uf/dtheta_j - P sum_i dk(x_i,x_i)/dtheta_j / (2 sigma2)
 *   dF/dsigma_n2 = (-N P + (sum_p yty_p + P t) / sigma2 - P tr A + P m - P tr B^-1 - ||C||_F^2 - ||Chat||_F^2) / (2 sigma2)
 *   dF/dz_rq     = the gradient section's expression with this R and this G_uu
 * -- at P = 1 the gradient section term for term; eps and the tie conventions are that section's.  Outputs: nll = -F with the P
 * bounds summed in column order, grad = d nll / d theta (natural parameters, cgp_nll_grad's order), gradZ = d nll / d Z, and
 * optionally the P bounds.  The only other route is P calls of cgp_sparse_nll_grad_batch at the same (theta, Z): P forward and P
 * backward passes over N and 6 P block solves on matrices that do not depend on the targets.  Here the forward chain is the
 * section above's at M = 0, the six block solves run once, and the second pass over N contracts over the m + P rows of the
 * augmented panel [K_uf; Y] instead of m + 1 (R is never stored): for P <= 16 ceil((m + 1) / 16) - m no 16-row tile more than at
 * P = 1.  The launches are the gradient section's eight; its kernels take P from the call.
 *
 * Layouts.  Host form: as cgp_sparse_nll_grad_batch with Y (batch, P, N), gradZ (batch, m, d) or NULL, logml (batch, P) or NULL,
 * info (batch) or NULL.  Device form: cgp_sparse_nll_grad_batch_device's with dY (batch, P, N), dgradZ (batch, d, m) or NULL, dlogml
 * (batch, P) or NULL.  CGP_F64 contexts, all five kernel ids, 1 <= P <= CGP_SPARSE_MAX_P.
 *
 * Promises.
 *  1. Every call of the three sections above -- the forward calls with one and several columns, the single-column gradient and its
 *     optimiser -- is bitwise what it was before this section existed.
 *  2. logml[p] is bitwise cgp_fit_predict_sparse_multi_batch_device's at any M; nll is bitwise the negated left-to-right float64
 *     sum of those P values.
 *  3. At P = 1, nll, grad and gradZ are bitwise cgp_sparse_nll_grad_batch[_device]'s on that column.
 *  4. A fit's outputs are a function of its own data and of (N, m, P, d, kernel, whether gradZ was asked) only: bitwise independent
 *     of the batch size, the slot and the neighbours; no floating-point atomics, every sum in a fixed order.
 *  5. Host form (for a fit that needed no ladder step), device form and a replayed graph agree bitwise.
 *  6. grad is bitwise the same with and without gradZ, and with and without logml.
 *  7. A following sparse forward call or single-column gradient call is bitwise what it is without this call; scratch left full of
 *     NaN by a call of another shape moves nothing.
 *  8. NOT promised: bitwise invariance under a permutation of the columns -- the sum over p is the inner dimension of a matrix-core
 *     loop and of the rank-P term of Q.  nll, grad and gradZ then agree to 1e-9 (the bar two routes of this library are held to);
 *     logml[p] still permutes bitwise.
 *  9. A NaN among one column's targets gives NaN in nll, grad and gradZ of that fit, leaves the other columns' logml bitwise what
 *     they were and info at 0, and does not touch the neighbouring fits.
 * A fit whose info is not 0 has NaN in nll, grad, gradZ and its P logml entries.
 *
 * cgp_sparse_multi_grad_reserve: only what the columns add to the gradient scratch.  Needs a cgp_sparse_reserve, a
 * cgp_sparse_grad_reserve and a cgp_sparse_multi_reserve that cover it (max_batch within each, max_p within the last), else
 * CGP_ESTATE, and is sized by the gradient reservation's max_m_ind as it stands at the call: with LD = 16 ceil((max_m_ind + 1) / 16),
 * mr = ceil(max_m_ind / 16) and k = ceil((max_p - 1) / 16) it allocates
 *   8 max_batch (16 mr (LD + 16 k) [k > 0] + max_p) bytes
 * (max_m_ind = 512: max_p = 4 or 16 2.2 MB, max_p = 64 2.4 MB per fit; max_m_ind = 256: 0.6 MB): the matrix-core operand image of
 * [T | M] / (2 sigma2), 16 mr LDa doubles with LDa = 16 ceil((m + P) / 16), which the single-column call keeps in A's spent LD^2
 * block and which no longer fits there once the targets add a tile row (m = 512, P = 64: 303 104 against 278 784); a call with LDa
 * = LD -- every call at P = 1 -- keeps it where it was.  1 <= max_batch <= the context's and 1 <= max_p <= CGP_SPARSE_MAX_P, else
 * CGP_EINVAL; CGP_ENOMEM leaves no reservation; calling it again replaces the reservation.  A later reservation of the other three
 * does not widen it: batch, N, m and P of a call must fit all four.  Blocks.  cgp_destroy frees it.
 *
 * Status of the calls below, in this order: CGP_EINVAL in a CGP_F32 context, for batch, N, d, P or m < 1, P > CGP_SPARSE_MAX_P, m >
 * 512, an unknown kernel id or RBF x Brownian with d != 1; without any of the four reservations CGP_ESTATE; batch, N, m or P beyond
 * any of them, d beyond the context's max_d CGP_ECAPACITY; a NULL required pointer, theta_stride or grad_stride < ntheta CGP_EINVAL;
 * the optimiser also CGP_EINVAL for a theta <= 0.  All of these return before anything is enqueued.
 *
 * cgp_profile_*: the slots of the gradient section (flops of slot 0: N (m + P)(m + P + 1), of slot 3: 2 N (m + P) LDa per fit).
 *
 * Not provided: FITC; a trend on the sparse fits; the resident windows; fp32 contexts; a cgp_sweep_* form. */
int cgp_sparse_multi_grad_reserve(cgp_ctx *ctx, int max_batch, int max_p);
/* Host buffers, blocks.  A fit whose K_uu fails climbs the jitter ladder of cgp_fit_predict_sparse_batch, re-submitted alone into
 * its slot with all its columns; the gradient is then that of the summed bound at that jitter.  Returns a negative error, else 0 or
 * the first non-zero info. */
int cgp_sparse_multi_nll_grad_batch(cgp_ctx *ctx, int batch, int N, int d, int P, int m, int kernel_id, const double *X,
                                    const double *Y, const double *Z, const double *theta, int theta_stride, double *nll,
                                    double *grad, int grad_stride, double *gradZ, double *logml, int *info);
/* Device-resident variant: the gradient section's eight launches in one linear chain on hip_stream; no allocation, no
 * synchronisation, no jitter ladder (capturable into a hipGraph with default settings).  dnll, dgrad and dinfo are required. */
int cgp_sparse_multi_nll_grad_batch_device(cgp_ctx *ctx, int batch, int N, int d, int P, int m, int kernel_id, const double *dX,
                                           const double *dY, const double *dZ, const double *dtheta, const double *djitter,
                                           double *dnll, double *dgrad, int grad_stride, double *dgradZ, double *dlogml,
                                           int *dinfo, void *hip_stream);
/* cgp_optimize_sparse_batch's L-BFGS on this nll from theta_inout and Z_inout (batch, m, d); optimize_z 0 or 1.  X and Y are
 * uploaded once, theta and Z per round.  logml_sum (or NULL): the summed bound at the returned point, from one evaluation more --
 * bitwise the column-order sum of what cgp_fit_predict_sparse_multi_batch returns there when no ladder step was needed; n_evals
 * (or NULL): evaluations of each fit. */
int cgp_optimize_sparse_multi_batch(cgp_ctx *ctx, int batch, int N, int d, int P, int m, int kernel_id, const double *X,
                                    const double *Y, double *Z_inout, double *theta_inout, int theta_stride, int optimize_z,
                                    int max_evals, double *logml_sum, int *n_evals);

/* ---- multi-target fits: gradient and optimiser of the summed logML ------------------------------------
 * m.optimize() of the multi-column model (gp_slip_node.py:36 with Y (N, P)): ONE theta per fit maximises
 *   sum_p logml[p] = -P/2 log|Ky| - 1/2 tr(Y^T Ky^-1 Y) - N P / 2 log 2 pi.
 * With Ky = L L^T, Z = L^-1 Y and A = Ky^-1 Y (N x P), GPy's ExactGaussianInference gives
 *   nll = -sum_p logml[p],    dL/dK = 1/2 (A A^T - P Ky^-1),    grad = d nll / d theta (natural parameters, cgp_nll_grad's order)
 * -- cgp_nll_grad's sums with w_ij = sum_p A_ip A_jp - P Ky^-1_ij; at P = 1 exactly cgp_nll_grad.  One gradient-mode
 * factorisation (needs max_m >= N, as every gradient call) serves all P columns; on top of it come N^2 P flops for Z, N^2 P for
 * A and N^2 P / 2 for the rank-P term, all on the fp64 matrix cores.  The only other route to this gradient is P calls of
 * cgp_nll_grad at the same theta: P factorisations of the same matrix.  CGP_F64 contexts only (CGP_EINVAL in a CGP_F32 context
 * before anything is enqueued; the context stays usable).  All five kernel ids.  Every shape takes the tiled schedules: the
 * one-launch short-window kernel (k_small) holds no multi-column form, so windows of at most 160 samples run the large-window
 * machinery here (as in the Matern and leave-one-out sections).
 *
 * cgp_multi_grad_reserve: scratch for A of up to max_batch fits with up to max_p targets: max_batch x (the context's max_n rounded
 * up to 128) x (max_p rounded up to 16) doubles (+ max_batch x max_p).  It needs a cgp_multi_reserve that covers it (max_batch and
 * max_p within that reservation), else CGP_ESTATE.  1 <= max_batch <= the context's, 1 <= max_p <= 4096, else CGP_EINVAL;
 * CGP_ENOMEM leaves no reservation; calling it again replaces the reservation.  Blocks.  cgp_destroy frees it.  A call below must
 * fit BOTH reservations as they are when it is made.
 *
 * Status of the three calls, before anything is enqueued: CGP_F32 context or P < 1: CGP_EINVAL; a reservation missing: CGP_ESTATE;
 * batch or P beyond one: CGP_ECAPACITY; then the shape rules of cgp_nll_grad / cgp_optimize_batch (CGP_EINVAL / CGP_ECAPACITY,
 * max_m >= N among them); a NULL required pointer, theta_stride or grad_stride < ntheta, and for the optimiser a theta <= 0:
 * CGP_EINVAL.  A failed call leaves the context usable.
 *
 * Determinism.  Run to run bitwise.  A fit's nll, gradient and logml are a function of its own data and of the schedule the call's
 * number of fits selects, never of its slot or its neighbours; no atomics, every sum in a fixed order.  The host form and the
 * device form of the same call are bitwise equal.  NOT promised: bitwise invariance under a permutation of the columns of Y -- the
 * sum over p is the inner dimension of a matrix-core loop; nll and gradient then agree to rounding only (logml[p] still permutes
 * bitwise).
 *
 * Cost (one MI355X, N = 2048, d = 6, SE-ARD, one evaluation of a lone fit; DESIGN.md section 9e has the table): 3.3 - 3.6 ms for
 * P = 1 ... 512, against 1.87 ms per column for P calls of cgp_nll_grad: P = 1 0.56 x, P = 8 4.5 x, P = 64 35 x, P = 512 263 x; 64 fits
 * x P = 8: 45 x.  For P = 1 call cgp_nll_grad: the crossover is between P = 1 and P = 2 (the multi call carries the solve for Z, a
 * 1.2 ms chain over N that does not shrink with P). */
int cgp_multi_grad_reserve(cgp_ctx *ctx, int max_batch, int max_p);
/* cgp_multi_nll_grad_batch: host buffers, layouts as cgp_fit_predict_multi_batch: X (batch, N, d), Y (batch, P, N), theta (batch,
 * theta_stride); outputs nll (batch), grad (batch, grad_stride), logml (batch, P) or NULL, info (batch) or NULL.  GPy's jitter
 * ladder per fit exactly as cgp_loo_batch runs it (the fits that failed only, one at a time, mean(diag) 1e-6 10^k, k = 0..4); the
 * results of a retried fit are those on the Ky that finally factored.  A fit whose info stays non-zero has NaN in nll, in its
 * gradient and in its P logml entries; its neighbours are unaffected.  Returns a negative error, else 0 or the first non-zero
 * per-fit status (cgp_loo_batch's convention).  Blocks. */
int cgp_multi_nll_grad_batch(cgp_ctx *ctx, int batch, int N, int d, int P, int kernel_id,
                             const double *X, const double *Y, const double *theta, int theta_stride,
                             double *nll, double *grad, int grad_stride, double *logml, int *info);
/* Device-resident variant: dX (batch, d, N), dY (batch, P, N), dtheta (batch, CGP_MAX_THETA), djitter (batch) or NULL; dnll (batch),
 * dgrad (batch, grad_stride), dlogml (batch, P) or NULL, dinfo (batch) int32 (required).  The gradient-mode fit schedule on each
 * fit's column 0 plus seven launches on hip_stream: no allocation, no synchronisation, no ladder (capturable into a hipGraph) --
 * read dinfo and re-submit the failed fits with djitter set.  A fit with dinfo != 0 gets NaN. */
int cgp_multi_nll_grad_batch_device(cgp_ctx *ctx, int batch, int N, int d, int P, int kernel_id,
                                    const double *dX, const double *dY, const double *dtheta, const double *djitter,
                                    double *dnll, double *dgrad, int grad_stride, double *dlogml, int *dinfo,
                                    void *hip_stream);
/* cgp_optimize_multi_batch: cgp_optimize_batch's host L-BFGS (Logexp transform, pgtol 1e-5, factr 1e7, the jitter ladder per trial
 * point, +inf for a point that stays infeasible) over the evaluation above: each fit's theta (batch, theta_stride) is replaced by
 * its optimum; logml_sum (batch) = sum_p logml[p] there and n_evals (batch) may be NULL.  max_evals <= 0: 1000.  Blocks. */
int cgp_optimize_multi_batch(cgp_ctx *ctx, int batch, int N, int d, int P, int kernel_id,
                             const double *X, const double *Y, double *theta_inout, int theta_stride, int max_evals,
                             double *logml_sum, int *n_evals);

/* ---- multi-device sweep (SURVEY.md 8b "cgp_fit_predict_batch(ctx[], ...)", 8e) --------------------
 * One engine context and one host thread per listed device; a batch of independent windows is cut into
 * contiguous per-device blocks (device i gets fits [start_i, stop_i), the first batch % ndev devices
 * one fit more -- cgp_sweep_shard returns the range), every block runs cgp_fit_predict_batch on its own
 * device concurrently, and the per-fit summaries {logml, max sigma = 2 sqrt(max var), info} are gathered
 * on the host in global fit order (`summary` is (batch, 3), may be NULL).  No data-path collective:
 * the path shards across fits only, a single fit is never split.  This is the entry point that lets
 * the reference's C++ ROS host (gp_predictor) shard a Monte-Carlo ensemble without Python; the
 * one-process-per-GPU form over RCCL is corenav_gp_amd/sharding.py + bench.py --gpus N.  `devices` may
 * name a device more than once (several contexts on one GPU: the self-test of a one-GPU box).
 * Argument meaning, outputs and return value as cgp_fit_predict_batch; max_batch_total = the largest
 * batch a call will carry.  Returns NULL / CGP_ECAPACITY like cgp_create / cgp_fit_predict_batch.
 * Reproducibility across shardings: a fit's result does not depend on its slot in a call or on its neighbours, and
 * in CGP_F64 not on how many fits share the call either -- a sweep equals one context running the whole batch BITWISE.
 * In CGP_F32 calls of up to 96 fits factor the 128 x 128 diagonal tile in a different (fatter) form than larger calls
 * do, so a fit's fp32 result depends on the size of the call it rides in to single-precision rounding (inside the
 * 1e-3 bar): a 512-fit sweep over 8 shards of 64 agrees with the 512-fit call to rounding, not bitwise
 * (tests/test_gpu_parity.py::test_sweep_fp32_matches_single_context_to_rounding). */
typedef struct cgp_sweep cgp_sweep;
cgp_sweep *cgp_sweep_create(const int *devices, int ndev, int max_n, int max_m, int max_d, int max_batch_total,
                            int dtype);
void cgp_sweep_destroy(cgp_sweep *sweep);
int cgp_sweep_ndev(const cgp_sweep *sweep);
int cgp_sweep_shard(const cgp_sweep *sweep, int batch, int i, int *start, int *stop);
int cgp_sweep_fit_predict(cgp_sweep *sweep, int batch, int N, int d, int M, int kernel_id, const double *X,
                          const double *y, const double *Xs, const double *theta, int theta_stride,
                          int include_noise, double *mean, double *var, double *logml, int *info,
                          double *summary);
/* Device-resident form: shard i's inputs already live on device i in the layout of cgp_fit_predict_batch_device
 * (its (stop_i - start_i) fits only), every argument an array of ndev per-shard device pointers -- dX[i] (n_i, d, N),
 * dy[i], dXs[i], dtheta[i] (n_i, CGP_MAX_THETA) fp64, djitter[i] or a NULL array, outputs dmean[i], dvar[i], dlogml[i],
 * dinfo[i]; hip_streams[i] the stream of device i to enqueue on (a NULL ARRAY = every context's own stream, an element
 * follows the hip_stream convention above).  Returns when every shard's work has been ENQUEUED, without synchronising:
 * no PCIe copy and no host round trip inside the call (a 64-fit shard is 0.8 ms of device time).  Wait with the streams
 * you passed, or cgp_sweep_synchronize for the contexts' own streams.  No jitter retry, as cgp_fit_predict_batch_device.
 * Threads: shard 0 is issued by the calling thread, the others by persistent worker threads created with the sweep (no
 * thread is created per call); a sweep over ONE device is exactly that context's call.  Current device: every entry point
 * that takes a context makes that context's device current on the thread it runs on (hipSetDevice) and leaves it so; after a
 * cgp_sweep_* call the CALLING thread's current device is therefore devices[0] -- a caller with its own work on another device
 * sets it again. */
int cgp_sweep_fit_predict_device(cgp_sweep *sweep, int batch, int N, int d, int M, int kernel_id, const void *const *dX,
                                 const void *const *dy, const void *const *dXs, const double *const *dtheta,
                                 const double *const *djitter, int include_noise, void *const *dmean, void *const *dvar,
                                 double *const *dlogml, int *const *dinfo, void *const *hip_streams);
int cgp_sweep_synchronize(cgp_sweep *sweep);
/* The engine context of shard i (owned by the sweep): for cgp_set_streams, cgp_set_refine, cgp_last_error, cgp_profile_* on a shard. */
cgp_ctx *cgp_sweep_context(const cgp_sweep *sweep, int i);

/* Stream groups of a batch.  n = 0 (the default): the engine decides -- an fp32 call of 56 ... 96 fits (BASELINE configs[2] as
 * sharded over 8 GPUs: 64 per GPU) is cut into TWO groups whose launch schedules run concurrently, group 0 on the caller's
 * stream and group 1 on one of the context's worker streams, forked from / joined to the caller's stream with events, so
 * the chain-bound early launches of one group run beside the MFMA-bound ones of the other (0.99 -> 0.90 ms per 64-fit
 * call on one context); every other call is one group.  Whether two streams really overlap depends on how the runtime mapped
 * them onto its hardware queues (the process's history), so the engine MEASURES: per (caller stream, fits, block steps), after two
 * warm-up calls, four such calls run as two groups and four as one, bracketed by events on the caller's stream; the faster form is
 * kept, measured again after 24, 48, ... 256 calls (a context's first calls run on a part still coming out of idle, where both
 * forms measure alike) and whenever three monitored calls in a row come out 1.3 x slower than the chosen form measured.  No call
 * blocks for this: every decision is read with hipEventQuery (a call whose answer is not in yet runs as two groups), and a stream
 * that is being captured into a hipGraph is never touched with a timing event (the call takes the form already decided, or two
 * groups forked / joined with plain events, which the capture records as edges).  A caller that wants the form fixed passes n = 1
 * or n = 2.  n = 1: always one group.  n = 2..8: up to n groups for full-batch
 * calls too (hundreds of fits gain nothing measurable).  Results do not depend on the setting (a fit's arithmetic is the
 * same in any group). */
int cgp_set_streams(cgp_ctx *ctx, int n);

/* Development aid (-DCGP_ABLATION builds; all zero otherwise): in-kernel s_memtime sums.  [0, 8) potf2
 * phases of block 0 (CGP_DBG & 512); [64 + 8k, 64 + 8k + 8) per-phase sums of k_panel at block step k
 * over all workgroups, slot 7 of each group = workgroup count (CGP_DBG & 1024).  Reading resets them. */
#define CGP_DEBUG_SLOTS 512
int cgp_debug_read(cgp_ctx *ctx, long long out[CGP_DEBUG_SLOTS]);
/* Development aid: the raw result record of the last short-window launch (cgp_nll_grad / cgp_optimize* of a window of at
 * most 160 samples in an fp64 context, csrc/cgp_small.hpp): [0] logML, [1] evaluations, [2] L-BFGS status, [3] iterations,
 * [4] info, [5] jitter, [8..18) gradient, [20..30) theta, [32..48) per-phase s_memtime sums (-DCGP_ABLATION builds; zero
 * otherwise: tools/small_phases.py). */
#define CGP_SMALL_OUT 48
int cgp_debug_small(cgp_ctx *ctx, double out[CGP_SMALL_OUT]);
/* Development aid: device addresses and byte sizes of the context's large buffers, as pairs
 * out[2 i] = address, out[2 i + 1] = bytes for i = 0 factor panels (Lw), 1 W images (Winv), 2 diagonal-tile images,
 * 3 panel-tile images, 4 inputs X, 5 running predictive sums, 6 latency partial tiles, 7 latency images
 * (tools/ctx_placement.py prints them next to the timings of a context). */
#define CGP_DEBUG_BUFFERS 8
int cgp_debug_buffers(cgp_ctx *ctx, unsigned long long out[2 * CGP_DEBUG_BUFFERS]);
/* Development aid: the launches a cgp_window_push / cgp_window_push_device of T ticks would make from the windows' present
 * state, from the routine the push itself cuts its ticks with; nothing is launched and the context is unchanged.  Per launch
 * out[4 i ..] = {kind, arg, t0, nt}: ticks [t0, t0 + nt) of the push go to k_window_ticks with `arg` threads per window
 * (CGP_PLAN_TICKS), to k_window_pairs with `arg` windows per workgroup (CGP_PLAN_PAIRS) or to k_window_multi with `arg` ticks per
 * pass (CGP_PLAN_MULTI).  At most `cap` records are written; returns the number of launches (call again with a larger array if
 * it exceeds cap), CGP_ESTATE without windows or after a push whose launches failed.  The tests assert with it which kernel a
 * case runs; the crossovers between the kernels are measured constants that move. */
#define CGP_PLAN_TICKS 0
#define CGP_PLAN_PAIRS 1
#define CGP_PLAN_MULTI 2
int cgp_debug_window_plan(cgp_ctx *ctx, int T, int *out, int cap);

/* ---- online sliding-window GP (BASELINE configs[3]; not reference behaviour) -------------------
 * `nwin` independent windows of at most N samples each live on the device.  cgp_window_push feeds
 * T ticks to every window in ONE launch: per tick the oldest sample leaves a full window (rank-1
 * Cholesky update), the new one enters (forward substitution), and the tick's outputs are the
 * one-step-ahead predictive mean / variance of the incoming y BEFORE it is added, and the log
 * marginal likelihood of the window after it.  theta (nwin, theta_stride) is fixed per window.
 * xs (nwin, T, d), ys (nwin, T); outputs (nwin, T).  Returns 0, or the 1-based tick at which a window
 * lost positive definiteness: of the first such window in index order, counted within the push in which it failed.  The window
 * keeps that code (cgp_window_state) and every later push returns it again, whatever its own length, until cgp_window_set_theta
 * or cgp_window_init replaces the window; the other windows go on unaffected.  cgp_window_push blocks until the outputs are in the caller's arrays (a small push is read and
 * written by the kernels in pinned host memory; a one-tick push waits on the windows' status words there rather than on the
 * stream: 74 us per tick of one N = 512 window from a C caller).  Steady-state ticks of a longer push go two per pass over the
 * factors, four from 512 windows: the outputs are those of the tick-by-tick stream to rounding. */
int cgp_window_init(cgp_ctx *ctx, int nwin, int N, int d, int kernel_id, const double *theta, int theta_stride);
int cgp_window_push(cgp_ctx *ctx, int T, const double *xs, const double *ys, int include_noise,
                    double *pred_mean, double *pred_var, double *logml);
/* Device-resident variant for streaming benchmarks: dxs/dys/outputs are device pointers, enqueued on
 * hip_stream (NULL = legacy default stream, CGP_STREAM_CTX = the context's own) without synchronising. */
int cgp_window_push_device(cgp_ctx *ctx, int T, const double *dxs, const double *dys, int include_noise,
                           double *dpred_mean, double *dpred_var, double *dlogml, void *hip_stream);
/* Current size of window `w` and the first failing tick (0 = none). */
int cgp_window_state(cgp_ctx *ctx, int w, int *n, int *info);
/* Forecast from the windows as they stand after the last push: predictive mean and variance of every window at M test
 * points of its own, xs (nwin, M, d) row-major, outputs (nwin, M).  What the reference's producer publishes per recording
 * window (gp_slip_node.py:45-61: mean and variance over the next 600 ticks; sigma = 2 sqrt(var) feeds cgp_predict_stop),
 * computed from the factor, z = L^-1 y and inputs the pushes maintain instead of from a refit:
 *   V = L^-1 k(X, xs),  mean_j = sum_i V_ij z_i,  var_j = max(k(xs_j, xs_j) - sum_i V_ij^2, 1e-15) (+ sigma_n^2 when include_noise)
 * (cgp_predict's conventions), always in fp64, n^2 M flops per window on the fp64 matrix cores.  The windows are not modified:
 * a push after a forecast gives bitwise what it gives without it.  An empty window (no sample pushed yet) answers with the
 * prior: mean 0, var k(xs_j, xs_j) (+ sigma_n^2).  A window that lost positive definiteness in an earlier push gets NaN in all
 * of its outputs; the other windows are unaffected.  Returns CGP_ESTATE without windows, CGP_EINVAL for M < 1 or a NULL
 * pointer, else 0 or, like cgp_window_push, the 1-based tick at which a window failed.  Blocks until the outputs are in the
 * caller's arrays. */
int cgp_window_predict(cgp_ctx *ctx, int M, const double *xs, int include_noise, double *mean, double *var);
/* Device-resident variant: dxs / dmean / dvar are device pointers; two launches enqueued on hip_stream (NULL = legacy
 * default stream, CGP_STREAM_CTX = the context's own) after the pushes enqueued there earlier, without allocation or
 * synchronisation (capturable into a hipGraph).  It cannot see a failed window: its NaN outputs and cgp_window_state do. */
int cgp_window_predict_device(cgp_ctx *ctx, int M, const double *dxs, int include_noise, double *dmean, double *dvar,
                              void *hip_stream);
/* Predictive gradients from the windows as they stand after the last push (m.predictive_gradients(Xnew) on a window that is
 * maintained instead of refitted): xs (nwin, M, d) as for cgp_window_predict, mean / var (nwin, M), each may be NULL,
 * dmean / dvar (nwin, M, d) row-major, either may be NULL, not both (CGP_EINVAL).  Formulas, kernel derivatives (all five
 * kernel ids), the id-2 tie convention and sign(0) = 0 are those of the "predictive gradients" section above, with
 * alpha = L^-T z and B = L^-T L^-1 K(X, xs) on the window's n samples:
 *   dmean[m][q] =                     sum_i dk(x*_m, x_i)/dx*_q alpha_i
 *   dvar [m][q] = dk(x*_m, x*_m)/dx*_q - 2 sum_i dk(x*_m, x_i)/dx*_q B[i][m]
 * -- the gradient of the UNCLIPPED latent variance; include_noise only affects var.  mean / var, where passed, are bitwise
 * what cgp_window_predict returns for the same arguments (the forward pass is the same code).  Always fp64, whatever the
 * context's dtype; 2 n^2 M flops per window on the fp64 matrix cores (the forecast's forward substitution and its mirror
 * image).  The windows are not modified (L, z, the samples and the state words are not written, the slabs' strict upper
 * triangle is neither read nor written): a push after the call gives bitwise what it gives without it.  An empty window
 * answers with the prior: mean 0, var k(xs_j, xs_j) (+ sigma_n^2), dmean 0, dvar = d k(x*, x*) / dx* (zero for ids 0, 1, 3, 4;
 * sigma_r^2 sigma_b^2 sign(x*) for id 2); a window still filling works; a window that lost positive definiteness gets NaN in
 * all of its outputs, the others are unaffected.  A window's outputs depend on its own state and on N (which selects the
 * kernel form) only, never on its slot, on nwin or on its neighbours; no atomics, every sum runs in a fixed order; the host
 * and the device form are bitwise equal.  No reservation call is needed.  Uses the scratch of the diagonal blocks' inverses
 * (shared with cgp_window_predict) and the alpha scratch of cgp_window_nll_grad: it is not to run concurrently with
 * cgp_window_predict, cgp_window_nll_grad, cgp_window_loo or the joint forecast on other streams of the same context.
 * Returns CGP_ESTATE without windows, CGP_EINVAL for M < 1, a NULL xs or both gradients NULL, else 0 or, like
 * cgp_window_predict, the 1-based tick at which a window failed.  Blocks until the outputs are in the caller's arrays. */
int cgp_window_predict_gradients(cgp_ctx *ctx, int M, const double *xs, int include_noise,
                                 double *mean, double *var, double *dmean, double *dvar);
/* Device-resident variant: device pointers with the same NULL rules (dmean_out / dvar_out are the (nwin, M) mean and
 * variance, ddmean / ddvar the (nwin, M, d) gradients); three launches enqueued on hip_stream (NULL = legacy default stream,
 * CGP_STREAM_CTX = the context's own), without allocation or synchronisation (capturable into a hipGraph).  Nothing outside
 * the documented extents is written, every documented element of a passed array is written, element alignment suffices.
 * It cannot see a failed window: its NaN outputs and cgp_window_state do. */
int cgp_window_predict_gradients_device(cgp_ctx *ctx, int M, const double *dxs, int include_noise,
                                        double *dmean_out, double *dvar_out, double *ddmean, double *ddvar,
                                        void *hip_stream);

/* ---- multi-target sliding windows: P target columns share a window's resident factor -----------------
 * The window form of the multi-target fits above: every tick brings P targets on the same inputs (the four wheels' slip and
 * whatever else is sampled on the same time axis), and a forecast answers with P mean rows, ONE variance and P log marginal
 * likelihoods from the ONE resident factor -- instead of P copies of every window, P rank-1 updates per tick and P forecast
 * solves.  Formulas (those of the multi-target section), on the window's n samples, Y (n x P) its targets:
 *   Z = L^-1 Y          V = L^-1 K(X, xs)
 *   mean[p, m] = sum_i V[i, m] Z[i, p]
 *   var[m]     = max(k(xs_m, xs_m) - sum_i V[i, m]^2, 1e-15) (+ sigma_n^2 when include_noise)
 *   logml[p]   = -1/2 sum_i Z[i, p]^2 - sum_i log L_ii - n/2 log 2 pi        (sum_i log L_ii read from the diagonal in a fixed order)
 * CGP_F64 contexts only: every entry point of this section returns CGP_EINVAL in a CGP_F32 context before anything is enqueued.
 * All five kernel ids.
 *
 * How it is kept.  Column 0 goes through the push kernels exactly as cgp_window_push feeds them: the per-tick outputs of a
 * multi-target push (one-step-ahead mean / variance, logML) describe COLUMN 0 ONLY and are bitwise what cgp_window_push gives for
 * that column.  All P columns (column 0 included) are also written to a per-window target store, a circular buffer of the last N
 * ticks; Z is formed from it and the factor AS IT STANDS whenever a forecast asks.  So after cgp_window_set_theta or
 * cgp_window_optimize the next multi-target forecast is right for every column with no further call, and a failed window that
 * cgp_window_set_theta revives answers for every column, the samples pushed while it was failed included.
 *
 * cgp_window_multi_reserve: once after cgp_window_init, while every window is still empty (CGP_ESTATE otherwise, and without
 * windows): the target store, nwin x P x N doubles, the scratch for Z, nwin x ceil(P / 16) x (N rounded up to 16) x 16 doubles,
 * and a block for column 0 of a push.  1 <= P <= 64, else CGP_EINVAL.  CGP_ENOMEM leaves no reservation; calling it again (windows
 * still empty) replaces the reservation; cgp_window_init and cgp_destroy drop it.  Blocks (it synchronises the device).
 * While a reservation exists cgp_window_push and cgp_window_push_device return CGP_ESTATE: a single-target push would leave the
 * other columns behind.
 *
 * cgp_window_push_multi: xs (nwin, T, d), Ys (nwin, T, P) -- a tick's P targets contiguous -- outputs (nwin, T) for column 0.  P
 * must equal the reservation's (CGP_EINVAL).  Return value and failure semantics are cgp_window_push's.  Blocks.
 *
 * cgp_window_predict_multi: xs (nwin, M, d), mean (nwin, P, M), var (nwin, M) (shared by the P targets), logml (nwin, P) or NULL.
 * An empty window answers with the prior: mean 0, var k(xs_m, xs_m) (+ sigma_n^2), logml 0.  A window that lost positive
 * definiteness has NaN in all P mean rows, in var and in its P logml entries; its neighbours are unaffected.  Read-only on the
 * windows (L, z, the samples and the state words are not written): a push after a forecast is bitwise the push without it, and
 * two forecasts in a row are identical (the scratch carries no state).  Returns CGP_ESTATE without windows or without a
 * reservation, CGP_EINVAL for a P that is not the reservation's, M < 1 or a NULL required pointer, else 0 or, like
 * cgp_window_predict, the 1-based tick at which a window failed.  Blocks.
 *
 * Determinism.  var is bitwise cgp_window_predict's var for the same arguments (the same code, the same arithmetic).  A column's
 * mean row and logml are a function of its own targets, of the window and of N (which selects the kernel form): never of its
 * position p, of P, of the other columns, of the window's slot or of its neighbours.  Permuting the columns permutes the outputs
 * bitwise.  No atomics; every sum runs in a fixed order over the window's real n samples.  Column 0's mean row agrees with
 * cgp_window_predict's mean to rounding, not bitwise: the resident z is updated incrementally, Z is a fresh solve.
 *
 * The other window calls on a multi-target context -- cgp_window_predict, cgp_window_predict_gradients, cgp_window_predict_cov,
 * cgp_window_sample, cgp_window_loo, cgp_window_nll_grad and cgp_window_optimize -- keep working and speak of COLUMN 0.
 * The summed objective of the P columns and its optimiser are cgp_window_multi_nll_grad and cgp_window_optimize_multi, below
 * cgp_window_optimize.  Not provided: multi-target joint forecast / leave-one-out / predictive gradients, and one-step-ahead
 * outputs for the columns >= 1.
 * Cost of a forecast: the forecast's n^2 M flops, n^2 P for Z and 2 n M P for the mean rows, per window, on the fp64 matrix
 * cores.  Shares the scratch of the diagonal blocks' inverses with cgp_window_predict: not to run concurrently with the other
 * window forecasts on other streams of the same context. */
int cgp_window_multi_reserve(cgp_ctx *ctx, int P);
int cgp_window_push_multi(cgp_ctx *ctx, int T, int P, const double *xs, const double *Ys, int include_noise,
                          double *pred_mean, double *pred_var, double *logml);
/* Device-resident variant: device pointers, enqueued on hip_stream (NULL = legacy default stream, CGP_STREAM_CTX = the context's
 * own) without synchronising: one small launch that stores the targets, then cgp_window_push_device's launches.  The block that
 * holds column 0 is sized for pushes of up to max(N, 256) ticks; a longer push than any before it grows it first (an allocation,
 * not capturable).  The extent contract at cgp_fit_predict_batch_device applies. */
int cgp_window_push_multi_device(cgp_ctx *ctx, int T, int P, const double *dxs, const double *dYs, int include_noise,
                                 double *dpred_mean, double *dpred_var, double *dlogml, void *hip_stream);
int cgp_window_predict_multi(cgp_ctx *ctx, int M, int P, const double *xs, int include_noise,
                             double *mean, double *var, double *logml);
/* Device-resident variant: device pointers (dlogml may be NULL); three launches enqueued on hip_stream, without allocation,
 * attribute call or synchronisation (capturable into a hipGraph, like cgp_window_predict_device).  Nothing outside the documented
 * extents is written, every documented element is written, element alignment suffices.  It cannot see a failed window: its NaN
 * outputs and cgp_window_state do. */
int cgp_window_predict_multi_device(cgp_ctx *ctx, int M, int P, const double *dxs, int include_noise,
                                    double *dmean, double *dvar, double *dlogml, void *hip_stream);

/* ---- explicit basis functions (a trend) on the multi-target windows ------------------------------------------
 * The window form of the trend section above (its formulas, its rank rule, on the window's n samples).  The basis at the samples
 * is what the caller pushed as the LAST q COLUMNS of a multi-target context (cgp_window_push_multi with P = targets + q): basis
 * values travel through the target store like any column and the push path is not touched.  The first P - q columns are the
 * targets.  Needs cgp_window_multi_reserve's P and 1 <= q < P, q <= CGP_MAX_TREND.
 *
 * cgp_window_trend_reserve: after cgp_window_multi_reserve, at any fill state of the windows (CGP_ESTATE without windows or
 * without that reservation; CGP_EINVAL in a CGP_F32 context, for q outside 1 .. min(P - 1, CGP_MAX_TREND) or max_m < 1): nwin x
 * (P (max_m + 1) + 16 (P rounded up to 16) + 256) doubles.  CGP_ENOMEM leaves no reservation; calling it again replaces it;
 * cgp_window_multi_reserve, cgp_window_init and cgp_destroy drop it.  Blocks.
 *
 * cgp_window_predict_trend: xs (nwin, M, d), Hs (nwin, q, M); mean (nwin, P - q, M), var (nwin, M), beta (nwin, P - q, q), logml
 * (nwin, P - q), tinfo (nwin); beta, logml and tinfo may be NULL.  A window with n < q samples, the empty window included, has a
 * rank-deficient A and answers by the rank rule: NaN, tinfo = n + 1 for a basis in general position (a vague prior has no forecast
 * to give there).  A window that lost positive definiteness answers NaN with tinfo = 0; cgp_window_set_theta revives it with no
 * further call.  Read-only on the windows: a push after the call is bitwise the push without it.  Status: CGP_EINVAL in a CGP_F32
 * context; CGP_ESTATE without windows or with either reservation missing; CGP_EINVAL for a P or q that is not the
 * reservations', M < 1 or a NULL required pointer; CGP_ECAPACITY for M > max_m; else 0 or, like cgp_window_predict, the 1-based
 * tick at which a window failed.  Blocks.  Host form, device form, a replayed graph and a window's slot do not change a bit of a
 * window's outputs.  Stream exclusion as cgp_window_predict_multi (the scratch of the diagonal blocks' inverses and the Z scratch
 * are shared with it).  What the trend section does not provide is not provided here either. */
int cgp_window_trend_reserve(cgp_ctx *ctx, int q, int max_m);
int cgp_window_predict_trend(cgp_ctx *ctx, int M, int P, int q, const double *xs, const double *Hs, int include_noise,
                             double *mean, double *var, double *beta, double *logml, int *tinfo);
/* Device-resident variant: device pointers, all required; cgp_window_predict_multi_device's three launches and three more on
 * hip_stream, without allocation, attribute call or synchronisation (capturable).  Nothing outside the documented extents is
 * written, every documented element is written. */
int cgp_window_predict_trend_device(cgp_ctx *ctx, int M, int P, int q, const double *dxs, const double *dHs, int include_noise,
                                    double *dmean, double *dvar, double *dbeta, double *dlogml, int *dtinfo,
                                    void *hip_stream);

/* ---- hyper-parameters of the resident windows, replaced and re-estimated in place ----------------
 * The reference re-estimates its hyper-parameters on every window (gp_slip_node.py:36, m.optimize()); cgp_window_init fixes
 * theta.  The three entry points below change it on the windows a context holds, from what is resident on the device (the
 * factor, z = L^-1 y, the inputs, the targets): no host mirror of the samples, no re-init, no ticks pushed again.
 *
 * cgp_window_set_theta: for every selected window (select[w] != 0; select == NULL: all) store theta (nwin, theta_stride; the
 * layout of cgp_window_init) and the record derived from it, form Ky = K + (sigma_n^2 + 1e-8) I from the window's resident
 * inputs, factor it in place at the window's current origin and write z = L^-1 y and the window's log marginal likelihood
 * (logml[w]; 0 for an empty window).  Origin, size and tick count do not change; a window still filling or empty works (its size
 * is read from the device state).  The window's failure word is SET from the result: 0 when the factorisation succeeded -- this
 * is how a window that lost positive definiteness in a push (cgp_window_state info != 0, NaN forecasts) is revived, e.g. with a
 * larger sigma_n^2 -- and otherwise the LAPACK-style 1-based index of the first non-positive pivot, counted in the window's
 * order, oldest first (sample 1 is the oldest the window holds, however far its ring has moved), which info[w] also
 * receives: cgp_window_state, the forecast's NaN rule and later pushes then treat the window exactly like one a push failed
 * (logml[w] is NaN).  No jitter ladder (the pushes have none).  theta is validated no more than cgp_window_init validates it:
 * a theta under which Ky is not positive definite, or a non-finite one, shows up as a failed window, not as an argument error.
 * Unselected windows are not touched, bit for bit (their logml / info entries are 0); a window's result depends neither on
 * its slot nor on its neighbours nor on select.  logml and info may be NULL.  Returns CGP_ESTATE without windows, CGP_EINVAL for
 * a NULL theta or theta_stride < ntheta, else 0 or the 1-based index of the first window that failed.  Blocks.
 * n^3 / 3 flops per window on the fp64 matrix cores. */
int cgp_window_set_theta(cgp_ctx *ctx, const double *theta, int theta_stride, const unsigned char *select, double *logml,
                         int *info);
/* Device-resident variant: dtheta (nwin, theta_stride), dselect (nwin bytes or NULL), dlogml (nwin or NULL) and dinfo (nwin
 * or NULL) are device pointers; one launch on hip_stream (NULL = legacy default stream, CGP_STREAM_CTX = the context's own)
 * without allocation or synchronisation (capturable into a hipGraph).  Entries of unselected windows are not written.
 * Returns 0 or an argument / runtime error; failed windows show in dinfo and cgp_window_state. */
int cgp_window_set_theta_device(cgp_ctx *ctx, const double *dtheta, int theta_stride, const unsigned char *dselect,
                                double *dlogml, int *dinfo, void *hip_stream);
/* cgp_window_nll_grad: the NEGATIVE log marginal likelihood of every window and its gradient with respect to the natural
 * parameters (cgp_nll_grad's conventions and theta layout) AT THE THETA THE WINDOW HOLDS, from the factor, z and the inputs as
 * they stand after any number of pushes: dL/dK = 0.5 (alpha alpha^T - Ky^-1), alpha = L^-T z, contracted with dK/dtheta; Ky^-1
 * is never stored (2 n^3 / 3 flops per window on the fp64 matrix cores).  nll (nwin), grad (nwin, grad_stride).  A failed
 * window answers NaN, an empty one 0 and a zero gradient.  The factor (lower triangle and diagonal), z, the samples and the
 * state words are not written: a push after the call gives bitwise what it gives without it.  Shares a scratch buffer with
 * cgp_window_predict: the two are not to run concurrently on different streams.  Returns CGP_ESTATE without windows,
 * CGP_EINVAL for a NULL pointer or grad_stride < ntheta, else 0.  Blocks. */
int cgp_window_nll_grad(cgp_ctx *ctx, double *nll, double *grad, int grad_stride);
/* Device-resident variant: four launches on hip_stream, no allocation, no synchronisation (capturable into a hipGraph). */
int cgp_window_nll_grad_device(cgp_ctx *ctx, double *dnll, double *dgrad, int grad_stride, void *hip_stream);
/* cgp_window_loo: leave-one-out cross-validation (formulas: the cgp_loo section above) of every resident window as it stands
 * after the last push, at the theta it holds, from the factor, z, the inputs and the targets; fp64 whatever the context's dtype,
 * as cgp_window_predict is.  loo_mean / loo_var / loo_lpd (nwin, N) in the window's own order, oldest sample first; lpd_sum
 * (nwin); each may be NULL, not all four.  Entries [n, N) of a window still filling are NaN; an empty window has all-NaN rows
 * and lpd_sum = 0; a window that lost positive definiteness has NaN everywhere, lpd_sum included.  One wave per window and 16
 * samples runs the forward half of cgp_window_nll_grad's substitution (n^3 / 3 flops per window on the fp64 matrix cores), so a
 * call costs less than the gradient's.  The windows are not modified: the factor (lower triangle and diagonal), z, the
 * samples and the state words are not written, and a push after the call gives bitwise what it gives without it.  The call uses
 * the slabs' strict upper triangle and the scratch buffers of cgp_window_predict and cgp_window_nll_grad: it is not to run
 * concurrently with cgp_window_predict, cgp_window_nll_grad or the joint forecast on other streams of the same context.
 * Returns CGP_ESTATE without windows, CGP_EINVAL when every output is NULL, else 0.  Blocks. */
int cgp_window_loo(cgp_ctx *ctx, double *loo_mean, double *loo_var, double *loo_lpd, double *lpd_sum);
/* Device-resident variant: four launches on hip_stream, no allocation, no synchronisation (capturable into a hipGraph). */
int cgp_window_loo_device(cgp_ctx *ctx, double *dloo_mean, double *dloo_var, double *dloo_lpd, double *dlpd_sum,
                          void *hip_stream);
/* cgp_window_optimize: m.optimize() on the resident windows.  One L-BFGS (the optimiser of cgp_optimize_batch: Logexp-
 * transformed parameters, pgtol 1e-5, factr 1e7, at most max_evals evaluations per window, <= 0 meaning 1000) per selected
 * window, started at the theta the window holds -- every entry must be > 0, else CGP_EINVAL before anything is changed.  One
 * round = cgp_window_set_theta_device at the trial points + cgp_window_nll_grad_device on the context's stream and one copy
 * back; each window keeps its own line search, finished windows are deselected.  A trial point whose Ky is not positive
 * definite is an infeasible point for the line search (no jitter ladder: the pushes that follow would not carry one).  On
 * return every selected window holds its best theta and the factor that belongs to it; unselected windows are untouched;
 * pushes and forecasts simply continue.  theta_out (nwin, theta_stride), logml_out (nwin), n_evals (nwin) may be NULL; only
 * the entries of selected windows are written.  Returns CGP_ESTATE / CGP_EINVAL / 0.  Blocks. */
int cgp_window_optimize(cgp_ctx *ctx, int max_evals, const unsigned char *select, double *theta_out, int theta_stride,
                        double *logml_out, int *n_evals);

/* ---- multi-target sliding windows: the P columns' summed log marginal likelihood, its gradient and its optimiser ----
 * The window form of cgp_multi_nll_grad_batch / cgp_optimize_multi_batch: with Y (n, P) the reference's m.optimize() maximises
 * sum_p logml[p] over ONE theta, and a multi-target window set re-estimates its hyper-parameters for the model it forecasts,
 * from what is resident -- the factor, the inputs and the target store -- with no host mirror of the samples:
 *   Z = L^-1 Y    A = L^-T Z = Ky^-1 Y
 *   nll  = - sum_p logml[p]                                     (logml[p] as cgp_window_predict_multi defines it, summed in p order)
 *   dnll/dtheta_q = -1/2 sum_ij (sum_p A_ip A_jp - P (Ky^-1)_ij) dK_ij/dtheta_q
 * One pass over the factor serves all P columns (2 n^3 / 3 + n^2 P flops per window and 2 n^2 P more for A and the rank-P term,
 * on the fp64 matrix cores); P single-target window sets cost P such passes.  CGP_F64 contexts only, all five kernel ids,
 * 1 <= P <= 64.
 *
 * cgp_window_multi_grad_reserve: after cgp_window_multi_reserve, whose P it takes (CGP_ESTATE without windows or without that
 * reservation; CGP_EINVAL in a CGP_F32 context): the scratch for A, nwin x ceil(P / 16) x (N rounded up to 16) x 16 doubles
 * in the Z scratch's tile order, zeroed, and nwin x P doubles for the per-column values of a call that passes no logml.  It holds
 * no stream state, so it may be called at any fill state of the windows.  CGP_ENOMEM leaves no reservation; calling it again
 * replaces the reservation; cgp_window_multi_reserve, cgp_window_init and cgp_destroy drop it.  Blocks (it synchronises the
 * device).
 *
 * cgp_window_multi_nll_grad: nll (nwin), grad (nwin, grad_stride), logml (nwin, P) or NULL.  The gradient is with respect to the
 * natural parameters, in cgp_window_nll_grad's layout and conventions.  Everything is evaluated AT THE THETA THE WINDOW HOLDS,
 * from the factor, the inputs and the target store as they stand and from n read on the device: a window that is still filling
 * works, and after cgp_window_set_theta every column is right with no further call.  A failed window answers NaN in nll, in the
 * gradient and in its P logml entries; an empty window answers 0, a zero gradient and logml 0; neighbours are unaffected.
 * Status, checked before anything is enqueued: CGP_EINVAL in a CGP_F32 context; CGP_ESTATE without windows or with either
 * reservation missing; CGP_EINVAL for a P that is not the reservation's, a NULL nll or grad, or grad_stride < ntheta; else 0.
 * Blocks.
 * Read-only on the windows: the factor's lower triangle and diagonal, z, the samples, the target store and its tick word and the
 * state words are not written -- a push, a forecast or a cgp_window_nll_grad after the call is bitwise what it is without it.
 * Like cgp_window_nll_grad it uses the slabs' strict upper triangle, the scratch of the diagonal blocks' inverses and the gradient
 * scratch, and like cgp_window_predict_multi the Z scratch: it is not to run beside cgp_window_predict, cgp_window_predict_multi,
 * cgp_window_predict_gradients, cgp_window_nll_grad, cgp_window_loo, cgp_window_set_theta or the joint forecast on other streams
 * of the same context.
 * Determinism: no atomics, every sum in a fixed order.  A window's result depends on the window, its targets, P and N only, not
 * on its slot or its neighbours; two calls in a row, the host and the device form and a graph replay are bitwise equal; nll and
 * grad do not depend on whether logml is passed.  Permuting the columns permutes logml bitwise and moves nll and grad by
 * rounding only.  At P = 1 the result agrees with cgp_window_nll_grad to rounding, not bitwise (the resident z is incremental, Z
 * is a fresh solve).
 * Against the routes without it (measured, 1 024 windows x N = 512, d = 3, SE-ARD; DESIGN section 9i has the table): one
 * evaluation costs 52 ms whatever P <= 16 is (54 ms at P = 64) against 38 ms of one cgp_window_nll_grad_device, so against P
 * single-target evaluations the crossover is P = 2 (0.73 x at P = 1, 2.9 x at 4, 11.7 x at 16, 45 x at 64).  Against
 * cgp_multi_nll_grad_batch on a host mirror of the samples (11 ... 17 ms, upload included) it LOSES at every P, by 3.3 ... 4.8 x:
 * the in-place evaluation is slower than the batch engine's refit, as cgp_window_nll_grad is; what it saves is the mirror.
 *
 * cgp_window_optimize_multi: cgp_window_optimize with the summed objective -- the same L-BFGS driver, the same round
 * (cgp_window_set_theta_device at the trial points, the evaluation above, one copy back), a non-positive-definite trial point
 * infeasible, the best theta's factor put back where the last trial was not the best.  A start theta <= 0 in a selected window:
 * CGP_EINVAL before anything is changed.  Afterwards the selected windows hold the optimum and its factor: the next
 * cgp_window_predict_multi is right for every column with no further call, the next push continues under the new theta.
 * theta_out (nwin, theta_stride), logml_sum_out (nwin; sum_p logml[p] at the optimum), n_evals (nwin) may be NULL; only the
 * entries of selected windows are written.  Status as cgp_window_multi_nll_grad, and CGP_EINVAL for theta_stride < ntheta with a
 * theta_out.  Blocks. */
int cgp_window_multi_grad_reserve(cgp_ctx *ctx);
int cgp_window_multi_nll_grad(cgp_ctx *ctx, int P, double *nll, double *grad, int grad_stride, double *logml);
/* Device-resident variant: device pointers (dlogml may be NULL); five launches enqueued on hip_stream, without allocation,
 * attribute call or synchronisation (capturable into a hipGraph, like cgp_window_nll_grad_device).  Nothing outside the
 * documented extents is written, every documented element is written (the first ntheta entries of every gradient row), element
 * alignment suffices. */
int cgp_window_multi_nll_grad_device(cgp_ctx *ctx, int P, double *dnll, double *dgrad, int grad_stride, double *dlogml,
                                     void *hip_stream);
int cgp_window_optimize_multi(cgp_ctx *ctx, int P, int max_evals, const unsigned char *select, double *theta_out,
                              int theta_stride, double *logml_sum_out, int *n_evals);

/* ---- sliding windows: the leave-one-out objective, its gradient and its optimiser ----
 * The window form of cgp_loo_nll_grad_batch / cgp_optimize_loo_batch (the cgp_loo_nll_grad section above has the algebra): a
 * window set re-estimates its hyper-parameters by the leave-one-out pseudo-likelihood from what is resident -- the factor L of
 * Ky = K + (sigma_n^2 + 1e-8) I, z, the inputs and the targets -- with no host mirror of the samples and no jitter ladder:
 *   alpha = L^-T z    kd_i = (Ky^-1)_ii    c_i = 1/2 (1 / kd_i + alpha_i^2 / kd_i^2)    b_i = alpha_i / kd_i    beta = Ky^-1 b
 *   nlpd = - lpd_sum                                                   (lpd_sum as cgp_window_loo defines it)
 *   dnlpd/dtheta_q = -1/2 sum_ij (-2 sum_k Ky^-1_ik c_k Ky^-1_kj + beta_i alpha_j + alpha_i beta_j) dK_ij/dtheta_q
 * fp64 whatever the context's dtype, as cgp_window_loo and cgp_window_nll_grad are; all five kernel ids, d <= 8.  Per window
 * 4 n^3 / 3 flops for Ky^-1 and cgp_window_loo's pass and n^3 for the product, on the fp64 matrix cores.
 *
 * cgp_window_loo_grad_reserve: after cgp_window_init (CGP_ESTATE without windows).  With NP = N rounded up to 64 (the product
 * kernel's super-tile) and S = NP / 64 it holds Ky^-1 of every window, nwin x NP x NP doubles (2.1 GB for 1 024 x N = 512), and
 * one block of nwin x (N + ceil(N / 16) + 1 + 3 NP + 12 S (S + 1) / 2) doubles: loo_var, cgp_window_loo's chunk sums, lpd_sum,
 * the vectors c, b and beta, and the product kernel's twelve partial sums per super-tile pair.  It holds no stream state, so it
 * may be called at any fill state of the windows.  CGP_ENOMEM leaves no reservation and a usable context; calling it again
 * replaces the reservation; cgp_window_init and cgp_destroy drop it.  Blocks (it synchronises the device).
 *
 * cgp_window_loo_nll_grad: nlpd (nwin), grad (nwin, grad_stride; only the first ntheta entries of a row are written), logml
 * (nwin) or NULL -- the log marginal likelihood at no extra cost.  The gradient is with respect to the natural parameters, in
 * cgp_window_nll_grad's layout.  Everything is evaluated AT THE THETA THE WINDOW HOLDS, from the factor, z, the inputs and the
 * targets as they stand and from n, the origin and the failure word read on the device: a window that is still filling works,
 * n = 1 included.  A failed window answers NaN in nlpd, in the gradient and in logml; an empty window answers 0, a zero
 * gradient and 0; neighbours are unaffected.  nlpd is bitwise cgp_window_loo's lpd_sum negated and logml bitwise
 * cgp_window_nll_grad's nll negated (their launches run first, as they stand).
 * Status, checked before anything is enqueued: CGP_ESTATE without windows or without the reservation; CGP_EINVAL for a NULL
 * nlpd or grad, grad_stride < ntheta, or more than 65 535 windows; else 0.  Blocks.
 * Read-only on the windows: the factor's lower triangle and diagonal, z, the samples and the state words are not written -- a
 * push, a forecast, a cgp_window_nll_grad or a cgp_window_loo after the call is bitwise what it is without it.  Like
 * cgp_window_loo it uses the slabs' strict upper triangle, the scratch of the diagonal blocks' inverses, the alpha buffer and
 * the gradient scratch: it is not to run beside cgp_window_predict, cgp_window_predict_multi, cgp_window_predict_gradients,
 * cgp_window_nll_grad, cgp_window_multi_nll_grad, cgp_window_loo, cgp_window_set_theta, a push or the joint forecast on other
 * streams of the same context.
 * Determinism: no atomics, every sum in a fixed order.  A window's result depends on the window alone, not on its slot or its
 * neighbours; two calls in a row, the host and the device form and a graph replay are bitwise equal; nlpd and grad do not depend
 * on whether logml is passed, nor on what the scratch held before (every reader masks the rows and columns from n on).
 * Against the routes without it (measured, 1 024 windows x N = 512, d = 3, SE-ARD; DESIGN section 9k has the table): one
 * evaluation costs 52 ms (26 ms of it Ky^-1, 12 ms cgp_window_loo's pass, 12 ms the product) against 223 ms for central differences
 * on the windows -- 2 ntheta = 10 rounds of cgp_window_set_theta_device + cgp_window_loo_device -- so it wins 4.3 x there and
 * carries no finite-difference noise.  Against cgp_loo_nll_grad_batch on a host mirror of the samples (12.7 ms, upload included)
 * it LOSES, by 4.1 x, and a full cgp_window_optimize_loo loses to cgp_optimize_loo_batch on the mirror by 5.3 x: the in-place
 * evaluation is slower than the batch engine's refit, as cgp_window_nll_grad is; what it saves is the mirror.
 *
 * cgp_window_optimize_loo: cgp_window_optimize with the leave-one-out objective -- the same L-BFGS driver, the same round
 * (cgp_window_set_theta_device at the trial points, the evaluation above, one copy back), a non-positive-definite trial point
 * infeasible, the best theta's factor put back where the last trial was not the best.  A start theta <= 0 in a selected window:
 * CGP_EINVAL before anything is changed.  Afterwards the selected windows hold the optimum and its factor; pushes and forecasts
 * continue under it.  theta_out (nwin, theta_stride), lpd_sum_out (nwin; lpd_sum at the returned theta), n_evals (nwin) may be
 * NULL; only the entries of selected windows are written.  Status as cgp_window_loo_nll_grad, and CGP_EINVAL for theta_stride <
 * ntheta with a theta_out.  Blocks. */
int cgp_window_loo_grad_reserve(cgp_ctx *ctx);
int cgp_window_loo_nll_grad(cgp_ctx *ctx, double *nlpd, double *grad, int grad_stride, double *logml);
/* Device-resident variant: device pointers (dlogml may be NULL); nine launches enqueued on hip_stream, without allocation,
 * attribute call or synchronisation (capturable into a hipGraph, like cgp_window_loo_device).  Nothing outside the documented
 * extents is written, every documented element is written (the first ntheta entries of every gradient row), element alignment
 * suffices. */
int cgp_window_loo_nll_grad_device(cgp_ctx *ctx, double *dnlpd, double *dgrad, int grad_stride, double *dlogml, void *hip_stream);
int cgp_window_optimize_loo(cgp_ctx *ctx, int max_evals, const unsigned char *select, double *theta_out, int theta_stride,
                            double *lpd_sum_out, int *n_evals);

/* ---- joint forecast from the resident windows: full posterior covariance and sample paths ---------
 * cgp_window_predict answers with the marginals (the diagonal of the posterior).  The reference's model also offers the JOINT
 * posterior over the horizon -- predict(Xnew, full_cov=True) and posterior_samples_f(Xnew, size) -- which is what a
 * Monte-Carlo trajectory ensemble needs: one realisation of the whole slip curve per member, correlated from tick to tick.
 *
 * cgp_window_joint_reserve: once after cgp_window_init, scratch for joint forecasts of up to max_m test points per window
 * (V = L^-1 K(X, xs): nwin x N x max_m doubles, and the posterior covariance / its factor: nwin x max_m^2 doubles, both with
 * max_m and N rounded up to 16; 1 024 windows x N = 512 x max_m = 599 is 2.5 GB + 3.0 GB: the caller decides).
 * 1 <= max_m <= 1024, else CGP_EINVAL.  CGP_ESTATE without windows, CGP_ENOMEM when the device cannot hold it (an earlier
 * reservation is gone then).  Calling it again replaces the reservation; a later cgp_window_init drops it with the windows.
 * Blocks (it synchronises the device). */
int cgp_window_joint_reserve(cgp_ctx *ctx, int max_m);
/* cgp_window_predict_cov: mean (nwin, M) and the FULL posterior covariance cov (nwin, M, M) of every window at M test points
 * of its own, xs (nwin, M, d), all row-major:
 *   cov = K(xs, xs) - V^T V,  V = L^-1 K(X, xs)
 * Both triangles are written and are exactly equal.  mean and diag(cov) come from the solve cgp_window_predict runs and are
 * bitwise its mean / var: the diagonal is clipped at 1e-15 and include_noise != 0 adds sigma_n^2 to the DIAGONAL only (GPy's
 * predict(full_cov=True, include_likelihood=True)).  n^2 M + n M^2 flops per window on the fp64 matrix cores.  The windows are
 * not modified.  An empty window answers with the prior: mean 0, cov = K(xs, xs) (+ noise); a failed window gets NaN in all of
 * its outputs, the others are unaffected.  CGP_ESTATE without windows or without a reservation, CGP_EINVAL for M < 1 or a NULL
 * pointer, CGP_ECAPACITY for M > max_m, else 0 or, like cgp_window_predict, the 1-based tick at which a window failed.  Blocks.
 * Shares the scratch of the diagonal blocks' inverses with cgp_window_predict and cgp_window_nll_grad, and its own scratch with
 * cgp_window_sample: none of these are to run concurrently on different streams of one context. */
int cgp_window_predict_cov(cgp_ctx *ctx, int M, const double *xs, int include_noise, double *mean, double *cov);
/* Device-resident variant: device pointers, three launches enqueued one after the other on hip_stream (NULL = legacy default
 * stream, CGP_STREAM_CTX = the context's own), no allocation, no synchronisation (capturable into a hipGraph).  It cannot see
 * a failed window: its NaN outputs and cgp_window_state do. */
int cgp_window_predict_cov_device(cgp_ctx *ctx, int M, const double *dxs, int include_noise, double *dmean, double *dcov,
                                  void *hip_stream);
/* cgp_window_sample: S sample paths per window at its M test points, out (nwin, S, M) = mean + C xi, where C is the lower
 * Cholesky factor of
 *   A = cov_latent (+ sigma_n^2 I when include_noise)  +  jitter_rel * mean(diag(cov_latent (+ sigma_n^2 I))) * I
 * and xi (nwin, S, M) are standard normals SUPPLIED BY THE CALLER (torch.randn on the device, numpy on the host): the library
 * holds no random state, a call is a pure function of its arguments, reproducible across runs and shardings.  xi = unit vectors
 * returns C's columns (+ mean).  jitter_rel >= 0; a dense grid under a smooth kernel makes cov_latent numerically singular, so
 * callers should pass 1e-6 (the first rung of GPy's jitchol) unless they know better.  There is no ladder: a window whose A
 * is still not positive definite gets NaN paths and info[w] = the 1-based failing pivot (0 otherwise; a window that had
 * failed in an earlier push reports pivot 1); info may be NULL.  The dense covariance is never written to the caller.  Returns
 * 0 or the 1-based index of the first such window; CGP_ESTATE / CGP_EINVAL (also S < 1, jitter_rel < 0 or NaN) / CGP_ECAPACITY
 * as cgp_window_predict_cov.  Blocks. */
int cgp_window_sample(cgp_ctx *ctx, int M, const double *xs, int S, const double *xi, int include_noise, double jitter_rel,
                      double *out, int *info);
/* Device-resident variant: five launches on hip_stream, no allocation, no synchronisation (capturable into a hipGraph);
 * dinfo (nwin ints on the device) may be NULL.  Returns 0 or an argument / state / runtime error; failed factorisations show
 * in dinfo and as NaN paths. */
int cgp_window_sample_device(cgp_ctx *ctx, int M, const double *dxs, int S, const double *dxi, int include_noise,
                             double jitter_rel, double *dout, int *dinfo, void *hip_stream);

/* ---- fp32 contexts: mixed-precision refinement of alpha and the predictive mean -----------------
 * After the single-precision factorisation: alpha_0 = L^-T L^-1 y from the factor, then `steps` times
 *   r = y - Ky alpha   in DOUBLE precision, Ky entries re-evaluated from X on the fly (never stored),
 *   alpha += L^-T L^-1 r   through the fp32 factor, alpha kept in double,
 * and mean = K*^T alpha with K* evaluated in double -- GPy's own form of the mean (gp_slip_node.py:48 m.predict: mu = k*^T
 * woodbury_vector).  One step takes the mean of a dense one- or two-dimensional window from ~1e-3 of the oracle to ~1e-6
 * (tests/fuzz/d1_fp32_error.py); variance and logML come from the factor as before.  steps = -1 (the default): the engine decides --
 * one step (two for windows of more than 1 024 samples, where a step contracts less); for every fit of a window of d <= 3 input dimensions (the RBF x Brownian kernel included: +40 % per call at
 * N = 1024, M = 599), and for d > 3 only for the fits whose factor shows a dense window (prior variance / geometric mean of
 * the pivots L_ii^2 >= 12: the unrefined mean's error follows that ratio, tests/fuzz/rho_vs_error.py) -- BASELINE configs[2] (d = 6,
 * ratio 3 ... 11.5) has no such fit and pays one launch whose workgroups return at once (not measurable: 0.696 ms per 64-fit
 * call either way); a call with such a fit pays the latency of one refinement (~0.27 ms at N = 1024) whatever their number.  0: never; 1..3: that many
 * steps for every fit of every fp32 call.  cgp_get_alpha then returns the refined alpha (double precision).  No effect on
 * CGP_F64 contexts, nor on windows of more than 13 000 samples (the solve keeps the window's alpha in LDS). */
int cgp_set_refine(cgp_ctx *ctx, int steps);

/* ---- per-kernel timing for the roofline line (bench.py) --------------------------------------
 * on = 1: every launch is bracketed by hipEvents on its stream; on = 2 + k: only the update launch of block
 * step k (the other launches of the schedule stay back to back, so the bracketed one runs as it does in an
 * untimed step); on = 0: off.  cgp_profile_read drains the events.
 * kernel index: 0 update(syrk/gemm+gram) 1 potf2(+inverse) 2 trmm 3 finalize(mean/var/logml) 4 alpha.
 * flops = algorithmic flops issued by those launches (DESIGN.md section "Kernels"). */
#define CGP_PROF_KERNELS 5
int cgp_profile_enable(cgp_ctx *ctx, int on);
int cgp_profile_read(cgp_ctx *ctx, double ms[CGP_PROF_KERNELS], double flops[CGP_PROF_KERNELS],
                     long long launches[CGP_PROF_KERNELS]);

/* ---- GpPredictor host arithmetic (gp_predictor/src/gp_predictor.cpp) --------------------------
 * cgp_llh_to_enu: GpPredictor::llh_to_enu (gp_predictor.cpp:144-178). */
int cgp_llh_to_enu(double lat, double lon, double h, const double init_llh[3], const double init_ecef[3],
                   double enu[3]);
/* cgp_predict_stop: the covariance look-ahead of GpPredictor::GPCallBack (gp_predictor.cpp:58-130)
 * on the SetStopping response arrays (core_navigation/srv/SetStopping.srv:3-7).  HvecData has 60
 * entries; h_bug_compatible != 0 unpacks it with the reference's r*4+c indexing
 * (gp_predictor.cpp:38-42), 0 with r*15+c.  Outputs: *fired (threshold crossed), *stop_cmd (the
 * Float64 published on stop_cmd, :107-118), *i_out (odometry steps consumed), *xy_err. */
int cgp_predict_stop(const double *mean, const double *sigma, int M, const double *PvecData,
                     const double *QvecData, const double *STMvecData, const double *HvecData,
                     const double pos_llh[3], double arrival_time, double now, double threshold,
                     int h_bug_compatible, const double init_llh[3], const double init_ecef[3],
                     int *fired, double *stop_cmd, int *i_out, double *xy_err);

/* cgp_predict_stop_batch: the same look-ahead for `ntraj` trajectories at once ON THE DEVICE (one
 * wavefront per trajectory): mean/sigma (ntraj, M), P/Q/STM (ntraj, 225), HvecData
 * (ntraj, 60), pos_llh (ntraj, 3), arrival_time/now (ntraj); outputs (ntraj) each.  Host buffers. */
int cgp_predict_stop_batch(cgp_ctx *ctx, int ntraj, int M, const double *mean, const double *sigma,
                           const double *PvecData, const double *QvecData, const double *STMvecData,
                           const double *HvecData, const double *pos_llh, const double *arrival_time,
                           const double *now, double threshold, int h_bug_compatible, const double init_llh[3],
                           const double init_ecef[3], int *fired, double *stop_cmd, int *i_out, double *xy_err);

/* One GpPredictor::GPCallBack (gp_predictor.cpp:17-132) through the C++ class in
 * csrc/gp_predictor.h with an in-process NodeHandle: the SetStopping service answers with the given
 * arrays, the clock returns `arrival_time` on the first read (:22) and `now` afterwards (:107), and
 * whatever the node publishes on stop_cmd is returned.  Used by the replay harness and the tests. */
int cgp_gppredictor_callback(const double *mean, const double *sigma, int M, const double *PvecData,
                             const double *QvecData, const double *STMvecData, const double *HvecData,
                             const double pos_llh[3], double arrival_time, double now,
                             int h_bug_compatible, int *published, double *stop_cmd);

/* ---- producer side: slip + recording-window state machine of CoreNav::Update -----------------
 * (core_navigation/src/CoreNav.cpp:176,244-330; stopCallback :755-759; getCmdData :794-816).
 * cgp_recorder_update = one 10 Hz odometry update: wheel ground speeds {FL, FR, BL, BR}, INS forward
 * speed, commanded speed.  Returns 1 when a GP_Input window is published this tick; it is then
 * copied to time_out / slipwin_out and *n_out = its length.  If the window is longer than `cap` the
 * first cap entries are copied, *n_out still holds the full length and CGP_ECAPACITY is returned
 * (never a silent truncation).  *slip_out = the tick's slip value (may be NULL). */
typedef struct cgp_recorder cgp_recorder;
cgp_recorder *cgp_recorder_create(void);
void cgp_recorder_destroy(cgp_recorder *rec);
int cgp_recorder_update(cgp_recorder *rec, const double wheel_vel[4], double vlin, double cmd_x, double *slip_out,
                        double *time_out, double *slipwin_out, int cap, int *n_out);
void cgp_recorder_stop_cmd(cgp_recorder *rec, double cmd_stop);
void cgp_recorder_cmd(cgp_recorder *rec, double cmd_x);
/* state[8] = {odomUptCount, startRecording, stopRecording, gp_flag, first_driving_flag,
 *             new_stop_data_arrived_, skipped_windows, cmd_stop_} */
void cgp_recorder_state(const cgp_recorder *rec, double state[8]);

#ifdef __cplusplus
}
#endif
#endif /* CORENAV_GP_H_ */
