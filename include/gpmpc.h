/*
 * gpmpc.h -- C ABI of the MI355X-native GP-MPC rollout library (libgpmpc_hip.so).
 *
 * Drop-in boundary for the hot path of Thiagodcv/gaussian-process-mpc.  The
 * reference has no FFI of its own (it is pure Python on torch); the entry
 * points below are what a binding for this path has to call, and each one
 * names the reference interface it replaces (paths relative to the upstream
 * repository root).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - All matrices are row-major fp64.  "dev" = device (HBM) pointer, "host" =
 *    host pointer.  The caller owns every buffer; the library never frees or
 *    reallocates caller memory and keeps no global state besides the pack (exceptions: the opt-in timing
 *    counters of gpmpc_timing_enable, process-wide behind a mutex; GPMPC_* tuning environment variables, read once
 *    per pack at gpmpc_pack_create / gpmpc_pack_reload_tuning, never on the per-call path).
 *  - A pack lives on the HIP device that was current when it was created; every entry point that takes a pack
 *    returns GPMPC_E_DEVICE if the calling thread's current device differs (it never switches devices itself).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *    All work is enqueued asynchronously on it; nothing synchronises the
 *    device.  Calls are re-entrant across streams and host threads as long as workspaces differ: a pack is only read by a
 *    rollout, and what a pack OWNS -- its private streams / events (graph replay, the concurrent sub-batches of a mid-size
 *    batch), the captured graphs and the staging buffers of gpmpc_objective_gradient -- is guarded by a per-pack host lock
 *    (lazy creation, a stream capture from begin to end, a fork / join of a split launch, the callback entry are each one
 *    critical section).  ONE buffer of the pack is written by a rollout: the step-1 weights (ds x Np^2 doubles: 134 MB at N = 2048,
 *    ds = 4; 805 MB at N = 4096, ds = 6) that gpmpc_rollout allocates the first time a call takes horizon step 1 as a quadratic
 *    form (two-launch form, distinct lambdas, B >= 8, or GPMPC_STEP1_QUAD=1) and refills, on that call's stream, after a build
 *    or gpmpc_pack_set_noise.  The fill is followed by an event that every such call on any stream waits for before it launches,
 *    so the re-entrancy above holds; the build or set that made the weights stale must, as ever, be ordered before the rollouts
 *    on every stream.  If the allocation fails, the call runs as it did without the weights (the pair kernel's own step-1
 *    variant; no error is returned, gpmpc_last_error names the failed allocation) and is not retried until the next build.
 *    Functions that MODIFY a pack (build, resize, enable_fullcov, reload_tuning, autotune, destroy) must
 *    not run concurrently with anything else on that pack.
 *    HOST arrays (hyper-parameters, cost parameters) are consumed before the call
 *    returns -- they travel as kernel arguments --: the caller may free or overwrite
 *    them at once, whatever `stream` is waiting for.  DEVICE buffers must stay valid
 *    until the work enqueued on `stream` has run.
 *  - Return value: 0 on success, a negative GPMPC_E_* code otherwise.  No
 *    exception crosses the ABI.  NaNs produced by the arithmetic (negative
 *    variances, log of a non-positive determinant) are passed through, as in
 *    the reference.
 *  - Dimensions: D = ds + da <= GPMPC_MAX_D, ds <= GPMPC_MAX_DS.
 */
#ifndef GPMPC_H
#define GPMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMPC_MAX_D   8
#define GPMPC_MAX_DS  8

#define GPMPC_OK            0
#define GPMPC_E_ARG        -1   /* bad argument (NULL pointer, dimension out of range) */
#define GPMPC_E_ALLOC      -2   /* device allocation failed */
#define GPMPC_E_LAUNCH     -3   /* a HIP call or kernel launch failed */
#define GPMPC_E_WORKSPACE  -4   /* workspace too small */
#define GPMPC_E_STATE      -5   /* pack not built */
#define GPMPC_E_DEVICE     -6   /* the calling thread's current HIP device is not the one the pack was created on */

/* flags for gpmpc_rollout / gpmpc_moment_match */
#define GPMPC_WANT_GRAD      1u   /* also produce d cost / d U (rollout) or input Jacobians (moment_match) */
#define GPMPC_USE_GRAPH      4u   /* gpmpc_rollout: replay the launches of the rollout as one hipGraph.  The caller promises
                                     that the pointer arguments (inputs, outputs, workspace) are the same buffers on every
                                     call of one shape with this flag; a changed argument captures anew (4 shapes are kept
                                     per pack).  For launch-latency-bound small batches (B = 1 solver loops). */
#define GPMPC_FP32_ACCUM     8u   /* gpmpc_rollout, objective only: N^2 products and their sum in fp32 (exponent / exp in fp64) */
#define GPMPC_FP32_ALL      16u   /* gpmpc_rollout, objective only: transformed points, exponent, exp and sum in fp32.
                                     Both exist for the fp64-vs-fp32 tolerance sweep of BASELINE config 3: the variance is a
                                     cancelling sum and single precision FAILS the 1e-4 tolerance (profiles/r01/fp32_sweep.txt) */
#define GPMPC_COV_BUG_COMPAT 2u   /* cross-covariance with the reference's transposed cross term
                                     (src/tools/uncertainty_prop.py:446) instead of the consistent one */

typedef struct gpmpc_pack gpmpc_pack;   /* opaque: device-resident GP state */

/* Library / device probe.  Returns the number of visible HIP devices (>= 0) or a negative code. */
int gpmpc_device_count(void);
const char* gpmpc_version(void);
const char* gpmpc_last_error(void);     /* thread-local text of the last failing HIP call */

/* ---------------------------------------------------------------------------
 * GP state ("pack").  Replaces the per-call constant work of
 *   mean_prop_torch      src/tools/uncertainty_prop.py:324-327 (beta = Ky_inv @ y)
 *   variance_prop_torch  src/tools/uncertainty_prop.py:392-399 (Lambda_part, Ky_inv - beta beta^T)
 * and holds what Dynamics/GaussianProcessRegression hold on the device
 * (src/dynamics.py:33-37, src/gpr.py:24-36): X_train shared by all ds GPs,
 * per GP: beta, lambdas, sigma_f and the folded weight matrix
 *   M_a[i][j] = sym(Ky_inv_a - beta_a beta_a^T)[i][j] * sigma_f_a^4
 *               * exp(-1/4 (x_i-x_j)^T Lambda_a^-1 (x_i-x_j))
 * stored upper-triangular with off-diagonal weight 2.
 * ------------------------------------------------------------------------- */
int gpmpc_pack_create(gpmpc_pack** out, int n_train, int state_dim, int action_dim);
int gpmpc_pack_destroy(gpmpc_pack* pack);
/* Re-use the pack for n_train points when the padded size (multiple of 64) is unchanged -- GPMPC_E_ARG otherwise --; the pack
 * is "not built" until the next gpmpc_pack_build*; captured launch sequences (GPMPC_USE_GRAPH, gpmpc_objective_gradient) stay
 * valid (no rollout launch depends on the unpadded size).  For the closed loop, where Dynamics.append_train_data adds one
 * observation per step (src/simulator.py:55): no allocation per step. */
int gpmpc_pack_resize(gpmpc_pack* pack, int n_train);
/* Re-read the GPMPC_* tuning environment variables for this pack (they are otherwise read once, at
 * gpmpc_pack_create) and drop its captured graph.  For A/B runs and tests; no reference counterpart. */
int gpmpc_pack_reload_tuning(gpmpc_pack* pack);
/* Number of hipGraph captures gpmpc_rollout(GPMPC_USE_GRAPH) has done for this pack (up to 4 captured call shapes are
 * kept per pack, least recently used replaced).  Diagnostic; no reference counterpart. */
long long gpmpc_pack_graph_captures(const gpmpc_pack* pack);
/* Number of captures of the callback graph of gpmpc_objective_gradient this pack has done.  A refill of the pack (gpmpc_pack_resize /
 * gpmpc_pack_build*) keeps that graph unless the shared-lambda state flips; a new horizon, flags or cost re-capture.  Diagnostic. */
long long gpmpc_pack_callback_captures(const gpmpc_pack* pack);

/* A few host values (<= 512 bytes, a multiple of 4) -> device memory, ordered on `stream`, consumed before the call returns (they travel
 * as kernel arguments: no pageable-memory copy, no synchronisation).  The closed loop appends ONE observation per step
 * (src/simulator.py:55 -> src/gpr.py:109-119): the new input row and targets go straight into capacity-padded device buffers. */
int gpmpc_store_host(void* dst_dev, const void* src_host, size_t bytes, void* stream);

/* Build K_f, K_y = K_f + noise_var*I for one GP on the device
 * (GaussianProcessRegression.build_Ky_inv_mat, src/gpr.py:163-170; the inverse at :171 is
 * taken by the caller).  X dev [n][D]; lambdas host [D]; Kf, Ky dev [n][n] (Kf may be NULL).
 * noise_var is the value added on the diagonal (the reference adds float32(sigma_n^2)). */
int gpmpc_build_ky(int n, int D, const double* X_dev, const double* lambdas_host,
                   double sigma_f, double noise_var, double* Kf_dev, double* Ky_dev, void* stream);

/* Fill the pack.  X dev [N][D]; Y dev [N][ds] (column a = targets of GP a, as
 * Dynamics.append_train_data stores them, src/dynamics.py:51-60); Ky_inv dev [ds][N][N]
 * (src/gpr.py:171); lambdas host [ds][D]; sigma_f host [ds]. */
int gpmpc_pack_build(gpmpc_pack* pack, const double* X_dev, const double* Y_dev,
                     const double* Ky_inv_dev, const double* lambdas_host,
                     const double* sigma_f_host, void* stream);

/* Same for inverses that are NOT packed [ds][N][N]: row stride `ld` (>= N) and the stride `gp_stride` from one GP's matrix to
 * the next, both in doubles.  gp_stride = 0: ONE matrix for every GP (GPs fed the same inputs under identical hyper-parameters
 * have identical Ky_inv -- every experiment of the reference, src/experiments/pretrain_uncertainty.py:100-105 -- and a capacity-padded
 * buffer that grows by one observation per Simulator step, src/simulator.py:55, is read in place instead of being copied). */
int gpmpc_pack_build_strided(gpmpc_pack* pack, const double* X_dev, const double* Y_dev, const double* Ky_inv_dev,
                             size_t ld, size_t gp_stride, const double* lambdas_host, const double* sigma_f_host, void* stream);

/* Same, with beta given instead of the targets: beta dev [N][ds] (column a = beta_a), as the callers of
 * variance_prop_torch / covariance_prop_torch hold it (src/tools/uncertainty_prop.py:341, :402).
 * Ky_inv may be NULL: the weight matrices are then zero and only means and cross-covariances
 * (which need beta alone) are meaningful. */
int gpmpc_pack_build_beta(gpmpc_pack* pack, const double* X_dev, const double* beta_dev,
                          const double* Ky_inv_dev, const double* lambdas_host,
                          const double* sigma_f_host, void* stream);

/* Linear nominal model (no reference counterpart: src/dynamics.py:64 leaves nominal models out of the rollout).  GP a then models
 * the residual of m_a(z) = weights[a] . z + bias[a], z = (x, u): weights host [ds][D], bias host [ds], copied into device memory owned by
 * the pack before the call returns.  Both NULL clears the model; exactly one NULL is GPMPC_E_ARG.
 *  - The pack is "not built" afterwards (GPMPC_E_STATE) until the next gpmpc_pack_build*.  gpmpc_pack_build and
 *    gpmpc_pack_build_strided take the RAW targets and form beta from Y - X weights^T - bias on the device; gpmpc_pack_build_beta takes
 *    beta as given (the caller has already removed the nominal model from the targets).  gpmpc_pack_resize keeps the model.
 *  - gpmpc_rollout (plain and GPMPC_USE_GRAPH), gpmpc_rollout_jac and gpmpc_objective_gradient propagate
 *    mu' = mu_g + n . u + c,  var' = var_g + sum_k n_k^2 s_k + 2 sum_k n_k s_k dmu_g/du_k  (exact for a linear model) with the matching
 *    step Jacobians, in the two-launch form (head kernel + pair kernel per horizon step): gpmpc_plan_describe appends "nominal=1".
 *  - Switching the model on or off drops the captured graphs and the measured plans of the pack; new coefficients of a model that
 *    stays on do not (the kernels read them from device memory).
 *  - gpmpc_rollout_fullcov, gpmpc_moment_match and the GPMPC_FP32_* modes do not know the model: GPMPC_E_STATE on a nominal pack,
 *    with the reason in gpmpc_last_error. */
int gpmpc_pack_set_nominal(gpmpc_pack* pack, const double* weights_host, const double* bias_host, void* stream);
/* 1: a nominal model is set (its coefficients are copied to weights_host / bias_host where these are not NULL), 0: none; GPMPC_E_ARG. */
int gpmpc_pack_get_nominal(const gpmpc_pack* pack, double* weights_host, double* bias_host);

/* Noise model of the rollout, shared by all trajectories of a call (the reference hard-codes the first two, src/dynamics.py:148,162, and
 * has no third):
 *     init_cov    host [ds][ds], symmetric   default 1e-3 I          covariance of the start state.  gpmpc_rollout and everything on top of it
 *                                                                    use its diagonal (stored as vars[b][0][:]); gpmpc_rollout_fullcov the whole
 *                                                                    matrix (stored as covs[b][0])
 *     action_var  host [da]                  default float32(1e-3)   variance of input j at every step
 *     process_var host [ds]                  default 0               added to the predicted variance of state a at every step t >= 1:
 *                                                                    var_a = (sf_a^2 + w_a) - T - mu^2, in the full-covariance rollout on the
 *                                                                    diagonal of Sigma_t.  An additive constant: no Jacobian changes.
 * A NULL part is reset to its default; all three NULL restores the defaults (with which every call returns what it returned before this
 * entry point existed, bit for bit).  The values live in ONE device buffer owned by the pack, allocated and filled with the defaults by
 * gpmpc_pack_create and kept by gpmpc_pack_resize; the kernels read them from there, never as kernel arguments, and there is no variant
 * of any kernel for a model that is set: a set drops no captured graph and no measured plan, and a new init_cov before every solve replays
 * the one captured graph (gpmpc_pack_callback_captures stays as it is).  The host arrays are consumed before the call returns; the copy is
 * enqueued on `stream`.  set belongs to the functions that MODIFY a pack: the caller orders it against rollouts on other streams.
 * (Up to two launches carry the values; if one fails -- GPMPC_E_LAUNCH --, gpmpc_pack_get_noise still reports what the device holds.)
 * GPMPC_E_ARG with a text in gpmpc_last_error, the pack left as it was and nothing enqueued: a non-finite value; a negative diagonal entry
 * of init_cov; a negative entry of action_var or process_var; |P_kl - P_lk| > 1e-12 max |P| (else the mean of each off-diagonal pair is
 * stored).  Zero variances are legal (an exactly known start state or input: B_k = 1 / lambda_k).
 * gpmpc_moment_match takes S from its caller and does not read the model.  Not provided: a different init_cov per trajectory of a batch, a
 * full process-noise matrix, gradients with respect to the noise parameters, state feedback inside the moment-matched prediction (the
 * linearised rule has it: "Linearised propagation, full covariance"). */
int gpmpc_pack_set_noise(gpmpc_pack* pack, const double* init_cov_host, const double* action_var_host, const double* process_var_host,
                         void* stream);
/* The three parts into the arrays that are not NULL.  1: some part differs from its default, 0: none does; GPMPC_E_ARG. */
int gpmpc_pack_get_noise(const gpmpc_pack* pack, double* init_cov_host, double* action_var_host, double* process_var_host);

/* Allocate and maintain the cross-covariance weight matrices (one N x N matrix per GP pair a < b): needed by
 * gpmpc_rollout_fullcov and by the analytic cross-covariance Jacobians of gpmpc_moment_match.  Without it
 * cross-covariances are evaluated by a direct N^2 kernel, forward only. */
int gpmpc_pack_enable_fullcov(gpmpc_pack* pack, void* stream);

/* Inspection for tests / bindings.  gpmpc_pack_export copies into caller buffers (either may be NULL):
 * beta_out dev [ds][n_padded] (beta_a = Ky_inv_a y_a, zero padded); weights_out dev
 * [ds][n_padded][n_padded], element (i <= j) of M_a at [a][j][i], zero elsewhere. */
int gpmpc_pack_dims(const gpmpc_pack* pack, int* n_train, int* n_padded, int* state_dim, int* action_dim);
/* 1 if the last gpmpc_pack_build* found bit-identical length-scales for every GP (the setting of all of the reference's
 * experiments, e.g. src/experiments/pretrain_uncertainty.py:100-105): gpmpc_rollout then evaluates exponent and exp once
 * per pair for a group of GPs.  0 otherwise, negative on error.  Diagnostic; no reference counterpart. */
int gpmpc_pack_shared_lambda(const gpmpc_pack* pack);
int gpmpc_pack_export(const gpmpc_pack* pack, double* beta_out, double* weights_out, void* stream);

/* ---------------------------------------------------------------------------
 * Single-step exact moment matching for nq Gaussian inputs N(u_q, S_q), all ds GPs.
 * Replaces mean_prop_torch / variance_prop_torch / covariance_prop_torch
 * (src/tools/uncertainty_prop.py:296-338, :341-399, :402-465).  S may be a full
 * symmetric positive-definite matrix.
 *   u dev [nq][D], S dev [nq][D][D]
 *   out_mean dev [nq][ds]; out_var dev [nq][ds]
 *   out_cov  dev [nq][ds][ds] or NULL: full predictive covariance (diagonal = out_var,
 *            off-diagonal = cross-covariances; flag GPMPC_COV_BUG_COMPAT selects the
 *            reference's transposed cross term)
 *   out_l    dev [nq][ds][N] or NULL: the vector l of mean_prop_torch's second return value
 *            (l_i = c_m exp(-1/2 v_i^T B v_i), src/tools/uncertainty_prop.py:335-336)
 *   with GPMPC_WANT_GRAD (the first four non-NULL):
 *     dmean_du dev [nq][ds][D], dmean_dS dev [nq][ds][D][D] (symmetrised),
 *     dvar_du  dev [nq][ds][D], dvar_dS  dev [nq][ds][D][D] (symmetrised),
 *     dcov_du  dev [nq][ds][ds][D], dcov_dS dev [nq][ds][ds][D][D] or both NULL: Jacobians of the full covariance,
 *              diagonal (a, a) entries (= dvar_du / dvar_dS) included.  On a pack with gpmpc_pack_enable_fullcov and in the
 *              consistent form the pair kernel's cross units supply the off-diagonal entries; without the cross weights, or
 *              with GPMPC_COV_BUG_COMPAT, the direct N^2 kernel does (in that form [a][b] != [b][a], both are written).
 *              GPMPC_E_STATE only without GPMPC_WANT_GRAD or without out_cov; GPMPC_E_ARG if only one of the two is given.
 * gpmpc_moment_match_describe writes what a call of this shape would launch, as "key=value" words, and launches nothing:
 *   tiling=IxJ (tile of the pair kernel's work list) sbf=0|1 (scalar-broadcast kernel) tb=1|2 (queries per workgroup)
 *   waves= nunits= nwork= cross=pair|direct|none (who evaluates the cross-covariances) workspace= (the bytes this very call
 *   needs: at most gpmpc_moment_match_workspace_bytes, which covers every call of nq queries).  flags as for the call plus
 *   GPMPC_DESCRIBE_WANT_COV for a call with out_cov.  out_bytes >= 128.
 * ------------------------------------------------------------------------- */
#define GPMPC_DESCRIBE_WANT_COV 0x100u
int gpmpc_moment_match_describe(const gpmpc_pack* pack, int nq, unsigned flags, char* out, size_t out_bytes);
size_t gpmpc_moment_match_workspace_bytes(const gpmpc_pack* pack, int nq);
int gpmpc_moment_match(const gpmpc_pack* pack, int nq, const double* u_dev, const double* S_dev,
                       unsigned flags, double* out_mean, double* out_var, double* out_cov, double* out_l,
                       double* dmean_du, double* dmean_dS, double* dvar_du, double* dvar_dS,
                       double* dcov_du, double* dcov_dS,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Risk-sensitive cost (RiskSensitiveMPC.cost_torch, src/mpc.py:156-200).
 * gamma == 0 selects the risk-neutral limit tr(Q Sigma) + e^T Q e (the reference
 * divides by gamma and cannot evaluate it).
 * ------------------------------------------------------------------------- */
typedef struct gpmpc_cost_params {
    double gamma;
    double Q[GPMPC_MAX_DS * GPMPC_MAX_DS];            /* [ds][ds] row-major in the leading ds*ds entries */
    double R[GPMPC_MAX_D * GPMPC_MAX_D];              /* [da][da] */
    double R_delta[GPMPC_MAX_D * GPMPC_MAX_D];        /* [da][da], used when has_R_delta != 0 */
    double x_ref[GPMPC_MAX_DS];
    double u_ref[GPMPC_MAX_D];
    double last_u[GPMPC_MAX_D];                       /* last_traj[0:da], src/mpc.py:192 */
    int has_R_delta;
    int schedule_id;                                  /* 0: none.  Else the id of a cost schedule (below): x_ref and u_ref above are then IGNORED */
} gpmpc_cost_params;

/* ---------------------------------------------------------------------------
 * Cost schedule: time-varying references and a terminal weight (no reference counterpart: RiskSensitiveMPC holds one x_ref, one u_ref
 * and one Q, src/mpc.py:20-60).  A schedule is ONE device buffer owned by the library, addressed by a positive id that travels in
 * gpmpc_cost_params::schedule_id.  Its device layout, in doubles, fixed at creation (the device pointer of an id never changes):
 *     x_ref [H_max + 1][ds] | u_ref [H_max][da] | Q_f [ds][ds] | has_Qf, H     (the two flags stored as doubles, exactly: every load stays 8-byte aligned)
 * Meaning in a cost of horizon H_call <= H (the H of the last set; a shorter call uses the leading rows):
 *     state term of step i (0 <= i <= H_call):  e = mu_i - x_ref[i], weight Q_f where i == H_call and has_Qf, else Q of the struct -- in the
 *         quadratic form, the log-determinant and the gamma == 0 trace alike;
 *     input term of step j (0 <= j < H_call):   d = U_j - u_ref[j];   the R_delta term and last_u are as without a schedule.
 * The contents are read from device memory by the cost kernels, never passed as kernel arguments: a captured launch sequence
 * (GPMPC_USE_GRAPH, gpmpc_objective_gradient) keys on the id -- it is part of the struct -- and NOT on the contents, so a set between two
 * replays takes effect without a new capture.  Every entry point that takes cost_host resolves the id on the host first and returns
 * GPMPC_E_ARG, with a text in gpmpc_last_error, before any launch or graph replay, on an unknown or destroyed id, a ds / da that is not the
 * call's, or a call horizon above the schedule's H (GPMPC_E_DEVICE: the schedule lives on another device).
 * The table of ids is guarded by a host lock: create / destroy / set / get and calls that use schedules may run on concurrent host
 * threads.  A set is ordered on ITS stream: work on another stream that reads the same id while it is being rewritten is the caller's race,
 * as with U.  Ids count up from 1 and are not reused within a process.
 *   create   H_max >= 1, ds in 1..GPMPC_MAX_DS, da in 0..GPMPC_MAX_D; the buffer starts as zeros with H = 0 (unusable until the first set).
 *   destroy  waits for the device, then frees the buffer (GPMPC_E_DEVICE, nothing freed, where the current device is not the schedule's).
 *   set      x_ref_host [H + 1][ds]; u_ref_host [H][da] or NULL = zeros; Q_terminal_host [ds][ds] or NULL = no terminal weight (general: it
 *            need be neither symmetric nor diagonal).  H in 1..H_max, every value finite: GPMPC_E_ARG with a text otherwise, before anything
 *            is enqueued.  The host arrays are consumed before the call returns: they travel as kernel arguments in pieces of 512 bytes (the
 *            mechanism of gpmpc_store_host and gpmpc_pack_set_nominal, internally gpmpc_upload_small).  A refused or failed set leaves the
 *            schedule's H and terminal-weight flag as they were.
 *   set_dev  the same from device arrays, copied in stream order without the host (a closed loop that rolls its window on the device); the
 *            values cannot be checked for finiteness.
 *   get      any of the outputs may be NULL; *dev_out is the buffer (layout above). */
int gpmpc_cost_schedule_create(int H_max, int state_dim, int action_dim, int* id_out);
int gpmpc_cost_schedule_destroy(int id);
int gpmpc_cost_schedule_set(int id, int H, const double* x_ref_host, const double* u_ref_host, const double* Q_terminal_host, void* stream);
int gpmpc_cost_schedule_set_dev(int id, int H, const double* x_ref_dev, const double* u_ref_dev, const double* Q_terminal_dev, void* stream);
int gpmpc_cost_schedule_get(int id, int* H_max, int* state_dim, int* action_dim, int* H, int* has_Q_terminal, const double** dev_out);

/* Cost of B given trajectories with FULL covariance matrices (parity with cost_torch on
 * arbitrary, even non-symmetric, Sigma): means dev [B][H+1][ds], covs dev [B][H+1][ds][ds],
 * U dev [B][H][da] -> out_cost dev [B]. */
int gpmpc_cost(int B, int H, int state_dim, int action_dim, const gpmpc_cost_params* cost_host,
               const double* means_dev, const double* covs_dev, const double* U_dev,
               double* out_cost, void* stream);

/* The same cost with its derivatives: what `curr_cost.backward()` (src/mpc.py:251) leaves in the graph of
 * cost_torch (src/mpc.py:179-198) -- d_means dev [B][H+1][ds], d_covs dev [B][H+1][ds][ds] (element [k][l] =
 * d cost / d Sigma_kl of a general, possibly non-symmetric Sigma), d_U dev [B][H][da] (input and input-rate terms).
 * The three derivative outputs are given together or all NULL. */
int gpmpc_cost_grad(int B, int H, int state_dim, int action_dim, const gpmpc_cost_params* cost_host,
                    const double* means_dev, const double* covs_dev, const double* U_dev,
                    double* out_cost, double* d_means, double* d_covs, double* d_U, void* stream);

/* ---------------------------------------------------------------------------
 * The hot path: B independent shooting rollouts + cost + gradient.
 * Replaces, for each trajectory b,
 *   Dynamics.forward_propagate_torch(H, x0[b], U[b])      src/dynamics.py:126-191
 *   RiskSensitiveMPC.cost_torch(...)                        src/mpc.py:156-200
 *   RiskSensitiveMPC.objective(x) / gradient(x)             src/mpc.py:202-255
 * (the reference handles one trajectory per call; B > 1 is the batched form).
 * Semantics kept: Sigma_0 = 1e-3 I (float64), action-noise variance float32(1e-3),
 * diagonal covariance propagation, no clamp of negative variances.
 *   x0 dev [B][ds]; U dev [B][H][da]
 *   out_means dev [B][H+1][ds]; out_vars dev [B][H+1][ds]  (either may be NULL)
 *   out_cost dev [B]; out_grad dev [B][H][da] (required with GPMPC_WANT_GRAD)
 * Mid-size batches (a few to a few dozen trajectories) are run as 2-4 concurrent sub-batches (2 when launched plainly) on
 * streams owned by the pack, forked from and joined back into `stream` with events (parallel branches of the graph under
 * GPMPC_USE_GRAPH): the caller still sees ONE call ordered on ONE stream, results are bit-identical to the unsplit launch,
 * and the workspace size reported below covers the sub-batches' slices.  Small and mid-size batches (up to ~4700 tile
 * workgroups per horizon step) are one kernel launch per horizon step; larger ones two (head + pair kernel).
 * ------------------------------------------------------------------------- */
size_t gpmpc_rollout_workspace_bytes(const gpmpc_pack* pack, int B, int H, unsigned flags);
/* Diagnostic (no reference counterpart): what a rollout call of this shape launches, as one line of text --
 * "form=<fused_staged|fused_sb|fused_sb_shared|head+pair_sb|head+pair_sbs|head+pair_staged|lowprec> kernel=<dominant kernel instance>
 *  tiling=<rows>x<cols> workgroups=<per horizon step> launches_per_step=<1|2> split=<concurrent sub-batches> ..." --
 * with GPMPC_USE_GRAPH in `flags` for the split a graph replay would use.  bench.py names its dominant kernel with it, the
 * parity tests check which kernel form a shape reaches.  out_bytes >= 64; returns 0 or GPMPC_E_ARG. */
int gpmpc_plan_describe(const gpmpc_pack* pack, int B, int H, unsigned flags, char* out, size_t out_bytes);
/* Plan selection that MEASURES (no reference counterpart).  The kernel form of a rollout call -- tiling, one or two launches per
 * horizon step or the whole-horizon kernel, trajectories per wave, concurrent sub-batches -- is chosen from thresholds measured on
 * one MI355X; this call times the candidate plans of ONE call shape (B, H, objective-only or with gradient; GPMPC_USE_GRAPH in
 * `flags`: as graph replays, else as plain launches) on THIS device with the pack's own data -- each candidate a warm-up and the best
 * of three timed blocks, on scratch buffers of its own -- and makes the pack remember the fastest (up to 16 shapes; the default plan
 * stays unless beaten by more than 2 %).  Every plan sums in a fixed order: results stay bit-reproducible per plan, and differ between
 * plans by rounding only.  Synchronous (tens of milliseconds); not to be called while other host threads use the pack.
 * `report` (optional): "name:fused=..,tiling=..,...:ms;..." per candidate, the winner marked with '*', the default first.
 * Returns the number of candidates timed (> 0) or a negative code.  gpmpc_pack_autotune_clear forgets every measured plan; so do
 * gpmpc_pack_reload_tuning and a gpmpc_pack_build that changes the "all GPs share their length-scales" property. */
int gpmpc_pack_autotune(gpmpc_pack* pack, int B, int H, unsigned flags, char* report, size_t report_bytes);
int gpmpc_pack_autotune_clear(gpmpc_pack* pack);
int gpmpc_rollout(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                  const gpmpc_cost_params* cost_host, unsigned flags,
                  double* out_means, double* out_vars, double* out_cost, double* out_grad,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Differentiable propagation: Dynamics.forward_propagate_torch (src/dynamics.py:126-191) returns tensors with the autograd
 * graph attached, and RiskSensitiveMPC.gradient back-propagates through it (src/mpc.py:218, :251).  The two entry points
 * below are the forward and the backward of that graph:
 *   gpmpc_rollout_jac   means / variances of B rollouts (no cost) + the step Jacobians
 *                       out_jac dev [B][H][2ds][2ds+da]: rows (mu_t, var_t), columns (mu_{t-1}, var_{t-1}, u_{t-1})
 *   gpmpc_rollout_vjp   g_means, g_vars dev [B][H+1][ds] (upstream gradients of every step's mean / variance; either
 *                       may be NULL = zero) -> out_gU dev [B][H][da], out_gx0 dev [B][ds] or NULL.
 * ------------------------------------------------------------------------- */
size_t gpmpc_rollout_jac_workspace_bytes(const gpmpc_pack* pack, int B, int H);
int gpmpc_rollout_jac(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                      double* out_means, double* out_vars, double* out_jac,
                      void* workspace, size_t workspace_bytes, void* stream);
int gpmpc_rollout_vjp(int B, int H, int state_dim, int action_dim, const double* jac_dev,
                      const double* g_means, const double* g_vars, double* out_gU, double* out_gx0, void* stream);

/* ---------------------------------------------------------------------------
 * Linear chance constraints on the state (no reference counterpart: RiskSensitiveMPC.constraints returns 0 and jacobian zeros,
 * src/mpc.py:257-267).  n_rows rows (a_r, b_r, kappa_r), a_r in R^ds, kappa_r >= 0, held at every horizon step t = 1..H (step 0 is the
 * current state and does not depend on U):
 *     g[t][r] = a_r . mu_t + kappa_r sd[t][r] - b_r  <= 0,    q = sum_k a_rk^2 var_tk,   sd = sqrt(q)
 * kappa = Phi^-1(p) keeps the row with one-sided probability p under the predicted Gaussian; kappa = 0 constrains the mean only.
 * The rollout does not clamp negative variances: q <= 0 gives sd = 0 and NO variance part in the derivative (the row is then its mean
 * part); a NaN mean or variance of step t makes every row of step t NaN -- values and derivatives, 0 * NaN included -- and no other step's.
 *     out_g    dev [B][H][n_rows]
 *     out_gjac dev [B][H * n_rows][H * da]: row (t-1) n_rows + r, column tau da + j = d g[t][r] / d u_tau[j]
 *              = sum_k a_rk S_t[k][c] + (kappa_r / (2 sd)) sum_k a_rk^2 S_t[ds+k][c],  S_t = d(mu_t, var_t)/dU;
 *              columns tau >= t are stored as exactly 0.0 (causality): EVERY element is written, the buffer needs no memset.
 * One forward-sensitivity sweep over the step Jacobians (k_rollout_constraints, csrc/constraints.hip), one lane per column.
 * ------------------------------------------------------------------------- */
#define GPMPC_MAX_CONS 16
typedef struct gpmpc_state_constraints {
    int n_rows;
    int reserved;
    double A[GPMPC_MAX_CONS * GPMPC_MAX_DS];          /* [n_rows][ds] row-major in the leading n_rows*ds entries */
    double b[GPMPC_MAX_CONS];
    double kappa[GPMPC_MAX_CONS];
} gpmpc_state_constraints;

/* Pure function of a propagated trajectory, like gpmpc_rollout_vjp: any pack, any plan, with a nominal model or without.
 * means_dev, vars_dev [B][H+1][ds] and jac_dev [B][H][2ds][2ds+da] as gpmpc_rollout_jac (or gpmpc_rollout_constrained) left them; the
 * state columns of step 1's Jacobian are never read.  out_gjac NULL: values only (jac_dev is then not read and may be NULL).
 * GPMPC_E_ARG -- before anything is launched -- on a NULL cons / means / vars / out_g, out_gjac without jac_dev, n_rows outside
 * 1..GPMPC_MAX_CONS, a negative or NaN kappa, dimensions out of range. */
int gpmpc_rollout_constraints(int B, int H, int state_dim, int action_dim, const gpmpc_state_constraints* cons_host,
                              const double* means_dev, const double* vars_dev, const double* jac_dev,
                              double* out_g, double* out_gjac, void* stream);

/* gpmpc_rollout and the constraints in ONE device pass: the launches of gpmpc_rollout of this shape (as one batch: no concurrent
 * sub-batches) with the step Jacobians kept in the workspace, then k_rollout_constraints on the same stream.  out_cost, out_grad,
 * out_means, out_vars are bit-identical to gpmpc_rollout's under the same plan.  Without GPMPC_WANT_GRAD: cost and constraint values
 * only (out_grad, out_gjac not written, may be NULL).  out_means / out_vars may be NULL (kept in the workspace).
 * flags: GPMPC_WANT_GRAD or 0; GPMPC_USE_GRAPH and the GPMPC_FP32_* modes are GPMPC_E_ARG (text in gpmpc_last_error). */
size_t gpmpc_rollout_constrained_workspace_bytes(const gpmpc_pack* pack, int B, int H, unsigned flags);
int gpmpc_rollout_constrained(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                              const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host, unsigned flags,
                              double* out_means, double* out_vars, double* out_cost, double* out_grad,
                              double* out_g, double* out_gjac, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * MPPI planner on the device (no reference counterpart; DESIGN.md section 3c, kernels in csrc/mppi.hip).  Per iteration: K perturbed copies
 * of the current plan (the "mean") are rolled out as ONE objective-only batch, the best sample seen is kept, the mean moves to the
 * softmin-weighted average of the samples.  With state constraints a sample is feasible when none of its rows is violated; while no sample
 * is feasible the score is the total violation (feasibility restoration).  n = H * action_dim, column c = t * action_dim + j.
 * ------------------------------------------------------------------------- */
#define GPMPC_MPPI_MAX_SAMPLES 4096
typedef struct gpmpc_mppi_params {
    int n_samples;                     /* K, 1..GPMPC_MPPI_MAX_SAMPLES */
    int iterations;                    /* >= 1 (gpmpc_mppi_solve) */
    double sigma[GPMPC_MAX_D];         /* standard deviation of the perturbation of input j, > 0, in the leading action_dim entries */
    double sigma_decay;                /* > 0: iteration `it` perturbs with sigma * sigma_decay^it */
    double beta;                       /* > 0: temperature = beta * (mean of the finite scores - smallest score) */
    unsigned long long seed;           /* Philox key */
    unsigned int call_index;           /* last word of the Philox counter: one value per solve gives every solve its own stream */
    unsigned int reserved;
    double lb[GPMPC_MAX_D];            /* box of input j; -inf / +inf allowed, lb <= ub */
    double ub[GPMPC_MAX_D];
} gpmpc_mppi_params;

/* out_U dev [K][n]: out_U[k][c] = clamp(mean[c] + sigma_j * sigma_decay^iteration * eps[k][c], lb_j, ub_j), j = c mod action_dim; row 0 is
 * mean itself, bit for bit (its noise is generated and discarded).  eps is standard normal and a pure function of (seed, call_index,
 * iteration, element e = k * n + c): Philox4x32-10 with key (seed low, seed high) and counter (p low, p high, iteration, call_index),
 * p = e / 2, gives the words w0..w3; u1 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1/2) * 2^-53, u2 likewise from (w2, w3); Box-Muller with
 * r = sqrt(-2 ln u1): even e takes r cos(2 pi u2), odd e r sin(2 pi u2).  Every element of out_U is written.
 * mean dev [n].  out_x0_batch dev [K][state_dim] or NULL: x0 dev [state_dim] repeated K times, the start states of the rollout (x0 and
 * state_dim are not looked at otherwise).  params->iterations is not used here.
 * GPMPC_E_ARG -- before anything is launched, text in gpmpc_last_error -- on n_samples outside 1..GPMPC_MPPI_MAX_SAMPLES, a sigma, beta
 * or sigma_decay that is not positive (NaN included), lb > ub, iteration < 0, dimensions out of range. */
int gpmpc_mppi_sample(int H, int state_dim, int action_dim, const gpmpc_mppi_params* params_host, int iteration,
                      const double* mean_dev, const double* x0_dev, double* out_U, double* out_x0_batch, void* stream);

/* One update from an evaluated batch.  U dev [K][n]; cost dev [K]; g dev [K][H][n_rows] or NULL with n_rows = 0 (no constraints).
 *   v_k = sum over (t, r) of max(g, 0) (0 without constraints); a sample with a NaN in cost or g is dead; feasible = alive and v_k == 0.
 *   Candidates: the feasible samples, score s_k = cost_k -- or, when none is feasible, the alive samples, s_k = v_k.
 *   k* = the candidate of smallest score, lowest index on ties; its key is (0, cost) when feasible, else (v, cost).
 *   best_out [2 + n] = (key, plan) of k* where that key is lexicographically STRICTLY smaller than best_in's, else best_in.  best_in and
 *     best_out must be different buffers (every workgroup decides from the old key); a search starts from (+inf, +inf, start plan).
 *   T = beta * (mean of the finite scores - s_min); w_k = exp(-(s_k - s_min) / T) for finite scores, 0 otherwise; where T is not a positive
 *     finite number, w_k = 1 on the candidates with s_k == s_min, 0 elsewhere.  mean dev [n] <- sum w_k U_k / sum w_k (written, not read).
 *   No sample alive: mean is not touched, best_out = best_in.
 *   out_trace dev [6] = (best violation, best cost, samples feasible, samples alive, s_min, T); (., ., 0, 0, +inf, 0) with none alive.
 * Every sum has a fixed order (no atomics): results are bit-reproducible and do not depend on the grid. */
int gpmpc_mppi_update(int n_samples, int H, int action_dim, int n_rows, double beta, const double* U_dev, const double* cost_dev,
                      const double* g_dev, double* mean_dev, const double* best_in, double* best_out, double* out_trace, void* stream);

/* The whole search on ONE stream without a host synchronisation: for each of params->iterations iterations gpmpc_mppi_sample,
 * gpmpc_rollout (cons NULL) or gpmpc_rollout_constrained, each with flags 0 and as they are, gpmpc_mppi_update.  A pack with a linear
 * nominal model needs nothing: the rollout honours it.  x0 dev [ds]; start dev [n] the plan the search starts from.
 *   out_U dev [n]: the best plan seen; out_best dev [2] its (violation, cost): feasible when the violation is 0;
 *   out_trace dev [iterations][6], one row per update.  The caller copies them out once, after the call.
 * GPMPC_E_ARG as gpmpc_mppi_sample plus iterations < 1 and bad constraint rows, before anything is launched; GPMPC_E_STATE on a pack that
 * is not built; GPMPC_E_WORKSPACE. */
size_t gpmpc_mppi_solve_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_mppi_params* params_host,
                                        const gpmpc_state_constraints* cons_host);
int gpmpc_mppi_solve(const gpmpc_pack* pack, int H, const double* x0_dev, const double* start_dev, const gpmpc_cost_params* cost_host,
                     const gpmpc_state_constraints* cons_host, const gpmpc_mppi_params* params_host, double* out_U, double* out_best,
                     double* out_trace, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Lock-step multi-start L-BFGS on the device (no reference counterpart; DESIGN.md section 3d, kernels in csrc/lbfgs.hip).  K bounded
 * quasi-Newton searches advance together: one tick is one evaluation of the K trial points (a B = K rollout with gradient) and one step
 * of every start's state machine (accept the trial point and form a new two-loop direction, or halve the step).  The rule is that of
 * multistart.lockstep_lbfgs with line_points = 1 and no patience.  n = H * action_dim, column c = t * action_dim + j, m = history.
 *
 * The state of a search is ONE caller-owned buffer of doubles (integers and flags are stored as doubles, exactly).  With
 * r(x) = x rounded up to a multiple of 32, the fields follow each other in this order, offsets in doubles:
 *     summary   32         [0] starts not yet done, [1] best = argmin F (lowest index on ties; 0 when no F is finite), [2] F[best],
 *                          [3] K, [4] n, [5] m; the rest 0
 *     plan      r(n)       X[best]
 *     F         r(K)       value at X (+inf: a start that is not alive)
 *     converged r(K)       1: done by gtol, ftol or min_step
 *     alive     r(K)       0: the first point had a non-finite value or gradient
 *     iters     r(K)       accepted steps
 *     ticks     r(K)       ticks this start has taken part in (the largest is the tick count of the host search)
 *     done      r(K)
 *     A         r(K)       step length of the current trial point
 *     cnt       r(K)       pairs stored, 0..m
 *     head      r(K)       ring slot of the NEWEST pair: pair j (0 = newest) is in slot (head + j) mod m
 *     rho       r(K m)     [K][m] by slot, 1 / (s . y)
 *     X, G, D   r(K n) x 3 point, gradient, direction, each [K][n]
 *     U         r(K n)     [K][H][action_dim]: the trial points XT (X where done) -- the batch the next evaluation reads
 *     S, Y      r(K m n) x 2   [K][m][n] by slot
 * gpmpc_lbfgs_state_bytes is 8 times the sum of these sizes.  Everything before G is what a caller reads back after a search.
 * ------------------------------------------------------------------------- */
#define GPMPC_LBFGS_MAX_STARTS 256
#define GPMPC_LBFGS_MAX_HISTORY 16
typedef struct gpmpc_lbfgs_params {
    int n_starts;                      /* K, 1..GPMPC_LBFGS_MAX_STARTS */
    int history;                       /* m, 1..GPMPC_LBFGS_MAX_HISTORY */
    double gtol;                       /* >= 0: done when max |g_free| <= gtol */
    double ftol;                       /* >= 0: done when an accepted step gains (F - ft) <= ftol max(|F|, |ft|, 1) */
    double c1;                         /* >= 0: Armijo constant, ft <= F + c1 G . (XT - X) */
    double min_step;                   /* >= 0: done when A max|D| < min_step after a halving */
    double lb[GPMPC_MAX_D];            /* box of input j; -inf / +inf allowed, lb <= ub */
    double ub[GPMPC_MAX_D];
} gpmpc_lbfgs_params;

/* 0 on K, history or dimensions out of range. */
size_t gpmpc_lbfgs_state_bytes(int n_starts, int H, int action_dim, int history);

/* The start step.  X0 dev [K][n]; cost dev [K], grad dev [K][n]: the evaluation of clip(X0).
 *   X = clip(X0); a start with a non-finite cost or gradient is not alive: F = +inf, G = 0, done.  cnt = 0, the pairs are zeroed.
 *   free = not((x <= lb and g > 0) or (x >= ub and g < 0));  D = -g on the free components, A = min(1, 1 / |g_free|_2);
 *   done where max |g_free| <= gtol (converged where also alive);  U = clip(X + A D), X where done.  Then the summary (below).
 * cost and grad BOTH NULL: only U = clip(X0) is written -- the batch the start evaluation runs on -- nothing else of the state.
 * out_x0_batch dev [K][state_dim] or NULL: x0 dev [state_dim] repeated K times (x0 and state_dim are not looked at otherwise).
 * GPMPC_E_ARG -- before anything is launched, text in gpmpc_last_error -- on n_starts or history out of range, a gtol, ftol, c1 or
 * min_step that is negative or NaN, lb > ub (or a NaN bound), dimensions out of range; GPMPC_E_WORKSPACE when state_bytes is too small. */
int gpmpc_lbfgs_start(int H, int state_dim, int action_dim, const gpmpc_lbfgs_params* params_host, const double* X0_dev,
                      const double* cost_dev, const double* grad_dev, const double* x0_dev, double* out_x0_batch,
                      void* state, size_t state_bytes, void* stream);

/* One tick from the evaluation (ft, gt) = (cost [K], grad [K][n]) of the batch U of the state.  Per start, s = U - X:
 *   a done start is left bit for bit as it is;
 *   ok = finite(ft) and finite(gt) and ft <= F + c1 G . s;
 *   ok:      y = gt - G; the pair (s, y, 1 / s.y) becomes the newest one where s.y > 1e-10 sqrt((s.s)(y.y)), cnt = min(cnt + 1, m);
 *            small = (F - ft) <= ftol max(|F|, |ft|, 1);  X, F, G = U, ft, gt;  iters += 1;
 *            D = the two-loop recursion over the cnt stored pairs, newest first, on the gradient masked by `free`, scaled by
 *            s.y / y.y of the newest pair where y.y > 0, masked again; where D . g_free is not < 0 or D is not finite: D = -g_free and
 *            cnt = 0;  A = 1 with pairs stored, else min(1, 1 / |g_free|_2);  done and converged where small or max |g_free| <= gtol;
 *   not ok:  A = A / 2; done and converged where A max|D| < min_step.  X, G and the pairs are not touched.
 *   U = clip(X + A D), X where done.  Then the summary: best, F[best], plan = X[best], the count of starts not done.
 * Every dot product is a per-lane sum over c = lane, lane + 64, ... in ascending order followed by a butterfly over the 64 lanes
 * (partner lane ^ 32, ^ 16, ... ^ 1); no atomics: the result of a start is bit-reproducible and independent of K.
 * GPMPC_E_ARG / GPMPC_E_WORKSPACE as gpmpc_lbfgs_start. */
int gpmpc_lbfgs_tick(int H, int action_dim, const gpmpc_lbfgs_params* params_host, const double* cost_dev, const double* grad_dev,
                     void* state, size_t state_bytes, void* stream);

/* The search on ONE stream without a host synchronisation.  With first_tick == 0: U = clip(X0), gpmpc_rollout, the start step.  Then
 * n_ticks times (gpmpc_rollout with GPMPC_WANT_GRAD over the K rows of U, as it is; the tick), then the summary.  first_tick > 0 continues
 * from the state a previous call left in the SAME workspace (X0 is not read): between two calls the caller may read the summary and stop
 * once no start is left.  A pack with a linear nominal model needs nothing: the rollout honours it.
 *   x0 dev [ds]; X0 dev [K][n].  The workspace BEGINS with the state (layout above); the caller copies what it needs from there.
 * GPMPC_E_ARG as gpmpc_lbfgs_start plus first_tick < 0 and n_ticks < 0, before anything is launched; GPMPC_E_STATE on a pack that is not
 * built; GPMPC_E_WORKSPACE. */
size_t gpmpc_lbfgs_solve_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_lbfgs_params* params_host);
int gpmpc_lbfgs_solve(const gpmpc_pack* pack, int H, const double* x0_dev, const double* X0_dev, const gpmpc_cost_params* cost_host,
                      const gpmpc_lbfgs_params* params_host, int first_tick, int n_ticks, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------
 * Constrained multi-start on the device: an augmented Lagrangian over gpmpc_rollout_constrained, the lock-step L-BFGS above as the inner
 * search (no reference counterpart; DESIGN.md section 3e, kernels in csrc/auglag.hip).  Per start: R = H * n_rows constraint values
 * g_i <= 0 (row i = (t-1) n_rows + r), multipliers lam_i >= 0, one penalty rho > 0.
 *     t_i = lam_i + rho g_i;   psi_i = t_i where t_i > 0, 0 where t_i <= 0 (a NaN passes through)
 *     M       = f + (1 / (2 rho)) sum_i (psi_i^2 - lam_i^2)          i ascending, one chain
 *     dM[c]   = df[c] + sum_i psi_i g_jac[i][c]                      i ascending, one FMA chain per column from 0, then added to df[c]
 * A row with psi_i == 0 is NOT READ: whatever an inactive row of g_jac holds cannot reach dM.  A non-finite f or g_i makes M non-finite
 * (the tick then rejects the trial point, the start step marks the start not alive); dM of such a start is unspecified.
 *
 * The state of a solve is ONE caller-owned buffer of doubles, fields rounded up to 32 as above (R = H * n_rows), in this order:
 *     summary   32         [0] alive starts not yet settled, [1] best = argmin of the incumbent keys (violation, cost), lowest index on
 *                          ties, [2] [3] that key, [4] K, [5] n, [6] R; the rest 0
 *     plan      r(n)       the incumbent plan of `best`
 *     rho       r(K)       penalty
 *     V_prev    r(K)       V of the last update (+inf before the first)
 *     v         r(K)       max_i max(g_i, 0) of the last outer step (+inf before the first)
 *     f         r(K)       cost of the last outer step (+inf before the first)
 *     inc_v     r(K)       incumbent key: 0 where the incumbent is feasible (v <= feas_tol), else its v; +inf: none yet
 *     inc_f     r(K)       incumbent key: its cost
 *     alive     r(K)       the inner search's alive flag (1 before the first search)
 *     settled   r(K)       1: at the last update V <= feas_tol and the inner search had converged
 *     lam       r(K R)     [K][R]
 *     inc_x     r(K n)     [K][n] incumbent plans (clip(X0) before the first outer step)
 * gpmpc_auglag_state_bytes is 8 times the sum of these sizes (0 on K, n_rows or dimensions out of range).
 * ------------------------------------------------------------------------- */
typedef struct gpmpc_auglag_params {
    gpmpc_lbfgs_params inner;          /* the inner search: n_starts = K, history, gtol, ftol, c1, min_step, the box */
    double rho0;                       /* > 0: the penalty every start begins with */
    double growth;                     /* >= 1: rho <- min(rho_max, growth rho) where V > shrink V_prev */
    double shrink;                     /* in (0, 1] */
    double rho_max;                    /* > 0 */
    double lam_max;                    /* >= 0: multipliers are clipped to [0, lam_max] */
    double feas_tol;                   /* >= 0: a point is feasible when max_i g_i <= feas_tol */
    int inner_ticks;                   /* >= 1: ticks of the inner search per outer iteration (gpmpc_auglag_solve) */
    int reserved;
} gpmpc_auglag_params;

size_t gpmpc_auglag_state_bytes(int n_starts, int H, int action_dim, int n_rows);

/* Merit value and gradient of K starts from one evaluation.  f dev [K], grad dev [K][n], g dev [K][R], g_jac dev [K][R][n] as
 * gpmpc_rollout_constrained left them; lam dev [K][R], rho dev [K] -> out_M dev [K], out_grad dev [K][n] (every element written; must
 * not alias an input).  One lane per column (k_al_merit); a start's result depends neither on K nor on the grid.
 * GPMPC_E_ARG on a NULL pointer, K < 1, n_rows outside 1..GPMPC_MAX_CONS, dimensions out of range. */
int gpmpc_auglag_merit(int n_starts, int H, int action_dim, int n_rows, const double* f_dev, const double* grad_dev, const double* g_dev,
                       const double* gjac_dev, const double* lam_dev, const double* rho_dev, double* out_M, double* out_grad, void* stream);

/* One outer step of every start (K = params->inner.n_starts) from the evaluation f dev [K], g dev [K][R] of the points X dev [K][n]:
 *   a start with a non-finite f or g is dead for this step: NOTHING of it is written;
 *   v = max_i max(g_i, 0);  key = (0, f) where v <= feas_tol, else (v, f);  the incumbent (inc_v, inc_f, inc_x) becomes (key, X) where
 *     the key is lexicographically STRICTLY smaller;  the fields v and f take (v, f);
 *   with update != 0, in this order:  V = max_i |max(g_i, -lam_i / rho)| (old lam, rho);  lam_i <- min(lam_max, max(0, lam_i + rho g_i))
 *     (old rho);  rho <- min(rho_max, growth rho) where V > shrink V_prev;  V_prev <- V;  settled <- V <= feas_tol and conv[k] != 0.
 *   conv dev [K] or NULL (= 0 everywhere): the `converged` field of the inner search at entry.
 * Then the summary and the plan (k_al_finish); alive dev [K] or NULL: the inner search's `alive` field, copied into the state's first.
 * GPMPC_E_ARG -- before anything is launched, text in gpmpc_last_error -- as gpmpc_auglag_solve's parameter checks; GPMPC_E_WORKSPACE. */
int gpmpc_auglag_outer(int H, int action_dim, int n_rows, const gpmpc_auglag_params* params_host, int update, const double* f_dev,
                       const double* g_dev, const double* X_dev, const double* conv_dev, const double* alive_dev, void* state,
                       size_t state_bytes, void* stream);

/* The solve on ONE stream without a host synchronisation.  With E = gpmpc_rollout_constrained(GPMPC_WANT_GRAD) over the K rows of the
 * inner state's U:
 *   first_outer == 0:  the state above is initialised, U = clip(X0)
 *   for o = first_outer .. first_outer + n_outer - 1:
 *       o > 0: U <- X;   E;   the outer step (update = o > 0);   the merit with the new lam, rho;   gpmpc_lbfgs_start's step on (M, dM)
 *       from a copy of the points: history, step length and flags are reset;   inner_ticks x (E, merit, the tick of gpmpc_lbfgs_tick)
 *   finally:  U <- X;  E;  the outer step without update (incumbents only);  both summaries.
 * first_outer > 0 continues from the state a previous call left in the SAME workspace (X0 is not read): between two calls the caller may
 * read the summary and stop once summary[0] is 0.  A pack with a linear nominal model needs nothing.
 *   x0 dev [ds]; X0 dev [K][n].  The workspace BEGINS with the state (layout above), followed at gpmpc_auglag_state_bytes (a multiple of
 *   256) by the inner search's state (layout of gpmpc_lbfgs_state_bytes, F = the merit at X).
 * GPMPC_E_ARG -- before anything is launched, text in gpmpc_last_error -- on everything gpmpc_lbfgs_solve refuses in `inner`, a rho0,
 * growth or rho_max that is not positive (NaN included), growth < 1, shrink outside (0, 1], a negative or NaN feas_tol / lam_max,
 * inner_ticks < 1, first_outer < 0, n_outer < 0, and what gpmpc_rollout_constraints refuses in the rows; GPMPC_E_STATE on a pack that is
 * not built; GPMPC_E_WORKSPACE. */
size_t gpmpc_auglag_solve_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_state_constraints* cons_host,
                                          const gpmpc_auglag_params* params_host);
int gpmpc_auglag_solve(const gpmpc_pack* pack, int H, const double* x0_dev, const double* X0_dev, const gpmpc_cost_params* cost_host,
                       const gpmpc_state_constraints* cons_host, const gpmpc_auglag_params* params_host, int first_outer, int n_outer,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Full-covariance form of the hot path (BASELINE config 5): the state distribution carries the whole ds x ds
 * covariance; off-diagonal terms are the exact cross-covariances Cov[f_a, f_b] (covariance_prop_torch,
 * src/tools/uncertainty_prop.py:402-465, consistent form).  The reference's rollout propagates variances only
 * (src/dynamics.py:184-189 TODO); this is its extension to full Sigma with the same cost (src/mpc.py:156-200) and an
 * analytic gradient.  Needs gpmpc_pack_enable_fullcov (GPMPC_E_STATE otherwise).
 *   out_means dev [B][H+1][ds]; out_covs dev [B][H+1][ds][ds] (both required);
 *   out_cost dev [B]; out_grad dev [B][H][da] (with GPMPC_WANT_GRAD).
 * ------------------------------------------------------------------------- */
size_t gpmpc_rollout_fullcov_workspace_bytes(const gpmpc_pack* pack, int B, int H, unsigned flags);
int gpmpc_rollout_fullcov(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                          const gpmpc_cost_params* cost_host, unsigned flags,
                          double* out_means, double* out_covs, double* out_cost, double* out_grad,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Diagnostic (no reference counterpart): what gpmpc_rollout_fullcov launches for this call shape, as one line of text --
 * "form=<four_launch|two_launch> tiling=<rows>x<cols> workgroups=<of the pair kernel, per horizon step> columns_per_iteration=<1|2|4>
 *  head_workgroups_per_unit=<n> kernel=<pair kernel> shared_cross_units=<0|1> cross_tile_columns=<n>" (both forms).  Small batches run TWO launches per horizon step (round 4; fullcov.hip): a head
 * kernel that closes the previous step, assembles (u_t, S_t) and prepares every unit, and the pair kernel on narrow tiles; large batches
 * four (assemble, prepare, pair kernel on 256x256 tiles, close).  out_bytes >= 64; returns 0 or GPMPC_E_ARG. */
int gpmpc_rollout_fullcov_describe(const gpmpc_pack* pack, int B, int H, unsigned flags, char* out, size_t out_bytes);

/* ---------------------------------------------------------------------------
 * Full-covariance rollout: Jacobian and chance constraints (no reference counterpart; DESIGN.md section 3l, csrc/fullcov_cons.hip).
 * Both forms of gpmpc_rollout_fullcov keep the Jacobians of every moment-matched step; k_fc_pack_jac gathers them into the PACKED step
 * Jacobian of gpmpc_linearised_fc_step ("Linearised propagation, full covariance", below), p = ds + ds (ds + 1) / 2:
 *     out_jac dev [B][H][p][p + da]: rows (mu'_a, Sigma'_ab for a <= b, row-major), columns (mu_k, Sigma_kl for k <= l, u_j).
 *     An off-diagonal Sigma_kl = Sigma_lk is ONE variable: its column is d/dS_kl + d/dS_lk of the stored derivative, formed as that sum.
 *     Sigma is the STORED covariance (out_covs: process_var on the diagonal of every step t >= 1).  The state columns of step 1 are written
 *     (Sigma_0 = init_cov is a constant: gpmpc_linearised_fc_vjp / _constraints never read them).  Every element is written.
 * gpmpc_rollout_fullcov_jac is the counterpart of gpmpc_rollout_jac: means, covariances and that Jacobian, no cost.  Its pair
 * (out_means, out_covs, out_jac) is what gpmpc_linearised_fc_vjp and gpmpc_linearised_fc_constraints take.
 *
 * gpmpc_rollout_fullcov_constrained is the counterpart of gpmpc_rollout_constrained under the full rule,
 *     g[t][r] = a_r . mu_t + kappa_r sqrt(a_r^T Sigma_t a_r) - b_r,      Sigma_t as stored,
 * with the rules of gpmpc_rollout_constraints unchanged: a radicand <= 0 gives sd = 0 and no variance part, columns tau >= t of out_gjac are
 * exactly 0.0, every element is written.  out_g dev [B][H][n_rows], out_gjac dev [B][H n_rows][H da].
 *   With GPMPC_WANT_GRAD: the launches of gpmpc_rollout_fullcov (gradient), k_fc_pack_jac into the workspace, then the sweep of
 *   gpmpc_linearised_fc_constraints.  Without: the objective-only rollout (no Jacobian is kept) and the values-only sweep; out_grad and
 *   out_gjac are not written and may be NULL.  out_cost, out_grad, out_means, out_covs are bit-identical to gpmpc_rollout_fullcov's on the
 *   same inputs; out_g does not depend on the flag.  out_means / out_covs may be NULL (kept in the workspace).
 * Refused before anything is launched, text in gpmpc_last_error: GPMPC_E_STATE on what gpmpc_rollout_fullcov refuses in a pack (a linear
 * nominal model, not built, no gpmpc_pack_enable_fullcov); GPMPC_E_ARG on what gpmpc_check_constraints refuses in the rows (n_rows, kappa),
 * on flags other than GPMPC_WANT_GRAD (GPMPC_USE_GRAPH and the GPMPC_FP32_* modes included), on a bad cost schedule, action_dim < 1,
 * sizes beyond the sweeps' grids, state_dim > 6 (the cost kernel of the full-covariance rollout is built up to 6: gpmpc_rollout_fullcov
 * returns the same code there, after its rollout has been enqueued) and -- gpmpc_rollout_fullcov_constrained only, which runs that kernel --
 * a horizon beyond its LDS.  gpmpc_rollout_fullcov_jac runs no cost kernel: the LDS does not bound its horizon.  GPMPC_E_WORKSPACE.
 * ------------------------------------------------------------------------- */
size_t gpmpc_rollout_fullcov_jac_workspace_bytes(const gpmpc_pack* pack, int B, int H);
int gpmpc_rollout_fullcov_jac(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                              double* out_means, double* out_covs, double* out_jac,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_rollout_fullcov_constrained_workspace_bytes(const gpmpc_pack* pack, int B, int H, unsigned flags);
int gpmpc_rollout_fullcov_constrained(const gpmpc_pack* pack, int B, int H, const double* x0_dev, const double* U_dev,
                                      const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host, unsigned flags,
                                      double* out_means, double* out_covs, double* out_cost, double* out_grad,
                                      double* out_g, double* out_gjac, void* workspace, size_t workspace_bytes, void* stream);

/* The device solvers on the full-covariance rule: gpmpc_mppi_solve, gpmpc_lbfgs_solve and gpmpc_auglag_solve with ONE difference, the
 * evaluation of the batch -- gpmpc_rollout_fullcov_constrained objective-only (gpmpc_rollout_fullcov without constraints) for MPPI,
 * gpmpc_rollout_fullcov with GPMPC_WANT_GRAD for the L-BFGS search, gpmpc_rollout_fullcov_constrained with GPMPC_WANT_GRAD for the
 * augmented Lagrangian.  Parameters, state layouts, the order of the checks and every other kernel are those of the entries above, and
 * those entries return what they returned.  More refusals, after "not built" and before the cost schedule, all with text: GPMPC_E_STATE on a
 * pack with a linear nominal model or without gpmpc_pack_enable_fullcov; GPMPC_E_ARG on state_dim > 6 and on a horizon beyond the LDS of
 * the full-covariance cost kernel.  A workspace is sized by the query of the SAME rule. */
size_t gpmpc_mppi_solve_fullcov_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_mppi_params* params_host,
                                                const gpmpc_state_constraints* cons_host);
int gpmpc_mppi_solve_fullcov(const gpmpc_pack* pack, int H, const double* x0_dev, const double* start_dev, const gpmpc_cost_params* cost_host,
                             const gpmpc_state_constraints* cons_host, const gpmpc_mppi_params* params_host, double* out_U, double* out_best,
                             double* out_trace, void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_lbfgs_solve_fullcov_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_lbfgs_params* params_host);
int gpmpc_lbfgs_solve_fullcov(const gpmpc_pack* pack, int H, const double* x0_dev, const double* X0_dev, const gpmpc_cost_params* cost_host,
                              const gpmpc_lbfgs_params* params_host, int first_tick, int n_ticks, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t gpmpc_auglag_solve_fullcov_workspace_bytes(const gpmpc_pack* pack, int H, const gpmpc_state_constraints* cons_host,
                                                  const gpmpc_auglag_params* params_host);
int gpmpc_auglag_solve_fullcov(const gpmpc_pack* pack, int H, const double* x0_dev, const double* X0_dev, const gpmpc_cost_params* cost_host,
                               const gpmpc_state_constraints* cons_host, const gpmpc_auglag_params* params_host, int first_outer, int n_outer,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The solver callback pair RiskSensitiveMPC.objective(x) / gradient(x) (src/mpc.py:202-255) for ONE candidate, host in and
 * host out like the cyipopt callbacks themselves: x0_host [ds] current state, U_host [H][da] the candidate (Ipopt's x),
 * out_host [1 + H da] = cost, then d cost / d U row-major (flags = GPMPC_WANT_GRAD; 0: cost only, out_host [1]).
 * SYNCHRONOUS: returns when out_host is filled.  The pack owns the staging buffers (pinned host + device) and one
 * captured hipGraph -- upload, the H + 1 kernels of the diagonal-covariance rollout, download -- so a callback costs
 * the host one graph launch and one stream wait; a changed horizon / cost parameter set re-captures.  `stream`: the
 * stream the pack was last built on (the call is ordered behind it).  Not re-entrant per pack. */
int gpmpc_objective_gradient(gpmpc_pack* pack, int H, const double* x0_host, const double* U_host,
                             const gpmpc_cost_params* cost_host, unsigned flags, double* out_host, void* stream);

/* Kernel-level timing of the dominant (pair) kernel for bench.py: when enabled, every
 * gpmpc_rollout brackets its pair-kernel launches with HIP events on the launch stream.
 * gpmpc_pair_kernel_time returns accumulated milliseconds and launch count since the last reset
 * (it synchronises on the recorded events). */
int gpmpc_timing_enable(int on);
int gpmpc_pair_kernel_time(double* total_ms, long long* launches, int reset);
/* The same totals per kernel class: 0 = the full pair kernel, 1 = its horizon-step-1 variant (constant state inputs:
 * fewer moments, cheaper), 2 = the fused small-batch step kernel (one launch per horizon step: mean sums, finish work and
 * pair tiles together -- NOT a pair-only time), so that a roofline figure can be quoted for the dominant kernel alone.  Reset with
 * gpmpc_pair_kernel_time(..., 1). */
int gpmpc_pair_kernel_time_class(int kernel_class, double* total_ms, long long* launches);

/* Launch geometry, host-side views (no device work; for tests without a GPU).
 * gpmpc_debug_run_list: the balanced-run work list of the one-launch form for ONE trajectory of a large training set (items
 *   {GP, first row, first column, end column}; n_padded = N rounded up to 64; slots = workgroup slots of the device minus the
 *   2 state_dim role workgroups).  *n_items = 0 when the plain 256x64 list is within 1.1 generations.  items_out holds 4 * capacity ints
 *   (capacity = 0: count only).
 * gpmpc_debug_work_list: a tile work list exactly as a pack holds it -- units x row tiles x column tiles, the first n_tri_units keeping only
 *   the tiles that reach the diagonal; items {unit, first row, first column, end column} (tile_slot: the tile's index within its unit instead
 *   of the end column), XCD re-ordered when xcd_sort is set and the list has 16 items or more.  Same convention as gpmpc_debug_run_list; with
 *   capacity > 0 also ustart_out [units + 1] and, for a re-ordered list only (it is left untouched otherwise: a pack keeps none), perm_out
 *   [*n_items], the item positions grouped by unit.
 * gpmpc_debug_fcs_tables: the tile tables of the one-lambda full-covariance form for the variance-unit tiling 256 x cols_per_tile:
 *   ntile_out [3] tiles per trajectory and pair in the three widths, tiles_out [*n_tiles][3] = {64-row block, first column, columns} of the
 *   widest (capacity in tiles, 0: counts only), ustart_out [3][units + 1] the unit offsets per width (last entry: slots per trajectory).
 * gpmpc_debug_xcd_order: (trajectory, grid column) that workgroup `linear_id` of a (grid_x, n_traj) grid with n_tile tile columns runs in
 *   the XCD-aware dispatch order.
 * All: GPMPC_E_ARG on sizes that are no padded size / tile size / unit count of a pack, or a capacity below the count. */
int gpmpc_debug_run_list(int n_padded, int state_dim, int slots, int* items_out, int capacity, int* n_items);
int gpmpc_debug_work_list(int n_padded, int rows_per_tile, int cols_per_tile, int n_tri_units, int n_cross_units, int xcd_sort, int tile_slot,
                          int* items_out, int capacity, int* n_items, int* perm_out, int* ustart_out);
int gpmpc_debug_fcs_tables(int n_padded, int state_dim, int cols_per_tile, int* ntile_out, int* tiles_out, int capacity, int* n_tiles,
                           int* ustart_out);
int gpmpc_debug_xcd_order(int linear_id, int grid_x, int n_tile, int n_traj, int* traj, int* column);

/* ---------------------------------------------------------------------------
 * GP prediction at test points (GaussianProcessRegression.compute_pred_train_covariance /
 * predict_latent_vars, src/gpr.py:253-332) for ONE GP given by raw arrays.
 *   X dev [n][D]; lambdas host [D]; beta dev [n] = Ky_inv (y - f_nom(X)) (needed for out_mean);
 *   Ky_inv dev [n][n] (needed for out_cov); X_pred dev [p][D];
 *   out_K dev [p][n] or NULL; out_mean dev [p] or NULL (nominal-model term added by the caller);
 *   out_cov dev [p][p] or NULL = K** - K* Ky_inv K*^T + noise_var * I.
 * gpmpc_matvec: out[r] = A[r] . v for a row-major [rows][cols] matrix (beta = Ky_inv y,
 * src/tools/uncertainty_prop.py:327).
 * ------------------------------------------------------------------------- */
int gpmpc_matvec(int rows, int cols, const double* A_dev, const double* v_dev, double* out_dev, void* stream);
size_t gpmpc_predict_workspace_bytes(int n, int D, int p);
int gpmpc_predict(int n, int D, const double* X_dev, const double* lambdas_host, double sigma_f,
                  const double* beta_dev, const double* Ky_inv_dev, double noise_var,
                  int p, const double* X_pred_dev, double* out_K, double* out_mean, double* out_cov,
                  void* workspace, size_t workspace_bytes, void* stream);

/* O(N^2) append of ONE observation to an explicit inverse (Schur complement; the reference's abandoned
 * update_Ky_inv_mat, src/gpr.py:137-157) instead of the O(N^3) rebuild of src/gpr.py:171 after every
 * Simulator step (src/simulator.py:55).  Ky_inv dev [n][n]; k dev [n] = K_f(X, x_new); kappa = sigma_f^2 + noise_var;
 * out dev [(n+1)][(n+1)] (must not alias Ky_inv).  Opt-in: results differ from a rebuild by rounding (~cond * eps). */
size_t gpmpc_kinv_append_workspace_bytes(int n);
int gpmpc_kinv_append(int n, const double* Ky_inv_dev, const double* k_dev, double kappa, double* out_dev,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The whole data update of ONE appended observation for a GP kept in CAPACITY-PADDED buffers (closed loop: src/simulator.py:55 ->
 * src/gpr.py:90-122 store the row, :159-171 rebuild Kf, Ky and invert): k = K_f(X, x_new) (src/gpr.py:124-135), then Kf, Ky and
 * Ky_inv of the n + 1 points -- the Schur step of gpmpc_kinv_append -- written into the OUTPUT buffers (row stride ld_out >= n + 1)
 * from the INPUT buffers (row strides ld_k_in of Kf / Ky and ld_in of Ky_inv, >= n).  Inputs and outputs must not alias: the caller ping-pongs two buffer sets, so the
 * n-point matrices stay valid for whoever still reads them.  X dev [n][D] (the n OLD rows), x_new dev [D], lambdas host [D].
 * Two kernel launches (k_append_vw2: k, v = Ky_inv k and the Schur scalar; k_append_fill2: the three (n + 1)-point matrices), no allocation,
 * no host-side concatenation. */
size_t gpmpc_gp_append_workspace_bytes(int n, int D);
int gpmpc_gp_append(int n, int D, const double* X_dev, const double* x_new_dev, const double* lambdas_host, double sigma_f,
                    double noise_var, const double* Kf_in, const double* Ky_in, size_t ld_k_in, const double* Ky_inv_in, size_t ld_in,
                    double* Kf_out, double* Ky_out, double* Ky_inv_out, size_t ld_out, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Fixed-size training window (no reference counterpart: the reference's training set only grows).  With K = Ky_inv, b = K[:, p],
 * c = K[p, :], d = K[p, p] (K comes from LU and is not exactly symmetric: row and column forms are kept apart):
 *
 * REMOVE point `index`: out dev [(n-1)][(n-1)] (row stride ld_out >= n - 1) = K_ij - b_i c_j / d over i, j != index, compacted (rows
 * and columns after `index` move up by one): the inverse of Ky without that row and column.  n >= 2, 0 <= index < n, ld_in >= n,
 * out must not alias Ky_inv.  One launch, no workspace. */
int gpmpc_kinv_remove(int n, const double* Ky_inv_dev, size_t ld_in, int index, double* out_dev, size_t ld_out, void* stream);

/* REPLACE point `slot` by the input x_new (n stays n): the whole data update of one observation in a window of constant size, from one
 * buffer set into the other, argument conventions of gpmpc_gp_append (ld_out >= n).  With kt_i = k_f(x_i, x_new) for i != slot,
 * kt_slot = 0, kappa = sigma_f^2 + noise_var:
 *     v = K kt - b (c . kt) / d      w = K^T kt - c (b . kt) / d      q = 1 / (kappa - kt . v)
 *     Ky_inv_out_ij = K_ij - b_i c_j / d + q v_i w_j  (i, j != slot);  column slot = -q v, row slot = -q w, corner q
 *     Kf_out, Ky_out: row and column `slot` become kt (corner sigma_f^2, on Ky plus noise_var), everything else is copied
 * i.e. the removal above and the Schur step of gpmpc_kinv_append in one pass, the new point staying in the old one's place.
 * X dev [n][D] still holds the OLD row at `slot`; that row is not read.  Two kernel launches (k_replace_vw: kt, v, w;
 * k_replace_fill: q and the three matrices), no allocation, fixed summation order. */
size_t gpmpc_gp_replace_workspace_bytes(int n, int D);
int gpmpc_gp_replace(int n, int D, int slot, const double* X_dev, const double* x_new_dev, const double* lambdas_host, double sigma_f,
                     double noise_var, const double* Kf_in, const double* Ky_in, size_t ld_k_in, const double* Ky_inv_in, size_t ld_in,
                     double* Kf_out, double* Ky_out, double* Ky_inv_out, size_t ld_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Gradient of the log marginal likelihood w.r.t. the LOG hyper-parameters in one pass over Ky_inv: replaces the autograd
 * backward through inv / det of update_hyperparams (src/gpr.py:334-338; likelihood src/gpr.py:240-251) and the dense
 * N x N x D derivative tensors of kernel_matrix_gradient / marginal_likelihood_grad (src/gpr.py:173-238).
 * X dev [n][D] row-major; Ky_inv dev [n][n]; alpha dev [n] = Ky_inv r; resid dev [n] = r = y - f_nom(X);
 * lambdas host [D]; noise_var = sigma_n^2 as it sits on the diagonal of Ky.
 * out dev [D+3]: d ml/d log lambda_k (D), d ml/d log sigma_f, d ml/d log sigma_n, and r^T alpha (the data-fit term of ml). */
size_t gpmpc_ml_grad_workspace_bytes(int n, int D);
int gpmpc_ml_grad(int n, int D, const double* X_dev, const double* Ky_inv_dev, const double* alpha_dev,
                  const double* resid_dev, const double* lambdas_host, double sigma_f, double noise_var,
                  double* out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Sparse GP: FITC inducing points in the WHITENED form (no reference counterpart).  M pseudo-inputs Z [M][D] summarise n observations
 * for a group of GPs with identical hyper-parameters (lambda, sigma_f, sigma_n); the GPs' targets are the columns of Y.  With
 *     Kmm = k(Z, Z) + jitter I     L = chol(Kmm)     W = L^-1  (lower triangular, M x M; from the caller)
 *     v_n = W k(Z, x_n)            Lambda_n = sigma_f^2 + noise_var - |v_n|^2      (no clamp: a NaN or a negative value is passed on)
 *     G = sum_n v_n v_n^T / Lambda_n          r = sum_n v_n y_n^T / Lambda_n  [M][n_targets]
 *     B = I + G                    Binv = B^-1  (SYMMETRIC, from the caller: only its lower triangle is read)
 *     alpha = W^T Binv r  [M][n_targets]      Q = W^T (I - Binv) W  [M][M]
 * the posterior of GP a is mean k_*^T alpha[:, a], variance sigma_f^2 - k_*^T Q k_*: exactly what gpmpc_pack_build_beta takes as
 * (X := Z, beta := alpha^T, Ky_inv := Q) and gpmpc_predict as (X := Z, beta := alpha[:, a], Ky_inv := Q).  The textbook form
 * (Kmm + Kmn Lambda^-1 Knm)^-1 is NOT used: its condition number reaches 1e14.
 * All matrices row-major and dense ([M][M]) unless a row stride is named; k(z, x) = sigma_f^2 exp(-1/2 sum_d (z_d - x_d)^2 / lambda_d).
 * No atomics, fixed summation orders, launch geometry from the sizes only: two identical calls agree bit for bit; G and Q are exactly
 * symmetric; G does not depend on n_targets nor a column of r on the others.  Common refusals (GPMPC_E_ARG with a text in gpmpc_last_error,
 * before any launch): M < 1 or M > GPMPC_SPARSE_MAX_M, D outside 1...GPMPC_MAX_D, n_targets outside 1...GPMPC_MAX_DS, a row stride below
 * its row length, a NULL pointer.  A workspace below *_workspace_bytes: GPMPC_E_WORKSPACE.
 *
 * gpmpc_sparse_accumulate: G, r and stats [2] = {rows accumulated, min Lambda_n} over the n rows of X [n][D], Y [n][ld_y] (first n_targets
 *   columns).  Rows are taken in chunks of `chunk` (a multiple of 64; 0: the default, 4096): V_c = W k(Z, X_c) into the workspace ([M][chunk],
 *   kernel values generated on the fly, the triangle of W used), Lambda_c, then G += V_c Lambda_c^-1 V_c^T, r += V_c Lambda_c^-1 Y_c; chunks are
 *   added in call order.  accumulate 0: outputs overwritten (they may hold anything); 1: added to what G, r, stats hold.  A call over rows
 *   [0, n) equals one over [0, s) followed by accumulate = 1 over [s, n) bit for bit when s is a multiple of chunk; the result may depend on
 *   chunk and on nothing else.  The workspace size depends on (M, chunk) only.  Also refused: n < 1, chunk negative or no multiple of 64.
 *   The two N M^2 products exist in two forms, scalar fp64 FMA on 4 x 4 register tiles and v_mfma_f64_16x16x4_f64; gpmpc_sparse_set_form
 *   chooses between them for the whole process (GPMPC_SPARSE_FORM_FMA | GPMPC_SPARSE_FORM_MFMA; -1 only asks) and returns the form that was
 *   set before; anything else is GPMPC_E_ARG.  Every property above holds within a form; the two forms agree to rounding, not bit for bit.
 * gpmpc_sparse_finish: alpha and Q from W, Binv, r.  M^3-class, no pass over the data.
 * gpmpc_sparse_append: ONE observation x_new dev [D], y_new dev [n_targets], O(M^2) whatever n is:
 *     v = W k(Z, x); Lambda = sigma_f^2 + noise_var - |v|^2; t = Binv v; den = Lambda + v . t; u = W^T t
 *     G += v v^T / Lambda; r += v y^T / Lambda; Binv -= t t^T / den; Q += u u^T / den; alpha = W^T (Binv r); stats += {1, min}
 *   in place.  Six dependent launches (v | t | u | the M x M streams and r | Binv r | alpha), no allocation, no host round trip; G, Binv
 *   and Q stay exactly symmetric.
 * gpmpc_sparse_remove: the inverse of the append for ONE observation x_old dev [D], y_old dev [n_targets] that the state holds:
 *     v = W k(Z, x); Lambda = sigma_f^2 + noise_var - |v|^2; t = Binv v; den = Lambda - v . t; u = W^T t
 *     G -= v v^T / Lambda; r -= v y^T / Lambda; Binv += t t^T / den; Q -= u u^T / den; alpha = W^T (Binv r); stats[0] -= 1
 *   in place, six dependent launches like the append and under the same rules.  den is a cancelling difference (den / Lambda is small
 *   for a row that carries much of what the state knows); nothing is clamped: a NaN or non-positive den is passed on.  stats[1] is left
 *   alone: after a removal it is a LOWER BOUND on the Lambda of the rows held, no longer their minimum (a fresh accumulate restores it).
 *   Removing a row the state does not hold is not detected.  The workspace is the append's.
 * gpmpc_sparse_replace: x_old, y_old out and x_new, y_new in, in ONE pass over G, Binv and Q (the step of a full window).  The removed
 *   state is never formed: with t_o = Binv v_o, s_n = Binv v_n, den_o = Lambda_o - v_o . t_o,
 *     t_n = s_n + t_o (t_o . v_n) / den_o;  den_n = Lambda_n + v_n . t_n;  u_o = W^T t_o;  u_n = W^T t_n
 *     G = (G - v_o v_o^T / Lambda_o) + v_n v_n^T / Lambda_n;  r likewise;  Binv = (Binv + t_o t_o^T / den_o) - t_n t_n^T / den_n
 *     Q = (Q - u_o u_o^T / den_o) + u_n u_n^T / den_n;  alpha = W^T (Binv r);  stats[0] unchanged;  stats[1] = min(stats[1], Lambda_n)
 *   (the NaN-propagating minimum).  Six dependent launches: v_o, v_n | t_o, s_n | t_n, u_o, u_n | the M x M streams, r, stats | Binv r |
 *   alpha.  G and r equal gpmpc_sparse_remove followed by gpmpc_sparse_append BIT FOR BIT; Binv, Q and alpha agree with the two calls
 *   to rounding.  G, Binv and Q stay exactly symmetric.  Workspace: 7 M + M n_targets doubles (each part 256-byte aligned).
 * ------------------------------------------------------------------------- */
#define GPMPC_SPARSE_MAX_M 8192
#define GPMPC_SPARSE_FORM_FMA  0
#define GPMPC_SPARSE_FORM_MFMA 1
#define GPMPC_SPARSE_FORM_DEFAULT GPMPC_SPARSE_FORM_MFMA  /* the measured choice (0.80-0.83 of the FMA form's time): DESIGN.md section 3h */
int gpmpc_sparse_set_form(int form);
size_t gpmpc_sparse_accumulate_workspace_bytes(int n, int D, int M, int n_targets, int chunk);
int gpmpc_sparse_accumulate(int n, int D, int M, int n_targets, const double* X_dev, const double* Y_dev, size_t ld_y,
                            const double* Z_dev, const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f,
                            double noise_var, int chunk, int accumulate, double* G_dev, double* r_dev, double* stats_dev,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_sparse_finish_workspace_bytes(int M, int n_targets);
int gpmpc_sparse_finish(int M, int n_targets, const double* W_dev, size_t ld_w, const double* Binv_dev, const double* r_dev,
                        double* alpha_dev, double* Q_dev, void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_sparse_append_workspace_bytes(int M, int n_targets);
int gpmpc_sparse_append(int D, int M, int n_targets, const double* x_new_dev, const double* y_new_dev, const double* Z_dev,
                        const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f, double noise_var,
                        double* G_dev, double* r_dev, double* Binv_dev, double* Q_dev, double* alpha_dev, double* stats_dev,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_sparse_remove_workspace_bytes(int M, int n_targets);
int gpmpc_sparse_remove(int D, int M, int n_targets, const double* x_old_dev, const double* y_old_dev, const double* Z_dev,
                        const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f, double noise_var,
                        double* G_dev, double* r_dev, double* Binv_dev, double* Q_dev, double* alpha_dev, double* stats_dev,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t gpmpc_sparse_replace_workspace_bytes(int M, int n_targets);
int gpmpc_sparse_replace(int D, int M, int n_targets, const double* x_old_dev, const double* y_old_dev, const double* x_new_dev,
                         const double* y_new_dev, const double* Z_dev, const double* W_dev, size_t ld_w, const double* lambdas_host,
                         double sigma_f, double noise_var, double* G_dev, double* r_dev, double* Binv_dev, double* Q_dev,
                         double* alpha_dev, double* stats_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Particles: the pointwise posterior of all GPs at many points, and Monte-Carlo rollouts through it (the device counterpart of the
 * reference's statistical oracles, src/tools/uncertainty_prop.py:47, :139, :239 and src/test/test_dynamics.py:198-268).  DESIGN.md
 * section 3i.  The model is what gpmpc_pack_build_beta / _strided accept, by raw arrays (a pack cannot serve: its weights carry
 * exp(-1/4 |x_i - x_j|^2), which underflows for far pairs): a dense GP bundle (X_train, beta, Ky_inv) or a sparse one (Z, alpha, Q).
 *
 * For a point z = (x, u) and GP a:
 *     k_i  = sf_a^2 exp(-1/2 sum_d (X_id - z_d)^2 / lambda_ad)
 *     m_a  = sum_i beta_ia k_i  [+ W_a . z + b_a with a nominal model]
 *     q_a  = sum_i sum_j k_i Kinv_a[i][j] k_j         (ALL entries: Kinv comes from LU and is not symmetric)
 *     s2_a = sf_a^2 - q_a + process_var_a             (latent variance; returned UNCLAMPED)
 *     x'_a = m_a + sqrt(max(s2_a, 0)) eps_a           (the clamp exists only inside the square root)
 * A particle rollout of plan b with P particles: x_0^p = x0_b + L eps with L the lower Cholesky factor of init_cov (host; a zero pivot
 * gives a zero column); for t = 1...H: z = (x_{t-1}^p, U_b[t-1] + sqrt(action_var) eps_u), then x_t^p as above, the GPs drawn
 * independently given z.  Particle p of plan b is column b P + p of every [B P] array.
 *
 * Noise: Philox4x32-10 + Box-Muller, the generator of gpmpc_mppi_sample.  Key (seed low, seed high ^ 0x50415254); counter
 * (p, j, t, call_index) with p the particle index WITHIN its plan, j the pair index and t the step (0: the initial draw); counter j gives
 * the normals 2j (cosine) and 2j + 1 (sine).  At t = 0 the normals 0...ds-1 are the initial eps; at t >= 1 the normals 0...da-1 are the
 * action noise and da...da+ds-1 the GP draws.  Every plan of a batch sees the same noise (common random numbers); a value depends on
 * (seed, call_index, p, t, element) and on nothing else -- not B, P, chunk or the grid.
 *
 * No atomics, fixed summation orders, launch geometry from the sizes only: two identical calls agree bit for bit, and no result
 * depends on `chunk` (columns are independent).  All refusals are GPMPC_E_ARG with a text in gpmpc_last_error, before any launch:
 * a NULL pointer, dimensions outside GPMPC_MAX_*, n < 1, nq / P / B / H / T < 1, ld < n, a chunk that is negative or no multiple of 64, a
 * lambda or sigma_f that is not positive and finite, a non-finite or negative action_var / process_var, an init_cov that is non-finite,
 * asymmetric (|P_kl - P_lk| > 1e-12 max |P|) or has a negative pivot, constraint rows outside 1...GPMPC_MAX_CONS, more than 2^31 - 1
 * elements in one array.  A workspace below *_workspace_bytes (which return 0 for arguments that would be refused): GPMPC_E_WORKSPACE.
 * Not provided: gradients through particles, joint (function-space) sampling across steps, multi-GPU sharding,
 * a form that reads only one triangle of a symmetrised Kinv.  (A planner on the particles: "Particle cost" below.)
 * ------------------------------------------------------------------------- */
typedef struct gpmpc_gp_model {
    int n, state_dim, action_dim;                     /* training (or inducing) points; D = state_dim + action_dim */
    int has_nominal;                                  /* nom_w / nom_b are read */
    int has_noise;                                    /* init_cov / action_var / process_var are read; 0: the defaults of gpmpc_pack_set_noise */
    int reserved;
    const double* X;                                  /* dev [n][D] */
    const double* beta;                               /* dev [n][ds], column a = beta_a */
    const double* Kinv;                               /* dev: GP a's matrix at Kinv + a gp_stride, row stride ld (doubles) */
    size_t ld, gp_stride;                             /* ld >= n; gp_stride = 0: ONE matrix for every GP */
    double lambdas[GPMPC_MAX_DS * GPMPC_MAX_D];       /* [ds][D] row-major in the leading ds*D entries */
    double sigma_f[GPMPC_MAX_DS];
    double nom_w[GPMPC_MAX_DS * GPMPC_MAX_D];         /* [ds][D] */
    double nom_b[GPMPC_MAX_DS];
    double init_cov[GPMPC_MAX_DS * GPMPC_MAX_DS];     /* [ds][ds] */
    double action_var[GPMPC_MAX_D];                   /* [da] */
    double process_var[GPMPC_MAX_DS];                 /* [ds] */
} gpmpc_gp_model;

/* m and s2 at nq points z dev [nq][D] for all ds GPs: out_mean, out_var dev [nq][ds].  Columns are taken `chunk` at a time (a multiple of
 * 64; 0: the default, 4096), which bounds the workspace.  Per chunk and per group of GPs with bit-identical (lambda, sigma_f) -- the
 * check gpmpc_pack_shared_lambda makes --: k_pt_kstar materialises Ks[i][c] (and the partial sums of m), k_pt_quad forms the 64 x 64
 * tiles of Kinv Ks by v_mfma_f64_16x16x4_f64 and contracts each with the matching rows of Ks in its epilogue (the product is never
 * written), k_pt_finish adds the row blocks in ascending order.  With gp_stride = 0 and one group the quadratic form is evaluated once
 * for all GPs. */
size_t gpmpc_gp_posterior_workspace_bytes(const gpmpc_gp_model* model_host, int nq, int chunk);
int gpmpc_gp_posterior(const gpmpc_gp_model* model_host, int nq, const double* z_dev, double* out_mean, double* out_var, int chunk,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The normals of step t: out_eps dev [P][n_normals], element (p, e) = normal e of counter stream (p, ., t, call_index).  The rollout
 * uses n_normals = ds at t = 0 and da + ds at t >= 1.  n_normals in 1...GPMPC_MAX_D + GPMPC_MAX_DS, t >= 0. */
int gpmpc_particle_noise(int P, int n_normals, int t, unsigned long long seed, unsigned call_index, double* out_eps, void* stream);
/* One step of B plans x P particles: x_prev dev [B P][ds]; U_t dev, input j of plan b at U_t[b u_stride + j] (NULL with da = 0); eps dev
 * [P][da + ds]; out_next dev [B P][ds]; out_mean / out_var dev [B P][ds] or NULL.  Assembles z, evaluates the posterior, draws. */
size_t gpmpc_particle_step_workspace_bytes(const gpmpc_gp_model* model_host, int B, int P, int chunk);
int gpmpc_particle_step(const gpmpc_gp_model* model_host, int B, int P, const double* x_prev, const double* U_t, size_t u_stride,
                        const double* eps, double* out_next, double* out_mean, double* out_var, int chunk,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Statistics of particles dev [T][B P][ds] per plan and step: out_mean dev [B][T][ds] (sum in a fixed order / P), out_cov dev
 * [B][T][ds][ds] (two-pass, divisor P - 1: NaN for P = 1; exactly symmetric); with var dev [T][B P][ds] (or NULL) out_clamped dev int
 * [B][T] = particles with some s2 < 0; with cons_host (or NULL; A and b are read, kappa is not) out_viol dev [B][T][n_rows] = fraction of
 * particles with a_r . x > b_r and out_joint dev [B] = fraction violating any row at any step t >= 1.  Outputs that are not wanted may
 * be NULL, but for out_viol / out_joint, which are given exactly when cons_host is. */
int gpmpc_particle_stats(int B, int P, int T, int state_dim, const double* particles, const double* var,
                         const gpmpc_state_constraints* cons_host, double* out_mean, double* out_cov, int* out_clamped, double* out_viol,
                         double* out_joint, void* stream);
/* The rollout: noise(0) -> initial particles -> for t = 1...H: noise(t) -> step, then the statistics; one stream, no host round trip, no
 * allocation.  x0 dev [B][ds]; U dev [B][H][da]; out_particles dev [H+1][B P][ds]; out_mean dev [B][H+1][ds]; out_cov dev
 * [B][H+1][ds][ds]; out_clamped dev int [B][H] (steps 1...H, counted from the kept s2, not with atomics); out_viol dev [B][H+1][n_rows]
 * and out_joint dev [B] exactly when cons_host is given.  The particles are bit for bit those of the chain of gpmpc_particle_noise and
 * gpmpc_particle_step calls. */
size_t gpmpc_particle_rollout_workspace_bytes(const gpmpc_gp_model* model_host, int B, int P, int H, int chunk);
int gpmpc_particle_rollout(const gpmpc_gp_model* model_host, int B, int P, int H, const double* x0, const double* U,
                           unsigned long long seed, unsigned call_index, const gpmpc_state_constraints* cons_host,
                           double* out_particles, double* out_mean, double* out_cov, int* out_clamped, double* out_viol,
                           double* out_joint, int chunk, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Particle cost: the risk-sensitive cost and the chance constraints evaluated ON the particles of gpmpc_particle_rollout, and MPPI over
 * them -- the planner that optimises against the distribution validate_plan checks a moment-matched plan with (DESIGN.md section 3m,
 * kernels in csrc/particle_cost.hip).  It serves every model the particle rollout serves: dense, sparse, nominal, with a noise model.
 *
 * For plan b with P particles x_i^p, i = 0...H (exactly the particles of gpmpc_particle_rollout):
 *     J_b  = sum_{i = 0...H} s_i + input_cost(U_b)
 *     c_p  = e_p^T Q_i e_p,  e_p = x_i^p - x_ref,i       (Q_i, x_ref,i as the cost kernels choose them: the struct or the row of a cost
 *                                                         schedule, Q_f at i = H where the schedule has one; Q as given, symmetric or not)
 *     gamma == 0:  s_i = (1 / P) sum_p c_p
 *     otherwise:   a_p = -(gamma / 2) c_p,  M = max_p a_p,  s_i = -(2 / gamma) (M + log((1 / P) sum_p exp(a_p - M)))
 * input_cost is bit for bit the input and input-rate terms of gpmpc_cost: on the plan's own inputs (not the noisy ones), with u_ref,
 * R_delta / last_u and the schedule's input rows.  s_i is the sample version of the functional gpmpc_cost evaluates in closed form: for
 * x ~ N(mu, Sigma), a symmetric Q and I + gamma Q Sigma positive definite,
 *     -(2 / gamma) log E exp(-(gamma / 2) e^T Q e) = (1 / gamma) log det(I + gamma Q Sigma) + ebar^T (I + gamma Q Sigma)^-1 Q ebar.
 * Chance constraints, t = 1...H, row r: y_p = a_r . x_t^p - b_r, sorted ascending y_(1) <= ... <= y_(P);
 *     eps_r = 1/2 erfc(kappa_r / sqrt 2),  m_r = floor(eps_r P + 1e-9)   (host, double),   g[t-1][r] = y_(P - m_r).
 * This is the empirical counterpart of a . mu + kappa sd - b, the Phi(kappa) quantile of the margin, in the same units; g <= 0 exactly when
 * at most m_r particles violate the row, and g is continuous in U.  kappa = 0 constrains the MEDIAN of the margin where the Gaussian rule
 * constrains its mean.
 * NaN: a NaN coordinate in any particle of (b, i) makes s_i, J_b and every g[b][i-1][.] NaN, and nothing else (gpmpc_mppi_update treats
 * such a sample as dead).
 *
 * Kernels: one 256-thread workgroup per (plan, step); thread i owns the particles i, i + 256, ... in ascending order, the 256 partial sums
 * are folded in halves, the maximum is exact; per row the margins are sorted in LDS (bitonic, padded with -inf to a power of two) and one
 * value is read, so ties are harmless.  No atomics, fixed summation orders: two identical calls agree bit for bit; a plan evaluated alone
 * gives the bits it has inside a batch; gpmpc_particle_evaluate equals gpmpc_particle_cost on the particles gpmpc_particle_rollout stores
 * for the same (seed, call_index), whatever `chunk`; gpmpc_mppi_solve_particles equals the chain of its three public parts.
 * All refusals are GPMPC_E_ARG with a text in gpmpc_last_error, before any launch: everything gpmpc_particle_rollout refuses (in the solve
 * also what gpmpc_mppi_solve_linearised refuses of its parameters), P outside 1...GPMPC_PARTICLE_COST_MAX_P, a bad cost schedule, bad
 * constraint rows, out_g not given exactly when cons_host is.  A workspace below *_workspace_bytes (which return 0 for arguments that
 * would be refused): GPMPC_E_WORKSPACE.
 * Not provided: gradients through particles, CVaR or other risk measures, joint (function-space) sampling across steps, a state feedback
 * inside the prediction, multi-GPU sharding.
 * ------------------------------------------------------------------------- */
#define GPMPC_PARTICLE_COST_MAX_P 4096
/* A pure function of stored particles dev [H+1][B P][ds] (the layout of gpmpc_particle_rollout's out_particles) and the plans U dev
 * [B][H][da] (NULL with da = 0): out_cost dev [B]; out_stage dev [B][H+1] or NULL (the s_i); out_g dev [B][H][n_rows], given exactly when
 * cons_host is.  out_cost is the same bits with and without out_stage. */
int gpmpc_particle_cost(int B, int P, int H, int state_dim, int action_dim, const gpmpc_cost_params* cost_host,
                        const gpmpc_state_constraints* cons_host, const double* particles, const double* U, double* out_cost,
                        double* out_stage, double* out_g, void* stream);
/* Rollout and cost in one pass that never stores the horizon: noise(0) -> initial particles -> stage 0; for t = 1...H: noise(t) ->
 * gpmpc_particle_step -> stage t and the rows of step t; then the sum.  One stream, no host round trip, no allocation; two particle
 * buffers that alternate, so the workspace has no term proportional to H B P.  x0 dev [B][ds]; outputs as gpmpc_particle_cost. */
size_t gpmpc_particle_evaluate_workspace_bytes(const gpmpc_gp_model* model_host, int B, int P, int H, int chunk);
int gpmpc_particle_evaluate(const gpmpc_gp_model* model_host, int B, int P, int H, const double* x0, const double* U,
                            unsigned long long seed, unsigned call_index, const gpmpc_cost_params* cost_host,
                            const gpmpc_state_constraints* cons_host, double* out_cost, double* out_stage, double* out_g, int chunk,
                            void* workspace, size_t workspace_bytes, void* stream);
/* gpmpc_mppi_solve_linearised with the evaluation above in the place of the rollout: per iteration gpmpc_mppi_sample (with the start
 * state once per sample), gpmpc_particle_evaluate (B = n_samples, default chunk), gpmpc_mppi_update.  Outputs and trace as there.
 * COMMON RANDOM NUMBERS: the particle noise is that of (params->seed, params->call_index) -- its Philox key differs from the sampler's --
 * and it is THE SAME in every iteration of a solve.  The key of the best plan kept compares costs across iterations, which is sound only
 * on ONE fixed sample-average objective; a fresh draw per iteration would let a lucky draw win. */
size_t gpmpc_mppi_solve_particles_workspace_bytes(const gpmpc_gp_model* model_host, int H, int P, const gpmpc_mppi_params* params_host,
                                                  const gpmpc_state_constraints* cons_host);
int gpmpc_mppi_solve_particles(const gpmpc_gp_model* model_host, int H, int P, const double* x0_dev, const double* start_dev,
                               const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host,
                               const gpmpc_mppi_params* params_host, double* out_U, double* out_best, double* out_trace, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Linearised propagation: the first-order (Taylor, "mean-equivalent") rule of the cautious-MPC literature, beside the exact moment matching
 * of gpmpc_rollout (no reference counterpart; DESIGN.md section 3j, kernels in csrc/linprop.hip).  The model is a gpmpc_gp_model, dense or
 * sparse (Z, alpha, Q in the place of X, beta, Kinv), with its nominal and noise model.
 *
 * One step.  Inputs: the mean mu (ds), the diagonal variance v (ds), the input u (da).  z = (mu, u), D = ds + da,
 * S = (v_1 ... v_ds, action_var_1 ... action_var_da).  Step 0 of a rollout is mu_0 = x0, v_0 = diag(init_cov) (the defaults of
 * gpmpc_pack_set_noise when has_noise = 0).  For GP a, with d_id = (X_id - z_d) / lambda_ad:
 *     k_i    = sf_a^2 exp(-1/2 sum_d (X_id - z_d)^2 / lambda_ad)
 *     m_a    = sum_i beta_ia k_i                      [+ W_a . z + b_a with a nominal model]
 *     g_ad   = d m_a / d z_d = sum_i beta_ia k_i d_id [+ W_ad]
 *     q_a    = sum_ij k_i Kinv_a[i][j] k_j            (ALL entries: Kinv comes from LU and is not symmetric)
 *     r_a    = (Kinv_a + Kinv_a^T) k
 *     d q_a / d z_d = sum_i r_ai k_i d_id
 *     w_ad   = g_ad S_d
 *     h_ad   = sum_i beta_ia k_i [ d_id (d_i . w_a) - w_ad / lambda_ad ]     (= sum_l d^2 m_a / d z_l d z_d w_al; the nominal part has no curvature)
 *     mu'_a  = m_a
 *     v'_a   = (sf_a^2 - q_a) + sum_d g_ad^2 S_d + process_var_a             (unclamped, as everywhere in this library)
 * q is evaluated as 1/2 k^T r from the one product r = (Kinv + Kinv^T) k (a staged tile holds Kinv[i][j] + Kinv[j][i]), so q and dq/dz come
 * from the same numbers.  The step Jacobian has the layout of gpmpc_rollout_jac, [2ds][2ds+da], rows (mu', v'), columns (mu, v, u):
 *     row mu'_a:  g_ak in the mu columns, 0 in the v columns, g_a,ds+j in the u columns
 *     row v'_a:   -dq_a/dz_k + 2 h_ak in the mu columns, g_ak^2 in the v columns, -dq_a/dz_{ds+j} + 2 h_a,ds+j in the u columns
 * The propagation is diagonal, as in gpmpc_rollout: cross-covariances between states are dropped (the rule that carries the whole Sigma,
 * and a state feedback inside the prediction: "Linearised propagation, full covariance" below).
 *
 * No atomics, fixed summation orders, launch geometry from the sizes only: two identical calls agree bit for bit and no result depends on
 * `chunk` (columns, i.e. plans, are independent; a multiple of 64, 0: 4096).  B = 1 runs the same tile kernels with padded columns.
 * All refusals are GPMPC_E_ARG with a text in gpmpc_last_error, before any launch: a NULL pointer, dimensions outside GPMPC_MAX_*, n < 1,
 * B / H < 1 (or B H above 2^40 Jacobian elements), ld < n, a chunk that is negative or no multiple of 64, a lambda or sigma_f that is not positive
 * and finite, a non-finite nominal model, a negative or non-finite diagonal entry of init_cov, action_var or process_var, u_stride <
 * action_dim or jac_stride < 2ds (2ds+da) with B > 1, outputs of a step that alias its inputs, flags other than GPMPC_WANT_GRAD
 * (GPMPC_USE_GRAPH and the GPMPC_FP32_* modes: not yet / never), out_jac without GPMPC_WANT_GRAD, a cost without out_cost (or without
 * out_grad under GPMPC_WANT_GRAD), constraint rows without out_g (out_gjac), bad constraint rows, a bad cost schedule, a cost with
 * action_dim = 0 or with a horizon beyond the cost kernel's LDS (about 48 KiB / (8 (2 + 2ds + da)) steps), constraint rows with
 * action_dim = 0; in gpmpc_mppi_solve_linearised
 * also what gpmpc_mppi_solve refuses.  A workspace below *_workspace_bytes (which return 0 for arguments that would be refused):
 * GPMPC_E_WORKSPACE.
 *
 * Two forms of the step (gpmpc_linearised_set_form; the step, the rollout and the MPPI solve all go through the one dispatcher):
 *   TILE    the 64-column MFMA tile kernels of csrc/linprop.hip, whatever B is: the form for large batches, and the default.
 *   STREAM  csrc/linprop_stream.hip, for a few columns: matrix-vector work.  k of one (column, GP) is a "vector"; vectors are taken
 *           GPMPC_LINPROP_STREAM_COLS at a time (with a matrix per GP: that many columns of one GP; with gp_stride = 0: that many
 *           consecutive (column, GP) pairs, so B = 1 with ds <= 4 is ONE pass over the one matrix for all GPs).  Every element of Kinv is
 *           fetched once per group, 16 bytes per lane along a row, and used for all its vectors: for the rows of Kinv k, and with the
 *           Jacobian for 32-row partial column sums of Kinv^T k, which a later kernel adds in ascending block order (no transposed read).
 *           q = k^T (Kinv k).  Three launches per step without the Jacobian, five with it, independent of the number of GPs; every GP
 *           evaluates its own exp.  Any B the TILE form takes is accepted (columns run 16 at a time); `chunk` is validated and not used.
 *   AUTO    STREAM when B <= GPMPC_LINPROP_AUTO_MAX_B, TILE above; bit for bit the form it picked.
 * The form is read on the host when a call is enqueued.  gpmpc_linearised_*_workspace_bytes return the need of the selected form (AUTO: the
 * larger of the two; TILE: the values they always returned).
 * STREAM, bit for bit: two identical calls agree; column c of a call of any B equals the B = 1 call on that column (every vector has its own
 * accumulators, also across a group or 16-column boundary); mean and variance are the same with and without the Jacobian; the rollout equals
 * the chain of step calls; out_g / out_gjac equal gpmpc_rollout_constraints on the returned arrays; gpmpc_mppi_solve_linearised equals the
 * host loop.  NOT bit for bit: STREAM against TILE (other summation routes); both are held to the same long double reference.
 * Not provided: switching the default form, the device L-BFGS / augmented-Lagrangian solvers on this
 * rule, graph capture, a form that reads one triangle of a symmetrised Kinv, second-order mean corrections, multi-GPU sharding, gradients
 * w.r.t. hyper-parameters or noise parameters.
 * ------------------------------------------------------------------------- */
#define GPMPC_LINPROP_FORM_TILE   0
#define GPMPC_LINPROP_FORM_STREAM 1
#define GPMPC_LINPROP_FORM_AUTO   2
#define GPMPC_LINPROP_FORM_DEFAULT GPMPC_LINPROP_FORM_TILE   /* every call returns the bits it always returned */
#define GPMPC_LINPROP_STREAM_COLS 4    /* vectors per pass over Kinv: 8 rows x 4 vectors of fp64 accumulators per lane */
/* MEASURED (profiles/linprop/stream_ab.txt; one MI355X, H = 20, ds = 4, da = 1, ms per call, median of five blocks; the reference of the
 * ratios is the TILE form of the commit before STREAM existed, timed in the same session): STREAM / TILE, objective only | with gradient
 *      B    N=2048, Kinv per GP   N=2048, one Kinv      N=300, Kinv per GP    sparse, M=256
 *      1    0.039 | 0.055         0.128 | 0.199         0.113 | 0.130         0.449 | 0.468
 *      2    0.040 | 0.057         0.129 | 0.200         0.114 | 0.127         0.457 | 0.477
 *      4    0.041 | 0.059         0.132 | 0.206         0.116 | 0.132         0.448 | 0.485
 *      8    0.055 | 0.071         0.147 | 0.230         0.116 | 0.136         0.450 | 0.474
 *     16    0.094 | 0.111         0.235 | 0.328         0.122 | 0.140         0.463 | 0.488
 *     32    0.189 | 0.219         0.464 | 0.654         0.242 | 0.274         0.894 | 0.972
 *     64    0.372 | 0.423         0.926 | 1.303         0.464 | 0.525         1.781 | 1.869
 *    256    1.490 | 1.678         3.646 | 5.121         1.766 | 1.968         7.379 | 8.198
 * 32 is the largest B of the grid at which STREAM is not slower than TILE on every shape, with and without the gradient. */
#define GPMPC_LINPROP_AUTO_MAX_B  32
/* Process-wide.  -1 only asks.  Returns the previous form; anything else is refused (GPMPC_E_ARG, gpmpc_last_error) and changes nothing. */
int gpmpc_linearised_set_form(int form);
/* One step of B plans: mu_prev, var_prev dev [B][ds]; U_t dev, input j of plan b at U_t[b u_stride + j] (NULL with da = 0); out_mu, out_var
 * dev [B][ds]; out_jac dev or NULL, the block of plan b at out_jac + b jac_stride (in doubles: a rollout writes [B][H][2ds][2ds+da] in
 * place).  Without out_jac neither dq/dz nor h is computed.  want_jac of the size query: whether out_jac will be given. */
size_t gpmpc_linearised_step_workspace_bytes(const gpmpc_gp_model* model_host, int B, int want_jac, int chunk);
int gpmpc_linearised_step(const gpmpc_gp_model* model_host, int B, const double* mu_prev, const double* var_prev, const double* U_t,
                          size_t u_stride, double* out_mu, double* out_var, double* out_jac, size_t jac_stride, int chunk,
                          void* workspace, size_t workspace_bytes, void* stream);
/* B rollouts of H steps on one stream, no host round trip, no allocation.  x0 dev [B][ds]; U dev [B][H][da]; out_means, out_vars dev
 * [B][H+1][ds] or NULL (kept in the workspace); out_jac dev [B][H][2ds][2ds+da] or NULL (GPMPC_WANT_GRAD only).  Means, variances and
 * Jacobians are bit for bit those of the chain of gpmpc_linearised_step calls.  flags: GPMPC_WANT_GRAD or 0; without it no Jacobian is
 * computed at all.  cost_host (or NULL: out_cost / out_grad are not touched): out_cost dev [B] and, with GPMPC_WANT_GRAD, out_grad dev
 * [B][H][da] from the tail kernel of gpmpc_rollout (the risk-sensitive cost on the diagonal covariances and its adjoint sweep over the step
 * Jacobians; cost schedules are honoured).  cons_host (or NULL): out_g dev [B][H][n_rows] and, with GPMPC_WANT_GRAD, out_gjac dev
 * [B][H n_rows][H da], bit for bit what gpmpc_rollout_constraints gives on the returned arrays. */
size_t gpmpc_linearised_rollout_workspace_bytes(const gpmpc_gp_model* model_host, int B, int H, unsigned flags, int chunk);
int gpmpc_linearised_rollout(const gpmpc_gp_model* model_host, int B, int H, const double* x0, const double* U,
                             const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host, unsigned flags,
                             double* out_means, double* out_vars, double* out_jac, double* out_cost, double* out_grad, double* out_g,
                             double* out_gjac, int chunk, void* workspace, size_t workspace_bytes, void* stream);
/* gpmpc_mppi_solve with a gpmpc_gp_model in the place of the pack: per iteration gpmpc_mppi_sample, gpmpc_linearised_rollout objective
 * only (flags 0, default chunk; with the constraint values when cons_host is given), gpmpc_mppi_update.  Outputs and trace as there. */
size_t gpmpc_mppi_solve_linearised_workspace_bytes(const gpmpc_gp_model* model_host, int H, const gpmpc_mppi_params* params_host,
                                                   const gpmpc_state_constraints* cons_host);
int gpmpc_mppi_solve_linearised(const gpmpc_gp_model* model_host, int H, const double* x0_dev, const double* start_dev,
                                const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host,
                                const gpmpc_mppi_params* params_host, double* out_U, double* out_best, double* out_trace, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Linearised propagation, full covariance, with a linear state feedback: the rule above with the whole Sigma carried and the predicted
 * input u_t = v_t + K_t (x_t - mu_t), as in the cautious-MPC literature (kernels in csrc/linprop_fc.hip).  The two
 * belong together: feedback makes the covariance of z = (x, u) non-diagonal by construction, Cov[x, u] = Sigma K^T.
 *
 * One step.  Inputs: the mean mu (ds), the symmetric covariance Sigma (ds x ds; only the upper triangle k <= l is read), the nominal input
 * v (da), a gain K (da x ds, or none: 0).  zbar = (mu, v), because the mean of u is v.  D = ds + da.  k_i, d_id, m_a, g_ad, q_a, r_a and
 * d q_a / d z_d are those of "Linearised propagation" above, nominal model included, evaluated at zbar.  For GP a:
 *     Hm_a[d][l] = sum_i beta_ia k_i (d_id d_il - [d = l] / lambda_ad)      (= d^2 m_a / d z_d d z_l; the nominal part has no curvature)
 *     T   = [I_ds ; K]  (D x ds)        Sz = T Sigma T^T + diag(0...0, action_var)        (D x D, symmetric)
 *     P_a = G_a T  (ds)                 i.e. P_ak = g_ak + sum_j g_a,ds+j K_jk             (the closed-loop gradient)
 *     W_b = Sz G_b^T  (D)
 *     mu'_a     = m_a
 *     Sigma'_ab = [a = b] (sf_a^2 - q_a + process_var_a) + G_a . W_b      (unclamped; computed for a <= b and mirrored: exactly symmetric)
 * Equivalently Sigma' = diag(s2) + P Sigma P^T + G_u diag(action_var) G_u^T.  The GPs are independent given z, so the latent part is
 * diagonal.  With K = 0 and a diagonal Sigma the diagonal of Sigma' is v' of the diagonal rule.
 *
 * State vector and Jacobian.  s = (mu_1 ... mu_ds, Sigma_kl for k <= l, row-major), of length p = ds + ds (ds + 1) / 2.  The step Jacobian
 * is [p][p + da], rows s', columns (s, v); an off-diagonal Sigma_kl = Sigma_lk counts as ONE variable; every element is written:
 *     d mu'_a / d mu_k = g_ak        d mu'_a / d v_j = g_a,ds+j        d mu'_a / d Sigma_kl = 0
 *     d Sigma'_ab / d zbar_d  = -[a = b] d q_a / d z_d + (Hm_a W_b)_d + (Hm_b W_a)_d          (d over the mu and the v columns)
 *     d Sigma'_ab / d Sigma_kl = P_ak P_bl + P_al P_bk  (k < l),   P_ak P_bk  (k = l)
 * For a = b, K = 0 and a diagonal Sigma the zbar columns are 2h - dq/dz of the diagonal rule.
 *
 * Rollout.  mu_0 = x0, Sigma_0 = init_cov, the whole matrix (the upper triangle, mirrored), as in the full-covariance moment-matching
 * forms; the step at t uses K_t.  The cost is the risk-sensitive cost on full covariances, the kernels behind gpmpc_cost / gpmpc_cost_grad
 * at (mu_t, Sigma_t, v_t), cost schedules honoured; the gradient is an adjoint sweep over the packed Jacobians seeded by d_means and
 * d_covs (the adjoint of the variable Sigma_kl, k < l, is d_covs[k][l] + d_covs[l][k]), plus d_U.  Chance constraints use the whole
 * matrix, g[t][r] = a_r . mu_t + kappa_r sqrt(a_r^T Sigma_t a_r) - b_r, their dense Jacobian [B][H n_rows][H da] from a forward-sensitivity
 * sweep over the packed Jacobians by the rules of gpmpc_rollout_constraints: a radicand <= 0 gives sd = 0 and no variance part, a NaN step
 * poisons its own rows only, columns tau >= t are exactly 0.0, every element is written.
 *
 * How it runs.  Stage A is the diagonal step itself, through the one dispatcher (TILE, STREAM or AUTO as selected), on a copy of the
 * model with action_var = 0 and a zeroed variance, with its Jacobian: that gives m, s2, g and -dq/dz, and holds all the O(N^2) work; out_mu
 * is bit for bit the out_mu of gpmpc_linearised_step in the same form.  New per step: k_lpf_hess (O(N D^2) per (plan, GP): the D (D + 1) / 2
 * second-derivative sums, N exp), k_lpf_hfin, and k_lpf_close (one wave per plan).  Without a Jacobian the Hessian pass is skipped; stage
 * A still computes g and dq/dz (Sigma' needs g), so the objective-only call costs more than the diagonal one's.  No atomics, fixed
 * summation orders, launch geometry from the sizes only: two identical calls agree bit for bit, nothing depends on `chunk`, Sigma' and
 * the mean are the same with and without the Jacobian, the rollout is the chain of step calls, out_g / out_gjac equal
 * gpmpc_linearised_fc_constraints on the returned arrays.
 *
 * The gain: const double* K_dev + size_t k_step_stride (in doubles).  NULL: no feedback.  Stride 0: one [da][ds] gain for every step;
 * stride da ds: [H][da][ds].  It lives in device memory: a closed loop can change it without touching an argument.
 *
 * Refusals (GPMPC_E_ARG with a text, before any launch): everything the diagonal entry points refuse, and a non-finite init_cov, an
 * asymmetric one (|P_kl - P_lk| > 1e-12 max |P|, the particles' rule) or one with a negative pivot; k_step_stride other than 0 or da ds; a
 * gain when da = 0; jac_stride < p (p + da) with B > 1; B H above 2^40 Jacobian elements; a horizon beyond the sweeps' grid.  The sweep
 * kernels keep no per-step state (the adjoint holds p doubles per plan in LDS, the constraints sweep 2 p doubles per lane), so unlike
 * the diagonal rule's tail kernel no LDS bounds H; the constraints sweep runs ceil(H da / 64) workgroups per plan along gridDim.y, which
 * gives the limit H da <= 64 x 65535.  The workspace-size queries return 0 for arguments that would be refused.
 *
 * MEASURED (profiles/linprop/fc_ab.txt; one MI355X, H = 20, ds = 4, da = 1, a Kinv per GP, ms per call, median of five alternating blocks;
 * the reference of the ratios is the diagonal linearised rollout of the same build): full / diagonal, objective only | with gradient
 *      shape, B             TILE              STREAM
 *      N=2048, B=1       1.285 | 1.055     2.360 | 1.768
 *      N=2048, B=16      1.284 | 1.039     1.789 | 1.380
 *      N=2048, B=256     1.342 | 1.065     1.533 | 1.025
 *      N=2048, B=4096    1.138 | 1.093     1.512 | 1.010
 *      N=300,  B=256     1.771 | 1.207     1.824 | 1.086
 *      sparse M=256, 256 2.269 | 1.826     1.739 | 1.105
 * With the gradient: the O(N D^2) pass and the per-plan close, small at N = 2048, visible at N = 300 and M = 256.  Objective only it is
 * worse than the operation count says, for the reason above (stage A delivers g only with its whole Jacobian).  Not measured: one Kinv for
 * all GPs, other ds / da / H, per-kernel times, hardware counters.
 * The input-cost term tr(R K Sigma K^T) and input constraints tightened by K Sigma K^T: "the commanded input", below.
 * Not provided: a gain per plan of a batch; the
 * device L-BFGS and augmented-Lagrangian solvers on this rule; graph capture; gains chosen by the optimiser; a
 * single-enqueue MPPI solve (the Python layer loops gpmpc_mppi_sample, this rollout, gpmpc_mppi_update).
 * ------------------------------------------------------------------------- */
/* One step of B plans.  mu_prev dev [B][ds]; cov_prev dev [B][ds][ds]; U_t dev, input j of plan b at U_t[b u_stride + j] (NULL with
 * da = 0); K_dev dev [da][ds] or NULL; out_mu dev [B][ds]; out_cov dev [B][ds][ds]; out_jac dev or NULL, the [p][p+da] block of plan b at
 * out_jac + b jac_stride.  want_jac of the size query: whether out_jac will be given. */
size_t gpmpc_linearised_fc_step_workspace_bytes(const gpmpc_gp_model* model_host, int B, int want_jac, int chunk);
int gpmpc_linearised_fc_step(const gpmpc_gp_model* model_host, int B, const double* mu_prev, const double* cov_prev, const double* U_t,
                             size_t u_stride, const double* K_dev, double* out_mu, double* out_cov, double* out_jac, size_t jac_stride,
                             int chunk, void* workspace, size_t workspace_bytes, void* stream);
/* B rollouts of H steps.  The arguments of gpmpc_linearised_rollout, except: out_covs dev [B][H+1][ds][ds] in the place of out_vars,
 * out_jac dev [B][H][p][p+da], and the gain pair. */
size_t gpmpc_linearised_fc_rollout_workspace_bytes(const gpmpc_gp_model* model_host, int B, int H, unsigned flags, int chunk);
int gpmpc_linearised_fc_rollout(const gpmpc_gp_model* model_host, int B, int H, const double* x0, const double* U, const double* K_dev,
                                size_t k_step_stride, const gpmpc_cost_params* cost_host, const gpmpc_state_constraints* cons_host,
                                unsigned flags, double* out_means, double* out_covs, double* out_jac, double* out_cost, double* out_grad,
                                double* out_g, double* out_gjac, int chunk, void* workspace, size_t workspace_bytes, void* stream);
/* Pure function of a propagated trajectory, like gpmpc_rollout_vjp: jac dev [B][H][p][p+da]; g_means dev [B][H+1][ds], g_covs dev
 * [B][H+1][ds][ds] (upstream gradients of every step's mean / covariance entries; either may be NULL: zero) -> out_gU dev [B][H][da]
 * and, unless NULL, out_gx0 dev [B][ds]. */
int gpmpc_linearised_fc_vjp(int B, int H, int state_dim, int action_dim, const double* jac_dev, const double* g_means,
                            const double* g_covs, double* out_gU, double* out_gx0, void* stream);
/* Pure function of a propagated trajectory, like gpmpc_rollout_constraints: means dev [B][H+1][ds], covs dev [B][H+1][ds][ds], jac dev
 * [B][H][p][p+da] (NULL with out_gjac NULL) -> out_g dev [B][H][n_rows] and, unless NULL, out_gjac dev [B][H n_rows][H da]. */
int gpmpc_linearised_fc_constraints(int B, int H, int state_dim, int action_dim, const gpmpc_state_constraints* cons_host,
                                    const double* means, const double* covs, const double* jac_dev, double* out_g, double* out_gjac,
                                    void* stream);

/* ---------------------------------------------------------------------------
 * Linearised propagation, full covariance: the commanded input (kernels in csrc/linprop_inputs.hip).  With a gain the
 * controller's input is a random variable.  Commanded input of step t = 0 ... H-1: mean v_t, covariance Su_t = K_t Sigma_t K_t^T (da x da),
 * K_t through the K_dev / k_step_stride pair of gpmpc_linearised_fc_rollout.  action_var stays what it is, actuator noise added inside
 * Sz, and is not part of Su_t.  K = NULL means Su_t = 0.
 *
 * Input cost.  c_b = sum_{j=0}^{H-1} tr(R K_j Sigma_j K_j^T) = sum_j sum_{a,b,k,l} R_ab K_bk Sigma_j[k][l] K_al, R that of the cost struct,
 * general and not necessarily symmetric.  It is the expectation of the input term (u - u_ref)^T R (u - u_ref) minus its value at the
 * mean, so it depends neither on u_ref nor on a cost schedule.  Local derivative in the convention of gpmpc_cost_grad (a general,
 * possibly non-symmetric Sigma):  d c / d Sigma_j[k][l] = sum_{a,b} K_al R_ab K_bk for j < H, and 0 for j = H.  Step 0 contributes a
 * constant (Sigma_0 = init_cov).  The steps are summed in ascending order by one workgroup per plan; no atomics.
 *
 * Input chance constraints.  Rows c_r . u <= d_r held with the quantile kappa_r: for t = 0 ... H-1 and row r, with a = K_t^T c_r (ds),
 *     q = a^T Sigma_t a      sd = sqrt(q)      g_u[t][r] = c_r . v_t + kappa_r sd - d_r   <= 0
 * by the rules of gpmpc_linearised_fc_constraints: q <= 0 gives sd = 0 and no variance part; a NaN in v_t or Sigma_t makes the rows of
 * step t NaN, and no other step's.  out_gu [B][H][n_u]; out_gujac [B][H n_u][H da], row t n_u + r, column tau da + j, every element
 * written.  With S_t the sensitivities of the packed state of step t (before the step is taken):
 *     tau > t :  exactly 0.0
 *     tau = t :  c_rj
 *     tau < t :  (kappa_r / (2 sd)) sum_{k<=l} w_kl S_t[Sigma_kl][tau, j],    w_kk = a_k^2,  w_kl = 2 a_k a_l (k < l)
 * Row t = 0 therefore has only its tau = 0 block.  The sweep is that of gpmpc_linearised_fc_constraints: grid (B, ceil(H da / 64)), one lane
 * per column, the sensitivities in LDS; values only when out_gujac is NULL.
 *
 * gpmpc_linearised_fc_rollout_inputs is gpmpc_linearised_fc_rollout with both: the existing launches, the input-cost kernel between
 * gpmpc_cost_grad and the adjoint sweep, the input-constraint kernel at the end.  With input_cost = 0 and ucons_host = NULL every output
 * is bit for bit the old entry's; means, covs, jac, g and g_jac are never affected; out_cost[b] = cost_plain[b] + c_b, one rounding, c_b as
 * gpmpc_feedback_input_cost returns it; out_grad is bit for bit d_U + gpmpc_linearised_fc_vjp(jac, d_means, d_covs + out_dcovs), the sum
 * of the two seeds being one rounding per element; out_gu / out_gujac are bit for bit gpmpc_feedback_input_constraints on the returned
 * arrays; objective only, the values are the same bits.  The workspace is that of gpmpc_linearised_fc_rollout.
 *
 * Refusals (GPMPC_E_ARG with a text, before any launch): everything gpmpc_linearised_fc_rollout refuses; action_dim < 1; n_rows outside
 * 1...GPMPC_MAX_CONS, a negative or NaN kappa; input_cost without a cost; out_gu / out_gujac not given exactly when ucons_host is (the
 * Jacobian only with GPMPC_WANT_GRAD); k_step_stride other than 0 or da ds.  The size query returns 0 for arguments that would be refused.
 *
 * Particles under the same feedback (the Monte-Carlo check of both effects).  u^p = v_b + K_t (x^p - mu_b), summed over k in ascending
 * order (gpmpc_particle_inputs; K_t = NULL copies v_b); gpmpc_particle_step_inputs is gpmpc_particle_step with an input per particle,
 * U_p dev [B P][da], in the place of U_t / u_stride (a variant of the assemble kernel; everything downstream is unchanged: action noise
 * is added to U_p as it is to U_t).  gpmpc_particle_rollout_feedback takes the arguments of gpmpc_particle_rollout plus the gain pair,
 * mu_ref dev [B][H+1][ds] (the mean trajectory the gain acts around, e.g. out_means of the linearised rollout) and the input rows; its
 * particles are bit for bit the chain gpmpc_particle_noise -> gpmpc_particle_inputs -> gpmpc_particle_step_inputs, and with K_dev = NULL
 * bit for bit those of gpmpc_particle_rollout: the same noise addressing, no new normals.  gpmpc_particle_input_stats follows the rules
 * of gpmpc_particle_stats on inputs [H][B P][da]: fixed-order sums, a two-pass covariance with divisor P - 1, exactly symmetric, a
 * violation is c_r . u > d_r, the joint figure runs over all rows and all steps 0 ... H-1.  Refused besides what the sibling entries
 * refuse: action_dim < 1, bad rows, a k_step_stride other than 0 or da ds, a NULL mu_ref together with a gain, out_uviol / out_ujoint not
 * given exactly when the rows are.
 *
 * Measurements, and what has not been measured: DESIGN.md section 3n.
 * Not provided: the rate term R_delta under feedback (its feedback part needs cross-step covariances: R_delta stays on the nominal
 * inputs); a gain per plan; gains chosen by the optimiser; the device L-BFGS / augmented-Lagrangian solvers on this rule; the
 * particle-cost planner under feedback; graph capture.
 * ------------------------------------------------------------------------- */
typedef struct gpmpc_input_constraints {
    int n_rows;                                       /* 1...GPMPC_MAX_CONS */
    int reserved;
    double C[GPMPC_MAX_CONS * GPMPC_MAX_D];           /* [n_rows][da] row-major in the leading n_rows*da entries */
    double d[GPMPC_MAX_CONS];
    double kappa[GPMPC_MAX_CONS];
} gpmpc_input_constraints;
/* Pure function of a trajectory, like gpmpc_linearised_fc_vjp: K_dev dev [da][ds] (k_step_stride 0) or [H][da][ds] (da ds), or NULL;
 * covs dev [B][H+1][ds][ds] -> out_c dev [B] and, unless NULL, out_dcovs dev [B][H+1][ds][ds], every element written. */
int gpmpc_feedback_input_cost(int B, int H, int state_dim, int action_dim, const gpmpc_cost_params* cost_host, const double* K_dev,
                              size_t k_step_stride, const double* covs_dev, double* out_c, double* out_dcovs, void* stream);
/* Pure function of a trajectory: U dev [B][H][da], covs dev [B][H+1][ds][ds], jac dev [B][H][p][p+da] (NULL with out_gujac NULL)
 * -> out_gu dev [B][H][n_rows] and, unless NULL, out_gujac dev [B][H n_rows][H da]. */
int gpmpc_feedback_input_constraints(int B, int H, int state_dim, int action_dim, const gpmpc_input_constraints* ucons_host,
                                     const double* K_dev, size_t k_step_stride, const double* U_dev, const double* covs_dev,
                                     const double* jac_dev, double* out_gu, double* out_gujac, void* stream);
size_t gpmpc_linearised_fc_rollout_inputs_workspace_bytes(const gpmpc_gp_model* model_host, int B, int H, unsigned flags, int chunk,
                                                          int input_cost, const gpmpc_input_constraints* ucons_host);
int gpmpc_linearised_fc_rollout_inputs(const gpmpc_gp_model* model_host, int B, int H, const double* x0, const double* U,
                                       const double* K_dev, size_t k_step_stride, const gpmpc_cost_params* cost_host,
                                       const gpmpc_state_constraints* cons_host, unsigned flags, double* out_means, double* out_covs,
                                       double* out_jac, double* out_cost, double* out_grad, double* out_g, double* out_gjac, int input_cost,
                                       const gpmpc_input_constraints* ucons_host, double* out_gu, double* out_gujac, int chunk,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* out_u dev [B P][da] from x_prev dev [B P][ds], input j of plan b at U_t[b u_stride + j], K_t dev [da][ds] or NULL, the mean of plan b
 * at mu_t + b mu_stride (NULL only with K_t NULL). */
int gpmpc_particle_inputs(int B, int P, int state_dim, int action_dim, const double* x_prev, const double* U_t, size_t u_stride,
                          const double* K_t, const double* mu_t, size_t mu_stride, double* out_u, void* stream);
size_t gpmpc_particle_step_inputs_workspace_bytes(const gpmpc_gp_model* model_host, int B, int P, int chunk);
int gpmpc_particle_step_inputs(const gpmpc_gp_model* model_host, int B, int P, const double* x_prev, const double* U_p, const double* eps,
                               double* out_next, double* out_mean, double* out_var, int chunk, void* workspace, size_t workspace_bytes,
                               void* stream);
/* inputs dev [H][B P][da] -> out_umean dev [B][H][da], out_ucov dev [B][H][da][da] (either may be NULL), and with rows out_uviol dev
 * [B][H][n_rows], out_ujoint dev [B] (both NULL without). */
int gpmpc_particle_input_stats(int B, int P, int H, int action_dim, const double* inputs, const gpmpc_input_constraints* ucons_host,
                               double* out_umean, double* out_ucov, double* out_uviol, double* out_ujoint, void* stream);
/* want_inputs of the size query: whether out_inputs will be given (without it the inputs of all steps live in the workspace). */
size_t gpmpc_particle_rollout_feedback_workspace_bytes(const gpmpc_gp_model* model_host, int B, int P, int H, int chunk, int want_inputs);
int gpmpc_particle_rollout_feedback(const gpmpc_gp_model* model_host, int B, int P, int H, const double* x0, const double* U,
                                    unsigned long long seed, unsigned call_index, const gpmpc_state_constraints* cons_host,
                                    double* out_particles, double* out_mean, double* out_cov, int* out_clamped, double* out_viol,
                                    double* out_joint, const double* K_dev, size_t k_step_stride, const double* mu_ref,
                                    const gpmpc_input_constraints* ucons_host, double* out_inputs, double* out_umean, double* out_ucov,
                                    double* out_uviol, double* out_ujoint, int chunk, void* workspace, size_t workspace_bytes,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPMPC_H */
