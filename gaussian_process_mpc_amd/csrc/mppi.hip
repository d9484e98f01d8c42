// MPPI (model-predictive path integral) planner on the device (include/gpmpc.h): K perturbed copies of the current plan
// are rolled out as ONE objective-only batch, the plan moves to their softmin-weighted mean, the best sample seen is kept.
//
//   k_mppi_sample   U[k][c] = clamp(mean[c] + sigma_j decay^it eps[k][c], lb_j, ub_j),  c = t da + j;  slot k = 0 is the mean itself.
//                   eps is counter-based (Philox4x32-10 + Box-Muller): a pure function of (seed, call index, iteration, element), whatever
//                   the grid.  One thread = one Philox counter = two normals = the elements e = 2p, 2p + 1 of the flattened [K][n] block.
//   k_mppi_update   scores the batch (cost, or total constraint violation while nothing is feasible), keeps the best sample, and writes
//                   the softmin-weighted mean.  Lanes run along c (coalesced rows of U), the four waves of a workgroup take a quarter of
//                   the samples each and are combined through LDS in a fixed order; scores and weights are recomputed by every workgroup
//                   (K <= 4096 values: cheaper than a second launch).  No atomics: every sum has one fixed order, the result for column c
//                   does not depend on the grid.
//
// Summation orders (tests/mppi_reference.py restates them; the trace of a solve is compared exactly):
//   v_k       sequential over the H m_c constraint values of sample k, v <- v + max(g, 0)
//   sums over k (sum of the finite scores, sum of the weights): thread i of 256 adds the terms k = i, i + 256, ... in ascending order,
//             then the 256 partial sums are folded in halves, p[i] <- p[i] + p[i + h], h = 128, 64, ... 1
//   mean[c]   wave w adds w_k U[k][c] over its quarter of the samples in ascending k (zero weights skipped), the four are added in wave
//             order, one division by the sum of the weights
#include "mppi_internal.h"   // the search itself, shared with linprop.hip and particle_cost.hip
#include <cmath>

#include "philox.h"      // Philox4x32-10, the 53-bit uniform, the fixed-order folds (shared with particles.hip)

// grid: ceil(max(ceil(K n / 2), K ds) / 256) x 256 threads.  P travels by value: sigma, bounds, seed and call index are kernel arguments.
__global__ __launch_bounds__(MPPI_THREADS) void k_mppi_sample(int n, int da, int ds, gpmpc_mppi_params P, unsigned iteration, double scale,
                                                              const double* __restrict__ mean, const double* __restrict__ x0,
                                                              double* __restrict__ U, double* __restrict__ x0b) {
    const long p = (long)blockIdx.x * MPPI_THREADS + threadIdx.x;
    const long total = (long)P.n_samples * n;
    if (x0b && p < (long)P.n_samples * ds) x0b[p] = x0[p % ds];          // the start state once per sample, for the rollout
    const long e0 = 2 * p;
    if (e0 >= total) return;
    const Philox4 r = philox4x32_10((unsigned)p, (unsigned)((unsigned long long)p >> 32), iteration, P.call_index,
                                    (unsigned)P.seed, (unsigned)(P.seed >> 32));
    const double u1 = mppi_uniform(r.w[0], r.w[1]), u2 = mppi_uniform(r.w[2], r.w[3]);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long e = e0 + h;
        if (e >= total) break;                                           // an odd last element uses half a counter
        const int c = (int)(e % n), j = c % da;
        const double m = mean[c];
        const double v = m + (P.sigma[j] * scale) * (rad * (h ? sn : cs));
        U[e] = e < n ? m : fmin(fmax(v, P.lb[j]), P.ub[j]);              // slot 0 is the mean, bit for bit: its noise is discarded
    }
}

// ---------------------------------------------------------------------------
// update
// ---------------------------------------------------------------------------
// grid: ceil(n / 64) workgroups of 256 threads; workgroup x owns the columns [64 x, 64 x + 64) of mean and best.
// best_in / best_out [2 + n] = (violation, cost, plan) must not alias: every workgroup decides from the OLD key, and every element of
// best_out is written (the old entry where the new key is not strictly smaller).  mean is written, never read; untouched with no sample alive.
__global__ __launch_bounds__(MPPI_THREADS) void k_mppi_update(int K, int n, int m, double beta, const double* __restrict__ U,
                                                              const double* __restrict__ cost, const double* __restrict__ g,
                                                              double* __restrict__ mean, const double* __restrict__ best_in,
                                                              double* __restrict__ best_out, double* __restrict__ trace) {
    __shared__ double sw[GPMPC_MPPI_MAX_SAMPLES];       // v_k (NaN: dead), then the score s_k, then the weight w_k
    __shared__ double red[MPPI_THREADS];
    __shared__ int redi[MPPI_THREADS];
    __shared__ double part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_huge_val();

    // 1. violation and liveness of every sample
    int nfeas = 0, nalive = 0;
    for (int k = tid; k < K; k += MPPI_THREADS) {
        const double ck = cost[k];
        bool dead = ck != ck;
        double v = 0.0;
        if (g) {
            const double* __restrict__ gk = g + (size_t)k * m;
            for (int i = 0; i < m; ++i) {
                const double gi = gk[i];
                dead |= gi != gi;
                v = v + (gi > 0.0 ? gi : 0.0);
            }
        }
        sw[k] = dead ? __builtin_nan("") : v;
        nalive += dead ? 0 : 1;
        nfeas += (!dead && v == 0.0) ? 1 : 0;
    }
    nfeas = mppi_fold_count(nfeas, redi);
    nalive = mppi_fold_count(nalive, redi);
    const double old_v = best_in[0], old_c = best_in[1];
    const int c = blockIdx.x * 64 + lane;
    if (nalive == 0) {                                  // (uniform over the grid) nothing to learn from: mean and best stay
        if (wave == 0 && c < n) best_out[2 + c] = best_in[2 + c];
        if (blockIdx.x == 0 && tid == 0) {
            best_out[0] = old_v; best_out[1] = old_c;
            trace[0] = old_v; trace[1] = old_c; trace[2] = 0.0; trace[3] = 0.0; trace[4] = inf; trace[5] = 0.0;
        }
        return;
    }
    const bool restore = nfeas == 0;                    // feasibility restoration: the score is the violation

    // 2. scores; candidates are the feasible samples, or the alive ones under restoration.  argmin with the lowest index on ties
    double bs = inf, fsum = 0.0;
    int bk = 0x7fffffff, nfin = 0;
    for (int k = tid; k < K; k += MPPI_THREADS) {
        const double v = sw[k];
        const bool cand = restore ? v == v : v == 0.0;
        const double s = cand ? (restore ? v : cost[k]) : inf;
        sw[k] = cand ? s : __builtin_nan("");           // NaN marks a sample that is no candidate (a candidate's score may be +inf)
        if (cand && (bk == 0x7fffffff || s < bs)) { bs = s; bk = k; }
        const bool fin = cand && s - s == 0.0;          // finite
        fsum = fsum + (fin ? s : 0.0);
        nfin += fin ? 1 : 0;
    }
    red[tid] = bs; redi[tid] = bk;
    __syncthreads();
    for (int h = MPPI_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const double s2 = red[tid + h]; const int k2 = redi[tid + h];
            const int k1 = redi[tid];
            if (k2 != 0x7fffffff && (k1 == 0x7fffffff || s2 < red[tid] || (s2 == red[tid] && k2 < k1))) { red[tid] = s2; redi[tid] = k2; }
        }
        __syncthreads();
    }
    const double smin = red[0];
    const int kstar = redi[0];
    __syncthreads();
    fsum = mppi_fold_sum(fsum, red);
    nfin = mppi_fold_count(nfin, redi);

    // 3. temperature and weights
    const double T = nfin > 0 ? beta * (fsum / (double)nfin - smin) : 0.0;
    const bool soft = T > 0.0 && T < inf;               // else: weight 1 on the candidates that tie with the minimum
    double wsum = 0.0;
    for (int k = tid; k < K; k += MPPI_THREADS) {
        const double s = sw[k];
        double w = 0.0;
        if (s == s) {
            if (soft) w = (s - s == 0.0) ? exp(-(s - smin) / T) : 0.0;
            else w = s == smin ? 1.0 : 0.0;
        }
        sw[k] = w;
        wsum = wsum + w;
    }
    wsum = mppi_fold_sum(wsum, red);                    // (its barriers also publish sw) >= 1: the weight of kstar is exp(0) or 1

    // 4. weighted mean of this workgroup's columns
    const int kq = (K + 3) / 4, k0 = wave * kq, k1 = (k0 + kq < K) ? k0 + kq : K;
    double acc = 0.0;
    if (c < n)
        for (int k = k0; k < k1; ++k) {
            const double w = sw[k];
            if (w != 0.0) acc = acc + w * U[(size_t)k * n + c];
        }
    part[wave][lane] = acc;
    __syncthreads();

    // 5. the best sample seen: key (violation, cost), lexicographic, replaced only by a strictly smaller one
    const double new_v = restore ? smin : 0.0, new_c = cost[kstar];
    const bool better = new_v < old_v || (new_v == old_v && new_c < old_c);
    if (wave == 0 && c < n) {
        mean[c] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / wsum;
        best_out[2 + c] = better ? U[(size_t)kstar * n + c] : best_in[2 + c];
    }
    if (blockIdx.x == 0 && tid == 0) {
        const double bv = better ? new_v : old_v, bc = better ? new_c : old_c;
        best_out[0] = bv; best_out[1] = bc;
        trace[0] = bv; trace[1] = bc; trace[2] = (double)nfeas; trace[3] = (double)nalive; trace[4] = smin; trace[5] = T;
    }
}

// ---------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------
// the part of the parameters that needs no dimension
int gpmpc_mppi_check_scalars(const gpmpc_mppi_params* P, const char* who) {
    if (!P) return GPMPC_E_ARG;
    if (P->n_samples < 1 || P->n_samples > GPMPC_MPPI_MAX_SAMPLES)
        return gpmpc_refuse(who, "n_samples = %d outside 1..%d", P->n_samples, GPMPC_MPPI_MAX_SAMPLES);
    if (P->iterations < 1) return gpmpc_refuse(who, "iterations = %d is less than 1", P->iterations);
    if (!(P->sigma_decay > 0.0)) return gpmpc_refuse(who, "sigma_decay = %g is not positive", P->sigma_decay);
    if (!(P->beta > 0.0)) return gpmpc_refuse(who, "beta = %g is not positive", P->beta);
    return GPMPC_OK;
}

// sigma and the bounds of input j are checked together, input by input
int gpmpc_mppi_check_inputs(const gpmpc_mppi_params* P, int da, const char* who) {
    for (int j = 0; j < da; ++j) {
        if (!(P->sigma[j] > 0.0)) return gpmpc_refuse(who, "sigma[%d] = %g is not positive", j, P->sigma[j]);
        if (!(P->lb[j] <= P->ub[j])) return gpmpc_refuse(who, "lb[%d] = %g exceeds ub[%d] = %g", j, P->lb[j], j, P->ub[j]);      // lb > ub, or NaN
    }
    return GPMPC_OK;
}

int gpmpc_mppi_launch_sample(int H, int ds, int da, const gpmpc_mppi_params& P, int iteration, const double* mean, const double* x0, double* U,
                             double* x0b, hipStream_t s) {
    const long n = (long)H * da, pairs = ((long)P.n_samples * n + 1) / 2, states = x0b ? (long)P.n_samples * ds : 0;
    const long threads = pairs > states ? pairs : states;
    const double scale = pow(P.sigma_decay, (double)iteration);
    hipLaunchKernelGGL(k_mppi_sample, dim3((unsigned)((threads + MPPI_THREADS - 1) / MPPI_THREADS)), dim3(MPPI_THREADS), 0, s, (int)n, da, ds,
                       P, (unsigned)iteration, scale, mean, x0, U, x0b);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_mppi_sample(int H, int ds, int da, const gpmpc_mppi_params* P, int iteration, const double* mean, const double* x0,
                                 double* out_U, double* out_x0_batch, void* stream) {
    if (!P || !mean || !out_U || iteration < 0 || !gpmpc_solver_dims_ok(H, ds, da) || (out_x0_batch && (!x0 || ds < 1))) return GPMPC_E_ARG;
    if (int rc = gpmpc_mppi_check_scalars(P, "gpmpc_mppi_sample")) return rc;
    if (int rc = gpmpc_mppi_check_inputs(P, da, "gpmpc_mppi_sample")) return rc;
    return gpmpc_mppi_launch_sample(H, ds, da, *P, iteration, mean, x0, out_U, out_x0_batch, (hipStream_t)stream);
}

extern "C" int gpmpc_mppi_update(int K, int H, int da, int n_rows, double beta, const double* U, const double* cost, const double* g,
                                 double* mean, const double* best_in, double* best_out, double* out_trace, void* stream) {
    if (!U || !cost || !mean || !best_in || !best_out || !out_trace || !gpmpc_solver_dims_ok(H, 0, da)) return GPMPC_E_ARG;
    if (K < 1 || K > GPMPC_MPPI_MAX_SAMPLES) return gpmpc_refuse("gpmpc_mppi_update", "the number of samples is outside 1..GPMPC_MPPI_MAX_SAMPLES");
    if (!(beta > 0.0)) return gpmpc_refuse("gpmpc_mppi_update", "beta is not positive");
    if (best_in == best_out) return gpmpc_refuse("gpmpc_mppi_update", "best_in and best_out must be different buffers");
    if (n_rows < 0 || n_rows > GPMPC_MAX_CONS || (g != nullptr) != (n_rows > 0))
        return gpmpc_refuse("gpmpc_mppi_update", "constraint values and n_rows in 1..GPMPC_MAX_CONS are given together (NULL and 0 without constraints)");
    const int n = H * da;
    hipLaunchKernelGGL(k_mppi_update, dim3((n + 63) / 64), dim3(MPPI_THREADS), 0, (hipStream_t)stream, K, n, H * n_rows, beta, U, cost, g, mean,
                       best_in, best_out, out_trace);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// workspace of a solve: the head of every MPPI solve (mppi_internal.h) | the rollout's own workspace
struct MppiLayout { gpmpc_mppi_head head; size_t off_roll, total; gpmpc_solver_eval_layout roll; };
static MppiLayout mppi_layout(const gpmpc_pack* p, int H, int K, int m_c, gpmpc_solver_rule rule) {
    MppiLayout L;
    gpmpc_carver c;
    L.head = gpmpc_mppi_head_take(c, H, p->ds, p->da, K, m_c);
    L.roll = gpmpc_solver_eval_bytes(rule, p, K, H, m_c != 0, 0);
    L.off_roll = c.take(L.roll.total);
    L.total = c.total();
    return L;
}

static size_t mppi_solve_bytes(gpmpc_solver_rule rule, const gpmpc_pack* p, int H, const gpmpc_mppi_params* P, const gpmpc_state_constraints* cons) {
    if (!p || !P || P->n_samples < 1 || P->n_samples > GPMPC_MPPI_MAX_SAMPLES) return 0;
    if (cons && (cons->n_rows < 1 || cons->n_rows > GPMPC_MAX_CONS)) return 0;
    if (!gpmpc_solver_dims_ok(H, p->ds, p->da)) return 0;
    return mppi_layout(p, H, P->n_samples, cons ? cons->n_rows : 0, rule).total;
}
extern "C" size_t gpmpc_mppi_solve_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_mppi_params* P, const gpmpc_state_constraints* cons) {
    return mppi_solve_bytes(GPMPC_RULE_DIAGONAL, p, H, P, cons);
}
extern "C" size_t gpmpc_mppi_solve_fullcov_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_mppi_params* P,
                                                           const gpmpc_state_constraints* cons) {
    return mppi_solve_bytes(GPMPC_RULE_FULLCOV, p, H, P, cons);
}

// the search of both entries; the rule decides the one evaluation (solver_frame.h)
static int mppi_solve(gpmpc_solver_rule rule, const char* who, const gpmpc_pack* p, int H, const double* x0, const double* start,
                      const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, const gpmpc_mppi_params* P, double* out_U,
                      double* out_best, double* out_trace, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !x0 || !start || !cost || !P || !out_U || !out_best || !out_trace || !workspace || H < 1) return GPMPC_E_ARG;
    if (int rc = gpmpc_mppi_check_scalars(P, who)) return rc;            // (before the pack is looked at)
    if (int rc = gpmpc_solver_enter(p, H, cost, cons, who, [&](int da) { return gpmpc_mppi_check_inputs(P, da, who); }, rule)) return rc;
    const int K = P->n_samples, m_c = cons ? cons->n_rows : 0;
    const MppiLayout L = mppi_layout(p, H, K, m_c, rule);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    char* ws = (char*)workspace;
    auto eval = [&](int, const double* x0b, const double* U, double* cst, double* g) {
        return gpmpc_solver_eval(rule, p, K, H, x0b, U, cost, cons, 0, cst, nullptr, g, nullptr, ws + L.off_roll, L.roll, stream);
    };
    return gpmpc_mppi_search(L.head, ws, H, p->ds, p->da, m_c, P, x0, start, eval, out_U, out_best, out_trace, stream);
}

extern "C" int gpmpc_mppi_solve(const gpmpc_pack* p, int H, const double* x0, const double* start, const gpmpc_cost_params* cost,
                                const gpmpc_state_constraints* cons, const gpmpc_mppi_params* P, double* out_U, double* out_best,
                                double* out_trace, void* workspace, size_t workspace_bytes, void* stream) {
    return mppi_solve(GPMPC_RULE_DIAGONAL, "gpmpc_mppi_solve", p, H, x0, start, cost, cons, P, out_U, out_best, out_trace, workspace,
                      workspace_bytes, stream);
}

extern "C" int gpmpc_mppi_solve_fullcov(const gpmpc_pack* p, int H, const double* x0, const double* start, const gpmpc_cost_params* cost,
                                        const gpmpc_state_constraints* cons, const gpmpc_mppi_params* P, double* out_U, double* out_best,
                                        double* out_trace, void* workspace, size_t workspace_bytes, void* stream) {
    return mppi_solve(GPMPC_RULE_FULLCOV, "gpmpc_mppi_solve_fullcov", p, H, x0, start, cost, cons, P, out_U, out_best, out_trace, workspace,
                      workspace_bytes, stream);
}
