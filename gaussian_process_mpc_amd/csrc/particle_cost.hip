// Particle cost: the entropic risk of the stage cost and empirical quantiles of the constraint margins over the particles of a rollout
// (gpmpc_particle_cost), the streaming evaluation that never stores the horizon (gpmpc_particle_evaluate), and MPPI over it
// (gpmpc_mppi_solve_particles).  Formulas, refusals and the bit-for-bit properties: include/gpmpc.h, "Particle cost"; the why and the
// measurements: DESIGN.md section 3m.
//
//   k_pc_step    one workgroup of 256 threads per (plan, step).  Thread i owns the particles i, i + 256, ... (ascending, as k_pt_stats):
//                c_p = e^T Q e in registers, a flag reduction for NaN coordinates, the exact maximum of a_p = -(gamma / 2) c_p, the sum of
//                exp(a_p - M) per thread and then folded in halves; per constraint row the margins go to LDS, padded with -inf to the next
//                power of two, a bitonic sort puts them in ascending order and ONE order statistic is read.
//   k_pc_close   one lane per plan: J = sum_i s_i (ascending) + the input terms of gpmpc_cost.
// Rules: no atomics; every output element is owned by one workgroup or one lane, which sums in a fixed order; launch geometry depends on
// sizes (and on which optional outputs are given) only.
// Host: the model is checked by particles.hip (gpmpc_pt_check_model: the core of model_frame.h, then the noise model), sizes and chunk by
// model_frame.h; gpmpc_mppi_solve_particles is its entry checks and gpmpc_mppi_search (mppi_internal.h) with pc_evaluate as the evaluation.
#include <cmath>
#include "model_frame.h"
#include "philox.h"
#include "particles_internal.h"
#include "mppi_internal.h"

#define PC_PER_THREAD (GPMPC_PARTICLE_COST_MAX_P / MPPI_THREADS)
#define PC_MAX_NORMALS (GPMPC_MAX_D + GPMPC_MAX_DS)

struct PcQuant { int m[GPMPC_MAX_CONS]; };     // m_r = floor(eps_r P + 1e-9) particles may violate row r

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// The input and input-rate terms of cost.hip::input_cost: the same operations in the same order (no contraction: the build has
// -ffp-contract=off), so the value is bit for bit what gpmpc_cost adds.  Loops run to the compile-time maxima under a predicate: no
// runtime-indexed per-thread array.
template <bool SCHED>
__device__ static double pc_input_cost(int H, int da, const gpmpc_cost_params& C, const double* __restrict__ uref_rows,
                                       const double* __restrict__ U) {
    double c = 0.0;
    for (int j = 0; j < H; ++j) {
        double d[GPMPC_MAX_D];
#pragma unroll
        for (int k = 0; k < GPMPC_MAX_D; ++k) d[k] = k < da ? U[j * da + k] - (SCHED ? uref_rows[(size_t)j * da + k] : C.u_ref[k]) : 0.0;
#pragma unroll
        for (int k = 0; k < GPMPC_MAX_D; ++k) {
            if (k >= da) continue;
            double rd = 0.0;
#pragma unroll
            for (int l = 0; l < GPMPC_MAX_D; ++l)
                if (l < da) rd += C.R[k * da + l] * d[l];
            c += d[k] * rd;
        }
        if (C.has_R_delta) {
#pragma unroll
            for (int k = 0; k < GPMPC_MAX_D; ++k) d[k] = k < da ? U[j * da + k] - (j == 0 ? C.last_u[k] : U[(j - 1) * da + k]) : 0.0;
#pragma unroll
            for (int k = 0; k < GPMPC_MAX_D; ++k) {
                if (k >= da) continue;
                double rd = 0.0;
#pragma unroll
                for (int l = 0; l < GPMPC_MAX_D; ++l)
                    if (l < da) rd += C.R_delta[k * da + l] * d[l];
                c += d[k] * rd;
            }
        }
    }
    return c;
}

// the maximum of 256 per-thread values (exact, so the order does not matter); returned to every thread, `red` free again after the call
__device__ __forceinline__ double pc_fold_max(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = MPPI_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) red[t] = fmax(red[t], red[t + h]);
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// grid (steps, B).  X: the particles of step i0 on, [i1 - i0][B P][ds]; workgroup (x, b) takes the steps i0 + x, i0 + x + gridDim.x, ... < i1
// of plan b.  stage [B][H + 1] or null; out_g [B][H][n_rows] (n_rows > 0).  out_cost non-null (then gridDim.x = 1 and the launch covers
// the steps 0 ... H): thread 0 adds the stage costs in ascending order and the input terms -- k_pc_close without a stage buffer.
template <bool SCHED>
__global__ __launch_bounds__(MPPI_THREADS) void k_pc_step(int B, int P, int H, int ds, int da, int i0, int i1, gpmpc_cost_params C,
                                                          const double* __restrict__ sched, int H_max, int n_rows,
                                                          gpmpc_state_constraints cons, PcQuant Qm, const double* __restrict__ X,
                                                          const double* __restrict__ U, double* __restrict__ stage,
                                                          double* __restrict__ out_g, double* __restrict__ out_cost) {
    __shared__ double s_y[GPMPC_PARTICLE_COST_MAX_P];
    __shared__ double red[MPPI_THREADS];
    __shared__ int redi[MPPI_THREADS];
    __shared__ double s_Q[GPMPC_MAX_DS * GPMPC_MAX_DS], s_xr[GPMPC_MAX_DS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    const double gam = C.gamma;
    int n2 = 1;
    while (n2 < P) n2 <<= 1;
    double J = 0.0;
    for (int i = i0 + (int)blockIdx.x; i < i1; i += (int)gridDim.x) {
        const double* __restrict__ x = X + ((size_t)(i - i0) * B + b) * P * ds;
        // the weight and the reference of this step, as the cost kernels choose them
        if (tid < ds * ds) {
            double q = C.Q[tid];
            if (SCHED && i == H) {
                const double* __restrict__ qf = sched + gpmpc_sched_off_q(H_max, ds, da);
                if (qf[ds * ds] != 0.0) q = qf[tid];
            }
            s_Q[tid] = q;
        }
        if (tid < ds) s_xr[tid] = SCHED ? sched[(size_t)i * ds + tid] : C.x_ref[tid];
        __syncthreads();
        // c_p = e^T Q e of this thread's particles; a NaN coordinate anywhere makes the step NaN
        double c[PC_PER_THREAD];
        int bad = 0;
#pragma unroll
        for (int q = 0; q < PC_PER_THREAD; ++q) {
            const int p = tid + MPPI_THREADS * q;
            c[q] = 0.0;
            if (p < P) {
                double e[GPMPC_MAX_DS];
#pragma unroll
                for (int k = 0; k < GPMPC_MAX_DS; ++k) {
                    const double xk = k < ds ? x[(size_t)p * ds + k] : 0.0;
                    bad |= xk != xk ? 1 : 0;
                    e[k] = k < ds ? xk - s_xr[k] : 0.0;
                }
                double cc = 0.0;
#pragma unroll
                for (int k = 0; k < GPMPC_MAX_DS; ++k) {
                    if (k >= ds) continue;
                    double qe = 0.0;
#pragma unroll
                    for (int l = 0; l < GPMPC_MAX_DS; ++l)
                        if (l < ds) qe += s_Q[k * ds + l] * e[l];
                    cc += e[k] * qe;
                }
                c[q] = cc;
            }
        }
        bad = mppi_fold_count(bad, redi);                  // (its barriers also release s_Q / s_xr for the next step)
        if (bad) {                                         // (uniform over the workgroup)
            if (tid == 0) {
                if (stage) stage[(size_t)b * (H + 1) + i] = nan;
                J += nan;
            }
            if (i >= 1)
                for (int r = tid; r < n_rows; r += MPPI_THREADS) out_g[((size_t)b * H + (i - 1)) * n_rows + r] = nan;
            continue;
        }
        double s;
        if (gam == 0.0) {
            double sum = 0.0;
#pragma unroll
            for (int q = 0; q < PC_PER_THREAD; ++q)
                if (tid + MPPI_THREADS * q < P) sum = sum + c[q];
            s = mppi_fold_sum(sum, red) / (double)P;
        } else {
            const double hg = -0.5 * gam;
            double amax = -inf;
#pragma unroll
            for (int q = 0; q < PC_PER_THREAD; ++q)
                if (tid + MPPI_THREADS * q < P) amax = fmax(amax, hg * c[q]);
            const double M = pc_fold_max(amax, red);
            double sum = 0.0;
#pragma unroll
            for (int q = 0; q < PC_PER_THREAD; ++q)
                if (tid + MPPI_THREADS * q < P) sum = sum + exp(hg * c[q] - M);
            sum = mppi_fold_sum(sum, red);
            s = -(2.0 / gam) * (M + log(sum / (double)P));
        }
        if (tid == 0) {
            if (stage) stage[(size_t)b * (H + 1) + i] = s;
            J += s;
        }
        // the order statistic y_(P - m_r) of every row: one row at a time through LDS
        if (i >= 1)
            for (int r = 0; r < n_rows; ++r) {
                for (int p = tid; p < n2; p += MPPI_THREADS) {
                    double y = -inf;
                    if (p < P) {
                        double g = 0.0;
#pragma unroll
                        for (int e = 0; e < GPMPC_MAX_DS; ++e)
                            if (e < ds) g = g + cons.A[r * ds + e] * x[(size_t)p * ds + e];
                        y = g - cons.b[r];
                    }
                    s_y[p] = y;
                }
                __syncthreads();
                for (int k = 2; k <= n2; k <<= 1)
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        for (int p = tid; p < n2; p += MPPI_THREADS) {
                            const int o = p ^ j;
                            if (o > p) {
                                const double u = s_y[p], v = s_y[o];
                                if ((u > v) == ((p & k) == 0)) { s_y[p] = v; s_y[o] = u; }
                            }
                        }
                        __syncthreads();
                    }
                // ascending with the n2 - P pads in front: y_(j) sits at n2 - P + j - 1
                if (tid == 0) out_g[((size_t)b * H + (i - 1)) * n_rows + r] = s_y[n2 - 1 - Qm.m[r]];
                __syncthreads();
            }
    }
    if (out_cost && tid == 0)
        out_cost[b] = J + pc_input_cost<SCHED>(H, da, C, SCHED ? sched + gpmpc_sched_off_u(H_max, ds) : nullptr, U + (size_t)b * H * da);
}

template <bool SCHED>
__global__ __launch_bounds__(64) void k_pc_close(int B, int H, int ds, int da, gpmpc_cost_params C, const double* __restrict__ sched, int H_max,
                                                 const double* __restrict__ stage, const double* __restrict__ U, double* __restrict__ out_cost) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double J = 0.0;
    for (int i = 0; i <= H; ++i) J += stage[(size_t)b * (H + 1) + i];
    out_cost[b] = J + pc_input_cost<SCHED>(H, da, C, SCHED ? sched + gpmpc_sched_off_u(H_max, ds) : nullptr, U + (size_t)b * H * da);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct PcProblem {                 // what the launches need besides the sizes
    const gpmpc_cost_params* cost;
    gpmpc_sched_ref sched;
    const gpmpc_state_constraints* cons;
    PcQuant Qm;
};

static void pc_quantiles(const gpmpc_state_constraints* cons, int P, PcQuant* out) {
    memset(out, 0, sizeof(*out));
    if (!cons) return;
    for (int r = 0; r < cons->n_rows; ++r) {
        const double eps = 0.5 * erfc(cons->kappa[r] / sqrt(2.0));
        long m = (long)floor(eps * (double)P + 1e-9);
        out->m[r] = (int)(m < 0 ? 0 : (m > P - 1 ? P - 1 : m));      // (kappa >= 0 gives m <= P / 2 already)
    }
}

// the steps i0 ... i1 - 1 from X (the particles of step i0 on); fused: one workgroup per plan that also closes the cost
static void pc_launch_steps(int B, int P, int H, int ds, int da, int i0, int i1, const PcProblem& pb, const double* X, const double* U,
                            double* stage, double* out_g, double* out_cost, hipStream_t s) {
    gpmpc_state_constraints cz;
    memset(&cz, 0, sizeof(cz));
    const int n_rows = pb.cons ? pb.cons->n_rows : 0;
    const dim3 grid(out_cost ? 1 : i1 - i0, B);
    if (pb.sched.dev)
        hipLaunchKernelGGL(k_pc_step<true>, grid, dim3(MPPI_THREADS), 0, s, B, P, H, ds, da, i0, i1, *pb.cost, pb.sched.dev, pb.sched.H_max,
                           n_rows, pb.cons ? *pb.cons : cz, pb.Qm, X, U, stage, out_g, out_cost);
    else
        hipLaunchKernelGGL(k_pc_step<false>, grid, dim3(MPPI_THREADS), 0, s, B, P, H, ds, da, i0, i1, *pb.cost, (const double*)nullptr, 0,
                           n_rows, pb.cons ? *pb.cons : cz, pb.Qm, X, U, stage, out_g, out_cost);
}

static void pc_launch_close(int B, int H, int ds, int da, const PcProblem& pb, const double* stage, const double* U, double* out_cost,
                            hipStream_t s) {
    if (pb.sched.dev)
        hipLaunchKernelGGL(k_pc_close<true>, dim3((B + 63) / 64), dim3(64), 0, s, B, H, ds, da, *pb.cost, pb.sched.dev, pb.sched.H_max, stage, U,
                           out_cost);
    else
        hipLaunchKernelGGL(k_pc_close<false>, dim3((B + 63) / 64), dim3(64), 0, s, B, H, ds, da, *pb.cost, (const double*)nullptr, 0, stage, U,
                           out_cost);
}

// sizes, P, the cost schedule and the constraint rows of every entry; fills pb
static int pc_check(const char* who, int B, int P, int H, int ds, int da, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                    const double* out_g, PcProblem* pb) {
    if (ds < 1 || ds > GPMPC_MAX_DS) return gpmpc_refuse(who, "state_dim = %d outside 1...GPMPC_MAX_DS", ds);
    if (da < 0 || ds + da > GPMPC_MAX_D) return gpmpc_refuse(who, "action_dim = %d: D = state_dim + action_dim outside 1...GPMPC_MAX_D", da);
    if (H < 1 || H > 65534) return gpmpc_refuse(who, "H outside 1...65534");
    if (int rc = gpmpc_pt_check_bp(who, B, P)) return rc;
    if (P > GPMPC_PARTICLE_COST_MAX_P) return gpmpc_refuse(who, "P = %d outside 1...GPMPC_PARTICLE_COST_MAX_P (%d)", P, GPMPC_PARTICLE_COST_MAX_P);
    if (B > 65535) return gpmpc_refuse(who, "B > 65535");
    if ((long)B * P * GPMPC_MAX_DS * (H + 1) > (1L << 40)) return gpmpc_refuse(who, "more than 2^40 particle values");
    if (!cost) return gpmpc_refuse(who, "NULL pointer (cost)");
    if (cons) { if (int rc = gpmpc_check_constraints(cons, who)) return rc; }
    if ((cons != nullptr) != (out_g != nullptr)) return gpmpc_refuse(who, "out_g is given exactly when constraint rows are");
    if (int rc = gpmpc_schedule_resolve(cost, ds, da, H, who, &pb->sched)) return rc;
    pb->cost = cost;
    pb->cons = cons;
    pc_quantiles(cons, P, &pb->Qm);
    return GPMPC_OK;
}

extern "C" int gpmpc_particle_cost(int B, int P, int H, int ds, int da, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                   const double* particles, const double* U, double* out_cost, double* out_stage, double* out_g, void* stream) {
    const char* who = "gpmpc_particle_cost";
    PcProblem pb;
    if (int rc = pc_check(who, B, P, H, ds, da, cost, cons, out_g, &pb)) return rc;
    if (!particles || !out_cost || (da > 0 && !U)) return gpmpc_refuse(who, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (out_stage) {
        pc_launch_steps(B, P, H, ds, da, 0, H + 1, pb, particles, U, out_stage, out_g, nullptr, s);
        pc_launch_close(B, H, ds, da, pb, out_stage, U, out_cost, s);
    } else {
        pc_launch_steps(B, P, H, ds, da, 0, H + 1, pb, particles, U, nullptr, out_g, out_cost, s);
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// workspace of an evaluation: eps [P][da + ds] | two particle buffers [B P][ds] | stage [B][H + 1] | a step's.  Nothing grows with H B P.
struct PcEvalLayout { size_t off_eps, off_x[2], off_stage, off_step, step_bytes, total; };
static PcEvalLayout pc_eval_layout(const gpmpc_gp_model* m, int B, int P, int H, int chunk) {
    PcEvalLayout L;
    gpmpc_carver c;
    const size_t d = sizeof(double), slab = (size_t)B * P * m->state_dim;
    L.off_eps = c.take(d * P * PC_MAX_NORMALS);
    L.off_x[0] = c.take(d * slab);
    L.off_x[1] = c.take(d * slab);
    L.off_stage = c.take(d * B * (H + 1));
    L.step_bytes = gpmpc_particle_step_workspace_bytes(m, B, P, chunk);
    L.off_step = c.take(L.step_bytes);
    L.total = c.total();
    return L;
}

static bool pc_eval_sizes_ok(const gpmpc_gp_model* m, int B, int P, int H, int chunk) {
    return gpmpc_model_sizes_ok(m) && B >= 1 && B <= 65535 && P >= 1 && P <= GPMPC_PARTICLE_COST_MAX_P && H >= 1 && H <= 65534 &&
           (long)B * P * GPMPC_MAX_D <= 0x7fffffffL && (long)B * P * GPMPC_MAX_DS * (H + 1) <= (1L << 40) && gpmpc_chunk_ok(chunk);
}

extern "C" size_t gpmpc_particle_evaluate_workspace_bytes(const gpmpc_gp_model* m, int B, int P, int H, int chunk) {
    if (!pc_eval_sizes_ok(m, B, P, H, chunk)) return 0;
    return pc_eval_layout(m, B, P, H, chunk).total;
}

// the evaluation behind both entries; everything is checked
static int pc_evaluate(const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U, unsigned long long seed,
                       unsigned call_index, const PcProblem& pb, double* out_cost, double* out_stage, double* out_g, int chunk,
                       const PcEvalLayout& L, char* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int ds = m->state_dim, da = m->action_dim;
    double* eps = (double*)(ws + L.off_eps);
    double* xb[2] = {(double*)(ws + L.off_x[0]), (double*)(ws + L.off_x[1])};
    double* stage = out_stage ? out_stage : (double*)(ws + L.off_stage);
    if (int rc = gpmpc_particle_noise(P, ds, 0, seed, call_index, eps, stream)) return rc;
    if (int rc = gpmpc_pt_initial(m, B, P, x0, eps, xb[0], s)) return rc;
    pc_launch_steps(B, P, H, ds, da, 0, 1, pb, xb[0], U, stage, out_g, nullptr, s);
    for (int t = 1; t <= H; ++t) {
        double *prev = xb[(t - 1) & 1], *next = xb[t & 1];
        if (int rc = gpmpc_particle_noise(P, da + ds, t, seed, call_index, eps, stream)) return rc;
        if (int rc = gpmpc_particle_step(m, B, P, prev, U ? U + (size_t)(t - 1) * da : nullptr, (size_t)H * da, eps, next, nullptr, nullptr, chunk,
                                         ws + L.off_step, L.step_bytes, stream))
            return rc;
        pc_launch_steps(B, P, H, ds, da, t, t + 1, pb, next, U, stage, out_g, nullptr, s);
    }
    pc_launch_close(B, H, ds, da, pb, stage, U, out_cost, s);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_particle_evaluate(const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U, unsigned long long seed,
                                       unsigned call_index, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                       double* out_cost, double* out_stage, double* out_g, int chunk, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    const char* who = "gpmpc_particle_evaluate";
    if (int rc = gpmpc_pt_check_model(who, m)) return rc;
    PcProblem pb;
    if (int rc = pc_check(who, B, P, H, m->state_dim, m->action_dim, cost, cons, out_g, &pb)) return rc;
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!x0 || !out_cost || !workspace || (m->action_dim > 0 && !U)) return gpmpc_refuse(who, "NULL pointer");
    const PcEvalLayout L = pc_eval_layout(m, B, P, H, chunk);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    return pc_evaluate(m, B, P, H, x0, U, seed, call_index, pb, out_cost, out_stage, out_g, chunk, L, (char*)workspace, stream);
}

// ---------------------------------------------------------------------------
// MPPI over the particle cost: the search of mppi_internal.h with the evaluation above
// ---------------------------------------------------------------------------
// workspace: the head of every MPPI solve | the evaluation's own workspace
struct PcMppiLayout { gpmpc_mppi_head head; size_t off_eval, total; PcEvalLayout eval; };
static PcMppiLayout pc_mppi_layout(const gpmpc_gp_model* m, int H, int P, int K, int m_c) {
    PcMppiLayout L;
    gpmpc_carver c;
    L.head = gpmpc_mppi_head_take(c, H, m->state_dim, m->action_dim, K, m_c);
    L.eval = pc_eval_layout(m, K, P, H, 0);
    L.off_eval = c.take(L.eval.total);
    L.total = c.total();
    return L;
}

extern "C" size_t gpmpc_mppi_solve_particles_workspace_bytes(const gpmpc_gp_model* m, int H, int P, const gpmpc_mppi_params* Pm,
                                                             const gpmpc_state_constraints* cons) {
    if (!Pm || Pm->n_samples < 1 || Pm->n_samples > GPMPC_MPPI_MAX_SAMPLES || !pc_eval_sizes_ok(m, Pm->n_samples, P, H, 0)) return 0;
    if (cons && (cons->n_rows < 1 || cons->n_rows > GPMPC_MAX_CONS)) return 0;
    if (!gpmpc_solver_dims_ok(H, m->state_dim, m->action_dim)) return 0;
    return pc_mppi_layout(m, H, P, Pm->n_samples, cons ? cons->n_rows : 0).total;
}

extern "C" int gpmpc_mppi_solve_particles(const gpmpc_gp_model* m, int H, int P, const double* x0, const double* start,
                                          const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, const gpmpc_mppi_params* Pm,
                                          double* out_U, double* out_best, double* out_trace, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    const char* who = "gpmpc_mppi_solve_particles";
    if (!m || !x0 || !start || !cost || !Pm || !out_U || !out_best || !out_trace || !workspace) return gpmpc_refuse(who, "NULL pointer");
    if (H < 1) return gpmpc_refuse(who, "H < 1");
    if (int rc = gpmpc_mppi_check_scalars(Pm, who)) return rc;
    if (int rc = gpmpc_pt_check_model(who, m)) return rc;
    const int ds = m->state_dim, da = m->action_dim;
    if (!gpmpc_solver_dims_ok(H, ds, da)) return gpmpc_refuse(who, "H, state_dim or action_dim outside what a solver takes");
    if (int rc = gpmpc_mppi_check_inputs(Pm, da, who)) return rc;
    const int K = Pm->n_samples, m_c = cons ? cons->n_rows : 0;
    PcProblem pb;
    // (out_g of the evaluation is the solve's own buffer: given exactly when rows are)
    if (int rc = pc_check(who, K, P, H, ds, da, cost, cons, cons ? (const double*)workspace : nullptr, &pb)) return rc;
    const PcMppiLayout L = pc_mppi_layout(m, H, P, K, m_c);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    char* ws = (char*)workspace;
    // the SAME particle noise in every iteration: one fixed sample-average objective, so that keys compare across iterations
    auto eval = [&](int, const double* x0b, const double* U, double* cst, double* g) {
        return pc_evaluate(m, K, P, H, x0b, U, Pm->seed, Pm->call_index, pb, cst, nullptr, g, 0, L.eval, ws + L.off_eval, stream);
    };
    return gpmpc_mppi_search(L.head, ws, H, ds, da, m_c, Pm, x0, start, eval, out_U, out_best, out_trace, stream);
}
