// Linear chance constraints on the state of a propagated rollout, and their whole Jacobian w.r.t. the inputs (include/gpmpc.h,
// DESIGN.md section 3b):
//     g[t][r] = a_r . mu_t + kappa_r sd[t][r] - b_r,   sd = sqrt(q),  q = sum_k a_rk^2 var_tk              t = 1..H, r < n_rows
//     d g[t][r] / dU = sum_k a_rk S_t[k][:] + (kappa_r / (2 sd)) sum_k a_rk^2 S_t[ds+k][:],   S_t = d(mu_t, var_t)/dU  [2ds][H da]
// A solver wants all H n_rows rows.  gpmpc_rollout_vjp gives one row per reverse sweep; the columns of S_t, on the other hand, evolve
// independently of each other through the step Jacobians J_t [2ds][2ds+da] that the rollout has already written,
//     S_t[:, c] = A_t S_{t-1}[:, c]            A_t = state block of J_t             (column c = tau da + j of input u_tau[j], tau < t-1)
//     S_t[:, c] = J_t[:, 2ds + j]                                                   (tau = t-1: the column starts from the input block)
//     S_t[:, c] = 0                                                                 (tau >= t: causality)
// so ONE forward sweep serves every row: one lane per column, the column's 2ds sensitivities in registers, no LDS and no barrier.
// Everything else -- J_t, a_r, kappa_r / (2 sd), sd -- is the same for every lane: J_t is read through wave-uniform addresses (scalar
// loads; the fp64 FMAs take the element as their scalar operand, the idiom of pair_kernel_sb.h), the rows (a_r, b_r, kappa_r) are
// kernel arguments, and the per-row factor is made uniform with v_readfirstlane.  After each step every lane stores its element of that
// step's n_rows Jacobian rows (coalesced along c); the first wave of a trajectory also stores g[t][0..n_rows).
//
// Summation order is fixed (k ascending, one FMA chain per sum): results are bit-reproducible, independent of B and of the grid.
// NaN: 0 * NaN is NaN, so a NaN mean / variance of step t reaches every row of step t; columns tau >= t are stored as the literal 0.0
// whatever the arithmetic gives.  A lane whose column has not started takes no part in the product (its result is discarded by a
// select, not multiplied by zero: a non-finite J_t cannot leak into a column that is still zero).
#include "gpmpc_internal.h"

__device__ __forceinline__ double cons_uniform(double v) {      // v holds the same value in every lane: keep it in SGPRs
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// grid (B, ceil(H da / 64)), one wave per workgroup.  JAC = false: values only (grid (B, 1); jac / out_gjac not touched).
template <int DS, bool JAC>
__global__ __launch_bounds__(64) void k_rollout_constraints(int H, int da, gpmpc_state_constraints C, const double* __restrict__ means,
                                                            const double* __restrict__ vars, const double* __restrict__ jac,
                                                            double* __restrict__ out_g, double* __restrict__ out_gjac) {
    constexpr int NZ = 2 * DS;
    const int b = blockIdx.x, lane = threadIdx.x, mc = C.n_rows, nc = NZ + da, ncols = H * da;
    const int c0 = blockIdx.y * 64;                         // first column of this wave (wave-uniform)
    const int c = c0 + lane;
    const bool live = c < ncols;
    const int tau = c / da, j = c - tau * da;               // input u_tau[j] of this lane's column
    const int tau0 = c0 / da;                               // earliest input step among the wave's columns
    const bool first = blockIdx.y == 0;
    double S[NZ];
#pragma unroll
    for (int r = 0; r < NZ; ++r) S[r] = 0.0;

    for (int t = 1; t <= H; ++t) {
        if (JAC && tau0 < t) {                              // (wave-uniform) some column of this wave is non-zero at step t
            const double* __restrict__ Jt = jac + ((size_t)b * H + (t - 1)) * NZ * nc;
            if (tau0 < t - 1) {                             // (wave-uniform) some column started before this step: S <- A_t S
                double n[NZ];
#pragma unroll
                for (int r = 0; r < NZ; ++r) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < NZ; ++k) acc = fma(Jt[r * nc + k], S[k], acc);
                    n[r] = acc;
                }
                const bool started = tau < t - 1;
#pragma unroll
                for (int r = 0; r < NZ; ++r) S[r] = started ? n[r] : 0.0;
            }
            if (live && tau == t - 1) {                     // this step's input: the column starts from the input block of J_t
#pragma unroll
                for (int r = 0; r < NZ; ++r) S[r] = Jt[r * nc + NZ + j];
            }
        }
        const double* __restrict__ mu = means + ((size_t)b * (H + 1) + t) * DS;
        const double* __restrict__ va = vars + ((size_t)b * (H + 1) + t) * DS;
        for (int r = 0; r < mc; ++r) {
            double am = 0.0, q = 0.0;
#pragma unroll
            for (int k = 0; k < DS; ++k) {
                const double a = C.A[r * DS + k];
                am = fma(a, mu[k], am);
                q = fma(a * a, va[k], q);
            }
            // q <= 0: sd = 0 and no variance part; NaN passes through (q > 0 and q <= 0 are both false for a NaN)
            const double sd = q > 0.0 ? sqrt(q) : (q <= 0.0 ? 0.0 : q);
            const double kap = C.kappa[r];
            if (first && lane == 0) out_g[((size_t)b * H + (t - 1)) * mc + r] = fma(kap, sd, am) - C.b[r];
            if (JAC) {
                const double cv = cons_uniform(q <= 0.0 ? 0.0 : kap / (2.0 * sd));
                double dm = 0.0, dv = 0.0;
#pragma unroll
                for (int k = 0; k < DS; ++k) {
                    const double a = C.A[r * DS + k];
                    dm = fma(a, S[k], dm);
                    dv = fma(a * a, S[DS + k], dv);
                }
                if (live) out_gjac[(((size_t)b * H + (t - 1)) * mc + r) * ncols + c] = tau < t ? fma(cv, dv, dm) : 0.0;
            }
        }
    }
}

template <int DS>
static int launch_constraints(int B, int H, int da, const gpmpc_state_constraints& C, const double* means, const double* vars,
                              const double* jac, double* out_g, double* out_gjac, hipStream_t s) {
    if (out_gjac)
        hipLaunchKernelGGL((k_rollout_constraints<DS, true>), dim3(B, (H * da + 63) / 64), dim3(64), 0, s, H, da, C, means, vars, jac,
                           out_g, out_gjac);
    else
        hipLaunchKernelGGL((k_rollout_constraints<DS, false>), dim3(B, 1), dim3(64), 0, s, H, da, C, means, vars, jac, out_g, out_gjac);
    return GPMPC_OK;
}

int gpmpc_check_constraints(const gpmpc_state_constraints* C, const char* who) {
    if (!C) return GPMPC_E_ARG;
    if (C->n_rows < 1 || C->n_rows > GPMPC_MAX_CONS) return gpmpc_refuse(who, "n_rows = %d outside 1..%d", C->n_rows, GPMPC_MAX_CONS);
    for (int r = 0; r < C->n_rows; ++r)
        if (!(C->kappa[r] >= 0.0)) return gpmpc_refuse(who, "kappa[%d] = %g is negative or NaN", r, C->kappa[r]);
    return GPMPC_OK;
}

extern "C" int gpmpc_rollout_constraints(int B, int H, int ds, int da, const gpmpc_state_constraints* C, const double* means,
                                         const double* vars, const double* jac, double* out_g, double* out_gjac, void* stream) {
    if (!C || !means || !vars || !out_g || (out_gjac && !jac) || B < 1 || H < 1 || ds < 1 || ds > GPMPC_MAX_DS || da < 1 ||
        da > GPMPC_MAX_D || (long)H * da > 64L * 65535)
        return GPMPC_E_ARG;
    if (int rc = gpmpc_check_constraints(C, "gpmpc_rollout_constraints")) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = gpmpc_dispatch_dim<1>(ds, [&](auto d) {
            return launch_constraints<decltype(d)::value>(B, H, da, *C, means, vars, jac, out_g, out_gjac, s);
        }))
        return rc;
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
