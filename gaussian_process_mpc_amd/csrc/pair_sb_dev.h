// What the scalar-broadcast forms of the N^2 pair sum share as code (pair_kernel_sb.h, pair_kernel_sbs.h, the 256-row tile roles of
// step_fused.h, the column loop of traj_persist.h): the width of a column row, and stages 2 and 3 of a staged batch of columns.  Only
// __device__ __forceinline__ templates: loop structure, prefetch depth, launch bounds and where a row is stored stay with each kernel.
// The formulation is described at the top of pair_kernel_sb.h:
//     exponent of pair (i, j), pre-scaled by N/ln2 (fast_exp.h):   qi + g[D] + sum_k hi2[k] g[k]
//     column row  G[j] = [h_j1..h_jD | q_j N/ln2 | h_j1^2..h_jNS2^2 | pad],   h = cv - sc x   (cv = sc u)
//     row terms   hi2[k] = 2 N/ln2 h_ik,  qi = N/ln2 |h_i|^2
// The fixed-order combine of a wave's four row sums is gpmpc_rows4 (gpmpc_internal.h, beside wave_row_sum).
// NOT shared, on purpose: the G row of a column, the row terms of a lane and the per-lane moment combination are still written out in
// each kernel.  A helper for any of them (arrays by reference, by value, through functors) changed the register allocation or the
// schedule of shipped kernels -- an array handed to a call is promoted to registers later than one used in place -- and these kernels
// are held to the assembly of their parent, instruction for instruction (profiles/pair_shared/isa_diff.txt).  Whoever changes one of
// those expressions changes it in every file that carries it, and compares the device assembly of all units (tools/isa_diff.py).
#pragma once
#include "gpmpc_internal.h"
#include "fast_exp.h"

template <int D, int NS2>
struct PairSbTraits {
    static constexpr int GW = (D + 1 + NS2 + 1) & ~1;     // doubles per G row (even: rows stay 16-byte aligned)
};

// Stages 2 and 3 of a staged batch of KC columns whose G rows g the caller has loaded (stage 1; the caller keeps its sched_barrier after
// those loads): all exponents and table reads (one LDS wait), then weights x exp and the row sums acc = [r | v_k | w_k] of NG GPs.
// This is gpmpc_exp_neg_scaled (fast_exp.h) split around the table read -- the two change together.  PQ_EARLY: the polynomial is
// evaluated beside the table read (in its shadow) instead of after it (where registers are short).
template <int D, int NS2, bool GRAD, int NG, int KC, bool PQ_EARLY, int GW, int NA>
__device__ __forceinline__ void gpmpc_sb_batch(const double (&g)[KC][GW], const double (*mw)[NG], const double (&hi2)[D], const double qi,
                                               const double* s_tab, double (&acc)[NG][NA]) {
    double fr[KC], pq[KC], Tv[KC];
    int ni[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        double sx = qi + g[c][D];
#pragma unroll
        for (int k = 0; k < D; ++k) sx = fma(hi2[k], g[c][k], sx);
        const double ax = __builtin_fabs(sx);
        ni[c] = (int)(-ax);
        fr[c] = __builtin_amdgcn_fract(ax);
        Tv[c] = s_tab[ni[c] & (GPMPC_EXP_N - 1)];
        if (PQ_EARLY) pq[c] = fma(fr[c], fma(fr[c], GPMPC_EXP_A3, GPMPC_EXP_A2), GPMPC_EXP_A1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        if (!PQ_EARLY) pq[c] = fma(fr[c], fma(fr[c], GPMPC_EXP_A3, GPMPC_EXP_A2), GPMPC_EXP_A1);
        const double e = ldexp(fma(Tv[c] * fr[c], pq[c], Tv[c]), ni[c] >> GPMPC_EXP_BITS);
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            const double P = mw[c][q] * e;
            acc[q][0] += P;
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[q][GRAD ? 1 + k : 0] = fma(P, g[c][k], acc[q][GRAD ? 1 + k : 0]);
#pragma unroll
                for (int k = 0; k < NS2; ++k) acc[q][GRAD ? 1 + D + k : 0] = fma(P, g[c][D + 1 + k], acc[q][GRAD ? 1 + D + k : 0]);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
