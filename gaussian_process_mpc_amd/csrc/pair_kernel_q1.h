// Horizon step 1 of the two-launch scalar-broadcast form as a quadratic form: no exponent and no exp per pair.
//
// The pair sum of pair_kernel_sb.h,  P_ij = M_ij exp(-|h_i + h_j|^2),  h_ik = sc_k (u_k - x_ik),  sc_k^2 = 1/8 / (lambda_k / 2 + s_k), has at t = 1 the
// input variances s_k of the pack's noise model (diag(init_cov), action_var): the same for every trajectory of every call until the model or the
// pack changes.  With  |h_i + h_j|^2 = 2 |h_i|^2 + 2 |h_j|^2 - |h_i - h_j|^2  and  h_i - h_j = sc o (x_j - x_i)  free of the trajectory,
//     P_ij = M1_ij kappa_i kappa_j,     kappa_i = exp(-2 |h_i|^2),     M1_ij = M_ij exp(+sum_k sc_k^2 (x_ik - x_jk)^2)     (pack_build.hip: k_pack_weights1)
// and the moments the FIRST variant of pair_kernel_sb.h produces -- Z0 = sum P, Z1_k = sum P (h_ik + h_jk) for the action dimensions k >= ds -- are
//     y_i = sum_{j >= i} M1_ij kappa_j,   y^k_i = sum_{j >= i} M1_ij (kappa_j h_jk),     Z0 = sum_i kappa_i y_i,   Z1_k = sum_i kappa_i (h_ik y_i + y^k_i):
// an upper-triangular matrix times 1 + da columns per trajectory.  Exact algebra; the O(N) values kappa_j, kappa_j h_jk are written by the head
// kernel of step 1 (step.hip) with the library exp, the row side recomputes its own from XT and pp with the same expressions.
//
// One workgroup = one 256-row tile of the work list x a block of T trajectories, lane = row.  Per column: one buffer load of M1_ij and (1 + da) T
// fused multiply-adds whose second factor is a wave-uniform value fetched by scalar loads (the column values of T consecutive trajectories are
// contiguous: cols[unit][j][b][1 + da]).  A trajectory's sums never meet its block mates': its bits do not depend on T, on B or on a sub-batch split.
// The last block of a batch that is no multiple of T reads up to (T - 1)(1 + da) doubles past its column's values -- the next column's, or, behind
// the last column, the rest of the G region of the workspace the values live in (step.hip checks the room) -- into accumulators nobody stores.
#pragma once
#include "gpmpc_internal.h"

// columns per iteration of the column loop: the M1_ij loads of four columns are in flight before the first is used
#define GPMPC_Q1_CU 4

template <int D, int DA, int T>
__global__ __launch_bounds__(256) void gpmpc_pair_kernel_q1(PairQ1Args A) {
    constexpr int NC = 1 + DA, DS = D - DA;
    __shared__ double s_red[16 * T * NC];         // [wave][row of 16 lanes][trajectory][value]

    // XCD-aware decode, as pair_kernel_sb.h with blocks of T trajectories in the place of its groups of TB
    int bg, wi;
    {
        const int groups = (A.B + T - 1) / T, items = A.nwork, R = A.rgroup;
        const int L = blockIdx.x, full = (items / (8 * R)) * (8 * R);
        if (L < full * groups) {
            const int q = L >> 3, ir = q % R, t = q / R;
            bg = t % groups;
            wi = ((t / groups) * R + ir) * 8 + (L & 7);
        } else { const int Lt = L - full * groups; wi = full + Lt / groups; bg = Lt % groups; }
    }
    const int unit = A.work[wi * 4 + 0], i0 = A.work[wi * 4 + 1], j0 = A.work[wi * 4 + 2], j1w = A.work[wi * 4 + 3];
    // the column loop ends at the count of columns that carry weight, read from the pack in device memory (no launch argument depends on N)
    const int ncw = *(const int __attribute__((address_space(4)))*)A.ncol;
    const int j1 = j1w < ncw ? j1w : ncw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Np = A.Np;
    const int iw0 = i0 + w * 64;                          // first row of this wave (wave-uniform)

    double acc[T][NC];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int n = 0; n < NC; ++n) acc[t][n] = 0.0;

    if (iw0 < Np) {
        // upper-triangular M1: the columns left of the wave's diagonal chunk carry zero weight
        const int jstart = j0 > iw0 ? j0 : iw0;
        const __amdgpu_buffer_rsrc_t Mrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<double*>(A.M1 + ((size_t)unit * Np + jstart) * Np + iw0), 0, 0x7fffffff, 0x00020000);
        const int lane8 = lane * 8;
        // the column values were written by the head kernel of this step and are constant for the launch: CONSTANT address space, so that
        // they are fetched by scalar loads (pair_kernel_sb.h says why)
        typedef const double __attribute__((address_space(4))) gpmpc_cdouble;
        const gpmpc_cdouble* __restrict__ cb = (const gpmpc_cdouble*)(A.cols + (((size_t)unit * Np) * A.B + (size_t)bg * T) * NC);
        const size_t cstride = (size_t)A.B * NC;
        int jc = jstart;
        for (; jc + GPMPC_Q1_CU <= j1; jc += GPMPC_Q1_CU) {
            double mij[GPMPC_Q1_CU];
#pragma unroll
            for (int q = 0; q < GPMPC_Q1_CU; ++q)
                mij[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(Mrs, lane8, (jc - jstart + q) * Np * 8, 0));
            __builtin_amdgcn_sched_barrier(0);            // the loads stay at the top of the iteration
#pragma unroll
            for (int q = 0; q < GPMPC_Q1_CU; ++q) {
                const gpmpc_cdouble* __restrict__ c = cb + (size_t)(jc + q) * cstride;
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int n = 0; n < NC; ++n) acc[t][n] = fma(mij[q], c[t * NC + n], acc[t][n]);
            }
        }
        for (; jc < j1; ++jc) {                           // (tiles and column counts are multiples of 8: not reached by the pack's work lists)
            const double mij = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(Mrs, lane8, (jc - jstart) * Np * 8, 0));
            const gpmpc_cdouble* __restrict__ c = cb + (size_t)jc * cstride;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int n = 0; n < NC; ++n) acc[t][n] = fma(mij, c[t * NC + n], acc[t][n]);
        }
    }

    // row side: h_i and kappa_i of this lane's row for each trajectory of the block (the expressions of the head kernel), the two sums, and the
    // fixed-order reduction of pair_kernel_sb.h
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = iw0 < Np ? A.XT[(size_t)k * Np + iw0 + lane] : 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        int b = bg * T + t;
        b = b < A.B ? b : A.B - 1;
        const double* __restrict__ prm = A.pp + ((size_t)b * A.ds + unit) * A.pps;
        double q = 0.0, ha[DA];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double h = fma(-prm[D + k], x[k], prm[k]);
            q = fma(h, h, q);
            if (k >= DS) ha[k - DS] = h;
        }
        const double kap = exp(-2.0 * q);
        double z[NC];
        z[0] = kap * acc[t][0];
#pragma unroll
        for (int n = 0; n < DA; ++n) z[1 + n] = kap * fma(ha[n], acc[t][0], acc[t][1 + n]);
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const double s = wave_row_sum(z[n]);
            if ((lane & 15) == 0) s_red[((w * 4 + (lane >> 4)) * T + t) * NC + n] = s;
        }
    }
    __syncthreads();
    // the slots of the FIRST variant: Z0, Z1_k for the action dimensions, zeros for the moments step 1 does not need
    for (int idx = tid; idx < T * A.nm; idx += blockDim.x) {
        const int t = idx / A.nm, m = idx - t * A.nm;
        const int b = bg * T + t;
        if (b < A.B) {
            const int n = m == 0 ? 0 : ((m - 1 >= DS && m - 1 < D) ? m - DS : -1);
            double s = 0.0;
            if (n >= 0)
                for (int ww = 0; ww < 4; ++ww) s += gpmpc_rows4(&s_red[(ww * 4 * T + t) * NC + n], T * NC);
            A.part[((size_t)b * A.nwork + wi) * A.nm + m] = s;
        }
    }
}

template <int D, int DA, int T>
static int launch_pair_q1_one(const PairQ1Args& a, hipStream_t s) {
    hipLaunchKernelGGL((gpmpc_pair_kernel_q1<D, DA, T>), dim3(((a.B + T - 1) / T) * a.nwork), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { gpmpc_set_error("step-1 pair kernel launch", e); return GPMPC_E_LAUNCH; }
    return GPMPC_OK;
}

// da in {1, 2} action dimensions, blocks of 8 or 16 trajectories
template <int D>
int gpmpc_launch_pair_q1_D(int da, const PairQ1Args& a, hipStream_t s) {
    if (a.nm != 1 && a.nm != 1 + 2 * D) return GPMPC_E_ARG;
    if (a.tblock != 8 && a.tblock != 16) return GPMPC_E_ARG;
    if constexpr (D >= 2) {
        if (da == 1) return a.tblock == 8 ? launch_pair_q1_one<D, 1, 8>(a, s) : launch_pair_q1_one<D, 1, 16>(a, s);
    }
    if constexpr (D >= 3) {
        if (da == 2) return launch_pair_q1_one<D, 2, 8>(a, s);      // (16 trajectories x 3 values: the column's 96 SGPRs spill)
    }
    return GPMPC_E_ARG;
}
