// Device side shared by the head kernel (step.hip) and the tail kernel (step_tail.hip) of the diagonal rollout: the kernel
// arguments, the layout of the per-GP scalars `sp`, and the finish phase of a horizon step, which both kernels run.
#pragma once
#include "gpmpc_internal.h"
#include "plan.h"

struct RollArgs {
    // pack
    const double* XT; const double* beta; const double* lam; const double* sf;
    int Np, ds, da, D;            // (padded size only: no launch argument may depend on the unpadded N, see gpmpc_graph_cache_invalidate)
    // problem
    const double* x0; const double* U; int B, H;
    // state trajectory (outputs or workspace): [B][H+1][ds]
    double* means; double* vars;
    // workspace
    double* pp;    // [B][ds][pps]   pair-kernel parameters of the current step
    double* sp;    // [2][B][ds][sps] per-GP scalars of step t at [t & 1], kept for the finish phase of the next head launch
    double* part;  // [B][nwork][nm]; work items of GP a are [ustart[a], ustart[a+1])
    const int* ustart;
    int ust_inline;    // ust[] below replaces ustart (the fused path splits tiles into column pieces: its own item ranges)
    int ust[GPMPC_MAX_DS + 1];
    const int* work;   // [nwork][4] when the items of a unit are NOT contiguous (XCD-sorted list), else null
    const int* perm;   // ... and then the item indices grouped by unit (ascending within a unit): unit a owns perm[ustart[a] .. ustart[a+1])
    double* jac;   // [B][H][2ds][2ds+da] or null
    double* G;     // [B][ds][Np][gw] column rows of the scalar-broadcast pair kernel, or null
    int gw;
    double* q1cols; // step-1 kernel (pair_kernel_q1.h): at t = 1 the head kernel writes [ds][Np][B][1 + da] column values HERE (inside the G region) and no G rows; else null
    int shared;   // shared-lambda path: G is [B][Np][gw], written by the workgroups of GP 0 only (pair_kernel_sbs.h)
    int pps, sps, nwork, nm, grad;
    // Row chunks of the head kernel (small batches of a large N: B ds workgroups walking all N rows are the slowest thing in
    // the step).  hchunks > 1: workgroup (b, a, c) takes rows [c, c+1) * hrows; the O(N) mean sums of step t are left as
    // partial sums mpart [2][B][ds][hchunks][1+2D] (parity t & 1) and combined by the FINISH phase of the next launch, which
    // then also forms mu and its derivatives; sp carries c_m and B_k instead (layout below).  hchunks <= 1: as before.
    int hchunks, hrows;
    double* mpart;
    int finished;      // every horizon step (H included) is already finished -- means, variances, Jacobians written -- by the whole-horizon
                       // kernel (traj_persist.h): the tail kernel goes straight to the cost terms
    // outputs of the tail
    double* out_cost; double* out_grad;
    gpmpc_cost_params cost;
    const double* nom;   // linear nominal model of the pack: [ds][D] weights, then [ds] biases (nominal kernel variants only), else null
    const double* sched; // cost schedule of the call (include/gpmpc.h: x_ref rows | u_ref rows | Q_f | has_Qf, H), read by the schedule variants of
    int sched_hmax;      // the tail kernel only, else null; the H_max its offsets are formed from
    const double* noise; // noise model of the pack (gpmpc_pack::noise_dev; layout in gpmpc_internal.h), read by the head kernel
};

// layout of sp (doubles): 0 c | 1 mu | 2 sf2 + w | 3 A[D] | 3+D scale[D] | 3+2D dmu_du[D] | 3+3D dmu_ds[D]
//   (w: the GP's process_var of the pack's noise model, added ONCE by whoever writes sp[2]: var = sp[2] - T - mu^2; c_m keeps the plain sf2)
//   with row chunks (hchunks > 1):      1 c_m                                  3+2D B[D]      3+3D unused
// (sps_of(D) = 3 + 4 D doubles: plan.h)
// Linear nominal model m_a(z) = n_a . z + c_a (GP a learns the residual): the step's moments become
//   mu' = mu_g + n . u + c,   var' = var_g + sum_k n_k^2 s_k + 2 sum_k w_k dmu_g/du_k,   w_k = n_k s_k   (Cov[z, g(z)] = S E[grad g])
// and, with q_i = sum_k w_k B_k v_ik, E1_l = sum_i p_i q_i v_il, E2_l = sum_i p_i q_i v_il^2, M1_l = sum_i p_i v_il, X = 2 sum_k w_k dmu_g/du_k:
//   dmu'/du_l = dmu_g/du_l + n_l,   dmu'/ds_l = dmu_g/ds_l
//   dvar'/du_l = dvar_g/du_l + 2 (c_m B_l E1_l - w_l B_l mu_g)
//   dvar'/ds_l = dvar_g/ds_l + n_l^2 + 2 n_l dmu_g/du_l - 1/2 B_l X + B_l^2 c_m (2 w_l M1_l - E2_l)          (state inputs l only)
// prep_step forms these ADDENDS once per (trajectory, GP) and leaves them behind the plain entries of sp; finish_step -- in every workgroup
// of the trajectory -- adds the same stored values in the same order.  Layout of the extension, from sps_of(D):
//   0 n . u + c | 1 addend of var | 2 addend of dvar/du [D] | 2+D addend of dvar/ds [D] | 2+2D n [D]        (the [D] blocks with the gradient only)
// The nominal variants run without row chunks (plan.hip).  sps_nominal(D) = sps_of(D) + 2 + 3 D doubles: plan.h

// Finish step t (>= 1) for trajectory b: reduce the pair-kernel partials of ALL ds GPs (mean/var of step t land in
// s_mu / s_var, LDS) and write to global memory the rows this workgroup owns: every GP if own < 0, else GP `own`
// only (the head kernel runs one workgroup per (trajectory, GP); each recomputes the cheap reduction and owns one GP).
#define GPMPC_RED_CH 8
template <bool NOM>
__device__ static void finish_step(const RollArgs& A, int b, int t, int own, double* s_z /* [ds*nm] */,
                                   double* s_red /* [ds*nm*GPMPC_RED_CH] */, double* s_mu, double* s_var,
                                   double* s_ms /* [MAX_DS*(1+2 MAX_D) + 4 MAX_DS] */) {
    const int ds = A.ds, D = A.D, nm = A.nm;
    const bool chunked = A.hchunks > 1;
    // the per-GP scalars of step t, fetched in ONE coalesced round trip that overlaps the reduction below (they were read one by
    // one, each its own round trip, by the ds threads that finish the step)
    __shared__ double s_spv[GPMPC_MAX_DS * (NOM ? 5 + 7 * GPMPC_MAX_D : 3 + 4 * GPMPC_MAX_D)];
    {
        const double* spb = A.sp + ((size_t)(t & 1) * A.B + b) * ds * A.sps;
        for (int e = threadIdx.x; e < ds * A.sps; e += blockDim.x) s_spv[e] = spb[e];
    }
    if (chunked) {      // mean sums of step t: the row chunks' partial sums, combined in chunk order
        const int nv = 1 + 2 * D;
        for (int o = threadIdx.x; o < ds * nv; o += blockDim.x) {
            const int a = o / nv, m = o - a * nv;
            const double* q = A.mpart + ((((size_t)(t & 1) * A.B + b) * ds + a) * A.hchunks) * nv + m;
            double sum = 0.0;
            for (int c = 0; c < A.hchunks; ++c) sum += q[(size_t)c * nv];
            s_ms[o] = sum;
        }
    }
    // Sum the per-tile partials of every (GP, moment) output; either way the summation order depends only on the
    // shapes, never on timing.
    if (A.nwork > 128 * ds && own < 0) {
        // Many items per GP, every GP owned (the tail kernel: the last step, nothing downstream has to agree with another
        // workgroup): one wave per GP, a lane takes whole work items -- the nm moments of an item are contiguous and the
        // loads of different items are independent -- and the wave sum is the final value.
        constexpr int NMAX = 1 + 2 * GPMPC_MAX_D;
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
        const double* p = A.part + (size_t)b * A.nwork * nm;
        for (int a = w; a < ds; a += nw) {
            double acc[NMAX];
#pragma unroll
            for (int m = 0; m < NMAX; ++m) acc[m] = 0.0;
            const int w0 = A.ust_inline ? A.ust[a] : (A.work ? 0 : A.ustart[a]);
            const int w1 = A.ust_inline ? A.ust[a + 1] : (A.work ? A.nwork : A.ustart[a + 1]);
            for (int wi = w0 + lane; wi < w1; wi += 64) {
                if (!A.ust_inline && A.work && A.work[4 * wi] != a) continue;
                const double* q = p + (size_t)wi * nm;
#pragma unroll
                for (int m = 0; m < NMAX; ++m) if (m < nm) acc[m] += q[m];
            }
#pragma unroll
            for (int m = 0; m < NMAX; ++m)
                if (m < nm) {
                    const double sw = wave_sum(acc[m]);
                    if (lane == 0) s_z[a * nm + m] = sw;
                }
        }
    } else if (A.nwork > 128 * ds) {
        // Many items per GP (256x64 tiles of a large N: 544 per GP at N = 4096, 15 moments each).  Only the workgroup that
        // writes GP a's Jacobian rows needs all its moments; every workgroup needs Z0 of every GP (the input variances of
        // the next step).  Owned GPs: thread = (moment m, group g), group g takes items g, g + GR, ... -- the nm moments of an
        // item are contiguous, so a pass reads GR * nm consecutive doubles -- then a fixed-order combine over the groups.
        // Z0 of EVERY GP (owned or not): one item per thread and pass, wave sums -- the same order in every workgroup of the
        // trajectory, so that all of them derive bit-identical input variances: the row-side transform (pp, one workgroup)
        // and the column rows (G, possibly several row-chunk workgroups) of a unit must agree to the last bit, the N^2 sum
        // amplifies a relative 1e-9 between them to 1e-2 of the variance.  (One wave per GP with a lane taking whole
        // items, all moments of all GPs in every workgroup, was 40 us of the head kernel at N = 4096.)
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
        const int GR = (int)blockDim.x / nm < 16 ? (int)blockDim.x / nm : 16;
        const int tm = threadIdx.x % nm, tg = threadIdx.x / nm;
        double* s_wz = s_ms + GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D);        // [ds][nw], behind the mean sums
        const double* p = A.part + (size_t)b * A.nwork * nm;
        const bool filter = !A.ust_inline && A.work;
        for (int a = 0; a < ds; ++a) {
            const int w0 = A.ust_inline ? A.ust[a] : (A.work ? 0 : A.ustart[a]);
            const int w1 = A.ust_inline ? A.ust[a + 1] : (A.work ? A.nwork : A.ustart[a + 1]);
            double z0 = 0.0;
            for (int wi = w0 + threadIdx.x; wi < w1; wi += blockDim.x) {
                if (filter && A.work[4 * wi] != a) continue;
                z0 += p[(size_t)wi * nm];
            }
            z0 = wave_sum(z0);
            if (lane == 0) s_wz[a * nw + w] = z0;
        }
        for (int a = 0; a < ds && nm > 1; ++a) {              // the other moments of the owned GP(s), one GP at a time
            if (own >= 0 && own != a) continue;               // (workgroup-uniform)
            const int w0 = A.ust_inline ? A.ust[a] : (A.work ? 0 : A.ustart[a]);
            const int w1 = A.ust_inline ? A.ust[a + 1] : (A.work ? A.nwork : A.ustart[a + 1]);
            if (tg < GR) {
                double sum = 0.0;
                for (int wi = w0 + tg; wi < w1; wi += GR) {
                    if (filter && A.work[4 * wi] != a) continue;
                    sum += p[(size_t)wi * nm + tm];
                }
                s_red[tm * GR + tg] = sum;
            }
            __syncthreads();
            if (threadIdx.x >= 1 && (int)threadIdx.x < nm) {
                const double* r = s_red + threadIdx.x * GR;
                double sum = 0.0;
                for (int g = 0; g < GR; ++g) sum += r[g];
                s_z[a * nm + threadIdx.x] = sum;
            }
            __syncthreads();                                  // s_red is reused by the next owned GP
        }
        __syncthreads();
        for (int a = threadIdx.x; a < ds; a += blockDim.x) {
            double sum = 0.0;
            for (int ww = 0; ww < nw; ++ww) sum += s_wz[a * nw + ww];
            s_z[a * nm] = sum;
        }
        if (nm > 1)
            for (int o = threadIdx.x; o < ds * nm; o += blockDim.x) {
                const int a = o / nm, m = o - a * nm;
                if (m > 0 && own >= 0 && own != a) s_z[o] = 0.0;       // not needed by this workgroup
            }
    } else {
        // Few items per GP: GPMPC_RED_CH threads share one output (each a strided subset of the work items, so the
        // global loads of a pass are independent), then a fixed-order combine.
        // Four loads in flight per thread (this reduction is a chain of L2 round trips, not of arithmetic: it was 44 % of the
        // head kernel at N = 1024, B = 16 with one load at a time); the XCD-sorted list is walked through its per-unit index
        // (perm) instead of filtering all items.
        const int nout = ds * nm, ch = threadIdx.x % GPMPC_RED_CH, per_pass = blockDim.x / GPMPC_RED_CH;
        for (int o0 = 0; o0 < nout; o0 += per_pass) {
            const int o = o0 + threadIdx.x / GPMPC_RED_CH;
            if (o < nout) {
                const int a = o / nm, m = o - a * nm;
                const double* p = A.part + (size_t)b * A.nwork * nm + m;
                const int w0 = A.ust_inline ? A.ust[a] : A.ustart[a], w1 = A.ust_inline ? A.ust[a + 1] : A.ustart[a + 1];
                const int* __restrict__ pm = (!A.ust_inline && A.work) ? A.perm : nullptr;
                double s = 0.0;
                for (int k = w0 + ch; k < w1; k += 4 * GPMPC_RED_CH) {
                    const int k1 = k + GPMPC_RED_CH, k2 = k + 2 * GPMPC_RED_CH, k3 = k + 3 * GPMPC_RED_CH;
                    const int c1 = k1 < w1 ? k1 : k, c2 = k2 < w1 ? k2 : k, c3 = k3 < w1 ? k3 : k;      // clamped: no divergent loads
                    const int i0 = pm ? pm[k] : k, i1 = pm ? pm[c1] : c1, i2 = pm ? pm[c2] : c2, i3 = pm ? pm[c3] : c3;
                    const double v0 = p[(size_t)i0 * nm], v1 = p[(size_t)i1 * nm], v2 = p[(size_t)i2 * nm], v3 = p[(size_t)i3 * nm];
                    s += (v0 + (k1 < w1 ? v1 : 0.0)) + ((k2 < w1 ? v2 : 0.0) + (k3 < w1 ? v3 : 0.0));
                }
                s_red[o * GPMPC_RED_CH + ch] = s;
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < nout; o += blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < GPMPC_RED_CH; ++c) s += s_red[o * GPMPC_RED_CH + c];
            s_z[o] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < ds) {
        const int a = threadIdx.x;
        const double* sp = s_spv + a * A.sps;
        const double* z = s_z + a * nm;
        const double* ms = s_ms + a * (1 + 2 * D);
        const double cm = sp[1];                                   // chunked layout only
        const double c = sp[0], mu = chunked ? cm * ms[0] : sp[1], sf2 = sp[2];
        const double T = c * z[0];
        const double* ex = sp + sps_of(D);                         // nominal model: the addends prep_step left (mu stays the GP's own mean)
        const double mu_out = NOM ? mu + ex[0] : mu;
        const double var = NOM ? (sf2 - T - mu * mu) + ex[1] : sf2 - T - mu * mu;
        s_mu[a] = mu_out;
        s_var[a] = var;
        if (own < 0 || own == a) {
            A.means[((size_t)b * (A.H + 1) + t) * ds + a] = mu_out;
            A.vars[((size_t)b * (A.H + 1) + t) * ds + a] = var;
            if (A.grad) {
                const int nc = 2 * ds + A.da;
                double* jm = A.jac + (((size_t)b * A.H + (t - 1)) * 2 * ds + a) * nc;        // row of mu_a
                double* jv = A.jac + (((size_t)b * A.H + (t - 1)) * 2 * ds + ds + a) * nc;   // row of var_a
                for (int k = 0; k < D; ++k) {
                    const double Ak = sp[3 + k], sc = sp[3 + D + k];
                    const double Bq = sp[3 + 2 * D + k];                       // chunked layout: B_k (same expressions as prep_step)
                    const double dmu_du = chunked ? -Bq * cm * ms[1 + k] : sp[3 + 2 * D + k];
                    const double dmu_ds = chunked ? -0.5 * mu * Bq + 0.5 * Bq * Bq * cm * ms[1 + D + k] : sp[3 + 3 * D + k];
                    const double dT_du = -4.0 * sc * c * z[1 + k];
                    const double dT_ds = Ak * (c * z[1 + D + k] - 0.5 * T);
                    double dv_du = -dT_du - 2.0 * mu * dmu_du;
                    double dv_ds = -dT_ds - 2.0 * mu * dmu_ds;
                    double dm_du = dmu_du;
                    if (NOM) { dm_du += ex[2 + 2 * D + k]; dv_du += ex[2 + k]; dv_ds += ex[2 + D + k]; }
                    if (k < ds) {
                        jm[k] = dm_du; jm[ds + k] = dmu_ds;
                        jv[k] = dv_du;  jv[ds + k] = dv_ds;
                    } else {            // action input: its variance is a constant
                        jm[2 * ds + (k - ds)] = dm_du;
                        jv[2 * ds + (k - ds)] = dv_du;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// step_tail.hip: finish step H, the cost and (grad) the adjoint sweep of A.B trajectories on s; GPMPC_E_ARG when the horizon does not fit
// the tail kernel's LDS budget
int gpmpc_launch_roll_tail(const RollArgs& A, bool grad, hipStream_t s);
// The 48 KB budget of its dynamic LDS: the per-step terms of the horizon plus the step Jacobians of all H steps (grad) or of one (no grad, and
// what the launcher falls back to with grad).  A horizon that fails with grad = false cannot be costed at all.
bool gpmpc_roll_tail_fits(int H, int ds, int da, bool grad);
