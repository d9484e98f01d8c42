// Per-step "head" / "tail" kernels of the rollout: the O(N) mean moments, the O(D) algebra that
// turns the pair-kernel moments into means, variances and their input Jacobians, the risk-sensitive
// cost and the reverse (adjoint) sweep over the horizon.
//
// Reference path restated here (one trajectory per workgroup, all ds GPs):
//   Dynamics.forward_propagate_torch   src/dynamics.py:145-189   (u_t, S_t assembly, diag covariance)
//   mean_prop_torch                    src/tools/uncertainty_prop.py:329-338
//   variance_prop_torch scalars        src/tools/uncertainty_prop.py:374-377, :399
//   RiskSensitiveMPC.cost_torch        src/mpc.py:179-198
//   RiskSensitiveMPC.gradient          src/mpc.py:251 (autograd backward -> analytic adjoint)
//
// Closed forms (S diagonal, s_k its entries, lambda_k the GP's squared length-scales):
//   B_k = 1/(s_k + lambda_k),  c_m = sf^2 prod_k (s_k/lambda_k + 1)^-1/2
//   mu = c_m sum_i beta_i exp(-1/2 sum_k B_k v_ik^2),  v_i = u - x_i
//   dmu/du_k = -B_k c_m sum_i p_i v_ik,   dmu/ds_k = -1/2 mu B_k + 1/2 B_k^2 c_m sum_i p_i v_ik^2
//   A_k = 1/(lambda_k/2 + s_k),  c = prod_k (2 s_k/lambda_k + 1)^-1/2,  h_ik = sqrt(A_k/8) v_ik
//   T = c Z0,  dT/du_k = -4 sqrt(A_k/8) c Z1_k,  dT/ds_k = A_k (c Z2_kk - T/2)
//   var = sf^2 - T - mu^2     (no clamp; src/tools/uncertainty_prop.py:399)
#include "gpmpc_internal.h"
#include "plan.h"
#include "fast_exp.h"
#include <cstdlib>
#include <new>

// Diagnostic build (-DGPMPC_SB_STAMPS): phase stamps of the head kernel, workgroup (0, 0, 0) of horizon step 5 (tools/sb_stamps.py)
#ifdef GPMPC_SB_STAMPS
static __device__ unsigned long long g_head_stamps[16];
#define GPMPC_HST(slot) do { if (t == 5 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) g_head_stamps[slot] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int gpmpc_debug_head_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_head_stamps), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -3;
}
#else
#define GPMPC_HST(slot) do { } while (0)
#endif

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
    int shared;    // shared-lambda path: G is [B][Np][gw], written by the workgroups of GP 0 only (pair_kernel_sbs.h)
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
};

// layout of sp (doubles): 0 c | 1 mu | 2 sf2 | 3 A[D] | 3+D scale[D] | 3+2D dmu_du[D] | 3+3D dmu_ds[D]
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

// Prepare step t (>= 1) for GP a: input moments (mean/var of step t-1 in s_mu / s_var, action t-1), the O(N) mean
// sums, the pair-kernel parameters.
// NOM: 0 no nominal model | 1 linear nominal model, objective only | 2 with the gradient (E1, E2 carried through the row loop)
template <int D, int NOM>
__device__ static void prep_step(const RollArgs& A, int b, int t, int a, int chunk, const double* s_mu, const double* s_var,
                                 double* s_u, double* s_s, double* s_scr, double* s_out, double* s_g) {
    const int ds = A.ds;
    // per-dimension scalars: one lane per input dimension (the divisions and square roots are long dependent chains;
    // every thread redoing all D of them, and thread 0 redoing them again at the end, was half of this kernel's time
    // for small batches)
    __shared__ double s_B[GPMPC_MAX_D], s_A[GPMPC_MAX_D], s_sc[GPMPC_MAX_D], s_r1[GPMPC_MAX_D], s_r2[GPMPC_MAX_D];
    __shared__ double s_n[NOM ? GPMPC_MAX_D : 1], s_wB[NOM ? GPMPC_MAX_D : 1];      // nominal model: n_ak and w_k B_k = n_ak s_k B_k
    constexpr int NV = 1 + 2 * D + (NOM == 2 ? 2 * D : 0);                          // sums of the row loop: [p | p v | p v^2 | E1 | E2]
    if (threadIdx.x < D) {
        const int k = threadIdx.x;
        double uk, sk;
        if (k < ds) {
            uk = s_mu[k];
            sk = s_var[k];
        } else {
            uk = A.U[((size_t)b * A.H + (t - 1)) * A.da + (k - ds)];
            sk = GPMPC_ACTION_VAR;
        }
        const double lam = A.lam[a * D + k];
        s_u[k] = uk;
        s_s[k] = sk;
        s_B[k] = 1.0 / (sk + lam);
        s_A[k] = 1.0 / (0.5 * lam + sk);
        s_sc[k] = sqrt(0.125 / (0.5 * lam + sk));          // the scale of the pair transform h = sc (u - x): pp and G rows use this value
        s_r1[k] = sk / lam + 1.0;                          // factors of det(S/Lambda + I) and det(2S/Lambda + I)
        s_r2[k] = 2.0 * sk / lam + 1.0;
        if (NOM) {
            const double nk = A.nom[a * D + k];
            s_n[k] = nk;
            s_wB[k] = (nk * sk) * s_B[k];
        }
    }
    __syncthreads();
    GPMPC_HST(2);
    double u[D], Bk[D], sck[D], wB[NOM == 2 ? D : 1];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        u[k] = s_u[k];
        Bk[k] = s_B[k];
        sck[k] = s_sc[k];
        if (NOM == 2) wB[k] = s_wB[k];
    }
    double* __restrict__ Grow = A.G ? (A.shared ? (a == 0 ? A.G + (size_t)b * A.Np * A.gw : nullptr)
                                                : A.G + ((size_t)b * ds + a) * A.Np * A.gw) : nullptr;
    double v[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) v[m] = 0.0;
    const bool chunked = A.hchunks > 1;
    const int r0 = chunked ? chunk * A.hrows : 0, r1 = chunked ? (r0 + A.hrows < A.Np ? r0 + A.hrows : A.Np) : A.Np;
    // The points of up to PF row blocks are fetched first (clamped addresses, one round trip for all of them), then the blocks
    // are evaluated in order: same per-thread summation order as a plain loop, a quarter of the exposed load latency.
    constexpr int PF = 4;
    for (int ib = r0; ib < r1; ib += PF * (int)blockDim.x) {
        double xpf[PF][D], bpf[PF];
#pragma unroll
        for (int r = 0; r < PF; ++r) {
            const int i = ib + r * (int)blockDim.x + (int)threadIdx.x, ic = i < r1 ? i : r1 - 1;
#pragma unroll
            for (int k = 0; k < D; ++k) xpf[r][k] = A.XT[(size_t)k * A.Np + ic];
            bpf[r] = A.beta[(size_t)a * A.Np + ic];
        }
#pragma unroll
        for (int r = 0; r < PF; ++r) {
        const int i0 = ib + r * (int)blockDim.x;               // uniform trip count: the G rows go through LDS
        if (i0 >= r1) break;
        const int i = i0 + threadIdx.x;
        if (i < r1) {
            double d[D], xk[D], q = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) { xk[k] = xpf[r][k]; d[k] = u[k] - xk[k]; q = fma(Bk[k] * d[k], d[k], q); }
            const double p = bpf[r] * exp(-0.5 * q);
            v[0] += p;
#pragma unroll
            for (int k = 0; k < D; ++k) { v[1 + k] = fma(p, d[k], v[1 + k]); v[1 + D + k] = fma(p * d[k], d[k], v[1 + D + k]); }
            if (NOM == 2) {
                double qn = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) qn = fma(wB[k], d[k], qn);
                const double pq = p * qn;
#pragma unroll
                for (int k = 0; k < D; ++k) { v[1 + 2 * D + k] = fma(pq, d[k], v[1 + 2 * D + k]); v[1 + 3 * D + k] = fma(pq * d[k], d[k], v[1 + 3 * D + k]); }
            }
            if (Grow) {    // column row of point i: [h (D) | |h|^2 | h_k^2 (k < ds) | pad], h = sc o u - sc o x as in the pair kernel
                double* g = s_g + threadIdx.x * A.gw;
                double qh = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double h = fma(-sck[k], xk[k], sck[k] * u[k]);
                    g[k] = h;
                    qh = fma(h, h, qh);
                    if (k < ds) g[D + 1 + k] = h * h;
                }
                g[D] = GPMPC_EXP_NEG_INV_C * qh;               // pre-scaled for gpmpc_exp_neg_scaled (fast_exp.h)
                for (int k = D + 1 + ds; k < A.gw; ++k) g[k] = 0.0;
            }
        }
        if (Grow) {        // rows of blockDim.x consecutive points are contiguous in G: write them out lane-contiguously
            __syncthreads();
            const int rows = (r1 - i0 < (int)blockDim.x) ? r1 - i0 : (int)blockDim.x;
            double* dst = Grow + (size_t)i0 * A.gw;
            for (int e = threadIdx.x; e < rows * A.gw; e += blockDim.x) dst[e] = s_g[e];
            __syncthreads();
        }
        }
    }
    GPMPC_HST(3);
    block_sum<NV>(v, s_scr, s_out);
    GPMPC_HST(4);
    if (chunked) {
        // partial sums of this row chunk; the constants of the step by chunk 0 (the next launch's finish phase forms mu)
        if (threadIdx.x < 1 + 2 * D)
            A.mpart[((((size_t)(t & 1) * A.B + b) * ds + a) * A.hchunks + chunk) * (1 + 2 * D) + threadIdx.x] = s_out[threadIdx.x];
        if (chunk == 0 && threadIdx.x < D) {
            const int k = threadIdx.x;
            const double sf = A.sf[a], sf2 = sf * sf;
            double detm = 1.0, detv = 1.0;
            for (int l = 0; l < D; ++l) { detm *= s_r1[l]; detv *= s_r2[l]; }
            const double cm = sf2 / sqrt(detm), c = 1.0 / sqrt(detv);
            double* sp = A.sp + (((size_t)(t & 1) * A.B + b) * ds + a) * A.sps;
            double* pp = A.pp + ((size_t)b * ds + a) * A.pps;
            if (k == 0) { sp[0] = c; sp[1] = cm; sp[2] = sf2; }
            const double sc = s_sc[k];
            sp[3 + k] = s_A[k]; sp[3 + D + k] = sc;
            sp[3 + 2 * D + k] = s_B[k];
            pp[k] = sc * s_u[k];
            pp[D + k] = sc;
        }
        return;
    }
    if (threadIdx.x < D) {                                    // lane k writes the entries of dimension k; lane 0 the scalars
        const int k = threadIdx.x;
        const double sf = A.sf[a], sf2 = sf * sf;
        double detm = 1.0, detv = 1.0;
        for (int l = 0; l < D; ++l) { detm *= s_r1[l]; detv *= s_r2[l]; }
        const double cm = sf2 / sqrt(detm), c = 1.0 / sqrt(detv);
        const double mu = cm * s_out[0];
        double* sp = A.sp + (((size_t)(t & 1) * A.B + b) * ds + a) * A.sps;   // other parity than the finish phase reads
        double* pp = A.pp + ((size_t)b * ds + a) * A.pps;
        if (k == 0) { sp[0] = c; sp[1] = mu; sp[2] = sf2; }
        const double Bq = s_B[k], sc = s_sc[k];
        sp[3 + k] = s_A[k]; sp[3 + D + k] = sc;
        sp[3 + 2 * D + k] = -Bq * cm * s_out[1 + k];
        sp[3 + 3 * D + k] = -0.5 * mu * Bq + 0.5 * Bq * Bq * cm * s_out[1 + D + k];
        pp[k] = sc * s_u[k];
        pp[D + k] = sc;
        if (NOM) {      // the addends of the nominal model (layout at sps_nominal); every lane forms the two sums over all dimensions in the same order
            double* ex = sp + sps_of(D);
            double lin = A.nom[A.ds * D + a], vlin = 0.0, cross = 0.0;
            for (int l = 0; l < D; ++l) {
                const double nl = s_n[l], wl = nl * s_s[l];
                lin = fma(nl, s_u[l], lin);
                vlin = fma(nl * nl, s_s[l], vlin);
                cross = fma(wl, -s_B[l] * cm * s_out[1 + l], cross);        // sum_l w_l dmu_g/du_l
            }
            if (k == 0) { ex[0] = lin; ex[1] = vlin + 2.0 * cross; }
            if (NOM == 2) {
                const double nk = s_n[k], wk = nk * s_s[k];
                ex[2 + k] = 2.0 * (cm * Bq * s_out[1 + 2 * D + k] - wk * Bq * mu);
                ex[2 + D + k] = nk * nk + 2.0 * nk * (-Bq * cm * s_out[1 + k]) - 0.5 * Bq * (2.0 * cross)
                                + Bq * Bq * cm * (2.0 * wk * s_out[1 + k] - s_out[1 + 3 * D + k]);
                ex[2 + 2 * D + k] = nk;
            }
        }
    }
}

// One workgroup per (trajectory, GP).  The finish phase of step t-1 reads sp/pp/part written by the previous
// launches and the prep phase overwrites sp/pp of ITS OWN GP only, so workgroups of one trajectory never race.
template <int D, int NOM>
__global__ __launch_bounds__(256) void k_roll_head(RollArgs A, int t) {
    __shared__ double s_z[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D)];
    __shared__ double s_zred[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D) * GPMPC_RED_CH];
    __shared__ double s_mu[GPMPC_MAX_DS], s_var[GPMPC_MAX_DS];
    __shared__ double s_u[GPMPC_MAX_D], s_s[GPMPC_MAX_D];
    __shared__ double s_scr[16 * (1 + 2 * D + (NOM == 2 ? 2 * D : 0))], s_out[1 + 2 * D + (NOM == 2 ? 2 * D : 0)];
    __shared__ double s_g[256 * (2 * D + 2)];             // staging of 256 G rows (gw <= 2D + 2)
    __shared__ double s_ms[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D) + 4 * GPMPC_MAX_DS];      // mean sums | Z0 wave sums
    const int b = blockIdx.x, a = blockIdx.y, chunk = blockIdx.z;
    GPMPC_HST(0);
    if (t == 1) {
        if (threadIdx.x < A.ds) {
            const double x = A.x0[(size_t)b * A.ds + threadIdx.x];
            s_mu[threadIdx.x] = x;
            s_var[threadIdx.x] = GPMPC_INIT_VAR;
            if (a == 0 && chunk == 0) {
                A.means[((size_t)b * (A.H + 1)) * A.ds + threadIdx.x] = x;
                A.vars[((size_t)b * (A.H + 1)) * A.ds + threadIdx.x] = GPMPC_INIT_VAR;
            }
        }
        __syncthreads();
    } else {
        finish_step<NOM != 0>(A, b, t - 1, chunk == 0 ? a : A.ds, s_z, s_zred, s_mu, s_var, s_ms);     // rows of GP a are written by chunk 0 only
    }
    GPMPC_HST(1);
    prep_step<D, NOM>(A, b, t, a, chunk, s_mu, s_var, s_u, s_s, s_scr, s_out, s_g);
    GPMPC_HST(5);
}

// ---------------------------------------------------------------------------
// cost (src/mpc.py:179-198) and its derivatives
// ---------------------------------------------------------------------------
// Per-step state cost with a general (possibly non-symmetric) covariance Sig [ds][ds]:
//   (1/gamma) log det(I + gamma Q Sig) + e^T (Q^-1 + gamma Sig)^-1 e,   e = mu - x_ref.
// (Q^-1 + gamma Sig)^-1 = (I + gamma Q Sig)^-1 Q =: Z, so one LU of Mx = I + gamma Q Sig gives the
// determinant and Z (no inverse of Q is formed).  Optionally returns d/dmu and d/dSig_kk.
// w: scratch, ds * 2ds doubles.  gamma == 0: tr(Q Sig) + e^T Q e.
// dsig (optional, [ds][ds], general Sigma): d/dSig_kl = Z_lk - gamma (Z^T e)_k (Z e)_l -- what autograd returns for the
// reference's expression with a non-symmetric Sig (src/mpc.py:182-185).
__device__ static double state_cost(int ds, const gpmpc_cost_params& C, const double* mu, const double* Sig, int sig_ld,
                                    bool sig_diag, double* w, double* dmu, double* dvar, double* dsig = nullptr) {
    const double g = C.gamma;
    double e[GPMPC_MAX_DS];
    for (int k = 0; k < ds; ++k) e[k] = mu[k] - C.x_ref[k];
    if (g == 0.0) {
        double c = 0.0;
        for (int k = 0; k < ds; ++k) {
            double qe = 0.0;
            for (int l = 0; l < ds; ++l) {
                qe += C.Q[k * ds + l] * e[l];
                const double sig_lk = sig_diag ? (l == k ? Sig[k] : 0.0) : Sig[l * sig_ld + k];
                c += C.Q[k * ds + l] * sig_lk;
            }
            c += e[k] * qe;
            if (dmu) {
                double qte = 0.0;
                for (int l = 0; l < ds; ++l) qte += C.Q[l * ds + k] * e[l];
                dmu[k] = qe + qte;
                if (dvar) dvar[k] = C.Q[k * ds + k];
                if (dsig) for (int l = 0; l < ds; ++l) dsig[k * ds + l] = C.Q[l * ds + k];
            }
        }
        return c;
    }
    const int ld = 2 * ds;     // augmented [Mx | Q]
    for (int r = 0; r < ds; ++r)
        for (int cc = 0; cc < ds; ++cc) {
            double s = 0.0;
            if (sig_diag) s = C.Q[r * ds + cc] * Sig[cc];
            else for (int l = 0; l < ds; ++l) s += C.Q[r * ds + l] * Sig[l * sig_ld + cc];
            w[r * ld + cc] = (r == cc ? 1.0 : 0.0) + g * s;
            w[r * ld + ds + cc] = C.Q[r * ds + cc];
        }
    double det = 1.0;
    for (int k = 0; k < ds; ++k) {           // Gauss-Jordan with partial pivoting
        int piv = k; double best = fabs(w[k * ld + k]);
        for (int r = k + 1; r < ds; ++r) { const double v = fabs(w[r * ld + k]); if (v > best) { best = v; piv = r; } }
        if (piv != k) {
            for (int cc = 0; cc < ld; ++cc) { const double tmp = w[k * ld + cc]; w[k * ld + cc] = w[piv * ld + cc]; w[piv * ld + cc] = tmp; }
            det = -det;
        }
        const double pv = w[k * ld + k];
        det *= pv;
        const double inv = 1.0 / pv;
        for (int cc = 0; cc < ld; ++cc) w[k * ld + cc] *= inv;
        for (int r = 0; r < ds; ++r) {
            if (r == k) continue;
            const double f = w[r * ld + k];
            for (int cc = 0; cc < ld; ++cc) w[r * ld + cc] = fma(-f, w[k * ld + cc], w[r * ld + cc]);
        }
    }
    // Z = w[:, ds:]
    double ze[GPMPC_MAX_DS], zte[GPMPC_MAX_DS], quad = 0.0;
    for (int k = 0; k < ds; ++k) {
        double s = 0.0, st = 0.0;
        for (int l = 0; l < ds; ++l) { s += w[k * ld + ds + l] * e[l]; st += w[l * ld + ds + k] * e[l]; }
        ze[k] = s; zte[k] = st;
        quad += e[k] * s;
    }
    if (dmu)
        for (int k = 0; k < ds; ++k) {
            dmu[k] = ze[k] + zte[k];
            if (dvar) dvar[k] = w[k * ld + ds + k] - g * zte[k] * ze[k];
            if (dsig) for (int l = 0; l < ds; ++l) dsig[k * ds + l] = w[l * ld + ds + k] - g * zte[k] * ze[l];
        }
    return log(det) / g + quad;
}

// Input-cost terms of ONE step j (src/mpc.py:188-198) with their gradient w.r.t. U_j written (not accumulated) to gUj:
// lets the tail evaluate the H steps on H threads.  The R_delta term couples neighbours: step j owns
// d/dU_j of both (U_j - U_{j-1})^T R_d (U_j - U_{j-1}) and (U_{j+1} - U_j)^T R_d (U_{j+1} - U_j).
__device__ static double input_cost_step(int j, int H, int da, const gpmpc_cost_params& C, const double* __restrict__ U,
                                         double* gUj) {
    double d[GPMPC_MAX_D], dd[GPMPC_MAX_D], dn[GPMPC_MAX_D];
    for (int k = 0; k < da; ++k) {
        const double uj = U[j * da + k];
        d[k] = uj - C.u_ref[k];
        dd[k] = uj - (j == 0 ? C.last_u[k] : U[(j - 1) * da + k]);
        dn[k] = (j + 1 < H) ? U[(j + 1) * da + k] - uj : 0.0;
    }
    double c = 0.0;
    for (int k = 0; k < da; ++k) {
        double rd = 0.0, rtd = 0.0;
        for (int l = 0; l < da; ++l) { rd += C.R[k * da + l] * d[l]; rtd += C.R[l * da + k] * d[l]; }
        c += d[k] * rd;
        double g = rd + rtd;
        if (C.has_R_delta) {
            double qd = 0.0, qtd = 0.0, qn = 0.0, qtn = 0.0;
            for (int l = 0; l < da; ++l) {
                qd += C.R_delta[k * da + l] * dd[l]; qtd += C.R_delta[l * da + k] * dd[l];
                qn += C.R_delta[k * da + l] * dn[l]; qtn += C.R_delta[l * da + k] * dn[l];
            }
            c += dd[k] * qd;
            g += (qd + qtd) - (qn + qtn);
        }
        if (gUj) gUj[k] = g;
    }
    return c;
}

// The same cost term for a DIAGONAL covariance with the state dimension known at compile time: everything lives in
// registers (the generic version above walks an LDS scratch and the kernel-argument Q with run-time indices, ~20 k
// cycles of dependent latency per call at ds = 3, which was most of the tail kernel for small batches).
template <int DS>
__device__ static double state_cost_diag(const gpmpc_cost_params& C, const double* __restrict__ mu,
                                         const double* __restrict__ var, double* dmu, double* dvar) {
    const double g = C.gamma;
    double e[DS], Q[DS][DS], sg[DS];
#pragma unroll
    for (int k = 0; k < DS; ++k) {
        e[k] = mu[k] - C.x_ref[k];
        sg[k] = var[k];
#pragma unroll
        for (int l = 0; l < DS; ++l) Q[k][l] = C.Q[k * DS + l];
    }
    if (g == 0.0) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < DS; ++k) {
            double qe = 0.0, qte = 0.0;
#pragma unroll
            for (int l = 0; l < DS; ++l) { qe += Q[k][l] * e[l]; qte += Q[l][k] * e[l]; }
            c += Q[k][k] * sg[k];
            c += e[k] * qe;
            if (dmu) { dmu[k] = qe + qte; dvar[k] = Q[k][k]; }
        }
        return c;
    }
    double w[DS][2 * DS];          // augmented [I + gamma Q Sig | Q]
#pragma unroll
    for (int r = 0; r < DS; ++r)
#pragma unroll
        for (int cc = 0; cc < DS; ++cc) {
            w[r][cc] = (r == cc ? 1.0 : 0.0) + g * (Q[r][cc] * sg[cc]);
            w[r][DS + cc] = Q[r][cc];
        }
    double det = 1.0;
#pragma unroll
    for (int k = 0; k < DS; ++k) {           // Gauss-Jordan with partial pivoting (row swaps as predicated moves)
        int piv = k;
        double best = fabs(w[k][k]);
#pragma unroll
        for (int r = k + 1; r < DS; ++r) { const double v = fabs(w[r][k]); if (v > best) { best = v; piv = r; } }
#pragma unroll
        for (int r = k + 1; r < DS; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int cc = 0; cc < 2 * DS; ++cc) {
                const double a = w[k][cc], bb = w[r][cc];
                w[k][cc] = sw ? bb : a;
                w[r][cc] = sw ? a : bb;
            }
        }
        if (piv != k) det = -det;
        const double pv = w[k][k];
        det *= pv;
        const double inv = 1.0 / pv;
#pragma unroll
        for (int cc = 0; cc < 2 * DS; ++cc) w[k][cc] *= inv;
#pragma unroll
        for (int r = 0; r < DS; ++r) {
            if (r == k) continue;
            const double f = w[r][k];
#pragma unroll
            for (int cc = 0; cc < 2 * DS; ++cc) w[r][cc] = fma(-f, w[k][cc], w[r][cc]);
        }
    }
    double ze[DS], zte[DS], quad = 0.0;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
        double s1 = 0.0, st = 0.0;
#pragma unroll
        for (int l = 0; l < DS; ++l) { s1 += w[k][DS + l] * e[l]; st += w[l][DS + k] * e[l]; }
        ze[k] = s1; zte[k] = st;
        quad += e[k] * s1;
    }
    if (dmu) {
#pragma unroll
        for (int k = 0; k < DS; ++k) {
            dmu[k] = ze[k] + zte[k];
            dvar[k] = w[k][DS + k] - g * zte[k] * ze[k];
        }
    }
    return log(det) / g + quad;
}

// Input-cost terms (src/mpc.py:188-198) for one trajectory; optionally accumulates d/dU into gU [H][da].
__device__ static double input_cost(int H, int da, const gpmpc_cost_params& C, const double* U, double* gU) {
    double c = 0.0;
    for (int j = 0; j < H; ++j) {
        double d[GPMPC_MAX_D];
        for (int k = 0; k < da; ++k) d[k] = U[j * da + k] - C.u_ref[k];
        for (int k = 0; k < da; ++k) {
            double rd = 0.0, rtd = 0.0;
            for (int l = 0; l < da; ++l) { rd += C.R[k * da + l] * d[l]; rtd += C.R[l * da + k] * d[l]; }
            c += d[k] * rd;
            if (gU) gU[j * da + k] += rd + rtd;
        }
        if (C.has_R_delta) {
            for (int k = 0; k < da; ++k) d[k] = U[j * da + k] - (j == 0 ? C.last_u[k] : U[(j - 1) * da + k]);
            for (int k = 0; k < da; ++k) {
                double rd = 0.0, rtd = 0.0;
                for (int l = 0; l < da; ++l) { rd += C.R_delta[k * da + l] * d[l]; rtd += C.R_delta[l * da + k] * d[l]; }
                c += d[k] * rd;
                if (gU) { gU[j * da + k] += rd + rtd; if (j > 0) gU[(j - 1) * da + k] -= rd + rtd; }
            }
        }
    }
    return c;
}

// Tail: finish step H, cost, adjoint sweep.  One workgroup (256 threads) per trajectory; the first
// GPMPC_TAIL_WORKERS threads evaluate the per-step cost terms (register-resident LU, state_cost_diag), then the
// reverse sweep over the (2ds) x (2ds+da) step Jacobians.
// dynamic LDS: [H+1] cost terms | [H+1][2ds] local derivatives | [H*da] grad | [H] input-cost terms | [H or 1][nz*nc] J
#define GPMPC_TAIL_WORKERS 32
template <bool ALLJ, int DS, bool NOM>
__global__ __launch_bounds__(256) void k_roll_tail(RollArgs A) {
    extern __shared__ double s_dyn[];
    __shared__ double s_z[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D)];
    __shared__ double s_zred[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D) * GPMPC_RED_CH];
    __shared__ double s_mu[GPMPC_MAX_DS], s_var[GPMPC_MAX_DS];
    __shared__ double s_adj[2][2 * GPMPC_MAX_DS];
    const int b = blockIdx.x, ds = A.ds, da = A.da, H = A.H, tid = threadIdx.x;
    const int nz = 2 * ds, nc = 2 * ds + da;
    __shared__ double s_ms[GPMPC_MAX_DS * (1 + 2 * GPMPC_MAX_D) + 4 * GPMPC_MAX_DS];      // mean sums | Z0 wave sums
    if (!A.finished) finish_step<NOM>(A, b, H, -1, s_z, s_zred, s_mu, s_var, s_ms);
    double* s_ct = s_dyn;
    double* s_dl = s_ct + (H + 1);
    double* s_gU = s_dl + (size_t)(H + 1) * nz;
    double* s_ci = s_gU + H * da;
    double* s_J = s_ci + H;
    const double* mu = A.means + (size_t)b * (H + 1) * ds;
    const double* var = A.vars + (size_t)b * (H + 1) * ds;
    if (ALLJ && A.grad) {                                 // issue the Jacobian loads before the (long, serial) cost terms
        const double* Jb = A.jac + (size_t)b * H * nz * nc;
        for (int q = tid; q < H * nz * nc; q += blockDim.x) s_J[q] = Jb[q];
    }
    for (int i = tid; i <= H && tid < GPMPC_TAIL_WORKERS; i += GPMPC_TAIL_WORKERS)
        s_ct[i] = state_cost_diag<DS>(A.cost, mu + i * ds, var + i * ds, A.grad ? s_dl + i * nz : nullptr,
                                      A.grad ? s_dl + i * nz + ds : nullptr);
    // input-cost terms: one thread per step, on the waves that do not carry the state-cost workers
    for (int j = tid - 64; j >= 0 && j < H; j += blockDim.x - 64)
        s_ci[j] = input_cost_step(j, H, da, A.cost, A.U + (size_t)b * H * da, A.grad ? s_gU + j * da : nullptr);
    // ALLJ: the Jacobians of ALL steps fit in LDS: fetch them in one round of independent loads while the cost terms are
    // finished, then wave 0 runs the whole reverse sweep alone -- no workgroup barriers, no exposed global-load latency
    // per step (small batches: 29 -> 16 us at H = 20).  Otherwise: one step per iteration, the Jacobian of the next
    // step prefetched into registers (nz*nc <= 288 doubles: <= 2 per thread).
    const double* Jg = A.grad ? A.jac + ((size_t)b * H + (H - 1)) * nz * nc : nullptr;
    double j0 = 0.0, j1 = 0.0;
    if (!ALLJ) {
        j0 = (Jg && tid < nz * nc) ? Jg[tid] : 0.0;
        j1 = (Jg && tid + 256 < nz * nc) ? Jg[tid + 256] : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i <= H; ++i) total += s_ct[i];
        for (int j = 0; j < H; ++j) total += s_ci[j];
        A.out_cost[b] = total;
    }
    if (!A.grad) return;
    if (tid < nz) s_adj[0][tid] = s_dl[H * nz + tid];
    int cur = 0;
    if (ALLJ) {
        if (tid >= 64) return;                            // wave 0 carries on alone: LDS ops of one wave execute in order
        for (int t = H; t >= 1; --t) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // s_adj[cur] / s_gU of the previous iteration are written
            if (tid < nc) {
                const double* Jt = s_J + (size_t)(t - 1) * nz * nc;
                double sum = 0.0;
                for (int r = 0; r < nz; ++r) sum = fma(Jt[r * nc + tid], s_adj[cur][r], sum);
                if (tid < nz) s_adj[cur ^ 1][tid] = s_dl[(t - 1) * nz + tid] + sum;
                else s_gU[(t - 1) * da + (tid - nz)] += sum;    // input-cost gradients were written before the barrier above
            }
            cur ^= 1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int q = tid; q < H * da; q += 64) A.out_grad[(size_t)b * H * da + q] = s_gU[q];
        return;
    }
    for (int t = H; t >= 1; --t) {
        if (tid < nz * nc) s_J[tid] = j0;
        if (tid + 256 < nz * nc) s_J[tid + 256] = j1;
        __syncthreads();                                  // J of step t and adj of step t are in LDS
        if (t > 1) {                                      // prefetch the Jacobian of step t-1
            const double* Jn = A.jac + ((size_t)b * H + (t - 2)) * nz * nc;
            j0 = tid < nz * nc ? Jn[tid] : 0.0;
            j1 = tid + 256 < nz * nc ? Jn[tid + 256] : 0.0;
        }
        if (tid < nc) {
            double sum = 0.0;
            for (int r = 0; r < nz; ++r) sum = fma(s_J[r * nc + tid], s_adj[cur][r], sum);
            if (tid < nz) s_adj[cur ^ 1][tid] = s_dl[(t - 1) * nz + tid] + sum;
            else s_gU[(t - 1) * da + (tid - nz)] += sum;   // input-cost gradients were written before the first barrier above
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int q = tid; q < H * da; q += blockDim.x) A.out_grad[(size_t)b * H * da + q] = s_gU[q];
}

// Stand-alone cost for given means / FULL covariances (cost_torch parity, src/mpc.py:156-200).
// d_means / d_covs / d_U (all or none): the analytic derivatives autograd takes of the reference's expression
// (src/mpc.py:251 backward through :179-198), for the differentiable cost_torch of the host mirror.
__global__ void k_cost_full(int B, int H, int ds, int da, gpmpc_cost_params C, const double* means, const double* covs,
                            const double* U, double* out, double* d_means, double* d_covs, double* d_U) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double w[GPMPC_MAX_DS * 2 * GPMPC_MAX_DS];
    double total = 0.0;
    for (int i = 0; i <= H; ++i) {
        const size_t o = (size_t)b * (H + 1) + i;
        total += state_cost(ds, C, means + o * ds, covs + o * ds * ds, ds, false, w, d_means ? d_means + o * ds : nullptr,
                            nullptr, d_means ? d_covs + o * ds * ds : nullptr);
    }
    if (d_U) for (int q = 0; q < H * da; ++q) d_U[(size_t)b * H * da + q] = 0.0;
    total += input_cost(H, da, C, U + (size_t)b * H * da, d_U ? d_U + (size_t)b * H * da : nullptr);
    out[b] = total;
}

// Vector-Jacobian product of the rollout (the backward pass of forward_propagate_torch's autograd graph,
// src/dynamics.py:126-191 under src/mpc.py:251): reverse sweep over the step Jacobians J_t [2ds][2ds+da] (rows: mu_t, var_t;
// columns: mu_{t-1}, var_{t-1}, u_{t-1}) seeded with the upstream gradients of EVERY step's mean and variance.
// One wave per trajectory; lane c owns column c.
__global__ __launch_bounds__(64) void k_rollout_vjp(int B, int H, int ds, int da, const double* __restrict__ jac,
                                                    const double* __restrict__ g_means, const double* __restrict__ g_vars,
                                                    double* __restrict__ out_gU, double* __restrict__ out_gx0) {
    __shared__ double s_adj[2][2 * GPMPC_MAX_DS];
    const int b = blockIdx.x, c = threadIdx.x, nz = 2 * ds, nc = 2 * ds + da;
    auto seed = [&](int t, int r) {
        const size_t o = ((size_t)b * (H + 1) + t) * ds;
        return r < ds ? (g_means ? g_means[o + r] : 0.0) : (g_vars ? g_vars[o + (r - ds)] : 0.0);
    };
    if (c < nz) s_adj[0][c] = seed(H, c);
    __syncthreads();
    int cur = 0;
    for (int t = H; t >= 1; --t) {
        const double* Jt = jac + ((size_t)b * H + (t - 1)) * nz * nc;
        if (c < nc) {
            double sum = 0.0;
            for (int r = 0; r < nz; ++r) sum = fma(Jt[r * nc + c], s_adj[cur][r], sum);
            if (c < nz) s_adj[cur ^ 1][c] = seed(t - 1, c) + sum;
            else out_gU[((size_t)b * H + (t - 1)) * da + (c - nz)] = sum;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (out_gx0 && c < ds) out_gx0[(size_t)b * ds + c] = s_adj[cur][c];      // mu_0 = x0; Sigma_0 is a constant
}

// ---------------------------------------------------------------------------
// host side of the rollout
// ---------------------------------------------------------------------------
static thread_local char g_err[256] = "";
void gpmpc_set_error(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
}
void gpmpc_set_error_text(const char* text) { snprintf(g_err, sizeof(g_err), "%s", text); }
extern "C" const char* gpmpc_last_error(void) { return g_err; }
extern "C" const char* gpmpc_version(void) { return "gpmpc-hip 0.1 (gfx950)"; }
extern "C" int gpmpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Opt-in timing of the pair kernel (bench.py): HIP events around every pair launch on the launch stream, accumulated
// per class (full kernel / horizon-step-1 variant).  One process-wide record behind a mutex: concurrent rollouts on
// different streams or host threads may all run with timing on.
#include <mutex>
#include <vector>
struct EvPair { hipEvent_t a, b; int cls; };
static struct {
    std::mutex mu;
    int on = 0;
    double ms[GPMPC_TIME_CLASSES] = {0.0, 0.0, 0.0};
    long long n[GPMPC_TIME_CLASSES] = {0, 0, 0};
    std::vector<EvPair> pending;
} g_time;

static void drain_events_locked() {
    for (const EvPair& ev : g_time.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            g_time.ms[ev.cls] += ms; ++g_time.n[ev.cls];
        }
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
    }
    g_time.pending.clear();
}
static bool timing_on() { std::lock_guard<std::mutex> lk(g_time.mu); return g_time.on != 0; }
extern "C" int gpmpc_timing_enable(int on) { std::lock_guard<std::mutex> lk(g_time.mu); g_time.on = on; return GPMPC_OK; }
extern "C" int gpmpc_pair_kernel_time(double* total_ms, long long* launches, int reset) {
    std::lock_guard<std::mutex> lk(g_time.mu);
    drain_events_locked();
    if (total_ms) *total_ms = g_time.ms[0] + g_time.ms[1] + g_time.ms[2];
    if (launches) *launches = g_time.n[0] + g_time.n[1] + g_time.n[2];
    if (reset) for (int c = 0; c < GPMPC_TIME_CLASSES; ++c) { g_time.ms[c] = 0.0; g_time.n[c] = 0; }
    return GPMPC_OK;
}
extern "C" int gpmpc_pair_kernel_time_class(int cls, double* total_ms, long long* launches) {
    if (cls < 0 || cls >= GPMPC_TIME_CLASSES) return GPMPC_E_ARG;
    std::lock_guard<std::mutex> lk(g_time.mu);
    drain_events_locked();
    if (total_ms) *total_ms = g_time.ms[cls];
    if (launches) *launches = g_time.n[cls];
    return GPMPC_OK;
}

// Bracket one launch with events when timing is on.  `launch` enqueues the kernel on s and returns its status.
template <class F>
static int timed_launch(int cls, hipStream_t s, F launch) {
    if (!timing_on()) return launch();
    EvPair ev; ev.cls = cls;
    GPMPC_HIP(hipEventCreate(&ev.a));
    GPMPC_HIP(hipEventCreate(&ev.b));
    GPMPC_HIP(hipEventRecord(ev.a, s));
    const int rc = launch();
    GPMPC_HIP(hipEventRecord(ev.b, s));
    std::lock_guard<std::mutex> lk(g_time.mu);
    if (g_time.pending.size() >= 4096) drain_events_locked();
    g_time.pending.push_back(ev);
    return rc;
}

int gpmpc_timed_pair(int D, bool diag, bool grad, int tb, int waves, const PairArgs& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FULL, s, [&] { return gpmpc_launch_pair(D, diag, grad, tb, waves, a, s); });
}
int gpmpc_timed_pair_sb(int D, bool grad, int tb, int ns2, int waves, const PairSbArgs& a, hipStream_t s) {
    return timed_launch(a.first_step ? GPMPC_TIME_FIRST : GPMPC_TIME_FULL, s,
                        [&] { return gpmpc_launch_pair_sb(D, grad, tb, ns2, waves, a, s); });
}
int gpmpc_timed_pair_sbs(int D, bool grad, int ng, int ns2, const PairSbsArgs& a, hipStream_t s) {
    return timed_launch(a.first_step ? GPMPC_TIME_FIRST : GPMPC_TIME_FULL, s,
                        [&] { return gpmpc_launch_pair_sbs(D, grad, ng, ns2, a, s); });
}
int gpmpc_timed_pair_sbf(int D, bool grad, int ns2, int waves, const PairSbfArgs& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FULL, s, [&] { return gpmpc_launch_pair_sbf(D, grad, ns2, waves, a, s); });
}

// (the plan selection -- gpmpc_choose_shape, gpmpc_layout_for -- and the tuned table: plan.hip)
// (split_count, the rule for concurrent sub-batches: plan.hip, gpmpc_split_count)

static int launch_persist(int D, bool grad, int ns2, int waves, int ng, const PersistArgs& a, hipStream_t s) {
    switch (D) {
        case 2: return gpmpc_launch_persist_D<2>(grad, ns2, waves, ng, a, s);
        case 3: return gpmpc_launch_persist_D<3>(grad, ns2, waves, ng, a, s);
        case 4: return gpmpc_launch_persist_D<4>(grad, ns2, waves, ng, a, s);
        case 5: return gpmpc_launch_persist_D<5>(grad, ns2, waves, ng, a, s);
        case 6: return gpmpc_launch_persist_D<6>(grad, ns2, waves, ng, a, s);
        case 7: return gpmpc_launch_persist_D<7>(grad, ns2, waves, ng, a, s);
        case 8: return gpmpc_launch_persist_D<8>(grad, ns2, waves, ng, a, s);
    }
    return GPMPC_E_ARG;
}

static int launch_step_fused(int D, bool grad, int ns2, int q, int ng, const FusedArgs& a, int t, hipStream_t s) {
    switch (D) {
        case 1: return gpmpc_launch_step_fused_D<1>(grad, ns2, q, ng, a, t, s);
        case 2: return gpmpc_launch_step_fused_D<2>(grad, ns2, q, ng, a, t, s);
        case 3: return gpmpc_launch_step_fused_D<3>(grad, ns2, q, ng, a, t, s);
        case 4: return gpmpc_launch_step_fused_D<4>(grad, ns2, q, ng, a, t, s);
        case 5: return gpmpc_launch_step_fused_D<5>(grad, ns2, q, ng, a, t, s);
        case 6: return gpmpc_launch_step_fused_D<6>(grad, ns2, q, ng, a, t, s);
        case 7: return gpmpc_launch_step_fused_D<7>(grad, ns2, q, ng, a, t, s);
        case 8: return gpmpc_launch_step_fused_D<8>(grad, ns2, q, ng, a, t, s);
    }
    return GPMPC_E_ARG;
}

template <int D>
static void launch_head(const RollArgs& A, int t, hipStream_t s) {
    const dim3 grid(A.B, A.ds, A.hchunks > 1 ? A.hchunks : 1);
    if (!A.nom) hipLaunchKernelGGL((k_roll_head<D, 0>), grid, dim3(256), 0, s, A, t);
    else if (A.grad) hipLaunchKernelGGL((k_roll_head<D, 2>), grid, dim3(256), 0, s, A, t);
    else hipLaunchKernelGGL((k_roll_head<D, 1>), grid, dim3(256), 0, s, A, t);
}

// ext_jac: caller-owned [B][H][2ds][2ds+da] buffer for the step Jacobians instead of the workspace's (gpmpc_rollout_jac);
// full_first: horizon step 1 keeps the derivatives w.r.t. its state inputs (needed for d/dx0).
static int enqueue_rollout(const gpmpc_pack* p, int B, int H, const double* x0, const double* U,
                           const gpmpc_cost_params* cost, unsigned flags, double* out_means, double* out_vars,
                           double* out_cost, double* out_grad, void* workspace, size_t workspace_bytes, void* stream,
                           double* ext_jac = nullptr, bool full_first = false, const RollShape* shape = nullptr) {
    if (!p || !x0 || !U || !cost || !out_cost || !workspace || B < 1 || H < 1) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    if (grad && !out_grad) return GPMPC_E_ARG;
    const int lowprec = (flags & GPMPC_FP32_ALL) ? 2 : ((flags & GPMPC_FP32_ACCUM) ? 1 : 0);
    if (lowprec && grad) return GPMPC_E_ARG;                   // the sweep modes are objective only
    if (lowprec && p->nominal) {
        gpmpc_set_error_text("gpmpc_rollout: the GPMPC_FP32_* modes do not know the linear nominal model of this pack");
        return GPMPC_E_STATE;
    }
    // shape: the launches of a larger batch this one is a sub-batch of, or of a candidate of gpmpc_pack_autotune; else chosen here
    const RollShape r = shape ? *shape : gpmpc_choose_shape(p, B, H, grad, lowprec != 0);
    const RollLayout L = gpmpc_layout_for(p, r, B, H, grad);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    RollArgs A;
    memset(&A, 0, sizeof(A));
    A.XT = p->XT; A.beta = p->beta; A.lam = p->lam; A.sf = p->sf;
    A.Np = p->Np; A.ds = p->ds; A.da = p->da; A.D = p->D;
    A.x0 = x0; A.U = U; A.B = B; A.H = H;
    A.means = out_means ? out_means : (double*)(ws + L.off_means);
    A.vars = out_vars ? out_vars : (double*)(ws + L.off_vars);
    A.pp = (double*)(ws + L.off_pp); A.sp = (double*)(ws + L.off_sp); A.part = (double*)(ws + L.off_part);
    A.jac = grad ? (ext_jac ? ext_jac : (double*)(ws + L.off_jac)) : nullptr;
    A.hchunks = r.hchunks; A.hrows = r.hrows; A.mpart = r.hchunks > 1 ? (double*)(ws + L.off_mpart) : nullptr;
    A.G = r.sb ? (double*)(ws + L.off_G) : nullptr; A.gw = L.gw;
    A.pps = L.pps; A.sps = L.sps; A.nwork = r.nwork; A.nm = L.nm; A.grad = grad ? 1 : 0;
    A.ustart = p->wl[0][r.tiling].ustart_dev;
    A.work = p->wl[0][r.tiling].contiguous ? nullptr : p->wl[0][r.tiling].work_dev;
    A.perm = p->wl[0][r.tiling].contiguous ? nullptr : p->wl[0][r.tiling].perm_dev;
    A.out_cost = out_cost; A.out_grad = out_grad; A.cost = *cost;
    A.nom = p->nominal ? p->nom_dev : nullptr;
    if (A.nom && (r.fused || r.hchunks > 1)) {                 // (a plan handed in from outside: the nominal variants exist for the two-launch form only)
        gpmpc_set_error_text("gpmpc_rollout: plan without a nominal variant on a nominal pack");
        return GPMPC_E_STATE;
    }
    if (r.shared) {                                          // partial sums laid out [GP][tile]
        A.shared = 1; A.ust_inline = 1; A.work = nullptr; A.perm = nullptr;
        for (int a = 0; a <= p->ds; ++a) A.ust[a] = a * p->sh_tiles[r.sh_list];
    }

    PairArgs P;
    P.M = p->M; P.XT = p->XT; P.pp = A.pp; P.part = A.part; P.work = p->wl[0][r.tiling].work_dev;
    P.Np = p->Np; P.B = B; P.nunits = p->ds; P.nwork = r.nwork; P.pps = L.pps; P.nm = L.nm;
    P.jside_off = 0; P.ntri = p->ds; P.ns2 = p->ds; P.colsplit = (r.tiling == 1 || r.tiling == 3) ? 1 : 0;

    if (r.fused == 3) {
        PersistArgs Q;
        memset(&Q, 0, sizeof(Q));
        Q.XT = p->XT; Q.beta = p->beta; Q.lam = p->lam; Q.sf = p->sf; Q.M = p->M; Q.Np = p->Np;
        Q.x0 = x0; Q.U = U; Q.B = B; Q.H = H;
        Q.means = A.means; Q.vars = A.vars; Q.jac = A.jac;
        Q.gscr = (double*)(ws + L.off_G);
        const int T = p->Np / 64;
        Q.total = ((p->ds + r.png - 1) / r.png) * 32 * T * (T + 1);
        Q.ncol = p->ncol_dev;
        const int rc = timed_launch(GPMPC_TIME_FUSED, s, [&] { return launch_persist(p->D, grad, p->ds, r.pwaves, r.png, Q, s); });
        if (rc != GPMPC_OK) return rc;
        A.finished = 1;
    } else
    if (r.fused) {
        FusedArgs F;
        memset(&F, 0, sizeof(F));
        const gpmpc_worklist& wl = p->wl[0][r.tiling];
        const bool fsh = r.fused == 2 && r.shared;          // groups of GPs with one lambda per tile workgroup
        const gpmpc_worklist& wsh = gpmpc_fused_shared_list(p, r);
        F.XT = p->XT; F.beta = p->beta; F.lam = p->lam; F.sf = p->sf; F.M = p->M; F.work = fsh ? wsh.work_dev : wl.work_dev;
        const int nwg = r.nwork * r.fq;                     // partial sums per trajectory (= tile workgroups, except fsh: ds x tiles)
        F.Np = p->Np; F.nwork = nwg;
        F.ntile = fsh ? wsh.nwork : nwg; F.tiles = fsh ? p->sh_tiles[1] : 0;
        F.tri64 = (r.tiling == 1) ? 1 : 0;                  // 64x64 list: items decoded arithmetically (no dependent load)
        for (int a = 0; a <= p->ds; ++a) { F.ustart[a] = fsh ? a * p->sh_tiles[1] : wl.ustart_host[a] * r.fq; A.ust[a] = F.ustart[a]; }
        A.ust_inline = 1; A.nwork = nwg;
        F.x0 = x0; F.U = U; F.B = B; F.H = H;
        F.means = A.means; F.vars = A.vars; F.jac = A.jac;
        F.sp = A.sp; F.part = A.part; F.partz = (double*)(ws + L.off_partz);
        F.sps = L.sps; F.nm = L.nm;
        F.gscr = r.fused == 2 ? (double*)(ws + L.off_G) : nullptr;
        F.ncol = p->ncol_dev;
        // XCD-aware dispatch order (step_fused.h): measured against the natural order (tools/lib_ab.py, profiles/r05/ab19_xcdmap*.txt; N:ds:B
        // gain): 2048:4: B = 2 -1 %, 3 +2 %, 4 +4 %, 6 +8 %, 8 +6 %; 1024:4: 2 -2 %, 4 -2.5 / +2 %, 8 +4 %, 16 / 24 level; 512:3: 32 / 64 +3 / +2 %;
        // 300:4:32 +16 %; one lambda: 2048:4:8 +8 %, 1024:4:32 +14 %, 512:3:64 +14 %, 300:4:64 +10 %.  As a candidate of gpmpc_pack_autotune
        // (autotune_xcd_verbose*.txt) it is the best or within the run-to-run spread (~3 %) of the best on every shape of the grid, also on
        // SMALL grids (N = 300, ds = 2, B = 64 +21 %; N = 200, ds = 4, B = 64, one lambda +27 %): there the natural order puts the same
        // tiles of every trajectory -- the heavy 256-row ones -- on the same XCDs, the remapped order rotates the remainder.  From B = 2 (B = 2 itself is level:
        // N = 2048 0.579 | 0.580, N = 1024 0.283 | 0.284 ms; sub-batches of two gain: N = 2048, B = 4 as 2 x 2 0.925 | 0.911).
        F.xcdmap = r.xcdmap >= 0 ? (r.xcdmap && B > 1) : B >= 2;
        for (int t = 1; t <= H; ++t) {
            const int rc = timed_launch(GPMPC_TIME_FUSED, s, [&] { return launch_step_fused(p->D, grad, p->ds, r.fused == 2 ? (r.tiling == 2 ? 0 : wl.jt) : r.fq, fsh ? r.fng : 1, F, t, s); });
            if (rc != GPMPC_OK) return rc;
        }
        A.part += (size_t)(H & 1) * B * nwg * L.nm;          // the tail finishes step H from the parity the last launch wrote
    }
    for (int t = 1; t <= H && !r.fused; ++t) {
        switch (p->D) {
            case 1: launch_head<1>(A, t, s); break;
            case 2: launch_head<2>(A, t, s); break;
            case 3: launch_head<3>(A, t, s); break;
            case 4: launch_head<4>(A, t, s); break;
            case 5: launch_head<5>(A, t, s); break;
            case 6: launch_head<6>(A, t, s); break;
            case 7: launch_head<7>(A, t, s); break;
            case 8: launch_head<8>(A, t, s); break;
            default: return GPMPC_E_ARG;
        }
        int rc;
        if (lowprec) {
            rc = gpmpc_launch_pair_lowprec(p->D, lowprec, P, s);
        } else if (r.shared) {
            const gpmpc_worklist& wl = p->wl_sh[r.sh_list];
            PairSbsArgs Q;
            Q.M = p->M; Q.XT = p->XT; Q.pp = A.pp; Q.G = A.G; Q.part = A.part; Q.work = wl.work_dev;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = wl.nwork; Q.tiles = p->sh_tiles[r.sh_list]; Q.jt = wl.jt;
            Q.pps = L.pps; Q.nm = L.nm; Q.rgroup = r.rgroup;
            Q.first_step = (t == 1 && !p->tune.no_first && !full_first) ? 1 : 0;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_sbs(p->D, grad, p->sh_ng, p->ds, Q, s);
        } else if (r.sb) {
            PairSbArgs Q;
            Q.M = p->M; Q.XT = p->XT; Q.pp = A.pp; Q.G = A.G; Q.part = A.part; Q.work = P.work;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = r.nwork; Q.pps = L.pps; Q.nm = L.nm; Q.rgroup = r.rgroup;
            Q.first_step = (t == 1 && !p->tune.no_first && !full_first) ? 1 : 0;
            Q.colunroll = r.colunroll;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_sb(p->D, grad, r.tb, p->ds, r.waves, Q, s);
        } else {
            rc = gpmpc_timed_pair(p->D, true, grad, r.tb, P.colsplit ? 4 : r.waves, P, s);
        }
        if (rc != GPMPC_OK) return rc;
    }
    const size_t nzc = (size_t)2 * p->ds * (2 * p->ds + p->da);
    const size_t lds0 = sizeof(double) * ((size_t)(H + 1) * (1 + 2 * p->ds) + (size_t)H * p->da + (size_t)H);
    const size_t lds_all = lds0 + sizeof(double) * nzc * (grad ? H : 1), lds_one = lds0 + sizeof(double) * nzc;
    const bool allj = lds_all <= 48 * 1024;
    if (!allj && lds_one > 48 * 1024) return GPMPC_E_ARG;   // horizon too long for the tail kernel's LDS budget
    const size_t lds = allj ? lds_all : lds_one;
#define GPMPC_TAIL_CASE(DSV)                                                                             \
    case DSV:                                                                                            \
        if (A.nom) {                                                                                     \
            if (allj) hipLaunchKernelGGL((k_roll_tail<true, DSV, true>), dim3(B), dim3(256), lds, s, A);     \
            else hipLaunchKernelGGL((k_roll_tail<false, DSV, true>), dim3(B), dim3(256), lds, s, A);         \
        } else if (allj) hipLaunchKernelGGL((k_roll_tail<true, DSV, false>), dim3(B), dim3(256), lds, s, A); \
        else hipLaunchKernelGGL((k_roll_tail<false, DSV, false>), dim3(B), dim3(256), lds, s, A);        \
        break;
    switch (p->ds) {
        GPMPC_TAIL_CASE(1) GPMPC_TAIL_CASE(2) GPMPC_TAIL_CASE(3) GPMPC_TAIL_CASE(4)
        GPMPC_TAIL_CASE(5) GPMPC_TAIL_CASE(6) GPMPC_TAIL_CASE(7) GPMPC_TAIL_CASE(8)
        default: return GPMPC_E_ARG;
    }
#undef GPMPC_TAIL_CASE
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}


// Key of a captured rollout: everything the launch sequence depends on besides device memory contents.
struct gpmpc_graph_key {
    int B, H; unsigned flags;
    const void *x0, *U, *means, *vars, *cost_out, *grad, *ws; size_t ws_bytes;
    gpmpc_cost_params cost;
};
// A few captured rollouts per pack (least recently used is replaced): a caller alternating two shapes -- objective-only and
// objective+gradient calls, two horizons, two batch sizes -- replays both instead of re-capturing on every call.
#define GPMPC_GRAPH_SLOTS 4
struct gpmpc_graph_cache {
    hipStream_t stream; hipEvent_t ev_in, ev_out;
    hipStream_t aux[GPMPC_MAX_SPLIT - 1]; hipEvent_t ev_fork, ev_join[GPMPC_MAX_SPLIT - 1];     // parallel branches of a split capture
    hipGraphExec_t exec[GPMPC_GRAPH_SLOTS]; int valid[GPMPC_GRAPH_SLOTS]; unsigned long long used[GPMPC_GRAPH_SLOTS];
    gpmpc_graph_key key[GPMPC_GRAPH_SLOTS];
    unsigned long long tick; long long captures;
};

void gpmpc_graph_cache_free(void* c) {
    gpmpc_graph_cache* g = (gpmpc_graph_cache*)c;
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (int k = 0; k < GPMPC_GRAPH_SLOTS; ++k) if (g->exec[k]) (void)hipGraphExecDestroy(g->exec[k]);
    if (g->ev_in) (void)hipEventDestroy(g->ev_in);
    if (g->ev_out) (void)hipEventDestroy(g->ev_out);
    if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
    for (int k = 0; k < GPMPC_MAX_SPLIT - 1; ++k) {
        if (g->ev_join[k]) (void)hipEventDestroy(g->ev_join[k]);
        if (g->aux[k]) (void)hipStreamDestroy(g->aux[k]);
    }
    if (g->stream) (void)hipStreamDestroy(g->stream);
    free(g);
}

// The pack changed under its captured launch sequences -- gpmpc_pack_build found that the "every GP has the same lambda" property
// flipped, which selects other kernels --: drop the instantiated graphs, keep the streams, events and staging buffers.
// (gpmpc_pack_resize does NOT come here: no rollout kernel takes the unpadded size N as a launch ARGUMENT -- RollArgs / FusedArgs carry
// only the padded Np, structurally; the tile kernels clip their column loops at ceil(N / 8) * 8 columns (round 5), but read that count
// from device memory, `ncol`, which gpmpc_pack_build refreshes in stream order -- so replays stay valid on the refilled buffers.)
void gpmpc_graph_cache_invalidate(void* c) {
    gpmpc_graph_cache* g = (gpmpc_graph_cache*)c;
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (int k = 0; k < GPMPC_GRAPH_SLOTS; ++k) {
        if (g->exec[k]) { (void)hipGraphExecDestroy(g->exec[k]); g->exec[k] = nullptr; }
        g->valid[k] = 0;
    }
}

// number of graph captures this pack has done so far (tests: alternating shapes must not re-capture)
extern "C" long long gpmpc_pack_graph_captures(const gpmpc_pack* p) {
    const gpmpc_graph_cache* g = p ? (const gpmpc_graph_cache*)p->graph_cache : nullptr;
    return g ? g->captures : 0;
}

// Per-pack host lock (gpmpc_pack::lock, created with the pack).  It serialises, per pack, everything that touches the pack's OWN
// streams, events and caches: the lazy creation of graph_cache / cb_cache, a stream capture from hipStreamBeginCapture to
// hipStreamEndCapture (the auxiliary streams are in capture state meanwhile: a plain split launch of another host thread on them
// would be recorded into that capture instead of executing), the fork / join of a split launch, and the solver-callback entry.
// Calls that use only the caller's stream and workspace (unsplit plain launches) do not take it.
void* gpmpc_lock_create() { return new (std::nothrow) std::recursive_mutex(); }
void gpmpc_lock_destroy(void* l) { delete (std::recursive_mutex*)l; }
struct PackGuard {
    std::recursive_mutex* m;
    explicit PackGuard(const gpmpc_pack* p) : m((std::recursive_mutex*)p->lock) { if (m) m->lock(); }
    ~PackGuard() { if (m) m->unlock(); }
    PackGuard(const PackGuard&) = delete; PackGuard& operator=(const PackGuard&) = delete;
};

// The pack's private streams / events (graph replay and split launches), created on first use (under the pack's lock).
static int ensure_graph_cache(gpmpc_pack* p, gpmpc_graph_cache** out) {
    gpmpc_graph_cache* g = (gpmpc_graph_cache*)p->graph_cache;
    if (!g) {
        g = (gpmpc_graph_cache*)calloc(1, sizeof(gpmpc_graph_cache));
        if (!g) return GPMPC_E_ALLOC;
        hipError_t ec = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (ec == hipSuccess) ec = hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming);
        if (ec == hipSuccess) ec = hipEventCreateWithFlags(&g->ev_out, hipEventDisableTiming);
        if (ec == hipSuccess) ec = hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming);
        for (int k = 0; k < GPMPC_MAX_SPLIT - 1 && ec == hipSuccess; ++k) {
            ec = hipStreamCreateWithFlags(&g->aux[k], hipStreamNonBlocking);
            if (ec == hipSuccess) ec = hipEventCreateWithFlags(&g->ev_join[k], hipEventDisableTiming);
        }
        if (ec != hipSuccess) { gpmpc_set_error("graph cache: stream / event creation", ec); gpmpc_graph_cache_free(g); return GPMPC_E_LAUNCH; }
        p->graph_cache = g;
    }
    *out = g;
    return GPMPC_OK;
}

static size_t split_bytes(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad, int S) {
    RollSlice sl[GPMPC_MAX_SPLIT];
    return gpmpc_split_slices(p, r, B, H, grad, S, sl);
}

// One rollout call as S sub-batches: sub-batch 0 on `origin`, the others on the pack's auxiliary streams, forked from and
// joined back into `origin` with events (inside a stream capture these become parallel branches of the graph).  The
// caller holds the pack's lock (PackGuard): two host threads sharing a pack must not interleave their fork / join pairs.
static int enqueue_split(gpmpc_pack* p, gpmpc_graph_cache* g, int S, const RollShape& whole, hipStream_t origin, int B, int H,
                         const double* x0, const double* U, const gpmpc_cost_params* cost, unsigned flags, double* out_means,
                         double* out_vars, double* out_cost, double* out_grad, void* workspace) {
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    int rc = GPMPC_OK;
    hipError_t ef = hipEventRecord(g->ev_fork, origin);
    char* wsp = (char*)workspace;
    const int ds = p->ds, da = p->da;
    RollSlice sl[GPMPC_MAX_SPLIT];
    gpmpc_split_slices(p, whole, B, H, grad, S, sl);
    for (int k = S - 1; k >= 0 && rc == GPMPC_OK && ef == hipSuccess; --k) {
        const int b0 = sl[k].b0, b1 = sl[k].b1;
        hipStream_t sk = k == 0 ? origin : g->aux[k - 1];
        if (k > 0) ef = hipStreamWaitEvent(sk, g->ev_fork, 0);
        if (ef != hipSuccess) break;
        rc = enqueue_rollout(p, b1 - b0, H, x0 + (size_t)b0 * ds, U + (size_t)b0 * H * da, cost, flags,
                             out_means ? out_means + (size_t)b0 * (H + 1) * ds : nullptr,
                             out_vars ? out_vars + (size_t)b0 * (H + 1) * ds : nullptr, out_cost + b0,
                             out_grad ? out_grad + (size_t)b0 * H * da : nullptr, wsp + sl[k].ws_off, sl[k].lay.total, sk, nullptr, false, &whole);
        if (k > 0 && rc == GPMPC_OK) ef = hipEventRecord(g->ev_join[k - 1], sk);
    }
    for (int k = 1; k < S && ef == hipSuccess; ++k) ef = hipStreamWaitEvent(origin, g->ev_join[k - 1], 0);
    if (ef != hipSuccess && rc == GPMPC_OK) { gpmpc_set_error("split launch (fork / join)", ef); rc = GPMPC_E_LAUNCH; }
    if (rc != GPMPC_OK) {
        // a sub-batch failed to enqueue: what the others already enqueued on the auxiliary streams still reads the caller's
        // buffers and is not joined into the caller's stream -- drain it before the error is returned (a stream that is
        // being captured cannot be synchronised: ending the capture discards its work)
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(origin, &st) == hipSuccess && st == hipStreamCaptureStatusNone)
            for (int k = 0; k < S - 1; ++k) (void)hipStreamSynchronize(g->aux[k]);
    }
    return rc;
}

// Replay the launches of a rollout as ONE hipGraph on a stream owned by the pack (the caller's stream may be the
// legacy default stream, which cannot be captured); ordered against the caller's stream with two events.
static int graph_rollout(gpmpc_pack* p, int B, int H, const double* x0, const double* U, const gpmpc_cost_params* cost,
                         unsigned flags, double* out_means, double* out_vars, double* out_cost, double* out_grad,
                         void* workspace, size_t workspace_bytes, hipStream_t user) {
    PackGuard lock(p);                                      // cache creation, capture (begin ... end) and replay: one host thread at a time
    gpmpc_graph_cache* g = nullptr;
    if (int rcg = ensure_graph_cache(p, &g)) return rcg;
    gpmpc_graph_key k;
    memset(&k, 0, sizeof(k));
    k.B = B; k.H = H; k.flags = flags; k.x0 = x0; k.U = U; k.means = out_means; k.vars = out_vars; k.cost_out = out_cost;
    k.grad = out_grad; k.ws = workspace; k.ws_bytes = workspace_bytes; k.cost = *cost;
    int slot = -1, lru = 0;
    for (int q = 0; q < GPMPC_GRAPH_SLOTS; ++q) {
        if (g->valid[q] && memcmp(&k, &g->key[q], sizeof(k)) == 0) { slot = q; break; }
        if (!g->valid[q]) { if (g->valid[lru]) lru = q; }
        else if (g->valid[lru] && g->used[q] < g->used[lru]) lru = q;
    }
    if (slot < 0) {
        slot = lru;
        if (g->exec[slot]) {                               // its last replay may still be running
            (void)hipStreamSynchronize(g->stream);
            (void)hipGraphExecDestroy(g->exec[slot]); g->exec[slot] = nullptr;
        }
        g->valid[slot] = 0;
        hipGraph_t graph = nullptr;
        const bool grad = (flags & GPMPC_WANT_GRAD) != 0, lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
        const RollShape whole = gpmpc_choose_shape(p, B, H, grad, lowprec);
        const int S = gpmpc_split_count(p, whole, B, lowprec, false, 0, H, grad ? 1 : 0);
        if (S > 1 && split_bytes(p, whole, B, H, grad, S) > workspace_bytes) return GPMPC_E_WORKSPACE;
        GPMPC_HIP(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
        int rc = GPMPC_OK;
        if (S <= 1) {
            rc = enqueue_rollout(p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace,
                                 workspace_bytes, g->stream);
        } else {
            rc = enqueue_split(p, g, S, whole, g->stream, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace);
        }
        hipError_t e = hipStreamEndCapture(g->stream, &graph);
        if (rc != GPMPC_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { gpmpc_set_error("hipStreamEndCapture", e); return GPMPC_E_LAUNCH; }
        e = hipGraphInstantiate(&g->exec[slot], graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { gpmpc_set_error("hipGraphInstantiate", e); return GPMPC_E_LAUNCH; }
        g->key[slot] = k; g->valid[slot] = 1; ++g->captures;
    }
    g->used[slot] = ++g->tick;
    GPMPC_HIP(hipEventRecord(g->ev_in, user));
    GPMPC_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
    GPMPC_HIP(hipGraphLaunch(g->exec[slot], g->stream));
    GPMPC_HIP(hipEventRecord(g->ev_out, g->stream));
    GPMPC_HIP(hipStreamWaitEvent(user, g->ev_out, 0));
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// Solver callback: objective + gradient of ONE candidate, host in / host out (src/mpc.py:202-255)
// ---------------------------------------------------------------------------
// Everything between Ipopt's x and the (cost, gradient) it gets back is ONE hipGraph owned by the pack:
//   memcpy H2D [x0 | U] from pinned staging -> the H + 1 kernels of the rollout -> memcpy D2H [cost | grad] into pinned staging
// so that a callback costs the host one hipGraphLaunch and one stream synchronisation.
struct gpmpc_cb_cache {
    hipStream_t stream; hipEvent_t ev_in; hipGraphExec_t exec; int valid;
    int H; unsigned flags; gpmpc_cost_params cost;
    double* h_in;  double* h_out;      // pinned: [ds + H da] and [1 + H da]
    double* d_in;  double* d_out;      // device mirrors
    void* ws; size_t ws_bytes; int cap_H;
    long long captures;                // how often the callback graph was captured (gpmpc_pack_callback_captures)
};

void gpmpc_cb_cache_free(void* c) {
    gpmpc_cb_cache* g = (gpmpc_cb_cache*)c;
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->ev_in) (void)hipEventDestroy(g->ev_in);
    if (g->h_in) (void)hipHostFree(g->h_in);
    if (g->h_out) (void)hipHostFree(g->h_out);
    if (g->d_in) (void)hipFree(g->d_in);
    if (g->d_out) (void)hipFree(g->d_out);
    if (g->ws) (void)hipFree(g->ws);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    free(g);
}

void gpmpc_cb_cache_invalidate(void* c) {
    gpmpc_cb_cache* g = (gpmpc_cb_cache*)c;
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    g->valid = 0;
}

// number of captures of the callback graph this pack has done so far (tests: a refill of the pack with the padded size and the
// shared-lambda state unchanged -- every step of the windowed closed loop -- must not re-capture)
extern "C" long long gpmpc_pack_callback_captures(const gpmpc_pack* p) {
    const gpmpc_cb_cache* g = p ? (const gpmpc_cb_cache*)p->cb_cache : nullptr;
    return g ? g->captures : 0;
}

extern "C" int gpmpc_objective_gradient(gpmpc_pack* p, int H, const double* x0_host, const double* U_host,
                                        const gpmpc_cost_params* cost, unsigned flags, double* out_host, void* stream) {
    if (!p || !x0_host || !U_host || !cost || !out_host || H < 1) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    PackGuard lock(p);                                      // the entry owns per-pack staging buffers and is synchronous: one caller at a time
    // per-kernel events cannot be recorded inside a captured graph: with timing on the same work is enqueued uncaptured
    const bool eager = timing_on();
    GraphModeGuard mode(eager ? 0 : 1);
    flags &= GPMPC_WANT_GRAD;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    const int nin = p->ds + H * p->da, nout = 1 + (grad ? H * p->da : 0);
    gpmpc_cb_cache* g = (gpmpc_cb_cache*)p->cb_cache;
    if (!g) {
        g = (gpmpc_cb_cache*)calloc(1, sizeof(gpmpc_cb_cache));
        if (!g) return GPMPC_E_ALLOC;
        // published only when complete: a half-initialised cache (null stream) must never be found by a later call
        hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming);
        if (e != hipSuccess) { gpmpc_set_error("gpmpc_objective_gradient: stream / event creation", e); gpmpc_cb_cache_free(g); return GPMPC_E_LAUNCH; }
        p->cb_cache = g;
    }
    if (H > g->cap_H) {                                   // (re)allocate for the longer horizon
        (void)hipStreamSynchronize(g->stream);
        if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
        g->valid = 0;
        if (g->h_in) (void)hipHostFree(g->h_in);
        if (g->h_out) (void)hipHostFree(g->h_out);
        if (g->d_in) (void)hipFree(g->d_in);
        if (g->d_out) (void)hipFree(g->d_out);
        if (g->ws) (void)hipFree(g->ws);
        g->h_in = g->h_out = g->d_in = g->d_out = nullptr; g->ws = nullptr; g->cap_H = 0;
        const size_t bin = sizeof(double) * (p->ds + (size_t)H * p->da), bout = sizeof(double) * (1 + (size_t)H * p->da);
        hipError_t ea = hipHostMalloc((void**)&g->h_in, bin, hipHostMallocDefault);
        if (ea == hipSuccess) ea = hipHostMalloc((void**)&g->h_out, bout, hipHostMallocDefault);
        if (ea == hipSuccess) ea = hipMalloc((void**)&g->d_in, bin);
        if (ea == hipSuccess) ea = hipMalloc((void**)&g->d_out, bout);
        g->ws_bytes = gpmpc_rollout_workspace_bytes(p, 1, H, GPMPC_WANT_GRAD);
        if (ea == hipSuccess) ea = hipMalloc(&g->ws, g->ws_bytes);
        if (ea != hipSuccess) { gpmpc_set_error("gpmpc_objective_gradient: staging allocation", ea); return GPMPC_E_ALLOC; }   // cap_H stays 0: retried next call
        g->cap_H = H;
    }
    {   // the pack may have been refilled under a plan that needs more scratch (e.g. lambdas no longer shared: G rows per GP);
        // checked on EVERY call -- a plan is a few hundred host instructions -- so that neither the captured nor the timed
        // (uncaptured) path ever runs with a stale size
        const size_t need = gpmpc_rollout_workspace_bytes(p, 1, H, GPMPC_WANT_GRAD);
        if (need > g->ws_bytes) {
            (void)hipStreamSynchronize(g->stream);
            if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
            g->valid = 0;
            if (g->ws) (void)hipFree(g->ws);
            g->ws = nullptr; g->ws_bytes = 0;
            if (hipError_t ea = hipMalloc(&g->ws, need); ea != hipSuccess) { gpmpc_set_error("gpmpc_objective_gradient: workspace", ea); g->cap_H = 0; return GPMPC_E_ALLOC; }
            g->ws_bytes = need;
        }
    }
    if (eager) {                                          // timing on: upload, the H + 1 launches, download -- uncaptured
        memcpy(g->h_in, x0_host, sizeof(double) * p->ds);
        memcpy(g->h_in + p->ds, U_host, sizeof(double) * (size_t)H * p->da);
        GPMPC_HIP(hipEventRecord(g->ev_in, (hipStream_t)stream));
        GPMPC_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
        GPMPC_HIP(hipMemcpyAsync(g->d_in, g->h_in, sizeof(double) * nin, hipMemcpyHostToDevice, g->stream));
        const int rc = enqueue_rollout(p, 1, H, g->d_in, g->d_in + p->ds, cost, flags, nullptr, nullptr, g->d_out,
                                       grad ? g->d_out + 1 : nullptr, g->ws, g->ws_bytes, g->stream);
        if (rc != GPMPC_OK) return rc;
        GPMPC_HIP(hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, g->stream));
        GPMPC_HIP(hipStreamSynchronize(g->stream));
        memcpy(out_host, g->h_out, sizeof(double) * nout);
        return GPMPC_OK;
    }
    if (!g->valid || g->H != H || g->flags != flags || memcmp(&g->cost, cost, sizeof(*cost)) != 0) {
        (void)hipStreamSynchronize(g->stream);
        if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
        g->valid = 0;
        hipGraph_t graph = nullptr;
        GPMPC_HIP(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
        hipError_t e1 = hipMemcpyAsync(g->d_in, g->h_in, sizeof(double) * nin, hipMemcpyHostToDevice, g->stream);
        int rc = enqueue_rollout(p, 1, H, g->d_in, g->d_in + p->ds, cost, flags, nullptr, nullptr, g->d_out,
                                 grad ? g->d_out + 1 : nullptr, g->ws, g->ws_bytes, g->stream);
        hipError_t e2 = hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, g->stream);
        hipError_t e = hipStreamEndCapture(g->stream, &graph);
        if (rc != GPMPC_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e1 != hipSuccess || e2 != hipSuccess || e != hipSuccess) {
            gpmpc_set_error("gpmpc_objective_gradient capture", e != hipSuccess ? e : (e1 != hipSuccess ? e1 : e2));
            if (graph) (void)hipGraphDestroy(graph);
            return GPMPC_E_LAUNCH;
        }
        e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { gpmpc_set_error("hipGraphInstantiate", e); return GPMPC_E_LAUNCH; }
        g->H = H; g->flags = flags; g->cost = *cost; g->valid = 1; ++g->captures;
    }
    memcpy(g->h_in, x0_host, sizeof(double) * p->ds);
    memcpy(g->h_in + p->ds, U_host, sizeof(double) * (size_t)H * p->da);
    // ordered behind whatever the caller's stream did to the pack (build / append), then one launch and one wait
    GPMPC_HIP(hipEventRecord(g->ev_in, (hipStream_t)stream));
    GPMPC_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
    GPMPC_HIP(hipGraphLaunch(g->exec, g->stream));
    GPMPC_HIP(hipStreamSynchronize(g->stream));
    memcpy(out_host, g->h_out, sizeof(double) * nout);
    return GPMPC_OK;
}

extern "C" int gpmpc_rollout(const gpmpc_pack* p, int B, int H, const double* x0, const double* U,
                             const gpmpc_cost_params* cost, unsigned flags, double* out_means, double* out_vars,
                             double* out_cost, double* out_grad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !cost) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    GraphModeGuard mode(((flags & GPMPC_USE_GRAPH) && !timing_on()) ? 1 : 0);
    if ((flags & GPMPC_USE_GRAPH) && !timing_on() && p->built && x0 && U && out_cost && workspace && B >= 1 && H >= 1)
        return graph_rollout(const_cast<gpmpc_pack*>(p), B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad,
                             workspace, workspace_bytes, (hipStream_t)stream);
    if (p->built && x0 && U && out_cost && workspace && B >= 4 && H >= 1 && !(flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) &&
        (!(flags & GPMPC_WANT_GRAD) || out_grad)) {
        // mid-size batch launched plainly: the same split into concurrent sub-batches as under graph replay, on the pack's
        // auxiliary streams, forked from / joined into the caller's stream
        const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
        const RollShape whole = gpmpc_choose_shape(p, B, H, grad, false);
        const int S = gpmpc_split_count(p, whole, B, false, true, 0, H, grad ? 1 : 0);
        if (S > 1 && split_bytes(p, whole, B, H, grad, S) <= workspace_bytes) {
            PackGuard lock(p);                              // the pack's auxiliary streams / events (shared with graph_rollout's captures)
            gpmpc_graph_cache* g = nullptr;
            if (int rcg = ensure_graph_cache(const_cast<gpmpc_pack*>(p), &g)) return rcg;
            return enqueue_split(const_cast<gpmpc_pack*>(p), g, S, whole, (hipStream_t)stream, B, H, x0, U, cost, flags, out_means,
                                 out_vars, out_cost, out_grad, workspace);
        }
    }
    return enqueue_rollout(p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace,
                           workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
// Plan selection that measures: time the candidate plans of ONE call shape on this device and keep the winner
// ---------------------------------------------------------------------------

extern "C" int gpmpc_pack_autotune(gpmpc_pack* p, int B, int H, unsigned flags, char* report, size_t report_bytes) {
    if (!p || B < 1 || H < 1) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    PackGuard lock(p);
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, use_graph = (flags & GPMPC_USE_GRAPH) != 0;
    gpmpc_tuned_table* tab = (gpmpc_tuned_table*)p->tuned;
    if (!tab) { tab = (gpmpc_tuned_table*)calloc(1, sizeof(gpmpc_tuned_table)); if (!tab) return GPMPC_E_ALLOC; p->tuned = tab; }
    for (int k = 0; k < GPMPC_TUNED_SLOTS; ++k)                   // re-tuning a shape replaces its entry
        if (tab->e[k].valid && tab->e[k].B == B && tab->e[k].H == H && tab->e[k].grad == (grad ? 1 : 0) && tab->e[k].graph == (use_graph ? 1 : 0)) tab->e[k].valid = 0;
    // ---- candidates: the default plan, then the plans the GPMPC_* overrides would force, de-duplicated -------------------------
    struct Cand { RollShape r; int S; double ms; const char* why; };
    Cand cand[48]; int nc = 0;
    auto add = [&](const gpmpc_tuning& tn, int split, const char* why) {
        if (nc >= 48) return;
        const RollShape r = gpmpc_choose_shape(p, B, H, grad, false, &tn);
        int S = gpmpc_split_count(p, r, B, false, !use_graph, split);
        if (S > 1 && r.fused == 3) S = 1;
        for (int k = 0; k < nc; ++k) if (gpmpc_same_shape(cand[k].r, r) && cand[k].S == S) return;
        cand[nc].r = r; cand[nc].S = S; cand[nc].ms = 0.0; cand[nc].why = why; ++nc;
    };
    const gpmpc_tuning base = p->tune;
    add(base, 0, "default");
    { gpmpc_tuning t = base; t.fused_sb = 0; add(t, 0, "fused_sb=0"); }
    { gpmpc_tuning t = base; t.fused_sb = 1; add(t, 0, "fused_sb=1"); }
    for (int tl : {0, 2, 4, 5, 6}) { gpmpc_tuning t = base; t.tiling = tl; add(t, 0, "tiling"); t.fused_sb = 1; add(t, 0, "tiling+fused_sb=1"); t.fused_sb = 0; add(t, 0, "tiling+fused_sb=0"); }
    for (int xm : {0, 1}) {                                      // (the one-launch forms with the other dispatch order)
        gpmpc_tuning t = base; t.xcdmap = xm; t.persist = 0; add(t, 0, xm ? "xcdmap=1" : "xcdmap=0");
        for (int tl : {2, 5, 6}) { gpmpc_tuning u = t; u.tiling = tl; u.fused_sb = 1; add(u, 0, xm ? "tiling+xcdmap=1" : "tiling+xcdmap=0"); }
    }
    { gpmpc_tuning t = base; t.persist = 16; add(t, 0, "persist=16"); t.persist = 8; add(t, 0, "persist=8"); t.persist = 0; add(t, 0, "persist=0"); }
    { gpmpc_tuning t = base; t.pair_sb = 0; t.persist = 0; add(t, 0, "pair_sb=0"); t.fused = 0; add(t, 0, "pair_sb=0,fused=0"); }
    { gpmpc_tuning t = base; t.fused = 0; t.persist = 0; add(t, 0, "fused=0"); }
    if (p->shared_lambda) { gpmpc_tuning t = base; t.shared = 0; t.persist = 0; add(t, 0, "shared=0"); }
    for (int sp : {1, 2, 4}) { gpmpc_tuning t = base; t.persist = 0; add(t, sp, "split"); }
    // ---- scratch: inputs (zeros: a valid problem), outputs, the largest workspace --------------------------------------------
    size_t wsb = 0;
    for (int k = 0; k < nc; ++k) {
        size_t need = gpmpc_layout_for(p, cand[k].r, B, H, grad).total;
        if (cand[k].S > 1) { const size_t sb = split_bytes(p, cand[k].r, B, H, grad, cand[k].S); if (sb > need) need = sb; }
        if (need > wsb) wsb = need;
    }
    const size_t nU = (size_t)B * H * p->da, nx = (size_t)B * p->ds;
    double *x0 = nullptr, *U = nullptr, *oc = nullptr, *og = nullptr; void* ws = nullptr;
    hipError_t e = hipMalloc((void**)&x0, sizeof(double) * nx);
    if (e == hipSuccess) e = hipMalloc((void**)&U, sizeof(double) * (nU ? nU : 1));
    if (e == hipSuccess) e = hipMalloc((void**)&oc, sizeof(double) * B);
    if (e == hipSuccess) e = hipMalloc((void**)&og, sizeof(double) * (nU ? nU : 1));
    if (e == hipSuccess) e = hipMalloc(&ws, wsb);
    hipStream_t st = nullptr; hipEvent_t ea = nullptr, eb = nullptr;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ea);
    if (e == hipSuccess) e = hipEventCreate(&eb);
    if (e == hipSuccess) e = hipMemsetAsync(x0, 0, sizeof(double) * nx, st);
    if (e == hipSuccess) e = hipMemsetAsync(U, 0, sizeof(double) * (nU ? nU : 1), st);
    gpmpc_graph_cache* gc = nullptr;
    int rc = e == hipSuccess ? ensure_graph_cache(p, &gc) : GPMPC_E_ALLOC;
    gpmpc_cost_params cost;
    memset(&cost, 0, sizeof(cost));
    cost.gamma = 0.0;
    for (int k = 0; k < p->ds; ++k) cost.Q[k * p->ds + k] = 1.0;
    for (int k = 0; k < p->da; ++k) cost.R[k * p->da + k] = 0.01;
    const unsigned fl = grad ? GPMPC_WANT_GRAD : 0;
    hipGraphExec_t execs[48] = {};
    const bool trace = getenv("GPMPC_AUTOTUNE_TRACE") != nullptr;      // diagnostic: names every candidate on stderr before it runs
    const bool was_timing = timing_on();
    if (was_timing) gpmpc_timing_enable(0);                   // per-kernel events cannot be recorded inside the captures below
    // ---- time every candidate: one captured graph (or the plain launches), one warm-up, then replays for >= ~2 ms or 3 times ----
    for (int pass = 0; pass < 2; ++pass)                          // two passes, the better time of each candidate: the first launches of a
    for (int kk = 0; kk <= nc && rc == GPMPC_OK; ++kk) {          // process (code upload, cold caches) must not be charged to the default plan
        // (the default plan is timed AGAIN at the end of each pass: measured first only, it came out 4 ... 8 % behind candidates that
        // launch exactly the same kernels -- profiles/r05/autotune_grid_mid.txt, N = 2048, B = 6 / 8 --, whatever the position effect is)
        const int k = kk == nc ? 0 : kk;
        if ((pass == 1 || kk == nc) && cand[k].ms < 0.0) continue;              // failed to enqueue before
        const Cand& c = cand[k];
        if (trace) fprintf(stderr, "[autotune] pass %d candidate %d (%s): fused=%d tiling=%d sb=%d tb=%d shared=%d pwaves=%d colunroll=%d split=%d\n", pass, k, c.why,
                           c.r.fused, c.r.tiling, c.r.sb, c.r.tb, c.r.shared, c.r.pwaves, c.r.colunroll, c.S);
        auto enqueue = [&](hipStream_t s) {
            return c.S <= 1 ? enqueue_rollout(p, B, H, x0, U, &cost, fl, nullptr, nullptr, oc, og, ws, wsb, s, nullptr, false, &c.r)
                            : enqueue_split(p, gc, c.S, c.r, s, B, H, x0, U, &cost, fl, nullptr, nullptr, oc, og, ws);
        };
        // One captured graph per candidate, kept for both passes and destroyed together after the last replay: capturing, instantiating
        // and destroying ~25 graphs (some with two or four parallel branches) back to back crashed intermittently inside
        // hipGraphLaunch (native backtrace: the replay of the re-captured default plan in pass 1; 1 run in ~10, round 4).
        hipGraphExec_t& exec = execs[k];
        if (use_graph && !exec) {
            // (every candidate also runs once as plain launches before it is captured: warm caches, and nothing is launched for the
            // first time in the process inside a capture)
            if (pass == 0) {
                const int r0 = enqueue(st);
                if (r0 != GPMPC_OK || hipStreamSynchronize(st) != hipSuccess) { cand[k].ms = -1.0; continue; }
            }
            hipGraph_t graph = nullptr;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { rc = GPMPC_E_LAUNCH; break; }
            const int r1 = enqueue(st);
            const hipError_t e1 = hipStreamEndCapture(st, &graph);
            if (r1 != GPMPC_OK || e1 != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); cand[k].ms = -1.0; continue; }
            const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e2 != hipSuccess) { cand[k].ms = -1.0; continue; }
        }
        auto run = [&]() { return use_graph ? (hipGraphLaunch(exec, st) == hipSuccess ? GPMPC_OK : GPMPC_E_LAUNCH) : enqueue(st); };
        int r2 = run();
        if (r2 == GPMPC_OK && hipStreamSynchronize(st) != hipSuccess) r2 = GPMPC_E_LAUNCH;
        double best = -1.0;
        for (int rep = 0; rep < 3 && r2 == GPMPC_OK; ++rep) {     // best of three blocks
            int n = 1;
            (void)hipEventRecord(ea, st);
            r2 = run();
            (void)hipEventRecord(eb, st);
            if (hipEventSynchronize(eb) != hipSuccess) { r2 = GPMPC_E_LAUNCH; break; }
            float ms1 = 0.f; (void)hipEventElapsedTime(&ms1, ea, eb);
            if (ms1 < 0.7f) {                                     // short call: a block of replays instead of one
                n = ms1 > 0.f ? (int)(2.0f / ms1) + 1 : 20; if (n > 200) n = 200;
                (void)hipEventRecord(ea, st);
                for (int q = 0; q < n && r2 == GPMPC_OK; ++q) r2 = run();
                (void)hipEventRecord(eb, st);
                if (hipEventSynchronize(eb) != hipSuccess) { r2 = GPMPC_E_LAUNCH; break; }
                (void)hipEventElapsedTime(&ms1, ea, eb);
            }
            const double per = (double)ms1 / n;
            if (best < 0.0 || per < best) best = per;
        }
        if (r2 != GPMPC_OK) cand[k].ms = -1.0;
        else if ((pass == 0 && kk < nc) || best < cand[k].ms) cand[k].ms = best;
    }
    (void)hipStreamSynchronize(st);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < nc; ++k) if (execs[k]) (void)hipGraphExecDestroy(execs[k]);
    if (was_timing) gpmpc_timing_enable(1);
    int win = -1;
    for (int k = 0; k < nc; ++k) if (cand[k].ms > 0.0 && (win < 0 || cand[k].ms < cand[win].ms)) win = k;
    // the default keeps its place unless a candidate beats it by more than the noise of this measurement (2 %)
    if (win > 0 && cand[0].ms > 0.0 && cand[win].ms > 0.98 * cand[0].ms) win = 0;
    if (rc == GPMPC_OK && win >= 0) {
        gpmpc_tuned_entry& te = tab->e[tab->next % GPMPC_TUNED_SLOTS];
        tab->next = (tab->next + 1) % GPMPC_TUNED_SLOTS;
        te.B = B; te.H = H; te.grad = grad ? 1 : 0; te.graph = use_graph ? 1 : 0; te.S = cand[win].S; te.shape = cand[win].r;
        te.ms_default = cand[0].ms; te.ms_best = cand[win].ms; te.valid = 1;
        gpmpc_graph_cache_invalidate(p->graph_cache);           // captured under the plan the thresholds chose
        gpmpc_cb_cache_invalidate(p->cb_cache);
    }
    if (report && report_bytes > 0) {
        size_t off = 0;
        report[0] = 0;
        for (int k = 0; k < nc && off + 96 < report_bytes; ++k)
            off += snprintf(report + off, report_bytes - off, "%s%s%s:fused=%d,tiling=%d,sb=%d,tb=%d,shared=%d,pwaves=%d,xcdmap=%d,split=%d:%.5f",
                            k ? ";" : "", k == win ? "*" : "", cand[k].why, cand[k].r.fused, cand[k].r.tiling, cand[k].r.sb, cand[k].r.tb, cand[k].r.shared,
                            cand[k].r.pwaves, cand[k].r.xcdmap, cand[k].S, cand[k].ms);
    }
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (st) (void)hipStreamDestroy(st);
    if (x0) (void)hipFree(x0);
    if (U) (void)hipFree(U);
    if (oc) (void)hipFree(oc);
    if (og) (void)hipFree(og);
    if (ws) (void)hipFree(ws);
    if (e != hipSuccess) { gpmpc_set_error("gpmpc_pack_autotune: scratch", e); return GPMPC_E_ALLOC; }
    if (rc != GPMPC_OK) return rc;
    return win < 0 ? GPMPC_E_LAUNCH : nc;
}

extern "C" int gpmpc_pack_autotune_clear(gpmpc_pack* p) {
    if (!p) return GPMPC_E_ARG;
    PackGuard lock(p);
    gpmpc_tuned_clear(p->tuned);
    gpmpc_graph_cache_invalidate(p->graph_cache);
    gpmpc_cb_cache_invalidate(p->cb_cache);
    return GPMPC_OK;
}

extern "C" int gpmpc_cost_grad(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* means,
                               const double* covs, const double* U, double* out_cost, double* d_means, double* d_covs,
                               double* d_U, void* stream) {
    if (!cost || !means || !covs || !U || !out_cost || B < 1 || H < 1 || ds < 1 || ds > GPMPC_MAX_DS || da < 0 ||
        da > GPMPC_MAX_D)
        return GPMPC_E_ARG;
    const int ng = (d_means != nullptr) + (d_covs != nullptr) + (d_U != nullptr);
    if (ng != 0 && ng != 3) return GPMPC_E_ARG;            // all three derivative outputs or none
    hipLaunchKernelGGL(k_cost_full, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, H, ds, da, *cost, means,
                       covs, U, out_cost, d_means, d_covs, d_U);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_cost(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* means,
                          const double* covs, const double* U, double* out_cost, void* stream) {
    return gpmpc_cost_grad(B, H, ds, da, cost, means, covs, U, out_cost, nullptr, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------------------
// Differentiable propagation: trajectory + step Jacobians, and their vector-Jacobian product
// ---------------------------------------------------------------------------
static inline size_t jac_scratch_bytes(const gpmpc_pack* p, int B, int H) {     // [cost | grad] of the (zero-cost) tail kernel
    return (sizeof(double) * (size_t)B * (1 + (size_t)H * p->da) + 255) & ~(size_t)255;
}
extern "C" size_t gpmpc_rollout_jac_workspace_bytes(const gpmpc_pack* p, int B, int H) {
    if (!p || B < 1 || H < 1) return 0;
    return gpmpc_rollout_workspace_bytes(p, B, H, GPMPC_WANT_GRAD) + jac_scratch_bytes(p, B, H);
}

extern "C" int gpmpc_rollout_jac(const gpmpc_pack* p, int B, int H, const double* x0, const double* U, double* out_means,
                                 double* out_vars, double* out_jac, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !x0 || !U || !out_means || !out_vars || !out_jac || !workspace || B < 1 || H < 1) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    const size_t base = gpmpc_rollout_workspace_bytes(p, B, H, GPMPC_WANT_GRAD), extra = jac_scratch_bytes(p, B, H);
    if (workspace_bytes < base + extra) return GPMPC_E_WORKSPACE;
    gpmpc_cost_params zero;                                 // propagation only: a zero cost keeps the tail kernel trivial
    memset(&zero, 0, sizeof(zero));
    double* scratch = (double*)((char*)workspace + base);
    return enqueue_rollout(p, B, H, x0, U, &zero, GPMPC_WANT_GRAD, out_means, out_vars, scratch, scratch + B, workspace, base,
                           stream, out_jac, true);
}

extern "C" int gpmpc_rollout_vjp(int B, int H, int ds, int da, const double* jac, const double* g_means,
                                 const double* g_vars, double* out_gU, double* out_gx0, void* stream) {
    if (!jac || !out_gU || B < 1 || H < 1 || ds < 1 || ds > GPMPC_MAX_DS || da < 1 || da > GPMPC_MAX_D || 2 * ds + da > 64)
        return GPMPC_E_ARG;
    hipLaunchKernelGGL(k_rollout_vjp, dim3(B), dim3(64), 0, (hipStream_t)stream, B, H, ds, da, jac, g_means, g_vars, out_gU,
                       out_gx0);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// Rollout + state chance constraints in one device pass (kernel: constraints.hip)
// ---------------------------------------------------------------------------
static int constrained_flags_ok(unsigned flags) {
    if (flags & ~GPMPC_WANT_GRAD) {
        gpmpc_set_error_text("gpmpc_rollout_constrained: only GPMPC_WANT_GRAD is accepted (no GPMPC_USE_GRAPH, no GPMPC_FP32_* mode in this version)");
        return 0;
    }
    return 1;
}

extern "C" size_t gpmpc_rollout_constrained_workspace_bytes(const gpmpc_pack* p, int B, int H, unsigned flags) {
    if (!p || B < 1 || H < 1 || !constrained_flags_ok(flags)) return 0;
    return gpmpc_rollout_workspace_bytes(p, B, H, flags);   // the step Jacobians, means and variances live in the rollout's own workspace
}

extern "C" int gpmpc_rollout_constrained(const gpmpc_pack* p, int B, int H, const double* x0, const double* U,
                                         const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags,
                                         double* out_means, double* out_vars, double* out_cost, double* out_grad, double* out_g,
                                         double* out_gjac, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !x0 || !U || !cost || !cons || !out_cost || !out_g || !workspace || B < 1 || H < 1) return GPMPC_E_ARG;
    if (!constrained_flags_ok(flags)) return GPMPC_E_ARG;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    if (grad && (!out_grad || !out_gjac)) return GPMPC_E_ARG;
    if (int rc = gpmpc_check_constraints(cons, "gpmpc_rollout_constrained")) return rc;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    if (!p->built) return GPMPC_E_STATE;
    GraphModeGuard mode(0);
    // the layout enqueue_rollout takes for this call: where it keeps J_t, means, variances
    const RollLayout L = gpmpc_layout_for(p, gpmpc_choose_shape(p, B, H, grad, false), B, H, grad);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    if (int rc = enqueue_rollout(p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace, workspace_bytes, stream))
        return rc;
    char* ws = (char*)workspace;
    return gpmpc_rollout_constraints(B, H, p->ds, p->da, cons, out_means ? out_means : (const double*)(ws + L.off_means),
                                     out_vars ? out_vars : (const double*)(ws + L.off_vars),
                                     grad ? (const double*)(ws + L.off_jac) : nullptr, out_g, grad ? out_gjac : nullptr, stream);
}
