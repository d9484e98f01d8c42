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
__host__ __device__ static inline int sps_of(int D) { return 3 + 4 * D; }
// Linear nominal model m_a(z) = n_a . z + c_a (GP a learns the residual): the step's moments become
//   mu' = mu_g + n . u + c,   var' = var_g + sum_k n_k^2 s_k + 2 sum_k w_k dmu_g/du_k,   w_k = n_k s_k   (Cov[z, g(z)] = S E[grad g])
// and, with q_i = sum_k w_k B_k v_ik, E1_l = sum_i p_i q_i v_il, E2_l = sum_i p_i q_i v_il^2, M1_l = sum_i p_i v_il, X = 2 sum_k w_k dmu_g/du_k:
//   dmu'/du_l = dmu_g/du_l + n_l,   dmu'/ds_l = dmu_g/ds_l
//   dvar'/du_l = dvar_g/du_l + 2 (c_m B_l E1_l - w_l B_l mu_g)
//   dvar'/ds_l = dvar_g/ds_l + n_l^2 + 2 n_l dmu_g/du_l - 1/2 B_l X + B_l^2 c_m (2 w_l M1_l - E2_l)          (state inputs l only)
// prep_step forms these ADDENDS once per (trajectory, GP) and leaves them behind the plain entries of sp; finish_step -- in every workgroup
// of the trajectory -- adds the same stored values in the same order.  Layout of the extension, from sps_of(D):
//   0 n . u + c | 1 addend of var | 2 addend of dvar/du [D] | 2+D addend of dvar/ds [D] | 2+2D n [D]        (the [D] blocks with the gradient only)
// The nominal variants run without row chunks (plan_rollout).
__host__ __device__ static inline int sps_nominal(int D) { return sps_of(D) + 2 + 3 * D; }

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

#define GPMPC_PERSIST_MAXNP_HOST 1024
struct RollPlan { int tiling, tb, waves, nwork, nm, pps, sps, sb, gw, rgroup, fused, fq, hchunks, hrows, shared, sh_list, colunroll /* columns per iteration of the sb kernel */, fng /* GPs per tile workgroup of the one-launch form with one lambda */, pwaves /* waves per workgroup of the whole-horizon kernel (fused = 3) */, xcdmap /* one-launch form, several trajectories: XCD-aware dispatch order 0 | 1 | -1 by the size of the launch */, png /* GPs per unit there: 1, or 2 with one lambda for all GPs */; size_t off_mpart; size_t off_G; size_t off_pp, off_sp, off_part, off_partz, off_jac, off_means, off_vars, total; };

// shape (optional): take every SHAPE decision (tiling, kernel, trajectories per wave, row chunks ...) from this plan of a larger
// batch and only size the buffers for B: the sub-batches of a split call then run exactly the launches the whole batch would,
// so their results are bit-identical to the unsplit call.
// Plans MEASURED for this pack (gpmpc_pack_autotune): a call shape found here takes its kernel form from the table instead of
// from the thresholds below.  Owned by the pack (gpmpc_pack::tuned), written only by gpmpc_pack_autotune.
#define GPMPC_TUNED_SLOTS 16
struct gpmpc_tuned_entry { int B, H, grad, graph, S, valid; RollPlan plan; double ms_default, ms_best; };
struct gpmpc_tuned_table { gpmpc_tuned_entry e[GPMPC_TUNED_SLOTS]; int next; };
// How the calling entry point will launch (captured graph replay = 1, plain launches = 0, unknown = -1): a plan and split count
// measured as graph replays -- launch overhead hidden, up to four parallel branches -- must not be applied to eager calls of the same
// shape, nor the reverse.  Set by the entry points for the duration of their planning (thread-local: the library is re-entrant).
static thread_local int tl_graph_mode = -1;
struct GraphModeGuard {
    int prev;
    explicit GraphModeGuard(int m) : prev(tl_graph_mode) { tl_graph_mode = m; }
    ~GraphModeGuard() { tl_graph_mode = prev; }
};
static const gpmpc_tuned_entry* tuned_lookup(const gpmpc_pack* p, int B, int H, bool grad) {
    const gpmpc_tuned_table* t = (const gpmpc_tuned_table*)p->tuned;
    if (!t) return nullptr;
    for (int k = 0; k < GPMPC_TUNED_SLOTS; ++k)
        if (t->e[k].valid && t->e[k].B == B && t->e[k].H == H && t->e[k].grad == (grad ? 1 : 0) &&
            (tl_graph_mode < 0 || t->e[k].graph == tl_graph_mode)) return &t->e[k];
    return nullptr;
}
void gpmpc_tuned_free(void* t) { free(t); }
void gpmpc_tuned_clear(void* t) { if (t) memset(t, 0, sizeof(gpmpc_tuned_table)); }      // plans measured under another kernel selection (lambdas no longer shared, new GPMPC_* overrides)

// tn_over (optional): GPMPC_* overrides to plan under instead of the pack's (gpmpc_pack_autotune enumerates candidates with it).
static void plan_rollout(const gpmpc_pack* p, int B, int H, bool grad, bool diag, RollPlan* r, bool lowprec = false,
                         const RollPlan* shape = nullptr, const gpmpc_tuning* tn_over = nullptr) {
    const int D = p->D;
    if (!shape && !tn_over && !lowprec && diag)                 // a measured plan for this call shape
        if (const gpmpc_tuned_entry* te = tuned_lookup(p, B, H, grad)) shape = &te->plan;
    // A pack with a linear nominal model is planned as under GPMPC_FUSED=0 GPMPC_FUSED_SB=0 GPMPC_PERSIST=0, whatever the overrides say:
    // only the head / tail kernels of this file know the model (step_fused.h and traj_persist.h keep their own finish code), and their
    // nominal variants run without row chunks (the extra sums E1, E2 are not carried through mpart).
    gpmpc_tuning tn_nom;
    if (p->nominal) { tn_nom = tn_over ? *tn_over : p->tune; tn_nom.fused = 0; tn_nom.fused_sb = 0; tn_nom.persist = 0; tn_nom.hchunks = 1; }
    const gpmpc_tuning& tn = p->nominal ? tn_nom : (tn_over ? *tn_over : p->tune);        // GPMPC_* overrides, read once at pack creation
    // The selection as it stands (diagonal rollout, da <= 2; every threshold is a measured crossover -- its numbers are in the
    // comment at its line, the method in DESIGN.md section 5, the maps in profiles/r02 and r03/batch_size_map.txt):
    //   W64 = B x tiles(256x64) < ~150 (~400 for N < 512), or N < 256           ONE launch per step, 64-row tiles, staged column loop
    //                                                                           (step_fused.h, Q = 1 | 4; the B = 1 solver callbacks)
    //   up to W64 ~4700 (~7000: <= 200 tiles per trajectory, or one lambda),    ONE launch per step, 256x16 / 32 / 64 tiles by the size of the launch,
    //   256 <= N <= ~4300                                                       scalar-broadcast column loop (step_fused.h, Q = 16 / 32 / 0; groups of GPs
    //                                                                           per tile workgroup with one lambda), two concurrent sub-batches
    //   W64 beyond, until a wide tiling fills the chip                          head kernel + pair_kernel_sb.h on 256x64 tiles, one trajectory per
    //                                                                           wave (pair_kernel_sbs.h with one lambda), 2-4 concurrent sub-batches
    //   ceil(B/2) x tiles(256x128) >= 2800, N > 512, D <= 5                     head + pair_kernel_sb.h on 256x128 tiles, two trajectories per wave
    //   ceil(B/2) x tiles(256x256) >= 2800 (1100 for N <= 512); D >= 6:         head + pair_kernel_sb.h on 256x256 tiles (the big batches: C3, C4);
    //   B x tiles(256x256) >= 1500; one lambda: B x tiles >= 1700               XCD-aware dispatch, rgroup 4
    //   full covariance / da > 2 / the fp32 sweep modes                         staged pair_kernel.h (fullcov.hip has its own plan)
    const bool sb_ok = diag && p->da <= 2;
    // 256x256 tiles once they give enough workgroups (profiles/r02/batch_size_map.txt): with two trajectories per wave
    // (D <= 5) from ~2800 on -- N = 2048: B = 32 5.28 k rollouts/s vs 5.45 k on 256x64, B = 48 equal, B = 64 6.02 k vs 5.76 k;
    // N = 1024: B = 96 18.5 k vs 19.2 k, B = 128 20.5 k vs 20.0 k --, with one per wave (D >= 6) from ~1500 on -- N = 4096, ds = 6:
    // ahead at every batch size from B = 2 (295 vs 282 rollouts/s) on.
    const bool tb2 = D <= 5 && B >= 2;
    const long wg0 = (long)(tb2 ? (B + 1) / 2 : B) * p->wl[0][0].nwork;
    // Small training sets (Np <= 512: at most 3 tiles per GP) switch earlier, from ~1100 workgroups: their 256x64 workgroups
    // run 64 columns on at most 4 waves behind a full prologue (N = 512, ds = 3, B = 256: 2.82 vs 3.20 ms per batch of 20 steps;
    // N = 300, ds = 2, B = 512: 0.88 vs 1.04 ms; N = 100, B = 2048: 1.30 vs 1.44 ms; below 1100 the 256x64 shape stays ahead).
    const long thr2 = p->Np <= 512 ? 1100 : 2800;
    const bool big = sb_ok ? wg0 >= (tb2 ? thr2 : 1500) : (long)((B + 1) / 2) * p->wl[0][0].nwork >= 1024;
    // (round 2: 2048 instead of 1024 work items -- below that the one-launch-per-step kernel of step_fused.h wins: N = 2048,
    // B = 2: 1.03 vs 1.19 ms per rollout; N = 1536, B = 4: 1.07 vs 1.23; N = 1024, B = 4: 0.67 vs 1.01)
    // (1700 since the head kernel is split over row chunks: N = 2048, B = 3: 1.16 vs 1.33 ms; N = 1536, B = 6: 1.31 vs 1.40)
    // (round 3, with four columns in flight and concurrent sub-batches on the 256x64 path: from 1250 work items for N >= 1024 --
    // N = 1024, B = 8 / 10: 0.92 vs 0.99 / 1.00 vs 1.18 ms; smaller training sets stay at 1700: N = 600, B = 16 0.89 vs 0.86 ms,
    // N = 400, B = 64 0.43 vs 0.38 ms -- profiles/r03/ab_fused_vs_sb_threshold.txt)
    // ... and, where the one-launch-per-step form on these tiles can run (step_fused.h, Q = 0: see r->fused below), from ~400 tile
    // workgroups: against the 64-row fused form N = 2048, B = 1 / 2 x1.19 / 1.43; N = 1024, B = 2 / 3 / 4 / 6 x1.06 / 1.24 / 1.19 / 1.34;
    // N = 512, ds = 3, B = 8 / 12 / 16 / 32 x1.01 / 1.16 / 1.19 / 1.38; N = 300, ds = 2, B = 32 / 64 x1.02 / 1.15; below ~300 workgroups
    // it loses (N = 1024, B = 1 x0.92; N = 512, B = 4 x0.77), and so do training sets of less than one row tile (N = 128, B = 128 x0.89)
    const long wg2 = (long)B * p->wl[0][2].nwork;
    const bool shared_on = p->shared_lambda && tn.shared != 0 && p->sh_ng >= 2;
    const bool fsb_can = sb_ok && !lowprec && p->da >= 1 && tn.fused_sb != 0 && (p->Np >= 256 || tn.fused_sb == 1) &&
                         p->wl[0][2].nwork <= 600 * p->ds;           // (N <= ~4300; measured up to N = 4096: B = 1 / 2 x1.22 / 1.18 at ds = 4, level at ds = 6)
    // ... and with NARROWER tiles (256x32, 256x16: work lists 5, 6) further down for training sets of at least two row tiles: a launch
    // of a few hundred 256x64 workgroups leaves most of the chip empty while each workgroup walks its 64 columns one L2 round trip
    // at a time (N = 2048, B = 1: 24.5 us per launch on 576 workgroups, profiles/r03/kernel_stats_C3_B1.csv); half / quarter tiles
    // give 2x / 4x the workgroups, each living half / a quarter as long (profiles/r03/ab_fused_sb_narrow_tiles.txt, ms per rollout
    // on 64 / 32 / 16 columns: N = 1024, B = 1 0.359 / 0.300 / 0.270 (64-row form 0.330), B = 2 0.409 / 0.359 / 0.359, B = 4
    // 0.561 / 0.484 / 0.514, B = 8 0.673 / 0.661 / 0.825; N = 1536, ds = 3, B = 1 0.391 / 0.330 / 0.308, B = 2 0.503 / 0.417 / 0.502;
    // N = 512, ds = 3, B = 8 0.434 / 0.357 / 0.325, B = 16 0.481 / 0.396 / 0.407; N = 2048, B = 1 0.554 / 0.539 / 0.679 -- every tile
    // workgroup re-reduces its trajectory's partial sums, 2304 of them there on 16 columns; N <= 448: the 64-row form stays ahead
    // until ~400 workgroups, N = 400, ds = 2, B = 16 0.179 vs 0.200 / 0.190)
    const bool narrow_ok = fsb_can && p->Np >= 512;
    const bool mid = !big && sb_ok && (wg2 >= (p->Np >= 1024 ? 1250 : 1700) || (fsb_can && wg2 >= (narrow_ok ? 150 : 400)));
    // 256x128 tiles with two trajectories per wave where they already give the workgroups the 256x256 tiles do not yet
    // (profiles/r03/ab_tiling_256x128.txt: N = 2048, B = 24 / 32 4.02 / 5.07 vs 4.78 / 6.12 ms on 256x64; N = 1024, B = 96 / 128
    // 4.51 / 5.71 vs 4.98 / 6.49 ms; from there on 256x256 is 3-4 % ahead)
    // (re-measured against the plan as it stood at the end of round 3, whose mid-size forms had moved: ahead from ~1600 of its own
    // workgroups -- N = 2048, B = 12 / 14 / 16 / 18 x1.00 / 1.05 / 1.10 / 1.05; N = 1024, B = 44 / 48 / 56 / 64 x1.01 / 1.05 / 1.07 / 1.11;
    // N = 1536, ds = 3, B = 24 / 32 x1.07 / 1.14; N = 2048, B = 10 x0.96)
    // ... but only beyond the reach of the one-launch form, which is ahead of it wherever both apply (N = 1024, B = 40 2.27 vs 2.57 ms;
    // N = 768, B = 72 2.35 vs 2.58; N = 600, B = 96 2.36 vs 2.64)
    const long fsb_max = shared_on ? 7000 : (p->wl[0][2].nwork <= 200 ? 9000 : (D <= 5 ? 7000 : 4700));      // (7000 at D <= 5 with the XCD-aware order: N = 2048, B = 12 two kernels on 256x128 tiles 2.70 | one launch 2.50 ms, B = 16 the other way round)           // (9000: N = 400, ds = 3, da = 2, B = 288 two-kernel form 2.09 | one launch per step 1.86 ms, profiles/r05/autotune_512_verbose.txt)
    const bool fsb_take = fsb_can && tn.fused_sb != 0 && wg2 <= fsb_max;
    // (Np = 512 -- two row tiles -- runs its mid range on the 256x128 tiling too: B = 288 / 320 / 384 / 640 x1.14 / 1.10 / 1.09 / 1.15 over 256x256,
    // profiles/r05/autotune_grid_second.txt)
    const bool mid512 = p->Np == 512 && B < 768 && !fsb_take && sb_ok && tb2 && (long)((B + 1) / 2) * p->wl[0][4].nwork >= 1600;
    const bool big128 = (!big || mid512) && !fsb_take && sb_ok && tb2 && (p->Np > 512 || mid512) && (long)((B + 1) / 2) * p->wl[0][4].nwork >= 1600;
    r->sb = (sb_ok && (big || mid)) ? 1 : 0;
    // (round 5: a small training set stays on the one-launch form as far as that reaches -- N = 400, ds = 3, da = 2, B = 288: 256x256 tiles, two
    // kernels per step 2.19 | one launch per step 1.88 ms, profiles/r05/autotune_grid_third.txt)
    const bool big_small_fused = big && p->Np <= 512 && fsb_take && sb_ok && tn.tiling < 0;
    const bool many = (long)p->wl[0][1].nwork > 256L * p->ds;        // > 256 one-wave tiles per GP (N >= 1472)
    r->tiling = big_small_fused ? 2 : ((big && !(mid512 && big128)) ? 0 : (big128 ? 4 : (mid ? 2 : (many ? 3 : 1))));
    if (r->tiling == 2 && narrow_ok && wg2 < 1000)           // 32 columns from ~300 workgroups of 64, 16 below (while the partial sums
        r->tiling = (wg2 >= 300 || p->wl[0][6].nwork > 1300) ? 5 : 6;      // of a trajectory stay within ~1300)
    // A training set whose LAST row tile is a quarter or half tile (Np = 320, 384: N = 257...384): its 256x64 workgroups carry one or
    // two waves of four; on 32 columns there are twice as many, half as long -- measured with gpmpc_pack_autotune (round 4,
    // profiles/r04/autotune_small_n.txt): N = 300, ds = 4, B = 48 / 64 / 96 / 128 / 160 x1.07 / 1.08 / 1.09 / 1.10 / 1.07, ds = 2,
    // B = 128 / 160 x1.06; N = 400 (Np = 448) and N = 512: level, N = 200 (one row tile): level.
    // (not with one lambda for all GPs: there the 64-column tiles are ahead -- round 5 grid, profiles/r05/autotune_grid_first_shared.txt:
    // N = 300, ds = 4, B = 128 0.58 | 0.38 ms, ds = 2, B = 320 0.49 | 0.33)
    // (round 5, with the XCD-aware dispatch order -- on from B = 2 unless switched off --: the 64-column tiles are ahead for distinct
    // lambdas as well: N = 300, ds = 4, B = 64 / 96 / 128 0.298 | 0.274, 0.42 | 0.35, 0.55 | 0.45 ms; ds = 2, B = 64 0.171 | 0.162 --
    // profiles/r05/autotune_xcd_verbose.txt: the rule stays for the natural order only)
    if (r->tiling == 2 && fsb_take && p->Np > 256 && p->Np <= 384 && wg2 >= 1000 && !shared_on && tn.xcdmap == 0) r->tiling = 5;
    if (tn.pair_sb >= 0) {                                   // 0 = staged kernel, 1 = scalar broadcast
        r->sb = (tn.pair_sb != 0 && sb_ok) ? 1 : 0;
        r->tiling = r->sb ? (big ? 0 : (big128 ? 4 : 2)) : (big ? 0 : (many ? 3 : 1));
    }
    if (tn.tiling >= 0) { const int v = tn.tiling; if (v == 0 || ((v == 1 || v == 3) && !r->sb) || ((v == 2 || v == 4) && r->sb) || ((v == 5 || v == 6) && r->sb && fsb_can)) r->tiling = v; }
    const bool wide = r->tiling == 0 || r->tiling == 4;          // 256-row tiles of the XCD-sorted lists
    // scalar-broadcast kernel: two trajectories per wave on the big tiling up to D = 5 (two independent dependency chains per
    // lane, one M_ij load for both: C3 +2.6 %, objective-only +14 %; 82 VGPRs); D = 7 (C4) is 2.5 % faster with one
    r->tb = r->sb ? ((wide && D <= 5 && B >= 2) ? 2 : 1) : (B >= 2 ? 2 : 1);
    if (tn.tb) { const int v = tn.tb; if (v == 1 || v == 2 || (v == 4 && !r->sb)) r->tb = v; }
    if (!diag && grad && r->tb > 2) r->tb = 2;
    // Dispatch interleave of the scalar-broadcast kernel (pair_kernel_sb.h): 4 row tiles per trajectory share each fetch
    // of the G rows (C3 fabric reads per launch 757 -> 418 MB by FETCH_SIZE at the same speed; C4 +0.5 %).
    r->rgroup = 4;
    if (tn.rgroup >= 1 && tn.rgroup <= 16) r->rgroup = tn.rgroup;
    if (!wide) r->rgroup = 1;
    if (lowprec) { r->sb = 0; r->tiling = 0; r->tb = 1; }      // tolerance-sweep kernels: 256x256 work list, one trajectory per workgroup
    // Small batches on the 64-row work lists: ONE launch per horizon step (step_fused.h) instead of head + staged pair
    // kernel -- the B = 1 callbacks of a solver loop are pure dependent latency (GPMPC_FUSED=0 keeps the two-kernel form).
    // (every workgroup of the fused kernel re-reduces the Z0 partials of ALL work items: quadratic in their number, fine up to
    // a few thousand -- N = 2048 has 2112 --, 16x off at the 6336 items of N = 4096, which keeps the two-kernel form)
    r->fused = (!r->sb && !lowprec && diag && (r->tiling == 1 || r->tiling == 3) && p->da <= 2 && tn.fused != 0 &&
                p->wl[0][r->tiling].nwork <= 4096) ? 1 : 0;
    // Mid-size batches on the 256x64 tiling: the same single launch per step with the scalar-broadcast column loop in the tile
    // workgroups (step_fused.h, Q = 0).  Every tile workgroup re-reduces the Z0 partial sums of its trajectory: up to 320 tiles
    // per GP (N <= 2048; 256 of them are prefetched in one round trip).
    // Measured against head + pair kernel with concurrent sub-batches (tools/env_ab.py --var GPMPC_FUSED_SB, synchronising after
    // each call; profiles/r03/ab_fused_sb.txt): N = 1024, B = 8 / 12 / 16 / 24 / 32 / 48 x1.29 / 1.42 / 1.26 / 1.08 / 1.04 / 0.98;
    // N = 2048, B = 4 / 6 / 8 / 12 x1.17 / 1.10 / 1.06 / 0.97; N = 768, B = 24 / 48 x1.36 / 1.13: up to ~4700 tile workgroups per
    // launch (beyond, the longer prologue of every tile workgroup costs more than the head kernel it replaces).
    // (up to 600 tiles per GP, N <= ~4300.  An earlier limit of 320 came from N = 4096, ds = 6, B = 1 at 4.35 vs 3.73 ms -- measured on D = 7
    // instances that spilled 21 registers; compiled for 4 waves per SIMD they are level there, and ds = 4 gains x1.2 at N = 3584 / 4096)
    // With ONE lambda for all GPs the shared-lambda pair kernel (two launches per step) is the alternative: the one-launch form
    // evaluating the exponent per GP is ahead of it up to ~3000 tile workgroups (profiles/r03/ab_fused_sb_vs_shared.txt:
    // N = 1024, B = 8 / 12 / 16 / 24 / 32 x1.52 / 1.45 / 1.20 / 0.99 / 0.75; N = 2048, B = 2 / 4 / 8 x1.37 / 1.29 / 0.85), and with
    // groups of GPs per tile workgroup (r->shared below) up to ~7000.
    // (training sets of up to ~200 tiles per trajectory, N <= 1024 at ds = 4, whose tile workgroups have less to re-reduce: ahead or
    // level up to ~7000 -- N = 1024, B = 32 / 48 1.88 / 2.72 vs 2.17 / 2.91 ms on one box, 1.95 / 2.83 vs 2.02 / 2.77 on another;
    // N = 768, B = 64 2.14 vs 2.44 ms)
    if (r->sb && r->tiling == 2 && r->tb == 1 && fsb_can && (tn.fused_sb == 1 || wg2 <= fsb_max))
        r->fused = 2;
    if (r->sb && (r->tiling == 5 || r->tiling == 6) && r->tb == 1 && fsb_can) r->fused = 2;   // narrower tiles: this form only
    if (r->fused) r->tb = 1;
    // a quarter of a tile's columns per workgroup while whole tiles would leave most SIMDs without a wave
    r->fq = (r->fused == 1 && r->tiling == 1 && (long)B * p->wl[0][1].nwork < 256) ? 4 : 1;
    r->waves = p->wl[0][r->tiling].waves;
    r->nwork = p->wl[0][r->tiling].nwork;
    // Shared length-scales: one exponent / exp per pair for a group of GPs (pair_kernel_sbs.h) wherever the scalar-broadcast
    // kernel would run.  256x256 tiles once they give ~1700 workgroups (one trajectory per workgroup), else 256x64.
    r->shared = 0; r->sh_list = 0;
    // groups of TWO GPs (twice the workgroups of the pack's group size, 17.5 instead of 14.25 instructions per pair and GP at D = 5) while
    // the launch is small: ms per batch, groups of 2 | groups of 4 | one GP per workgroup -- N = 1024, B = 8 0.65 | 0.80 | 0.69, B = 12
    // 0.70 | 0.87 | 0.81, B = 16 0.83 | 0.89 | 0.99, B = 24 1.07 | 1.16 | 1.44; N = 2048, B = 2 0.61 | 0.84 | 0.69, B = 4 0.86 | 0.95 | 1.03,
    // B = 8 1.51 | 1.38 | 1.91; N = 768, B = 16 0.64 | 0.73 | 0.72 (profiles/r03/ab_fused_shared.txt)
    r->fng = p->sh_ng;
    if (p->sh_ng > 2 && p->ds % 2 == 0 && p->wl_sh[3].work_dev && wg2 < 4200) r->fng = 2;
    // (two GPs: from ~700 tile workgroups -- N = 300, ds = 2, B = 64 / 128 0.195 / 0.205 -> 0.155 / 0.183 ms, profiles/r05/autotune_grid_second_shared.txt)
    if (r->sb && r->fused == 2 && r->tiling == 2 && shared_on && (wg2 >= (r->fng == 2 ? (p->ds == 2 ? 700 : 1000) : 2200) || tn.fused_sb == 1)) {
        // one lambda for all GPs AND the one-launch form: its tile workgroups take groups of sh_ng GPs (step_fused.h, NG > 1) on the
        // shared 256x64 list.  Three forms compete for such a pack (profiles/r03/ab_fused_shared.txt, ms per batch: groups of GPs in one
        // launch | one GP per tile workgroup in one launch | shared-lambda pair kernel, two launches): N = 1024, B = 8 0.81 | 0.67 | -,
        // B = 16 0.89 | 0.99 | -, B = 24 1.17 | 1.42 | 1.64, B = 32 1.45 | 1.84 | 1.67, B = 48 1.94 | - | 1.91; N = 2048, B = 2
        // 0.82 | 0.67, B = 4 0.94 | 1.03, B = 8 1.37 | 1.88 | 1.69, B = 12 2.06 | - | 2.05; N = 512, ds = 3, B = 32 0.64 | 0.56, B = 128
        // 1.10 | 1.48 | 1.41: per-GP workgroups (4x as many, narrower tiles) below ~2200 workgroups of 64 columns, groups up to ~7000
        r->shared = 1; r->sh_list = 1;
        r->tb = 1; r->waves = 4;
        r->nwork = p->ds * p->sh_tiles[1];
    } else
    if (r->sb && r->fused != 2 && !lowprec && p->shared_lambda && tn.shared != 0 && p->sh_ng >= 2) {
        r->shared = 1;
        // (round 3: a 256x128 list, wl_sh[2], is built for the A/B only -- GPMPC_TILING=4 --: with one trajectory per workgroup it has
        // nothing to share that the 256x64 tiles under the concurrent sub-batches do not have; N = 2048, B = 16...40 -3...-20 %,
        // N = 1024, B = 128 / 160 +2 / +3 % -- profiles/r03/ab_shared_tiling.txt.  256x256 from 1700 workgroups: N = 2048, B = 40
        // 4.90 (256x64) vs 5.32 ms, B = 48 5.71 vs 5.77; N = 1024, B = 160 5.10 vs 5.19)
        r->sh_list = ((long)B * p->wl_sh[0].nwork >= 1700) ? 0 : 1;
        if (tn.tiling == 0 || tn.tiling == 2 || tn.tiling == 4) r->sh_list = tn.tiling == 0 ? 0 : (tn.tiling == 2 ? 1 : 2);
        r->tb = 1; r->waves = 4;
        r->nwork = p->ds * p->sh_tiles[r->sh_list];           // partial sums per trajectory: [GP][tile]
        r->rgroup = r->sh_list != 1 ? ((tn.rgroup >= 1 && tn.rgroup <= 16) ? tn.rgroup : 4) : 1;
    }
    // One trajectory (or a few) of a training set whose 256x64 tiles would take several workgroup generations: balanced runs of up to 256
    // columns, ONE generation per trajectory (pack.hip, work list 7; step_fused.h, Q = 256)
    if (r->fused == 2 && r->tiling == 2 && !r->shared && !shape && tn.tiling < 0 && p->wl[0][7].work_dev) {
        r->tiling = 7;
        r->nwork = p->wl[0][7].nwork;
    }
    // Columns per iteration of the scalar-broadcast kernel: 4 on the 256x64 tiling (mid-size batches: latency tolerance of
    // the partly filled generations, pair_kernel_sb.h), 1 on full launches.
    // (tools/env_ab.py --var GPMPC_SB_UNROLL: +8...14 % up to ~2 generations of workgroups, -4 % from ~4 on)
    r->colunroll = (r->sb && !r->shared && !lowprec && r->tiling == 2 && r->tb == 1 && tn.colunroll != 1 &&
                  ((long)B * r->nwork <= 4096 || tn.colunroll == 4)) ? 4 : 1;
    r->xcdmap = tn.xcdmap;
    if (shape) {
        r->tiling = shape->tiling; r->tb = shape->tb; r->waves = shape->waves; r->nwork = shape->nwork; r->sb = shape->sb;
        r->rgroup = shape->rgroup; r->fused = shape->fused; r->fq = shape->fq; r->shared = shape->shared; r->sh_list = shape->sh_list; r->fng = shape->fng;
        r->colunroll = shape->colunroll; r->xcdmap = shape->xcdmap;
    }
    // Whole-horizon kernel, one workgroup per trajectory (traj_persist.h): large batches of a small training set -- at least about one
    // trajectory per CU, X within the kernel's LDS budget.  r->fused = 3; r->pwaves = waves per workgroup.
    r->pwaves = 0;
    // Measured against the step-per-launch plan (tools/lib_ab.py, profiles/r04/ab_persist.txt; ms per batch, H = 10, default | 16 waves |
    // 8 waves): N = 300, ds = 4: B = 128 0.70 | 0.92 | 1.29, B = 192 1.34 | 0.95 | 1.48, B = 256 1.31 | 0.99 | 1.56, B = 384 1.72 | 1.83 | 1.77,
    // B = 512 2.11 | 1.93 | 1.80; N = 300, ds = 2, B = 256 0.57 | 0.43 | 0.47; N = 200, ds = 2, B = 1024 0.58 | 0.57 | 0.48; N = 400, ds = 3,
    // da = 2, B = 256 2.11 | 1.68 | 2.54; N = 512, ds = 3, H = 20, B = 256 3.01 | 2.49 | 4.11; N = 640, B = 256 2.75 | 3.03; N = 1024,
    // H = 20, B = 256 10.9 | 14.4 (every workgroup streams all of M from L2 / Infinity Cache each step: 6.5 TB/s at N = 1024).
    // Round 5 (the kernel is x1.3-1.6 faster than the one the round-4 thresholds were fitted to; re-measured with gpmpc_pack_autotune over
    // N = 200 ... 640, B = 64 ... 1024: profiles/r05/autotune_grid_first*.txt, autotune_grid.txt): a COST comparison instead of fill thresholds.
    // One 16-wave workgroup per CU (or two of 8 waves), so the kernel's time goes in generations of num_cu (2 num_cu) trajectories; a partly
    // filled generation is shorter (less contention for the L2: N = 300, ds = 4: B = 128 / 192 / 256 0.56 / 0.59 / 0.69 ms): 0.64 + 0.36 fill of
    // a full one.  In units of a full 16-wave generation: cost16 = generations (last one discounted), cost8 = r8 x the same over 2 num_cu slots,
    // r8 = 1.6 (light trajectories) ... 2.0; the step-per-launch forms cost (B / num_cu) x inv_e(Np), inv_e = how much less efficient per
    // trajectory they are than a full generation of this kernel: 2.15 at Np = 256 (break-even B ~ 96), 1.55 at 320 (~140), 1.36 at 448 (~175),
    // 1.16 at 512 (~200), 1.05 at 640 (full generations only); with one lambda x1.25 (units of 3 / 4 GPs).  Np >= 512 beyond two generations:
    // never (every workgroup streams all of M each step; the 256x128 / 256x256 pair kernels are ahead: N = 512, B = 640 6.2 | 5.4 ms).
    {
        const int cu = p->num_cu > 0 ? p->num_cu : 256;
        auto gens_cost = [](int Bn, int slots) {
            const int full = Bn / slots, rem = Bn - full * slots;
            return (double)full + (rem > 0 ? 0.64 + 0.36 * (double)rem / slots : 0.0);
        };
        const bool psh = shared_on && p->ds >= 2 && D >= 3 && D <= 6;                   // (= pshared below)
        const bool all_in_one = psh && ((p->ds == 4 && D == 5) || (p->ds == 3 && D <= 5));   // 16-wave workgroups run ALL GPs of the pack in one unit
        const double work = (double)p->ds * p->Np * p->Np;
        // (an EFFECTIVE ratio, fitted on batches that end in a partly filled 8-wave generation; a refit on full generations -- 1.63 at N = 200, ds = 2,
        // 1.93 at 300 / 2 and 200 / 4 -- with its own partial-generation term moved more shapes away from the measured best than it brought back:
        // profiles/r05/autotune_grid_sixth.txt and the run before it)
        double r8 = 1.4 + 4.0e-12 * work * work;                                         // (grid: 1.46 at N = 200, ds = 2; 1.53 at 300 / 2; ~1.7 at 200 / 4; > 2.05 at 300 / 4)
        if (r8 > 2.2) r8 = 2.2;
        if (all_in_one) r8 *= 1.25;                                                      // (8-wave workgroups fall back to units of two GPs)
        const double cost16 = gens_cost(B, cu), cost8 = r8 * gens_cost(B, 2 * cu);
        const int Npq = p->Np;
        double inv_e = Npq <= 256 ? (p->ds <= 2 ? 2.15 : 1.95) : (Npq <= 320 ? 1.50 : (Npq <= 384 ? 1.50 : (Npq <= 448 ? 1.45 : (Npq <= 512 ? 1.16 : (Npq <= 576 ? 1.10 : 1.14)))));      // (640: 1.14 -- B = 224 step-per-launch 2.43 | whole horizon 2.25 ms, B = 192 the other way round)
        if (psh) inv_e *= p->ds <= 2 ? 1.0 : (Npq <= 448 ? 1.15 : 1.10);
        if (Npq >= 512 && B > 2 * cu && !psh) inv_e = 0.9;
        const double cost_spl = (double)B / cu * inv_e;
        int pw = 0;
        if ((cost16 <= cost8 ? cost16 : cost8) < 0.97 * cost_spl) pw = cost8 < cost16 ? 8 : 16;
        if (tn.persist == 8 || tn.persist == 16) pw = tn.persist;
        // With ONE lambda for all GPs the step-per-launch forms share exponent and exp across the GPs of a pair, this kernel does not
        // (yet): from three GPs on they are ahead of it (shared packs, ms per batch, step-per-launch | 16 waves | 8 waves: N = 300, ds = 4,
        // B = 256 0.87 | 0.99 | 1.56, B = 512 1.42 | 1.93 | 1.81; N = 512, ds = 3, B = 256 1.97 | 2.49; with two GPs the whole-horizon
        // kernel still wins: N = 300, ds = 2, B = 256 0.49 | 0.43, N = 200, B = 1024 0.70 | 0.56 | 0.47 -- profiles/r04/ab_persist_shared.txt)
        // ... so with one lambda this kernel runs over units of TWO GPs (traj_persist.h, NG = 2; instantiated up to D = 6), and packs it
        // cannot serve that way (D >= 7) keep the step-per-launch forms from three GPs on.  Shared packs, step-per-launch | units of two
        // GPs, 16 waves | 8 waves (profiles/r04/ab_persist_shared_ng2.txt): N = 300, ds = 4, B = 256 0.86 | 0.68 | 0.78, B = 512 1.41 | 1.27 | 1.10;
        // ds = 2, B = 256 0.49 | 0.33; ds = 5, B = 256 1.34 | 1.03; N = 200, ds = 2, B = 1024 0.69 | 0.43 | 0.33; N = 400, ds = 3, da = 2 1.44 | 1.39;
        // N = 512, ds = 3, H = 20 1.94 | 2.06 (not taken: up to Np = 448 with one lambda).  D = 7 loses with distinct lambdas too
        // (N = 300, ds = 6: 2.19 | 2.32; ds = 5, da = 2: 1.69 | 1.98 -- the accumulators leave the column loop one chain and two loads in
        // flight): taken up to D = 6.
        // an explicit kernel-form override (GPMPC_FUSED=0, GPMPC_PAIR_SB, GPMPC_TILING, GPMPC_FUSED_SB) asks for a step-per-launch form: an A/B
        // with those variables must not silently run this kernel instead (GPMPC_PERSIST=8|16 still forces it)
        const bool form_forced = tn.fused == 0 || tn.pair_sb >= 0 || tn.tiling >= 0 || tn.fused_sb >= 0;
        const bool pshared = shared_on && p->ds >= 2 && D >= 3 && D <= 6;
        const bool shared_ahead = shared_on && !pshared && p->ds >= 3;
        r->png = 1;
        // (never for the sub-batches of a split call: they run the launches of the WHOLE batch's plan -- a sub-batch that happened to fit
        // this kernel used to come back with this branch's work-list fields and the whole batch's form: an empty grid)
        if (!shape && diag && !lowprec && p->da >= 1 && p->da <= 2 && p->Np <= GPMPC_PERSIST_MAXNP_HOST && H * p->da <= 1024 && tn.persist != 0 &&
            pw && (tn.persist > 0 || (p->Np <= 640 && D <= 6 && !shared_ahead && !form_forced))) {
            r->fused = 3; r->sb = 0; r->shared = 0; r->tb = 1; r->rgroup = 1; r->colunroll = 1; r->fq = 1;
            r->pwaves = pw;
            // units of two GPs; ALL GPs of the pack in one unit where that instance exists (traj_persist.h: ds = 4 at D = 5, ds = 3 at D <= 5;
            // 16-wave workgroups only: two 8-wave workgroups per CU do not fit their static LDS)
            r->png = pshared ? ((pw == 16 && ((p->ds == 4 && D == 5) || (p->ds == 3 && D <= 5))) ? p->ds : 2) : 1;
            r->nwork = 0;
        }
    }
    if (shape) { r->fused = shape->fused; r->pwaves = shape->pwaves; r->png = shape->png; if (r->fused == 3) { r->sb = 0; r->shared = 0; r->nwork = 0; } }
    r->nm = gpmpc_num_moments(D, diag, grad);
    r->pps = D + D * D;
    r->sps = p->nominal ? sps_nominal(D) : sps_of(D);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n * sizeof(double) + 255) & ~(size_t)255; return o; };
    r->off_pp = take((size_t)B * p->ds * r->pps);
    r->off_sp = take((size_t)2 * B * p->ds * r->sps);
    r->off_part = take((size_t)(r->fused ? 2 * r->fq : 1) * B * r->nwork * r->nm);     // fused: double-buffered by step parity
    r->off_partz = take(r->fused ? (size_t)2 * r->fq * B * r->nwork : 0);
    // Row chunks of the head kernel (two-kernel form only): about 64 workgroups, at least 512 rows each.  N = 4096, ds = 6,
    // B = 1: the head kernel was 66 us of a 172 us step on 6 workgroups.
    r->hchunks = 0; r->hrows = 0;
    if (!r->fused && !lowprec) {
        int c = 64 / (B * p->ds);
        if (c > p->Np / 512) c = p->Np / 512;
        if (c > 16) c = 16;
        if (tn.hchunks >= 0) c = tn.hchunks;
        if (c > 1) { r->hrows = ((p->Np + c - 1) / c + 255) & ~255; r->hchunks = (p->Np + r->hrows - 1) / r->hrows; if (r->hchunks <= 1) r->hchunks = 0; }
    }
    if (shape) { r->hchunks = shape->hchunks; r->hrows = shape->hrows; }
    r->off_mpart = take(r->hchunks > 1 ? (size_t)2 * B * p->ds * r->hchunks * (1 + 2 * D) : 0);
    r->off_jac = take(grad ? (size_t)B * H * 2 * p->ds * (2 * p->ds + p->da) : 0);
    r->gw = gpmpc_sb_gw(D, p->ds);
    // column rows: [B][GP][Np][gw] written by the head kernel, or one [64][gw] slot per tile workgroup of the mid-size fused form
    r->off_G = take(r->fused == 3 ? (size_t)B * p->ds * p->Np * r->gw : r->fused == 2 ? (size_t)B * (r->shared ? p->wl_sh[(r->fng == 2 && p->sh_ng != 2) ? 3 : 1].nwork : r->nwork) * p->wl[0][r->tiling].jt * r->gw
                                  : (r->sb ? (size_t)B * (r->shared ? 1 : p->ds) * p->Np * r->gw : 0));
    r->off_means = take((size_t)B * (H + 1) * p->ds);
    r->off_vars = take((size_t)B * (H + 1) * p->ds);
    r->total = off;
}

// A MID-SIZE batch (256x64 tiling) runs as S sub-batches on S streams (parallel branches of the graph under graph replay).
// A horizon step is a serial chain head kernel -> pair kernel, and at these sizes neither fills the chip for long (the head
// kernel runs B ds workgroups, the pair kernel ends in a partly filled generation: tools/sb_stamps.py); two independent chains
// fill each other's gaps.
#define GPMPC_MAX_SPLIT 4
static int split_count(const gpmpc_pack* p, const RollPlan& r, int B, bool lowprec, bool eager = false, int split_over = 0,
                       int H = 0, int grad = -1) {
    if (lowprec || !r.sb) return 1;
    if (!split_over && H > 0 && grad >= 0)
        if (const gpmpc_tuned_entry* te = tuned_lookup(p, B, H, grad != 0)) { int S = te->S; if (eager && S > 2) S = 2; return S < 1 ? 1 : (S > B ? B : S); }
    const bool mid = r.shared ? r.sh_list == 1 : r.tiling == 2;
    // measured (tools/env_ab.py --var GPMPC_SPLIT, profiles/r03/split_ab.txt): N = 1024, B = 16: 11.3 -> 13.8 (2 branches) -> 14.3 k
    // rollouts/s (4); N = 2048, B = 4 / 16: +15 % / +13 %; a branch must keep at least two trajectories, and branches whose
    // pair launch alone fills the chip twice over gain nothing unless they are wide (N = 4096, B = 2 as 1 + 1: -20 %)
    // A caller who needs each result before the next call (a solver loop) sees the latency of ONE call: there every extra
    // branch also costs launch work up front, and a branch must keep ~900 workgroups per pair launch to pay for itself
    // (N = 1024, B = 16, synchronising after every call: 2 branches x1.12, 4 branches x0.93-1.02; B = 32: 4 branches x1.09-1.13;
    // with calls queued back to back 4 branches give x1.27 / x1.24 -- profiles/r03/split_latency_vs_throughput.txt).
    int S = 1;
    if (r.fused == 2) {
        // one launch per step: two branches are ahead everywhere (tools/env_ab.py --var GPMPC_SPLIT, N = 1024, B = 8 / 16 / 24: one branch
        // x1.03 / 0.86 / 0.94, two x1.11 / 1.01 / 1.06, four x1.02 / 0.95 / 1.01 of the two-kernel rule's choice)
        // ... but only from ~800 tile workgroups per launch on (gpmpc_pack_autotune, round 4: N = 200, ds = 2, B = 64 and ds = 4, B = 32
        // -- 512 tile workgroups -- run x1.21 faster unsplit; N = 200, ds = 4, B = 64 and everything larger keeps two), and a pair of
        // trajectories of a large training set splits too (N = 2048, B = 2: x1.04)
        // (groups of GPs per tile workgroup: count the workgroups, not the partial sums -- N = 300, ds = 2 with one lambda, B = 128: 768 workgroups,
        // 0.210 ms in two branches, 0.184 in one)
        const long wgs = (long)B * (r.shared && r.fng > 1 ? r.nwork / r.fng : r.nwork);
        S = ((B >= 4 && wgs >= 800) || (B >= 2 && wgs >= 1000 && wgs <= 2500)) ? 2 : 1;
    } else if (mid && B >= 4) {
        S = B / 2 < GPMPC_MAX_SPLIT ? B / 2 : GPMPC_MAX_SPLIT;
        while (S > 1 && (long)(B / S) * r.nwork >= 4096 && B / S < 8) --S;
        while (S > 1 && (long)(B / S) * r.nwork < 900) --S;
        if (S == 3) S = 2;
    }
    // 256x256 tiling with two trajectories per wave, up to ~8 generations of workgroups: two sub-batches fill each other's partly
    // filled last generation (N = 2048: B = 48 / 64 / 128 +11 / +9 / +4 %, B = 256 +-0; N = 1024, B = 128 / 256 +6 / +5 %;
    // one trajectory per wave (D >= 6, N = 4096): -3...-7 %, not split) -- profiles/r03/split_big_ab.txt
    if (!mid && !r.shared && (r.tiling == 0 || r.tiling == 4) && r.tb == 2 && B >= 16 && (long)((B + 1) / 2) * r.nwork <= 10000) S = 2;
    // Launched plainly (no graph) the branches are streams of the pack, which the runtime maps onto a handful of hardware queues
    // shared with every other stream of the process: four branches then ran from x1.27 to x0.87 of the unsplit call depending on
    // what else the process had created (N = 1024, B = 32 in a fresh process: 1 / 2 / 3 / 4 branches 2.15 / 1.95 / 1.92 / 2.47 ms
    // -- profiles/r03/split_eager_branches.txt); two are ahead in every process measured.
    if (eager && S > 2) S = 2;
    if (p->tune.split >= 1) S = p->tune.split;
    if (split_over >= 1) S = split_over;
    if (S > GPMPC_MAX_SPLIT) S = GPMPC_MAX_SPLIT;
    if (S > B) S = B;
    return S;
}
static size_t split_bytes(const gpmpc_pack* p, const RollPlan& r, int B, int H, bool grad, int S) {
    size_t sum = 0;
    for (int k = 0; k < S; ++k) {
        const int b0 = (int)((long)B * k / S), b1 = (int)((long)B * (k + 1) / S);
        RollPlan q;
        plan_rollout(p, b1 - b0, H, grad, true, &q, false, &r);
        sum += q.total;
    }
    return sum;
}

extern "C" size_t gpmpc_rollout_workspace_bytes(const gpmpc_pack* p, int B, int H, unsigned flags) {
    if (!p || B < 1 || H < 1) return 0;
    RollPlan r;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
    GraphModeGuard mode((flags & GPMPC_USE_GRAPH) ? 1 : 0);
    plan_rollout(p, B, H, grad, true, &r, lowprec);
    size_t need = r.total;
    const int S = split_count(p, r, B, lowprec, false, 0, H, grad ? 1 : 0);     // mid-size batches run as S concurrent sub-batches, each with its own slice
    if (S > 1) { const size_t sb = split_bytes(p, r, B, H, grad, S); if (sb > need) need = sb; }
    return need;
}

// What a rollout call of this shape launches, as text (bench.py names the dominant kernel with it, the tests check which form a
// shape reaches, tools/ compare plans): "form=<...> kernel=<...> tiling=<rows>x<cols> workgroups=<per step> launches_per_step=<n> split=<S> ..."
extern "C" int gpmpc_plan_describe(const gpmpc_pack* p, int B, int H, unsigned flags, char* out, size_t out_bytes) {
    if (!p || !out || out_bytes < 64 || B < 1 || H < 1) return GPMPC_E_ARG;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
    RollPlan r;
    GraphModeGuard mode((flags & GPMPC_USE_GRAPH) ? 1 : 0);
    plan_rollout(p, B, H, grad, true, &r, lowprec);
    const int S = split_count(p, r, B, lowprec, (flags & GPMPC_USE_GRAPH) == 0, 0, H, grad ? 1 : 0);
    static const int cfg[8][2] = {{256, 256}, {64, 64}, {256, 64}, {64, 128}, {256, 128}, {256, 32}, {256, 16}, {256, 256}};
    const int D = p->D, ds = p->ds;
    char kern[160];
    const char* form;
    long wgs;
    if (r.fused == 3) {
        form = "persist";
        snprintf(kern, sizeof(kern), "k_traj_persist<%d,%d,%s,%d>x%dwaves", D, ds, grad ? "true" : "false", r.png, r.pwaves);
        wgs = B;
    } else if (r.fused == 2) {
        const int q = r.tiling == 2 ? 0 : cfg[r.tiling][1], ng = r.shared ? r.fng : 1;
        const gpmpc_worklist& wsh = p->wl_sh[(r.fng == 2 && p->sh_ng != 2) ? 3 : 1];
        form = r.shared ? "fused_sb_shared" : "fused_sb";
        snprintf(kern, sizeof(kern), "k_step_fused<%d,%d,%s,%d,%d>", D, ds, grad ? "true" : "false", q, ng);
        wgs = (long)B * ((r.shared ? wsh.nwork : r.nwork) + 2 * ds);
    } else if (r.fused == 1) {
        form = "fused_staged";
        snprintf(kern, sizeof(kern), "k_step_fused<%d,%d,%s,%d,1>", D, ds, grad ? "true" : "false", r.fq);
        wgs = (long)B * (r.nwork * r.fq + 2 * ds);
    } else if (lowprec) {
        form = "lowprec"; snprintf(kern, sizeof(kern), "k_pair_lowprec<%d>", D); wgs = (long)B * r.nwork;
    } else if (r.shared) {
        form = "head+pair_sbs";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel_sbs<%d,%d,%d,%s,false>", D, p->sh_ng, ds, grad ? "true" : "false");
        wgs = (long)B * p->wl_sh[r.sh_list].nwork;
    } else if (r.sb) {
        form = "head+pair_sb";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel_sb<%d,%d,%d,%s,false,%d>", D, r.tb, ds, grad ? "true" : "false", r.colunroll == 4 ? 4 : 1);
        wgs = (long)((B + r.tb - 1) / r.tb) * r.nwork;
    } else {
        form = "head+pair_staged";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel<%d,true,%s,%d>", D, grad ? "true" : "false", r.tb);
        wgs = (long)((B + r.tb - 1) / r.tb) * r.nwork;
    }
    const int tl = r.shared && r.fused != 2 ? (r.sh_list == 0 ? 0 : (r.sh_list == 1 ? 2 : 4)) : r.tiling;
    snprintf(out, out_bytes, "form=%s kernel=%s tiling=%dx%d workgroups=%ld launches_per_step=%d split=%d tb=%d shared=%d hchunks=%d workspace=%zu%s",
             form, kern, cfg[tl][0], cfg[tl][1], wgs, r.fused == 3 ? 0 : (r.fused ? 1 : 2), S, r.tb, r.shared, r.hchunks, r.total,
             p->nominal ? " nominal=1" : "");
    return GPMPC_OK;
}

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
                           double* ext_jac = nullptr, bool full_first = false, const RollPlan* shape = nullptr) {
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
    RollPlan r;
    plan_rollout(p, B, H, grad, true, &r, lowprec != 0, shape);
    if (workspace_bytes < r.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    RollArgs A;
    memset(&A, 0, sizeof(A));
    A.XT = p->XT; A.beta = p->beta; A.lam = p->lam; A.sf = p->sf;
    A.Np = p->Np; A.ds = p->ds; A.da = p->da; A.D = p->D;
    A.x0 = x0; A.U = U; A.B = B; A.H = H;
    A.means = out_means ? out_means : (double*)(ws + r.off_means);
    A.vars = out_vars ? out_vars : (double*)(ws + r.off_vars);
    A.pp = (double*)(ws + r.off_pp); A.sp = (double*)(ws + r.off_sp); A.part = (double*)(ws + r.off_part);
    A.jac = grad ? (ext_jac ? ext_jac : (double*)(ws + r.off_jac)) : nullptr;
    A.hchunks = r.hchunks; A.hrows = r.hrows; A.mpart = r.hchunks > 1 ? (double*)(ws + r.off_mpart) : nullptr;
    A.G = r.sb ? (double*)(ws + r.off_G) : nullptr; A.gw = r.gw;
    A.pps = r.pps; A.sps = r.sps; A.nwork = r.nwork; A.nm = r.nm; A.grad = grad ? 1 : 0;
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
    P.Np = p->Np; P.B = B; P.nunits = p->ds; P.nwork = r.nwork; P.pps = r.pps; P.nm = r.nm;
    P.jside_off = 0; P.ntri = p->ds; P.ns2 = p->ds; P.colsplit = (r.tiling == 1 || r.tiling == 3) ? 1 : 0;

    if (r.fused == 3) {
        PersistArgs Q;
        memset(&Q, 0, sizeof(Q));
        Q.XT = p->XT; Q.beta = p->beta; Q.lam = p->lam; Q.sf = p->sf; Q.M = p->M; Q.Np = p->Np;
        Q.x0 = x0; Q.U = U; Q.B = B; Q.H = H;
        Q.means = A.means; Q.vars = A.vars; Q.jac = A.jac;
        Q.gscr = (double*)(ws + r.off_G);
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
        const gpmpc_worklist& wsh = p->wl_sh[(r.fng == 2 && p->sh_ng != 2) ? 3 : 1];      // groups of two GPs | of the pack's group size
        F.XT = p->XT; F.beta = p->beta; F.lam = p->lam; F.sf = p->sf; F.M = p->M; F.work = fsh ? wsh.work_dev : wl.work_dev;
        const int nwg = r.nwork * r.fq;                     // partial sums per trajectory (= tile workgroups, except fsh: ds x tiles)
        F.Np = p->Np; F.nwork = nwg;
        F.ntile = fsh ? wsh.nwork : nwg; F.tiles = fsh ? p->sh_tiles[1] : 0;
        F.tri64 = (r.tiling == 1) ? 1 : 0;                  // 64x64 list: items decoded arithmetically (no dependent load)
        for (int a = 0; a <= p->ds; ++a) { F.ustart[a] = fsh ? a * p->sh_tiles[1] : wl.ustart_host[a] * r.fq; A.ust[a] = F.ustart[a]; }
        A.ust_inline = 1; A.nwork = nwg;
        F.x0 = x0; F.U = U; F.B = B; F.H = H;
        F.means = A.means; F.vars = A.vars; F.jac = A.jac;
        F.sp = A.sp; F.part = A.part; F.partz = (double*)(ws + r.off_partz);
        F.sps = r.sps; F.nm = r.nm;
        F.gscr = r.fused == 2 ? (double*)(ws + r.off_G) : nullptr;
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
        A.part += (size_t)(H & 1) * B * nwg * r.nm;          // the tail finishes step H from the parity the last launch wrote
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
            Q.pps = r.pps; Q.nm = r.nm; Q.rgroup = r.rgroup;
            Q.first_step = (t == 1 && !p->tune.no_first && !full_first) ? 1 : 0;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_sbs(p->D, grad, p->sh_ng, p->ds, Q, s);
        } else if (r.sb) {
            PairSbArgs Q;
            Q.M = p->M; Q.XT = p->XT; Q.pp = A.pp; Q.G = A.G; Q.part = A.part; Q.work = P.work;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = r.nwork; Q.pps = r.pps; Q.nm = r.nm; Q.rgroup = r.rgroup;
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

// One rollout call as S sub-batches: sub-batch 0 on `origin`, the others on the pack's auxiliary streams, forked from and
// joined back into `origin` with events (inside a stream capture these become parallel branches of the graph).  The
// caller holds the pack's lock (PackGuard): two host threads sharing a pack must not interleave their fork / join pairs.
static int enqueue_split(gpmpc_pack* p, gpmpc_graph_cache* g, int S, const RollPlan& whole, hipStream_t origin, int B, int H,
                         const double* x0, const double* U, const gpmpc_cost_params* cost, unsigned flags, double* out_means,
                         double* out_vars, double* out_cost, double* out_grad, void* workspace) {
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    int rc = GPMPC_OK;
    hipError_t ef = hipEventRecord(g->ev_fork, origin);
    char* wsp = (char*)workspace;
    const int ds = p->ds, da = p->da;
    for (int k = S - 1; k >= 0 && rc == GPMPC_OK && ef == hipSuccess; --k) {
        const int b0 = (int)((long)B * k / S), b1 = (int)((long)B * (k + 1) / S);
        size_t woff = 0;
        for (int q = 0; q < k; ++q) {
            RollPlan pq;
            plan_rollout(p, (int)((long)B * (q + 1) / S) - (int)((long)B * q / S), H, grad, true, &pq, false, &whole);
            woff += pq.total;
        }
        RollPlan pk;
        plan_rollout(p, b1 - b0, H, grad, true, &pk, false, &whole);
        hipStream_t sk = k == 0 ? origin : g->aux[k - 1];
        if (k > 0) ef = hipStreamWaitEvent(sk, g->ev_fork, 0);
        if (ef != hipSuccess) break;
        rc = enqueue_rollout(p, b1 - b0, H, x0 + (size_t)b0 * ds, U + (size_t)b0 * H * da, cost, flags,
                             out_means ? out_means + (size_t)b0 * (H + 1) * ds : nullptr,
                             out_vars ? out_vars + (size_t)b0 * (H + 1) * ds : nullptr, out_cost + b0,
                             out_grad ? out_grad + (size_t)b0 * H * da : nullptr, wsp + woff, pk.total, sk, nullptr, false, &whole);
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
        RollPlan whole;
        plan_rollout(p, B, H, grad, true, &whole, lowprec);
        const int S = split_count(p, whole, B, lowprec, false, 0, H, grad ? 1 : 0);
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
        RollPlan whole;
        plan_rollout(p, B, H, grad, true, &whole, false);
        const int S = split_count(p, whole, B, false, true, 0, H, grad ? 1 : 0);
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
static bool same_shape(const RollPlan& a, const RollPlan& b) {
    if (a.fused == 3 && b.fused == 3) return a.pwaves == b.pwaves && a.png == b.png;      // the whole-horizon kernel has no tiling
    return a.tiling == b.tiling && a.tb == b.tb && a.sb == b.sb && a.fused == b.fused && a.fq == b.fq && a.shared == b.shared &&
           a.sh_list == b.sh_list && a.fng == b.fng && a.colunroll == b.colunroll && a.hchunks == b.hchunks && a.pwaves == b.pwaves &&
           a.rgroup == b.rgroup && a.nwork == b.nwork && a.xcdmap == b.xcdmap;
}

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
    struct Cand { RollPlan r; int S; double ms; const char* why; };
    Cand cand[48]; int nc = 0;
    auto add = [&](const gpmpc_tuning& tn, int split, const char* why) {
        if (nc >= 48) return;
        RollPlan r;
        plan_rollout(p, B, H, grad, true, &r, false, nullptr, &tn);
        int S = split_count(p, r, B, false, !use_graph, split);
        if (S > 1 && r.fused == 3) S = 1;
        for (int k = 0; k < nc; ++k) if (same_shape(cand[k].r, r) && cand[k].S == S) return;
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
        size_t need = cand[k].r.total;
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
        te.B = B; te.H = H; te.grad = grad ? 1 : 0; te.graph = use_graph ? 1 : 0; te.S = cand[win].S; te.plan = cand[win].r;
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
    if (p->tuned) memset(p->tuned, 0, sizeof(gpmpc_tuned_table));
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
    RollPlan r;                                             // the plan enqueue_rollout takes for this call: where it keeps J_t, means, variances
    plan_rollout(p, B, H, grad, true, &r, false);
    if (workspace_bytes < r.total) return GPMPC_E_WORKSPACE;
    if (int rc = enqueue_rollout(p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace, workspace_bytes, stream))
        return rc;
    char* ws = (char*)workspace;
    return gpmpc_rollout_constraints(B, H, p->ds, p->da, cons, out_means ? out_means : (const double*)(ws + r.off_means),
                                     out_vars ? out_vars : (const double*)(ws + r.off_vars),
                                     grad ? (const double*)(ws + r.off_jac) : nullptr, out_g, grad ? out_gjac : nullptr, stream);
}
