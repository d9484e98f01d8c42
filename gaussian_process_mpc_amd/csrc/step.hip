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
//
// Here: the head kernel and the enqueue of one rollout call.  The kernel arguments and the finish phase, which the tail kernel runs too, are
// in roll_dev.h; the tail kernel (cost, adjoint sweep) is in step_tail.hip.
#include "rollout.h"
#include "roll_dev.h"
#include "fast_exp.h"

// Diagnostic build (-DGPMPC_SB_STAMPS): phase stamps of the head kernel, workgroup (0, 0, 0) of horizon step 5 (tools/sb_stamps.py)
#ifdef GPMPC_SB_STAMPS
static __device__ unsigned long long g_head_stamps[16];
#define GPMPC_HST(slot)                                                                             \
    do {                                                                                            \
        if (t == 5 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0)    \
            g_head_stamps[slot] = __builtin_amdgcn_s_memtime();                                     \
    } while (0)
extern "C" int gpmpc_debug_head_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_head_stamps), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -3;
}
#else
#define GPMPC_HST(slot) do { } while (0)
#endif

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
            sk = A.noise[gpmpc_noise_off_action(ds) + (k - ds)];      // action_var of the pack's noise model
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
    // step 1 through pair_kernel_q1.h: the column values [kappa_j | kappa_j h_jk (k >= ds)] of this (trajectory, GP) instead of G rows
    double* __restrict__ q1c = (A.q1cols && t == 1) ? A.q1cols + ((size_t)a * A.Np * A.B + b) * (1 + A.da) : nullptr;
    double* __restrict__ Grow = (A.G && !q1c) ? (A.shared ? (a == 0 ? A.G + (size_t)b * A.Np * A.gw : nullptr)
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
            if (q1c) {     // h = sc o u - sc o x and |h|^2 as below and in the row side of pair_kernel_q1.h; library exp: O(N) work
                double hk[D], qh = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) { hk[k] = fma(-sck[k], xk[k], sck[k] * u[k]); qh = fma(hk[k], hk[k], qh); }
                const double kap = exp(-2.0 * qh);
                double* c = q1c + (size_t)i * A.B * (1 + A.da);
                c[0] = kap;
#pragma unroll
                for (int k = 0; k < D; ++k) if (k >= ds) c[1 + k - ds] = kap * hk[k];
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
            if (k == 0) { sp[0] = c; sp[1] = cm; sp[2] = sf2 + A.noise[gpmpc_noise_off_process(ds, A.da) + a]; }
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
        if (k == 0) { sp[0] = c; sp[1] = mu; sp[2] = sf2 + A.noise[gpmpc_noise_off_process(ds, A.da) + a]; }
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
            const double v0 = A.noise[threadIdx.x * (A.ds + 1)];          // diag(init_cov) of the pack's noise model
            s_mu[threadIdx.x] = x;
            s_var[threadIdx.x] = v0;
            if (a == 0 && chunk == 0) {
                A.means[((size_t)b * (A.H + 1)) * A.ds + threadIdx.x] = x;
                A.vars[((size_t)b * (A.H + 1)) * A.ds + threadIdx.x] = v0;
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
// enqueue of one rollout call (the plan: plan.hip; graph replay, split launch and the entry points: graph.hip)
// ---------------------------------------------------------------------------
template <int D>
static void launch_head(const RollArgs& A, int t, hipStream_t s) {
    const dim3 grid(A.B, A.ds, A.hchunks > 1 ? A.hchunks : 1);
    if (!A.nom) hipLaunchKernelGGL((k_roll_head<D, 0>), grid, dim3(256), 0, s, A, t);
    else if (A.grad) hipLaunchKernelGGL((k_roll_head<D, 2>), grid, dim3(256), 0, s, A, t);
    else hipLaunchKernelGGL((k_roll_head<D, 1>), grid, dim3(256), 0, s, A, t);
}

// One rollout call on c.stream: the head + pair launch of every horizon step (or the one-launch / whole-horizon form), then the tail.
int gpmpc_enqueue_rollout(const RollCall& c) {
    const gpmpc_pack* p = c.p;
    const int B = c.B, H = c.H;
    if (!p || !c.x0 || !c.U || !c.cost || !c.out_cost || !c.workspace || B < 1 || H < 1) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    const bool grad = (c.flags & GPMPC_WANT_GRAD) != 0;
    if (grad && !c.out_grad) return GPMPC_E_ARG;
    gpmpc_sched_ref sched;                                     // (entries that replay a graph or launch before they come here have resolved it already)
    if (int rcs = gpmpc_schedule_resolve(c.cost, p->ds, p->da, H, "gpmpc_rollout", &sched)) return rcs;
    const int lowprec = (c.flags & GPMPC_FP32_ALL) ? 2 : ((c.flags & GPMPC_FP32_ACCUM) ? 1 : 0);
    if (lowprec && grad) return GPMPC_E_ARG;                   // the sweep modes are objective only
    if (lowprec && p->nominal) {
        gpmpc_set_error_text("gpmpc_rollout: the GPMPC_FP32_* modes do not know the linear nominal model of this pack");
        return GPMPC_E_STATE;
    }
    const RollShape r = c.shape ? *c.shape : gpmpc_choose_shape(p, B, H, grad, lowprec != 0);
    const RollLayout L = gpmpc_layout_for(p, r, B, H, grad);
    if (c.workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = c.stream;
    char* ws = (char*)c.workspace;
    RollArgs A;
    memset(&A, 0, sizeof(A));
    A.XT = p->XT; A.beta = p->beta; A.lam = p->lam; A.sf = p->sf;
    A.Np = p->Np; A.ds = p->ds; A.da = p->da; A.D = p->D;
    A.x0 = c.x0; A.U = c.U; A.B = B; A.H = H;
    A.means = c.out_means ? c.out_means : (double*)(ws + L.off_means);
    A.vars = c.out_vars ? c.out_vars : (double*)(ws + L.off_vars);
    A.pp = (double*)(ws + L.off_pp); A.sp = (double*)(ws + L.off_sp); A.part = (double*)(ws + L.off_part);
    A.jac = grad ? (c.ext_jac ? c.ext_jac : (double*)(ws + L.off_jac)) : nullptr;
    A.hchunks = r.hchunks; A.hrows = r.hrows; A.mpart = r.hchunks > 1 ? (double*)(ws + L.off_mpart) : nullptr;
    A.G = r.sb ? (double*)(ws + L.off_G) : nullptr; A.gw = L.gw;
    A.pps = L.pps; A.sps = L.sps; A.nwork = r.nwork; A.nm = L.nm; A.grad = grad ? 1 : 0;
    A.ustart = p->wl[0][r.tiling].ustart_dev;
    A.work = p->wl[0][r.tiling].contiguous ? nullptr : p->wl[0][r.tiling].work_dev;
    A.perm = p->wl[0][r.tiling].contiguous ? nullptr : p->wl[0][r.tiling].perm_dev;
    A.out_cost = c.out_cost; A.out_grad = c.out_grad; A.cost = *c.cost;
    A.nom = p->nominal ? p->nom_dev : nullptr;
    A.sched = sched.dev; A.sched_hmax = sched.H_max;
    A.noise = p->noise_dev;
    // Horizon step 1 as a quadratic form (pair_kernel_q1.h): decided for the whole call by gpmpc_rollout, which has refilled the pack's step-1
    // weights on this stream; not for d/dx0 (full_first), whose step 1 needs every moment.  The column values take the front of the G region.
    const bool q1 = c.step1_quad && !c.full_first && p->M1 && gpmpc_step1_quad_plan(p, r, 0, lowprec != 0);
    const int q1t = p->tune.step1_t == 16 ? 16 : 8;
    if (q1) {
        const size_t cols = (size_t)B * p->ds * p->Np * (1 + p->da), room = (size_t)B * p->ds * p->Np * L.gw;
        if (cols + (size_t)q1t * (1 + p->da) > room) return GPMPC_E_WORKSPACE;      // (never: gw >= D + 2 > 1 + da, and Np >= 64)
        A.q1cols = A.G;
    }
    if (A.nom && (r.fused || r.hchunks > 1)) {     // (a plan handed in from outside: the nominal variants exist for the two-launch form only)
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
        Q.x0 = c.x0; Q.U = c.U; Q.B = B; Q.H = H;
        Q.means = A.means; Q.vars = A.vars; Q.jac = A.jac;
        Q.gscr = (double*)(ws + L.off_G);
        const int T = p->Np / 64;
        Q.total = ((p->ds + r.png - 1) / r.png) * 32 * T * (T + 1);
        Q.ncol = p->ncol_dev;
        Q.noise = p->noise_dev;
        const int rc = gpmpc_timed_persist(p->D, grad, p->ds, r.pwaves, r.png, Q, s);
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
        F.x0 = c.x0; F.U = c.U; F.B = B; F.H = H;
        F.means = A.means; F.vars = A.vars; F.jac = A.jac;
        F.sp = A.sp; F.part = A.part; F.partz = (double*)(ws + L.off_partz);
        F.sps = L.sps; F.nm = L.nm;
        F.gscr = r.fused == 2 ? (double*)(ws + L.off_G) : nullptr;
        F.ncol = p->ncol_dev;
        F.noise = p->noise_dev;
        // XCD-aware dispatch order (step_fused.h): measured against the natural order (tools/lib_ab.py, profiles/r05/ab19_xcdmap*.txt; N:ds:B
        // gain): 2048:4: B = 2 -1 %, 3 +2 %, 4 +4 %, 6 +8 %, 8 +6 %; 1024:4: 2 -2 %, 4 -2.5 / +2 %, 8 +4 %, 16 / 24 level; 512:3: 32 / 64 +3 / +2 %;
        // 300:4:32 +16 %; one lambda: 2048:4:8 +8 %, 1024:4:32 +14 %, 512:3:64 +14 %, 300:4:64 +10 %.  As a candidate of gpmpc_pack_autotune
        // (autotune_xcd_verbose*.txt) it is the best or within the run-to-run spread (~3 %) of the best on every shape of the grid, also on
        // SMALL grids (N = 300, ds = 2, B = 64 +21 %; N = 200, ds = 4, B = 64, one lambda +27 %): there the natural order puts the same
        // tiles of every trajectory -- the heavy 256-row ones -- on the same XCDs, the remapped order rotates the remainder.  From B = 2
        // (B = 2 itself is level: N = 2048 0.579 | 0.580, N = 1024 0.283 | 0.284 ms; sub-batches of two gain: N = 2048, B = 4 as 2 x 2 0.925 | 0.911).
        F.xcdmap = r.xcdmap >= 0 ? (r.xcdmap && B > 1) : B >= 2;
        const int fq = r.fused == 2 ? (r.tiling == 2 ? 0 : wl.jt) : r.fq;
        for (int t = 1; t <= H; ++t)
            if (int rc = gpmpc_timed_step_fused(p->D, grad, p->ds, fq, fsh ? r.fng : 1, F, t, s)) return rc;
        A.part += (size_t)(H & 1) * B * nwg * L.nm;          // the tail finishes step H from the parity the last launch wrote
    }
    for (int t = 1; t <= H && !r.fused; ++t) {
        const int first_step = (t == 1 && !p->tune.no_first && !c.full_first) ? 1 : 0;
        int rc = gpmpc_dispatch_dim<1>(p->D, [&](auto d) { launch_head<decltype(d)::value>(A, t, s); return GPMPC_OK; });
        if (rc != GPMPC_OK) return rc;
        if (lowprec) {
            rc = gpmpc_launch_pair_lowprec(p->D, lowprec, P, s);
        } else if (q1 && t == 1) {
            PairQ1Args Q;
            Q.M1 = p->M1; Q.XT = p->XT; Q.pp = A.pp; Q.cols = A.q1cols; Q.part = A.part; Q.work = P.work;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = r.nwork; Q.pps = L.pps; Q.nm = L.nm; Q.rgroup = r.rgroup;
            Q.tblock = q1t;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_q1(p->D, p->da, Q, s);
        } else if (r.shared) {
            const gpmpc_worklist& wl = p->wl_sh[r.sh_list];
            PairSbsArgs Q;
            Q.M = p->M; Q.XT = p->XT; Q.pp = A.pp; Q.G = A.G; Q.part = A.part; Q.work = wl.work_dev;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = wl.nwork; Q.tiles = p->sh_tiles[r.sh_list]; Q.jt = wl.jt;
            Q.pps = L.pps; Q.nm = L.nm; Q.rgroup = r.rgroup;
            Q.first_step = first_step;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_sbs(p->D, grad, p->sh_ng, p->ds, Q, s);
        } else if (r.sb) {
            PairSbArgs Q;
            Q.M = p->M; Q.XT = p->XT; Q.pp = A.pp; Q.G = A.G; Q.part = A.part; Q.work = P.work;
            Q.Np = p->Np; Q.B = B; Q.ds = p->ds; Q.nwork = r.nwork; Q.pps = L.pps; Q.nm = L.nm; Q.rgroup = r.rgroup;
            Q.first_step = first_step;
            Q.colunroll = r.colunroll;
            Q.ncol = p->ncol_dev;
            rc = gpmpc_timed_pair_sb(p->D, grad, r.tb, p->ds, r.waves, Q, s);
        } else {
            rc = gpmpc_timed_pair(p->D, true, grad, r.tb, P.colsplit ? 4 : r.waves, P, s);
        }
        if (rc != GPMPC_OK) return rc;
    }
    return gpmpc_launch_roll_tail(A, grad, s);
}
