// The full-covariance rollout for the chance constraints and the device solvers: the bridge from the step Jacobians both forms of
// gpmpc_rollout_fullcov leave in the workspace (fullcov.hip: dmean_du, dmean_dS, dcov_du, dcov_dS at [H][B] slices) to the packed step
// Jacobian [p][p + da], p = ds + ds (ds + 1) / 2, that the sweeps of linprop_fc.hip take (k_lpf_constraints, k_lpf_vjp: pure functions of
// means, covs and that Jacobian).  Layout and rules: include/gpmpc.h, "Full-covariance rollout: Jacobian and chance constraints"; the why:
// DESIGN.md section 3l.
//   k_fc_pack_jac   one lane per element of jac[B][H][p][p + da]: a gather from the four arrays, a coalesced store.  Every element is
//                   written, no atomics, the grid follows from the sizes.
// Entries: gpmpc_rollout_fullcov_jac (rollout without cost + pack), gpmpc_rollout_fullcov_constrained (rollout + tail, then -- with the
// gradient -- pack and the sweep; without it the values-only sweep), and the refusals the device solvers share.
#include <cstdio>
#include "gpmpc_internal.h"
#include "fullcov_internal.h"

#define FCC_MAX_P (GPMPC_MAX_DS + GPMPC_MAX_DS * (GPMPC_MAX_DS + 1) / 2)

// index e of the row-major upper triangle of an n x n matrix -> (a, b), a <= b
static __device__ __forceinline__ void fcc_untri(int e, int n, int& a, int& b) {
    a = 0;
    while (e >= n - a) { e -= n - a; ++a; }
    b = a + e;
}

// grid (ceil(B H p (p + da) / 256)).  Rows (mu'_a, Sigma'_ab for a <= b, row-major), columns (mu_k, Sigma_kl for k <= l, u_j): the convention of
// gpmpc_linearised_fc_step.  An off-diagonal Sigma_kl = Sigma_lk is ONE variable: its column is d/dS_kl + d/dS_lk, written as that sum, so the
// result does not depend on whether the stored derivative is symmetrised.  Only the state block of dS is read; all D columns of du.  The state
// columns of step 1 are written like any other (Sigma_0 is a constant; the sweeps never read them).
__global__ __launch_bounds__(256) void k_fc_pack_jac(int B, int H, int ds, int da, const double* __restrict__ dmean_du,
                                                      const double* __restrict__ dmean_dS, const double* __restrict__ dcov_du,
                                                      const double* __restrict__ dcov_dS, double* __restrict__ jac) {
    const int D = ds + da, p = ds + ds * (ds + 1) / 2, nc = p + da;
    const size_t per = (size_t)p * nc, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * H * per) return;
    const size_t bt = e / per;
    const int rc = (int)(e - bt * per), r = rc / nc, c = rc - r * nc;
    const int b = (int)(bt / H), t = (int)(bt - (size_t)b * H);          // step t + 1, slice t
    const size_t sl = (size_t)t * B + b;
    const double* __restrict__ du;
    const double* __restrict__ dS;
    if (r < ds) {
        du = dmean_du + (sl * ds + r) * D;
        dS = dmean_dS + (sl * ds + r) * D * D;
    } else {
        int a, bb;
        fcc_untri(r - ds, ds, a, bb);
        const size_t j = sl * ds * ds + (size_t)a * ds + bb;
        du = dcov_du + j * D;
        dS = dcov_dS + j * D * D;
    }
    double v;
    if (c < ds) v = du[c];
    else if (c < p) {
        int k, l;
        fcc_untri(c - ds, ds, k, l);
        v = k == l ? dS[k * D + k] : dS[k * D + l] + dS[l * D + k];
    } else v = du[ds + (c - p)];
    jac[e] = v;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// What gpmpc_rollout_fullcov refuses, with text, for the entries that would otherwise meet it after their first launch.
int gpmpc_fc_refuse(const gpmpc_pack* p, const char* who, int tail_H) {
    char text[256];
    const char* why = nullptr;
    if (p->nominal) why = "the full-covariance rollout does not know the linear nominal model of this pack";
    else if (!p->built) why = "the pack is not built";
    else if (p->npairs > 0 && !p->fullcov) why = "the pack has no cross-covariance weights (gpmpc_pack_enable_fullcov)";
    if (why) {
        snprintf(text, sizeof(text), "%s: %s", who, why);
        gpmpc_set_error_text(text);
        return GPMPC_E_STATE;
    }
    // k_fc_tail<DS> exists for DS <= 6, so gpmpc_rollout_fullcov has never returned a result beyond it (nor is either form of the rollout held
    // to a reference there): no entry takes more.  The tail keeps the horizon in LDS: that binds the calls that run it, and only those.
    if (p->ds > GPMPC_FC_TAIL_MAX_DS)
        return gpmpc_refuse(who, "the full-covariance rollout is built for state_dim <= %d, the pack has %d", GPMPC_FC_TAIL_MAX_DS, p->ds);
    if (tail_H > 0 && gpmpc_fc_tail_lds(p->ds, p->da, tail_H) > GPMPC_FC_TAIL_LDS_MAX)
        return gpmpc_refuse(who, "H = %d is beyond the LDS of the full-covariance rollout's cost kernel", tail_H);
    return GPMPC_OK;
}

// the limits of the sweeps of linprop_fc.hip (lpf_count_ok, lpf_sweep_fits) and of this file's one-dimensional grid
static int fcc_sizes(const gpmpc_pack* p, int B, int H, const char* who) {
    if (B < 1 || H < 1) return gpmpc_refuse(who, "B or H < 1");
    if (p->da < 1) return gpmpc_refuse(who, "the packed Jacobian needs action_dim >= 1");
    const long per = (long)FCC_MAX_P * (FCC_MAX_P + GPMPC_MAX_D);
    if ((long)B * H * per > (1L << 40) || (long)B * H * per / 256 >= 0x7fffffffL) return gpmpc_refuse(who, "B x H is too large");
    if ((long)H * p->da > 64L * 65535) return gpmpc_refuse(who, "H = %d is beyond the sweep's grid (H da <= 64 x 65535)", H);
    return GPMPC_OK;
}

static int fcc_pack(const FcArgs& A, double* jac, hipStream_t s) {
    const size_t p = (size_t)A.ds + (size_t)A.ds * (A.ds + 1) / 2, total = (size_t)A.B * A.H * p * (p + A.da);
    hipLaunchKernelGGL(k_fc_pack_jac, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, A.B, A.H, A.ds, A.da, (const double*)A.dmean_du,
                       (const double*)A.dmean_dS, (const double*)A.dcov_du, (const double*)A.dcov_dS, jac);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" size_t gpmpc_rollout_fullcov_jac_workspace_bytes(const gpmpc_pack* p, int B, int H) {
    return gpmpc_rollout_fullcov_workspace_bytes(p, B, H, GPMPC_WANT_GRAD);
}

extern "C" int gpmpc_rollout_fullcov_jac(const gpmpc_pack* p, int B, int H, const double* x0, const double* U, double* out_means,
                                         double* out_covs, double* out_jac, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_rollout_fullcov_jac";
    if (!p || !x0 || !U || !out_means || !out_covs || !out_jac || !workspace) return GPMPC_E_ARG;
    if (int rc = gpmpc_check_device(p)) return rc;
    if (int rc = gpmpc_fc_refuse(p, who, 0)) return rc;
    if (int rc = fcc_sizes(p, B, H, who)) return rc;
    FcArgs A;
    if (int rc = gpmpc_fc_run(p, B, H, x0, U, nullptr, GPMPC_WANT_GRAD, false, out_means, out_covs, nullptr, nullptr, workspace, workspace_bytes,
                              stream, &A))
        return rc;
    return fcc_pack(A, out_jac, (hipStream_t)stream);
}

// workspace of a constrained call: means [B][H+1][ds] | covs [B][H+1][ds][ds] | with the gradient: jac [B][H][p][p+da] | the rollout's own
struct FccLayout { size_t off_means, off_covs, off_jac, off_roll, roll_bytes, total; };
static FccLayout fcc_layout(const gpmpc_pack* p, int B, int H, bool grad) {
    FccLayout L;
    gpmpc_carver c;
    const size_t ds = p->ds, pp = ds + ds * (ds + 1) / 2, d = sizeof(double);
    L.off_means = c.take(d * B * (H + 1) * ds);
    L.off_covs = c.take(d * B * (H + 1) * ds * ds);
    L.off_jac = c.take(grad ? d * B * H * pp * (pp + p->da) : 0);
    L.roll_bytes = gpmpc_rollout_fullcov_workspace_bytes(p, B, H, grad ? GPMPC_WANT_GRAD : 0u);
    L.off_roll = c.take(L.roll_bytes);
    L.total = c.total();
    return L;
}

extern "C" size_t gpmpc_rollout_fullcov_constrained_workspace_bytes(const gpmpc_pack* p, int B, int H, unsigned flags) {
    if (!p || B < 1 || H < 1 || (flags & ~GPMPC_WANT_GRAD)) return 0;
    return fcc_layout(p, B, H, (flags & GPMPC_WANT_GRAD) != 0).total;
}

extern "C" int gpmpc_rollout_fullcov_constrained(const gpmpc_pack* p, int B, int H, const double* x0, const double* U,
                                                 const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags,
                                                 double* out_means, double* out_covs, double* out_cost, double* out_grad, double* out_g,
                                                 double* out_gjac, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_rollout_fullcov_constrained";
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    if (!p || !x0 || !U || !cost || !cons || !out_cost || !out_g || !workspace || (grad && (!out_grad || !out_gjac))) return GPMPC_E_ARG;
    if (int rc = gpmpc_check_device(p)) return rc;
    if (int rc = gpmpc_fc_refuse(p, who, 0)) return rc;
    if (flags & GPMPC_USE_GRAPH) return gpmpc_refuse(who, "GPMPC_USE_GRAPH is not supported by the constrained full-covariance rollout");
    if (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) return gpmpc_refuse(who, "the GPMPC_FP32_* modes are not supported by the full-covariance rollout");
    if (flags & ~GPMPC_WANT_GRAD) return gpmpc_refuse(who, "flags: GPMPC_WANT_GRAD or 0");
    if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    if (int rc = fcc_sizes(p, B, H, who)) return rc;
    if (int rc = gpmpc_fc_refuse(p, who, H)) return rc;      // (H >= 1 from here on: the tail's own limits)
    const FccLayout L = fcc_layout(p, B, H, grad);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    char* ws = (char*)workspace;
    double* means = out_means ? out_means : (double*)(ws + L.off_means);
    double* covs = out_covs ? out_covs : (double*)(ws + L.off_covs);
    double* jac = grad ? (double*)(ws + L.off_jac) : nullptr;
    FcArgs A;
    // (a bad cost schedule is refused in here, before the first launch)
    if (int rc = gpmpc_fc_run(p, B, H, x0, U, cost, flags, true, means, covs, out_cost, out_grad, ws + L.off_roll, L.roll_bytes, stream, &A)) return rc;
    if (grad) {
        if (int rc = fcc_pack(A, jac, (hipStream_t)stream)) return rc;
    }
    return gpmpc_linearised_fc_constraints(B, H, p->ds, p->da, cons, means, covs, jac, out_g, grad ? out_gjac : nullptr, stream);
}
