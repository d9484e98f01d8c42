// Linearised (first-order, "mean-equivalent") uncertainty propagation: mu' = m(z), v' = s2(z) + sum_d g_d^2 S_d at z = (mu, u), with the
// step Jacobian in the layout of gpmpc_rollout_jac.  Formulas, layouts and refusals: include/gpmpc.h, "Linearised propagation"; the why and
// what was measured: DESIGN.md section 3j.
//
// Per chunk of C columns (plans) and per group of GPs with bit-identical (lambda, sigma_f) (GpGroup, model_frame.h):
//   k_lp_kstar   Ks[i][c] = k(X_i, z_c), zero-padded to multiples of 64 both ways (written by the workgroups of the group's first GP), and the
//                row-block partial sums of m and of the D components of g:  kpart[bi][slot][0 | 1 + d][c]
//   k_lp_quad    workgroup (bc, bi, matrix): T = (Kinv + Kinv^T)[64 bi ...][:] Ks[:][64 bc ...] by MFMA stages (tile_stage.h) = the rows of r.
//                The staged tile is Kinv[i][k] + Kinv[k][i]: ONE product gives r, and q = 1/2 k^T r and dq/dz_d = sum_i r_i k_i d_id are
//                contracted from the SAME T in the epilogue, so the value and its derivative are derivatives of one another by construction
//                (a second product with the transposed tile would cost twice the MFMA work).  T is never written.
//   k_lp_sums    row blocks added in ascending order: m (+ nominal), g (+ nominal weights), q -> mu', v'; g kept for the Jacobian passes
//   k_lp_hess    second O(N D) pass with w = g o S:  hpart[bi][slot][d][c] = sum_i beta_i k_i (d_id (d_i . w) - w_d / lambda_d)
//   k_lp_jac     dq and h added in ascending order -> the two Jacobian rows of (column, GP), every element written (zeros included)
// Rules: no atomics; every output element is owned by one thread or one workgroup, which sums in a fixed order; launch geometry depends on
// sizes only; columns are independent, so no result depends on `chunk`.
#include <cmath>
#include "roll_dev.h"        // RollArgs, gpmpc_launch_roll_tail and its LDS budget: the cost and the adjoint sweep are the existing tail kernel
#include "mppi_internal.h"   // the MPPI search
#include "tile_stage.h"
#include "linprop_internal.h"   // the model frame, LpTail, LpIn, lp_z, and the STREAM form of the step (linprop_stream.hip)
#include <atomic>

static_assert(SP_T == GPMPC_MODEL_TILE, "the chunk rule of model_frame.h rounds to the tile of tile_stage.h");

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// grid (cnp / 64, np / 64, G.ng).  Thread (c = t & 63, q = t >> 6) owns column c0 + c and the rows i0 + 16 q ... + 15 (ascending) for GP slot z.
__global__ __launch_bounds__(256) void k_lp_kstar(int n, int cn, int D, int ds, const double* __restrict__ X, LpIn I,
                                                   const double* __restrict__ beta, GpGroup G, double* __restrict__ Ks, int ldk,
                                                   double* __restrict__ kpart, int nvk) {
    __shared__ double s_x[SP_T][GPMPC_MAX_D], s_b[SP_T], s_p[4][1 + GPMPC_MAX_D][SP_T];
    const int t = threadIdx.x, c = t & 63, q = t >> 6, slot = blockIdx.z;
    const int c0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T;
    for (int e = t; e < SP_T * GPMPC_MAX_D; e += 256) {
        const int i = e >> 3, d = e & 7;
        s_x[i][d] = (i0 + i < n && d < D) ? X[(size_t)(i0 + i) * D + d] : 0.0;
    }
    if (t < SP_T) s_b[t] = i0 + t < n ? beta[(size_t)(i0 + t) * ds + G.gp[slot]] : 0.0;
    double z[GPMPC_MAX_D];
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) z[d] = (c0 + c < cn && d < D) ? lp_z(I, c0 + c, d, ds) : 0.0;
    __syncthreads();
    double m = 0.0, g[GPMPC_MAX_D] = {};
    for (int r = 0; r < 16; ++r) {
        const int il = 16 * q + r;
        double d2 = 0.0, dd[GPMPC_MAX_D];
#pragma unroll
        for (int d = 0; d < GPMPC_MAX_D; ++d) {
            const double u = s_x[il][d] - z[d];
            d2 = fma(u * u, G.ilam[d], d2);
            dd[d] = u * G.ilam[d];
        }
        const double k = (i0 + il < n && c0 + c < cn) ? G.sf2 * exp(-0.5 * d2) : 0.0;
        if (slot == 0) Ks[(size_t)(i0 + il) * ldk + c0 + c] = k;
        const double bk = s_b[il] * k;
        m = m + bk;
#pragma unroll
        for (int d = 0; d < GPMPC_MAX_D; ++d) g[d] = fma(bk, dd[d], g[d]);
    }
    s_p[q][0][c] = m;
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) s_p[q][1 + d][c] = g[d];
    __syncthreads();
    for (int e = t; e < nvk * SP_T; e += 256) {
        const int v = e >> 6, cc = e & 63;
        kpart[(((size_t)blockIdx.y * ds + slot) * nvk + v) * ldk + c0 + cc] = (s_p[0][v][cc] + s_p[1][v][cc]) + (s_p[2][v][cc] + s_p[3][v][cc]);
    }
}

// grid (cnp / 64, np / 64, matrices).  Matrix z is GP G.gp[z]'s (gp_stride != 0) or the one matrix of all GPs.  nv = 1: q only; 1 + D: q and dq/dz.
// part[matrix][bi][0][c] = 1/2 sum_{i in tile} Ks[i][c] T[i][c];  part[matrix][bi][1 + d][c] = sum_{i in tile} Ks[i][c] T[i][c] d_id(c)
__global__ __launch_bounds__(256) void k_lp_quad(int n, int np, int cn, int D, int ds, const double* __restrict__ Kinv, size_t ld,
                                                  size_t gp_stride, GpGroup G, const double* __restrict__ X, LpIn I,
                                                  const double* __restrict__ Ks, int ldk, double* __restrict__ part, int nv) {
    __shared__ double s_a[SP_KB][SP_T + 1], s_b[SP_KB][SP_T + 1];
    __shared__ double s_x[SP_T][GPMPC_MAX_D], s_z[SP_T][GPMPC_MAX_D];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int c0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T, nbi = gridDim.y;
    const double* __restrict__ K = Kinv + (size_t)G.gp[blockIdx.z] * gp_stride;
    if (nv > 1)
        for (int e = t; e < SP_T * GPMPC_MAX_D; e += 256) {
            const int i = e >> 3, d = e & 7;
            s_x[i][d] = (i0 + i < n && d < D) ? X[(size_t)(i0 + i) * D + d] : 0.0;
            s_z[i][d] = (c0 + i < cn && d < D) ? lp_z(I, c0 + i, d, ds) : 0.0;
        }
    double acc[4][4] = {};
    // the next stage's operands travel in registers while this stage is multiplied
    double pa[4], pb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q;
            const int i = e >> 4, k = e & 15;            // symmetrised tile: Kinv[i0 + i][k0 + k] + Kinv[k0 + k][i0 + i]
            pa[q] = (i0 + i < n && k0 + k < n) ? K[(size_t)(i0 + i) * ld + k0 + k] + K[(size_t)(k0 + k) * ld + i0 + i] : 0.0;
            const int kk = e >> 6, c = e & 63;           // Ks tile: row k0 + kk (< np: the rows n ... np - 1 hold zeros), column c0 + c
            pb[q] = Ks[(size_t)(k0 + kk) * ldk + c0 + c];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < np; k0 += SP_KB) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q;
            s_a[e & 15][e >> 4] = pa[q];
            s_b[e >> 6][e & 63] = pb[q];
        }
        __syncthreads();
        if (k0 + SP_KB < np) fetch(k0 + SP_KB);
        sp_stage<true>(s_a, s_b, tx, ty, acc);
    }
    // k_i r_i of the thread's sixteen (row, column) pairs
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int qa = 0; qa < 4; ++qa) {
            const int i = i0 + sp_row<true>(ty, qa), c = c0 + tx + 16 * qb;
            sp_acc<true>(acc, qa, qb) = Ks[(size_t)i * ldk + c] * sp_acc<true>(acc, qa, qb);
        }
    for (int v = 0; v < nv; ++v) {
        const double il = v ? G.ilam[v - 1] : 0.0;
        __syncthreads();                                 // (s_a is free: it takes the per-thread sums, [ty][column])
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            double p = 0.0;
#pragma unroll
            for (int qa = 0; qa < 4; ++qa) {             // the thread's four rows of this column, ascending
                const double f = v ? (s_x[sp_row<true>(ty, qa)][v - 1] - s_z[tx + 16 * qb][v - 1]) * il : 0.5;
                p = fma(f, sp_acc<true>(acc, qa, qb), p);
            }
            s_a[ty][tx + 16 * qb] = p;
        }
        __syncthreads();
        if (t < SP_T) {
            double s = 0.0;
            for (int y = 0; y < 16; ++y) s += s_a[y][t];
            part[(((size_t)blockIdx.z * nbi + blockIdx.y) * nv + v) * ldk + c0 + t] = s;
        }
    }
}

// one thread per (column, GP of the group): mu', v', and g (with the nominal weights) for the Jacobian passes
__global__ __launch_bounds__(256) void k_lp_sums(int cn, int nbi, int D, int ds, int shared_mat, GpGroup G, LpTail M, LpIn I,
                                                  const double* __restrict__ kpart, int nvk, const double* __restrict__ part, int nv, int ldk,
                                                  double* __restrict__ out_mu, double* __restrict__ out_var, size_t os,
                                                  double* __restrict__ gbuf) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cn * G.ng) return;
    const int c = (int)(e / G.ng), slot = (int)(e - (long)c * G.ng), a = G.gp[slot], mat = shared_mat ? 0 : slot;
    double q = 0.0, m = 0.0;
    for (int b = 0; b < nbi; ++b) q += part[(((size_t)mat * nbi + b) * nv) * ldk + c];
    for (int b = 0; b < nbi; ++b) m += kpart[(((size_t)b * ds + slot) * nvk) * ldk + c];
    if (M.has_nominal) {
        double lin = M.nom_b[a];
        for (int d = 0; d < D; ++d) lin = fma(M.nom_w[a * D + d], lp_z(I, c, d, ds), lin);
        m += lin;
    }
    double lin2 = 0.0;
    for (int d = 0; d < D; ++d) {
        double g = 0.0;
        for (int b = 0; b < nbi; ++b) g += kpart[(((size_t)b * ds + slot) * nvk + 1 + d) * ldk + c];
        if (M.has_nominal) g += M.nom_w[a * D + d];
        const double S = d < ds ? I.var[(size_t)c * I.xs + d] : M.action_var[d - ds];
        lin2 = fma(g * g, S, lin2);
        if (gbuf) gbuf[((size_t)c * ds + slot) * GPMPC_MAX_D + d] = g;
    }
    out_mu[(size_t)c * os + a] = m;
    out_var[(size_t)c * os + a] = ((G.sf2 - q) + lin2) + M.process_var[a];
}

// grid (cnp / 64, np / 64, G.ng), threads as k_lp_kstar.  Reads Ks back (no second exp).
__global__ __launch_bounds__(256) void k_lp_hess(int n, int cn, int D, int ds, const double* __restrict__ X, LpIn I,
                                                  const double* __restrict__ beta, GpGroup G, LpTail M, const double* __restrict__ Ks, int ldk,
                                                  const double* __restrict__ gbuf, double* __restrict__ hpart) {
    __shared__ double s_x[SP_T][GPMPC_MAX_D], s_b[SP_T], s_p[4][GPMPC_MAX_D][SP_T];
    const int t = threadIdx.x, c = t & 63, q = t >> 6, slot = blockIdx.z;
    const int c0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T;
    for (int e = t; e < SP_T * GPMPC_MAX_D; e += 256) {
        const int i = e >> 3, d = e & 7;
        s_x[i][d] = (i0 + i < n && d < D) ? X[(size_t)(i0 + i) * D + d] : 0.0;
    }
    if (t < SP_T) s_b[t] = i0 + t < n ? beta[(size_t)(i0 + t) * ds + G.gp[slot]] : 0.0;
    const bool live = c0 + c < cn;
    double z[GPMPC_MAX_D], w[GPMPC_MAX_D], wl[GPMPC_MAX_D];
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) {
        const bool on = live && d < D;
        z[d] = on ? lp_z(I, c0 + c, d, ds) : 0.0;
        const double S = on ? (d < ds ? I.var[(size_t)(c0 + c) * I.xs + d] : M.action_var[d - ds]) : 0.0;
        w[d] = on ? gbuf[((size_t)(c0 + c) * ds + slot) * GPMPC_MAX_D + d] * S : 0.0;
        wl[d] = w[d] * G.ilam[d];
    }
    __syncthreads();
    double h[GPMPC_MAX_D] = {};
    for (int r = 0; r < 16; ++r) {
        const int il = 16 * q + r;
        double dd[GPMPC_MAX_D], dw = 0.0;
#pragma unroll
        for (int d = 0; d < GPMPC_MAX_D; ++d) {
            dd[d] = (s_x[il][d] - z[d]) * G.ilam[d];
            dw = fma(dd[d], w[d], dw);
        }
        const double bk = s_b[il] * Ks[(size_t)(i0 + il) * ldk + c0 + c];
#pragma unroll
        for (int d = 0; d < GPMPC_MAX_D; ++d) h[d] = fma(bk, dd[d] * dw - wl[d], h[d]);
    }
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) s_p[q][d][c] = h[d];
    __syncthreads();
    for (int e = t; e < D * SP_T; e += 256) {
        const int d = e >> 6, cc = e & 63;
        hpart[(((size_t)blockIdx.y * ds + slot) * GPMPC_MAX_D + d) * ldk + c0 + cc] = (s_p[0][d][cc] + s_p[1][d][cc]) + (s_p[2][d][cc] + s_p[3][d][cc]);
    }
}

// one thread per (column, GP of the group): rows mu'_a and v'_a of the column's [2ds][2ds + da] block, every element
__global__ __launch_bounds__(256) void k_lp_jac(int cn, int nbi, int D, int ds, int shared_mat, GpGroup G, const double* __restrict__ part,
                                                 int nv, const double* __restrict__ hpart, const double* __restrict__ gbuf, int ldk,
                                                 double* __restrict__ jac, size_t js) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cn * G.ng) return;
    const int c = (int)(e / G.ng), slot = (int)(e - (long)c * G.ng), a = G.gp[slot], mat = shared_mat ? 0 : slot;
    const int nc = ds + D;
    double* __restrict__ rowm = jac + (size_t)c * js + (size_t)a * nc;
    double* __restrict__ rowv = jac + (size_t)c * js + (size_t)(ds + a) * nc;
    for (int d = 0; d < D; ++d) {
        double dq = 0.0, h = 0.0;
        for (int b = 0; b < nbi; ++b) dq += part[(((size_t)mat * nbi + b) * nv + 1 + d) * ldk + c];
        for (int b = 0; b < nbi; ++b) h += hpart[(((size_t)b * ds + slot) * GPMPC_MAX_D + d) * ldk + c];
        const double g = gbuf[((size_t)c * ds + slot) * GPMPC_MAX_D + d];
        const int col = d < ds ? d : ds + d;             // (mu, v, u) columns: input j sits at 2 ds + j = ds + d
        rowm[col] = g;
        rowv[col] = 2.0 * h - dq;
        if (d < ds) { rowm[ds + d] = 0.0; rowv[ds + d] = g * g; }
    }
}

// step 0 of a rollout: means[b][0] = x0[b], vars[b][0] = diag(init_cov)
__global__ __launch_bounds__(256) void k_lp_init(int B, int ds, size_t stride, const double* __restrict__ x0, LpTail M, double* __restrict__ means,
                                                  double* __restrict__ vars) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * ds) return;
    const int b = (int)(e / ds), a = (int)(e - (long)b * ds);
    means[(size_t)b * stride + a] = x0[e];
    vars[(size_t)b * stride + a] = M.init_var[a];
}

// ---------------------------------------------------------------------------
// host: the form, checks
// ---------------------------------------------------------------------------
// which form of the step gpmpc_lp_step launches (process-wide; read once per call, in lp_layout)
static std::atomic<int> g_lp_form{GPMPC_LINPROP_FORM_DEFAULT};

extern "C" int gpmpc_linearised_set_form(int form) {
    if (form != GPMPC_LINPROP_FORM_TILE && form != GPMPC_LINPROP_FORM_STREAM && form != GPMPC_LINPROP_FORM_AUTO) {
        if (form == -1) return g_lp_form.load();
        return gpmpc_refuse("gpmpc_linearised_set_form", "form must be GPMPC_LINPROP_FORM_TILE, _STREAM, _AUTO or -1 (query)");
    }
    return g_lp_form.exchange(form);
}

// The core checks of the model (model_frame.h), then what the sums kernels need of it -- nominal model, diag(init_cov), action_var,
// process_var (or the defaults) -- with the refusals of the diagonal noise model.  (linprop_internal.h: linprop_fc.hip starts from it.)
int gpmpc_lp_check_model(const char* who, const gpmpc_gp_model* m, LpTail* out) {
    if (int rc = gpmpc_model_check_core(who, m)) return rc;
    const int ds = m->state_dim, da = m->action_dim, D = ds + da;
    memset(out, 0, sizeof(*out));
    out->has_nominal = m->has_nominal ? 1 : 0;
    if (m->has_nominal) {
        memcpy(out->nom_b, m->nom_b, sizeof(double) * ds);
        memcpy(out->nom_w, m->nom_w, sizeof(double) * ds * D);
    }
    for (int a = 0; a < ds; ++a) out->init_var[a] = GPMPC_INIT_VAR;
    for (int j = 0; j < da; ++j) out->action_var[j] = GPMPC_ACTION_VAR;
    if (m->has_noise) {
        for (int a = 0; a < ds; ++a) {
            const double v = m->init_cov[a * ds + a];
            if (!gpmpc_finite(v) || v < 0.0) return gpmpc_refuse(who, "init_cov[%d][%d] = %g is negative or not finite", a, a, v);
            out->init_var[a] = v;
            if (!gpmpc_finite(m->process_var[a]) || m->process_var[a] < 0.0)
                return gpmpc_refuse(who, "process_var[%d] = %g is negative or not finite", a, m->process_var[a]);
            out->process_var[a] = m->process_var[a];
        }
        for (int j = 0; j < da; ++j) {
            if (!gpmpc_finite(m->action_var[j]) || m->action_var[j] < 0.0)
                return gpmpc_refuse(who, "action_var[%d] = %g is negative or not finite", j, m->action_var[j]);
            out->action_var[j] = m->action_var[j];
        }
    }
    return GPMPC_OK;
}

static bool lp_count_ok(long B, long H) { return B >= 1 && H >= 1 && B * H * (2L * GPMPC_MAX_DS) * (2L * GPMPC_MAX_DS + GPMPC_MAX_D) <= (1L << 40); }

// workspace of a step: Ks [np][C] | kpart [nbi][ds][1 + D][C] | part [ds][nbi][nv][C] | with the Jacobian: hpart [nbi][ds][MAX_D][C] | g [C][ds][MAX_D]
// `form`: the process-wide form read ONCE when the layout of a call is made.  Under TILE the offsets and the total are what they always were;
// STREAM carves its own arrays from `base` on (gpmpc_lps_workspace_bytes); AUTO sizes for the larger of the two.
// (struct LpLayout: linprop_internal.h)
static LpLayout lp_layout(const gpmpc_gp_model* m, int chunk, long ncols, bool want_jac, gpmpc_carver& c) {
    LpLayout L;
    L.form = g_lp_form.load();
    L.base = c.total();
    const int ds = m->state_dim, D = ds + m->action_dim;
    L.nbi = (m->n + SP_T - 1) / SP_T;
    L.np = L.nbi * SP_T;
    L.C = gpmpc_chunk_cols(ncols, chunk);
    L.nv = want_jac ? 1 + D : 1;
    const size_t d = sizeof(double);
    L.off_ks = c.take(d * L.np * L.C);
    L.off_kpart = c.take(d * L.nbi * ds * (1 + D) * L.C);
    L.off_part = c.take(d * ds * L.nbi * L.nv * L.C);
    L.off_hpart = c.take(want_jac ? d * L.nbi * ds * GPMPC_MAX_D * L.C : 0);
    L.off_g = c.take(want_jac ? d * L.C * ds * GPMPC_MAX_D : 0);
    L.total = c.total();
    if (L.form != GPMPC_LINPROP_FORM_TILE) {
        const size_t stream = L.base + gpmpc_lps_workspace_bytes(m, ncols, want_jac);
        L.total = (L.form == GPMPC_LINPROP_FORM_AUTO && L.total > stream) ? L.total : stream;
        c.off = L.total;
    }
    return L;
}

// One step of B columns.  mu_prev / var_prev: column b at + b xs; U_t: + b us; outputs at + b os; jac (or null): + b js.
// THE place that picks the form: the step, the rollout, (through the rollout) the MPPI solve and stage A of linprop_fc.hip all come here.
int gpmpc_lp_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                   size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, const LpLayout& L, char* ws, hipStream_t s) {
    if (L.form == GPMPC_LINPROP_FORM_STREAM || (L.form == GPMPC_LINPROP_FORM_AUTO && B <= GPMPC_LINPROP_AUTO_MAX_B))
        return gpmpc_lps_step(m, tail, B, mu_prev, var_prev, xs, U_t, us, out_mu, out_var, os, jac, js, ws + L.base, s);
    const int ds = m->state_dim, da = m->action_dim, D = ds + da;
    GpGroup groups[GPMPC_MAX_DS];
    const int ngroups = gpmpc_model_groups(m, groups);
    double* Ks = (double*)(ws + L.off_ks);
    double* kpart = (double*)(ws + L.off_kpart);
    double* part = (double*)(ws + L.off_part);
    double* hpart = (double*)(ws + L.off_hpart);
    double* gbuf = jac ? (double*)(ws + L.off_g) : nullptr;
    const int shared_mat = m->gp_stride == 0, nvk = 1 + D, nv = L.nv;
    for (long c0 = 0; c0 < B; c0 += L.C) {
        const int cn = (int)(B - c0 < L.C ? B - c0 : L.C), cnp = (cn + SP_T - 1) / SP_T * SP_T;
        LpIn I;
        I.mu = mu_prev + (size_t)c0 * xs; I.var = var_prev + (size_t)c0 * xs; I.U = U_t ? U_t + (size_t)c0 * us : nullptr;
        I.xs = xs; I.us = us;
        for (int g = 0; g < ngroups; ++g) {
            const GpGroup& G = groups[g];
            hipLaunchKernelGGL(k_lp_kstar, dim3(cnp / SP_T, L.nbi, G.ng), dim3(256), 0, s, m->n, cn, D, ds, m->X, I, m->beta, G, Ks, L.C, kpart, nvk);
            hipLaunchKernelGGL(k_lp_quad, dim3(cnp / SP_T, L.nbi, shared_mat ? 1 : G.ng), dim3(256), 0, s, m->n, L.np, cn, D, ds, m->Kinv, m->ld,
                               m->gp_stride, G, m->X, I, (const double*)Ks, L.C, part, nv);
            hipLaunchKernelGGL(k_lp_sums, dim3(gpmpc_blocks256((long)cn * G.ng)), dim3(256), 0, s, cn, L.nbi, D, ds, shared_mat, G, tail, I,
                               (const double*)kpart, nvk, (const double*)part, nv, L.C, out_mu + (size_t)c0 * os, out_var + (size_t)c0 * os, os, gbuf);
            if (jac) {
                hipLaunchKernelGGL(k_lp_hess, dim3(cnp / SP_T, L.nbi, G.ng), dim3(256), 0, s, m->n, cn, D, ds, m->X, I, m->beta, G, tail,
                                   (const double*)Ks, L.C, (const double*)gbuf, hpart);
                hipLaunchKernelGGL(k_lp_jac, dim3(gpmpc_blocks256((long)cn * G.ng)), dim3(256), 0, s, cn, L.nbi, D, ds, shared_mat, G, (const double*)part,
                                   nv, (const double*)hpart, (const double*)gbuf, L.C, jac + (size_t)c0 * js, js);
            }
        }
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// for linprop_fc.hip (linprop_internal.h)
LpLayout gpmpc_lp_layout(const gpmpc_gp_model* m, int chunk, long ncols, bool want_jac) {
    gpmpc_carver c;
    return lp_layout(m, chunk, ncols, want_jac, c);
}

// ---------------------------------------------------------------------------
// host: entries
// ---------------------------------------------------------------------------
extern "C" size_t gpmpc_linearised_step_workspace_bytes(const gpmpc_gp_model* m, int B, int want_jac, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || !lp_count_ok(B, 1) || !gpmpc_chunk_ok(chunk)) return 0;
    gpmpc_carver c;
    return lp_layout(m, chunk, B, want_jac != 0, c).total;
}

extern "C" int gpmpc_linearised_step(const gpmpc_gp_model* m, int B, const double* mu_prev, const double* var_prev, const double* U_t,
                                     size_t u_stride, double* out_mu, double* out_var, double* out_jac, size_t jac_stride, int chunk,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_linearised_step";
    LpTail tail;
    if (int rc = gpmpc_lp_check_model(who, m, &tail)) return rc;
    if (B < 1) return gpmpc_refuse(who, "B < 1");
    if (!lp_count_ok(B, 1)) return gpmpc_refuse(who, "B is too large");
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!mu_prev || !var_prev || !out_mu || !out_var || !workspace || (m->action_dim > 0 && !U_t)) return gpmpc_refuse(who, "NULL pointer");
    if (out_mu == mu_prev || out_var == var_prev || out_mu == var_prev || out_var == mu_prev || out_mu == out_var)
        return gpmpc_refuse(who, "the outputs must not alias the inputs or each other");
    const int ds = m->state_dim, da = m->action_dim;
    if (u_stride < (size_t)da && B > 1) return gpmpc_refuse(who, "u_stride < action_dim");
    if (out_jac && jac_stride < (size_t)(2 * ds) * (2 * ds + da) && B > 1) return gpmpc_refuse(who, "jac_stride < 2 ds (2 ds + da)");
    gpmpc_carver c;
    const LpLayout L = lp_layout(m, chunk, B, out_jac != nullptr, c);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    return gpmpc_lp_step(m, tail, B, mu_prev, var_prev, ds, U_t, u_stride, out_mu, out_var, ds, out_jac, jac_stride, L, (char*)workspace,
                   (hipStream_t)stream);
}

// workspace of a rollout: means [B][H+1][ds] | vars [B][H+1][ds] | with the gradient: jac [B][H][2ds][2ds+da] | a step's
struct LpRollLayout { size_t off_means, off_vars, off_jac; LpLayout step; size_t total; };
static LpRollLayout lp_roll_layout(const gpmpc_gp_model* m, int B, int H, bool grad, int chunk) {
    LpRollLayout R;
    gpmpc_carver c;
    const int ds = m->state_dim, da = m->action_dim;
    const size_t d = sizeof(double);
    R.off_means = c.take(d * B * (H + 1) * ds);
    R.off_vars = c.take(d * B * (H + 1) * ds);
    R.off_jac = c.take(grad ? d * B * H * (2 * ds) * (2 * ds + da) : 0);
    R.step = lp_layout(m, chunk, B, grad, c);
    R.total = c.total();
    return R;
}

extern "C" size_t gpmpc_linearised_rollout_workspace_bytes(const gpmpc_gp_model* m, int B, int H, unsigned flags, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || !lp_count_ok(B, H) || (flags & ~GPMPC_WANT_GRAD) || !gpmpc_chunk_ok(chunk)) return 0;
    return lp_roll_layout(m, B, H, (flags & GPMPC_WANT_GRAD) != 0, chunk).total;
}

extern "C" int gpmpc_linearised_rollout(const gpmpc_gp_model* m, int B, int H, const double* x0, const double* U,
                                        const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags,
                                        double* out_means, double* out_vars, double* out_jac, double* out_cost, double* out_grad, double* out_g,
                                        double* out_gjac, int chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_linearised_rollout";
    LpTail tail;
    if (int rc = gpmpc_lp_check_model(who, m, &tail)) return rc;
    if (B < 1) return gpmpc_refuse(who, "B < 1");
    if (H < 1) return gpmpc_refuse(who, "H < 1");
    if (!lp_count_ok(B, H)) return gpmpc_refuse(who, "B x H is too large");
    if (flags & GPMPC_USE_GRAPH) return gpmpc_refuse(who, "GPMPC_USE_GRAPH is not supported by the linearised rollout (not yet)");
    if (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) return gpmpc_refuse(who, "the GPMPC_FP32_* modes are not supported by the linearised rollout");
    if (flags & ~GPMPC_WANT_GRAD) return gpmpc_refuse(who, "flags: GPMPC_WANT_GRAD or 0");
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    const int ds = m->state_dim, da = m->action_dim;
    if (!x0 || !workspace || (da > 0 && !U)) return gpmpc_refuse(who, "NULL pointer");
    if (out_jac && !grad) return gpmpc_refuse(who, "out_jac needs GPMPC_WANT_GRAD: without it no Jacobian is computed");
    if (cost && (!out_cost || (grad && !out_grad))) return gpmpc_refuse(who, "NULL pointer (out_cost, or out_grad with GPMPC_WANT_GRAD)");
    if (cons && (!out_g || (grad && !out_gjac))) return gpmpc_refuse(who, "NULL pointer (out_g, or out_gjac with GPMPC_WANT_GRAD)");
    if (cons) if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    gpmpc_sched_ref sched;
    sched.dev = nullptr; sched.H_max = 0;
    if (cost) {
        if (da < 1) return gpmpc_refuse(who, "a cost needs action_dim >= 1");
        if (!gpmpc_roll_tail_fits(H, ds, da, false)) return gpmpc_refuse(who, "H = %d is too long for the cost kernel", H);
        if (int rc = gpmpc_schedule_resolve(cost, ds, da, H, who, &sched)) return rc;
    }
    // (gpmpc_rollout_constraints would refuse it too, but after the steps are enqueued and without a text)
    if (cons && da < 1) return gpmpc_refuse(who, "constraints need action_dim >= 1");
    const LpRollLayout R = lp_roll_layout(m, B, H, grad, chunk);
    if (workspace_bytes < R.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* means = out_means ? out_means : (double*)(ws + R.off_means);
    double* vars = out_vars ? out_vars : (double*)(ws + R.off_vars);
    double* jac = grad ? (out_jac ? out_jac : (double*)(ws + R.off_jac)) : nullptr;
    const size_t xs = (size_t)(H + 1) * ds, js = (size_t)H * (2 * ds) * (2 * ds + da), jblock = (size_t)(2 * ds) * (2 * ds + da);
    hipLaunchKernelGGL(k_lp_init, dim3(gpmpc_blocks256((long)B * ds)), dim3(256), 0, s, B, ds, xs, x0, tail, means, vars);
    for (int t = 1; t <= H; ++t) {
        if (int rc = gpmpc_lp_step(m, tail, B, means + (size_t)(t - 1) * ds, vars + (size_t)(t - 1) * ds, xs, U ? U + (size_t)(t - 1) * da : nullptr,
                             (size_t)H * da, means + (size_t)t * ds, vars + (size_t)t * ds, xs, jac ? jac + (size_t)(t - 1) * jblock : nullptr, js,
                             R.step, ws, s))
            return rc;
    }
    if (cost) {
        RollArgs A;
        memset(&A, 0, sizeof(A));
        A.ds = ds; A.da = da; A.D = ds + da;
        A.x0 = x0; A.U = U; A.B = B; A.H = H;
        A.means = means; A.vars = vars; A.jac = jac;
        A.grad = grad ? 1 : 0;
        A.finished = 1;                                  // every step is written: the tail goes straight to the cost terms and the adjoint sweep
        A.out_cost = out_cost; A.out_grad = out_grad; A.cost = *cost;
        A.sched = sched.dev; A.sched_hmax = sched.H_max;
        if (int rc = gpmpc_launch_roll_tail(A, grad, s)) return rc;
    }
    if (cons)
        if (int rc = gpmpc_rollout_constraints(B, H, ds, da, cons, means, vars, grad ? jac : nullptr, out_g, grad ? out_gjac : nullptr, stream))
            return rc;
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// MPPI over the linearised rollout: the search of mppi_internal.h with a model in the place of the pack
// ---------------------------------------------------------------------------
// workspace: the head of every MPPI solve | the rollout's own workspace
struct LpMppiLayout { gpmpc_mppi_head head; size_t off_roll, roll_bytes, total; };
static LpMppiLayout lp_mppi_layout(const gpmpc_gp_model* m, int H, int K, int m_c) {
    LpMppiLayout L;
    gpmpc_carver c;
    L.head = gpmpc_mppi_head_take(c, H, m->state_dim, m->action_dim, K, m_c);
    L.roll_bytes = lp_roll_layout(m, K, H, false, 0).total;
    L.off_roll = c.take(L.roll_bytes);
    L.total = c.total();
    return L;
}

extern "C" size_t gpmpc_mppi_solve_linearised_workspace_bytes(const gpmpc_gp_model* m, int H, const gpmpc_mppi_params* P,
                                                              const gpmpc_state_constraints* cons) {
    if (!gpmpc_model_sizes_ok(m) || !P || P->n_samples < 1 || P->n_samples > GPMPC_MPPI_MAX_SAMPLES) return 0;
    if (cons && (cons->n_rows < 1 || cons->n_rows > GPMPC_MAX_CONS)) return 0;
    if (!gpmpc_solver_dims_ok(H, m->state_dim, m->action_dim)) return 0;
    return lp_mppi_layout(m, H, P->n_samples, cons ? cons->n_rows : 0).total;
}

extern "C" int gpmpc_mppi_solve_linearised(const gpmpc_gp_model* m, int H, const double* x0, const double* start, const gpmpc_cost_params* cost,
                                           const gpmpc_state_constraints* cons, const gpmpc_mppi_params* P, double* out_U, double* out_best,
                                           double* out_trace, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_mppi_solve_linearised";
    if (!m || !x0 || !start || !cost || !P || !out_U || !out_best || !out_trace || !workspace) return gpmpc_refuse(who, "NULL pointer");
    if (H < 1) return gpmpc_refuse(who, "H < 1");
    if (int rc = gpmpc_mppi_check_scalars(P, who)) return rc;
    if (cons) if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    LpTail tail;
    if (int rc = gpmpc_lp_check_model(who, m, &tail)) return rc;
    const int ds = m->state_dim, da = m->action_dim;
    if (!gpmpc_solver_dims_ok(H, ds, da)) return gpmpc_refuse(who, "H, state_dim or action_dim outside what a solver takes");
    if (int rc = gpmpc_mppi_check_inputs(P, da, who)) return rc;
    if (!gpmpc_roll_tail_fits(H, ds, da, false)) return gpmpc_refuse(who, "H = %d is too long for the cost kernel", H);
    gpmpc_sched_ref sched;
    if (int rc = gpmpc_schedule_resolve(cost, ds, da, H, who, &sched)) return rc;
    const int K = P->n_samples, m_c = cons ? cons->n_rows : 0;
    const LpMppiLayout L = lp_mppi_layout(m, H, K, m_c);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    char* ws = (char*)workspace;
    auto eval = [&](int, const double* x0b, const double* U, double* cst, double* g) {
        return gpmpc_linearised_rollout(m, K, H, x0b, U, cost, cons, 0, nullptr, nullptr, nullptr, cst, nullptr, g, nullptr, 0, ws + L.off_roll,
                                        L.roll_bytes, stream);
    };
    return gpmpc_mppi_search(L.head, ws, H, ds, da, m_c, P, x0, start, eval, out_U, out_best, out_trace, stream);
}
