// STREAM form of the linearised step (include/gpmpc.h, "Linearised propagation"): the same inputs, outputs, layouts
// and formulas as the TILE form of linprop.hip, for a FEW columns.  The O(N^2) part is matrix-vector work: every element of Kinv is fetched
// ONCE per group of GPMPC_LINPROP_STREAM_COLS vectors and used for all of them, for y = Kinv k and, with the Jacobian, for Kinv^T k as well.
//
// A "vector" is k of one (column, GP): f = c ds + a.  With a matrix per GP a group holds the vectors of LPS_COLS consecutive columns of ONE
// GP; with gp_stride = 0 it holds LPS_COLS consecutive f, so B = 1, ds <= LPS_COLS is one pass over the one matrix for all GPs.
// Per chunk of LPS_CHUNK columns, whatever the number of GPs or of (lambda, sigma_f) groups:
//   k_lps_kstar  grid (np / 256, ds, columns): ks[f][i] = k_a(X_i, z_c), zero for i >= n (np = n rounded up to 128 ... 256), and the
//                256-row partial sums of m and g:  kpart[f][bi][0 | 1 + d]
//   k_lps_quad   grid (np / LPS_RB, matrices, groups): a workgroup owns LPS_RB rows, a wave LPS_RW of them; a lane reads 16 bytes of each
//                row per 128-column chunk.  y[f][j] = (Kinv k)_j complete; qpart[f][rb] = sum_{j in block} k_j y_j; with the Jacobian
//                colpart[f][rb][i] = sum_{j in block} Kinv[j][i] k_j: rows ascending within a wave, then waves 0 ... 3.
//   k_lps_sums   one thread per vector: blocks added in ascending order -> mu', v'; g kept for the Jacobian
//   k_lps_grad   grid as k_lps_kstar: r_i = y_i + (sum_rb colpart[rb][i], ascending); 256-row partial sums of dq/dz_d = sum_i r_i k_i d_id and
//                of h_d:  jpart[f][bi][d | MAX_D + d]
//   k_lps_jac    one thread per vector: the two Jacobian rows, every element written
// Three launches without the Jacobian, five with it.  q = k^T (Kinv k) here (the TILE form: 1/2 k^T (Kinv + Kinv^T) k): the same number by
// another route, so STREAM and TILE agree within the bounds of the reference, not bit for bit.
// Rules: no atomics; every output element is owned by one thread or one workgroup, which sums in a fixed order (block reductions are
// trees over the thread index, wave reductions butterflies over the lane index); launch geometry depends on sizes only; every vector
// has its own accumulators, so a column's bits do not depend on what else is in its group, its chunk or the batch.
// Host: no checks of its own -- gpmpc_lps_step is reached through the dispatcher of linprop.hip (gpmpc_lp_step) on a checked model; the
// kernels take the hyper-parameters GP by GP as LpHyp (linprop_internal.h), which linprop_fc.hip's kernels take too.
// Cost of the row block: colpart holds np / LPS_RB partial vectors per (column, GP): at N = 2048, LPS_RB = 32 that is 1 MiB per vector,
// written and read once per step (1/8 of a per-GP Kinv per column of the group on top of the one read of Kinv).
#include <cmath>
#include <cstdint>
#include "linprop_internal.h"   // LpTail, LpHyp, LpIn, lp_z

#define LPS_COLS GPMPC_LINPROP_STREAM_COLS
#define LPS_RB 32                   // rows of a workgroup: N = 2048, ds = 4 gives 64 x 4 = 256 workgroups per group of vectors
#define LPS_RW (LPS_RB / 4)         // rows of a wave
#define LPS_CHUNK 16                // columns per set of launches: bounds colpart at 16 ds (np / 32) np doubles
#define LPS_NV (1 + GPMPC_MAX_D)
static_assert(LPS_COLS == 4, "the lane maps of k_lps_quad are written for four vectors");

// the tree over the thread index: s[v][0] = sum of s[v][0 ... 255], the same association for every v and every call
template <int NV>
static __device__ __forceinline__ void lps_block_sum(double (*s)[256], int t) {
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h)
#pragma unroll
            for (int v = 0; v < NV; ++v) s[v][t] = s[v][t] + s[v][t + h];
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lps_kstar(int n, int np, int D, int ds, const double* __restrict__ X, LpIn I,
                                                    const double* __restrict__ beta, LpHyp Hy, double* __restrict__ ks,
                                                    double* __restrict__ kpart) {
    __shared__ double s_p[LPS_NV][256];
    const int t = threadIdx.x, i = blockIdx.x * 256 + t, a = blockIdx.y, c = blockIdx.z;
    const size_t f = (size_t)c * ds + a;
    double d2 = 0.0, dd[GPMPC_MAX_D];
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) {
        const double u = (i < n && d < D) ? X[(size_t)i * D + d] - lp_z(I, c, d, ds) : 0.0;
        const double il = d < D ? Hy.ilam[a][d] : 0.0;
        d2 = fma(u * u, il, d2);
        dd[d] = u * il;
    }
    const double k = i < n ? Hy.sf2[a] * exp(-0.5 * d2) : 0.0;
    if (i < np) ks[f * np + i] = k;                      // (np is a multiple of 128, the grid of 256)
    const double bk = i < n ? beta[(size_t)i * ds + a] * k : 0.0;
    s_p[0][t] = bk;
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) s_p[1 + d][t] = bk * dd[d];
    lps_block_sum<LPS_NV>(s_p, t);
    if (t < LPS_NV) kpart[(f * gridDim.x + blockIdx.x) * LPS_NV + t] = s_p[t][0];
}

// slot s of group z: the vector it stands for, or -1
static __device__ __forceinline__ long lps_vec(int shared, int ds, int a, int z, int s, int cn) {
    if (shared) { const long f = (long)z * LPS_COLS + s; return f < (long)cn * ds ? f : -1; }
    const int c = z * LPS_COLS + s;
    return c < cn ? (long)c * ds + a : -1;
}

template <bool VEC>
static __device__ __forceinline__ double2 lps_load2(const double* __restrict__ row, int i, int n) {
    double2 v;
    if (VEC && i + 1 < n) return *reinterpret_cast<const double2*>(row + i);
    v.x = i < n ? row[i] : 0.0;
    v.y = i + 1 < n ? row[i + 1] : 0.0;
    return v;
}

// VEC: rows are 16-byte aligned (base, ld and gp_stride even): the same arithmetic either way.
template <bool JAC, bool VEC>
__global__ __launch_bounds__(256) void k_lps_quad(int n, int np, int ds, int cn, int shared, const double* __restrict__ Kinv, size_t ld,
                                                   size_t gp_stride, const double* __restrict__ ks, double* __restrict__ y,
                                                   double* __restrict__ qpart, double* __restrict__ colpart) {
    __shared__ double s_kj[LPS_RB][LPS_COLS], s_y[LPS_RB][LPS_COLS];
    __shared__ double s_col[JAC ? 4 : 1][LPS_COLS][JAC ? 128 : 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int rb = blockIdx.x, a = blockIdx.y, z = blockIdx.z, nrb = gridDim.x;
    const int j0 = rb * LPS_RB, jw = j0 + w * LPS_RW;
    const double* __restrict__ K = Kinv + (shared ? (size_t)0 : (size_t)a * gp_stride);
    long f[LPS_COLS];
#pragma unroll
    for (int s = 0; s < LPS_COLS; ++s) f[s] = lps_vec(shared, ds, a, z, s, cn);
    if (f[0] < 0) return;                                // (a whole group beyond the vectors: the grid is rounded up in the shared case only)
    if (t < LPS_RB * LPS_COLS) {
        const int r = t >> 2, s = t & 3;
        const long fs = lps_vec(shared, ds, a, z, s, cn);
        s_kj[r][s] = (fs >= 0 && j0 + r < np) ? ks[(size_t)fs * np + j0 + r] : 0.0;
    }
    __syncthreads();
    double racc[LPS_RW][LPS_COLS] = {};
    double2 kv[LPS_RW], kn[LPS_RW];
    auto fetch = [&](int i, double2* dst) {
#pragma unroll
        for (int r = 0; r < LPS_RW; ++r) {
            dst[r].x = 0.0; dst[r].y = 0.0;
            if (jw + r < n) dst[r] = lps_load2<VEC>(K + (size_t)(jw + r) * ld, i, n);
        }
    };
    fetch(2 * lane, kv);
    for (int i0 = 0; i0 < np; i0 += 128) {
        const int i = i0 + 2 * lane;
        if (i0 + 128 < np) fetch(i + 128, kn);           // the next chunk's rows travel while this one is multiplied
        double2 kx[LPS_COLS];
#pragma unroll
        for (int s = 0; s < LPS_COLS; ++s) {
            kx[s].x = 0.0; kx[s].y = 0.0;
            if (f[s] >= 0) kx[s] = *reinterpret_cast<const double2*>(ks + (size_t)f[s] * np + i);
        }
        double2 cacc[LPS_COLS];
#pragma unroll
        for (int s = 0; s < LPS_COLS; ++s) { cacc[s].x = 0.0; cacc[s].y = 0.0; }
#pragma unroll
        for (int r = 0; r < LPS_RW; ++r)
#pragma unroll
            for (int s = 0; s < LPS_COLS; ++s) {
                racc[r][s] = fma(kv[r].x, kx[s].x, racc[r][s]);
                racc[r][s] = fma(kv[r].y, kx[s].y, racc[r][s]);
                if (JAC) {
                    const double kj = s_kj[w * LPS_RW + r][s];
                    cacc[s].x = fma(kv[r].x, kj, cacc[s].x);
                    cacc[s].y = fma(kv[r].y, kj, cacc[s].y);
                }
            }
        if (JAC) {
#pragma unroll
            for (int s = 0; s < LPS_COLS; ++s) { s_col[w][s][2 * lane] = cacc[s].x; s_col[w][s][2 * lane + 1] = cacc[s].y; }
            __syncthreads();
#pragma unroll
            for (int e = t; e < LPS_COLS * 128; e += 256) {
                const int s = e >> 7, il = e & 127;
                const long fs = lps_vec(shared, ds, a, z, s, cn);
                if (fs >= 0) colpart[((size_t)fs * nrb + rb) * np + i0 + il] = ((s_col[0][s][il] + s_col[1][s][il]) + s_col[2][s][il]) + s_col[3][s][il];
            }
            __syncthreads();
        }
        if (i0 + 128 < np)
#pragma unroll
            for (int r = 0; r < LPS_RW; ++r) kv[r] = kn[r];
    }
    // the wave's rows: a butterfly over the lanes (every lane ends with the sum, in the same association)
#pragma unroll
    for (int r = 0; r < LPS_RW; ++r)
#pragma unroll
        for (int s = 0; s < LPS_COLS; ++s) {
            double v = racc[r][s];
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
            if (lane == 0) s_y[w * LPS_RW + r][s] = v;
        }
    __syncthreads();
    if (t < LPS_RB * LPS_COLS) {
        const int r = t >> 2, s = t & 3;
        const long fs = lps_vec(shared, ds, a, z, s, cn);
        if (fs >= 0 && j0 + r < np) y[(size_t)fs * np + j0 + r] = s_y[r][s];
    }
    if (t < LPS_COLS) {
        const long fs = lps_vec(shared, ds, a, z, t, cn);
        double q = 0.0;
        for (int r = 0; r < LPS_RB; ++r) q = fma(s_kj[r][t], s_y[r][t], q);
        if (fs >= 0) qpart[(size_t)fs * nrb + rb] = q;
    }
}

// one thread per vector f = c ds + a: mu', v', and g (with the nominal weights) for the Jacobian passes.  The tail of k_lp_sums.
__global__ __launch_bounds__(256) void k_lps_sums(int cn, int nbk, int nrb, int D, int ds, LpHyp Hy, LpTail M, LpIn I,
                                                   const double* __restrict__ kpart, const double* __restrict__ qpart,
                                                   double* __restrict__ out_mu, double* __restrict__ out_var, size_t os,
                                                   double* __restrict__ gbuf) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= (long)cn * ds) return;
    const int c = (int)(f / ds), a = (int)(f - (long)c * ds);
    double q = 0.0, m = 0.0;
    for (int b = 0; b < nrb; ++b) q += qpart[(size_t)f * nrb + b];
    for (int b = 0; b < nbk; ++b) m += kpart[((size_t)f * nbk + b) * LPS_NV];
    if (M.has_nominal) {
        double lin = M.nom_b[a];
        for (int d = 0; d < D; ++d) lin = fma(M.nom_w[a * D + d], lp_z(I, c, d, ds), lin);
        m += lin;
    }
    double lin2 = 0.0;
    for (int d = 0; d < D; ++d) {
        double g = 0.0;
        for (int b = 0; b < nbk; ++b) g += kpart[((size_t)f * nbk + b) * LPS_NV + 1 + d];
        if (M.has_nominal) g += M.nom_w[a * D + d];
        const double S = d < ds ? I.var[(size_t)c * I.xs + d] : M.action_var[d - ds];
        lin2 = fma(g * g, S, lin2);
        if (gbuf) gbuf[(size_t)f * GPMPC_MAX_D + d] = g;
    }
    out_mu[(size_t)c * os + a] = m;
    out_var[(size_t)c * os + a] = ((Hy.sf2[a] - q) + lin2) + M.process_var[a];
}

// grid (np / 256, ds, columns).  Reads ks back (no second exp).
__global__ __launch_bounds__(256) void k_lps_grad(int n, int np, int nrb, int D, int ds, const double* __restrict__ X, LpIn I,
                                                   const double* __restrict__ beta, LpHyp Hy, LpTail M, const double* __restrict__ ks,
                                                   const double* __restrict__ y, const double* __restrict__ colpart,
                                                   const double* __restrict__ gbuf, double* __restrict__ jpart) {
    __shared__ double s_p[2 * GPMPC_MAX_D][256];
    const int t = threadIdx.x, i = blockIdx.x * 256 + t, a = blockIdx.y, c = blockIdx.z;
    const size_t f = (size_t)c * ds + a;
    const bool in = i < np;                              // (np is a multiple of 128, the grid of 256)
    double ct = 0.0;
    if (in)
        for (int b = 0; b < nrb; ++b) ct += colpart[(f * nrb + b) * np + i];
    const double k = in ? ks[f * np + i] : 0.0;
    const double r = in ? y[f * np + i] + ct : 0.0;      // r = Kinv k + Kinv^T k
    const double rk = r * k, bk = i < n ? beta[(size_t)i * ds + a] * k : 0.0;
    double dd[GPMPC_MAX_D], wl[GPMPC_MAX_D], dw = 0.0;
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) {
        const bool on = d < D;
        const double il = on ? Hy.ilam[a][d] : 0.0;
        dd[d] = (i < n && on) ? (X[(size_t)i * D + d] - lp_z(I, c, d, ds)) * il : 0.0;
        const double S = on ? (d < ds ? I.var[(size_t)c * I.xs + d] : M.action_var[d - ds]) : 0.0;
        const double wd = on ? gbuf[f * GPMPC_MAX_D + d] * S : 0.0;
        wl[d] = wd * il;
        dw = fma(dd[d], wd, dw);
    }
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) {
        s_p[d][t] = rk * dd[d];
        s_p[GPMPC_MAX_D + d][t] = bk * (dd[d] * dw - wl[d]);
    }
    lps_block_sum<2 * GPMPC_MAX_D>(s_p, t);
    if (t < 2 * GPMPC_MAX_D) jpart[(f * gridDim.x + blockIdx.x) * (2 * GPMPC_MAX_D) + t] = s_p[t][0];
}

// one thread per vector: rows mu'_a and v'_a of the column's [2ds][2ds + da] block, every element.  The tail of k_lp_jac.
__global__ __launch_bounds__(256) void k_lps_jac(int cn, int nbk, int D, int ds, const double* __restrict__ jpart,
                                                  const double* __restrict__ gbuf, double* __restrict__ jac, size_t js) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= (long)cn * ds) return;
    const int c = (int)(f / ds), a = (int)(f - (long)c * ds);
    const int nc = ds + D;
    double* __restrict__ rowm = jac + (size_t)c * js + (size_t)a * nc;
    double* __restrict__ rowv = jac + (size_t)c * js + (size_t)(ds + a) * nc;
    for (int d = 0; d < D; ++d) {
        double dq = 0.0, h = 0.0;
        for (int b = 0; b < nbk; ++b) dq += jpart[((size_t)f * nbk + b) * (2 * GPMPC_MAX_D) + d];
        for (int b = 0; b < nbk; ++b) h += jpart[((size_t)f * nbk + b) * (2 * GPMPC_MAX_D) + GPMPC_MAX_D + d];
        const double g = gbuf[(size_t)f * GPMPC_MAX_D + d];
        const int col = d < ds ? d : ds + d;             // (mu, v, u) columns: input j sits at 2 ds + j = ds + d
        rowm[col] = g;
        rowv[col] = 2.0 * h - dq;
        if (d < ds) { rowm[ds + d] = 0.0; rowv[ds + d] = g * g; }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// workspace of a step: ks [C ds][np] | y [C ds][np] | kpart [C ds][nbk][1 + MAX_D] | qpart [C ds][nrb] | with the Jacobian:
// colpart [C ds][nrb][np] | jpart [C ds][nbk][2 MAX_D] | g [C ds][MAX_D];  C = min(columns, LPS_CHUNK)
struct LpsLayout { size_t off_ks, off_y, off_kpart, off_qpart, off_colpart, off_jpart, off_g, total; int np, nbk, nrb, C; };
static LpsLayout lps_layout(const gpmpc_gp_model* m, long ncols, bool want_jac) {
    LpsLayout L;
    gpmpc_carver c;
    L.np = (m->n + 127) / 128 * 128;
    L.nbk = (L.np + 255) / 256;
    L.nrb = L.np / LPS_RB;
    L.C = (int)(ncols < LPS_CHUNK ? ncols : LPS_CHUNK);
    const size_t d = sizeof(double), nf = (size_t)L.C * m->state_dim;
    L.off_ks = c.take(d * nf * L.np);
    L.off_y = c.take(d * nf * L.np);
    L.off_kpart = c.take(d * nf * L.nbk * LPS_NV);
    L.off_qpart = c.take(d * nf * L.nrb);
    L.off_colpart = c.take(want_jac ? d * nf * L.nrb * L.np : 0);
    L.off_jpart = c.take(want_jac ? d * nf * L.nbk * 2 * GPMPC_MAX_D : 0);
    L.off_g = c.take(want_jac ? d * nf * GPMPC_MAX_D : 0);
    L.total = c.total();
    return L;
}

size_t gpmpc_lps_workspace_bytes(const gpmpc_gp_model* m, long ncols, bool want_jac) { return lps_layout(m, ncols, want_jac).total; }

int gpmpc_lps_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                   size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, char* ws, hipStream_t s) {
    const int ds = m->state_dim, D = ds + m->action_dim, n = m->n;
    const LpsLayout L = lps_layout(m, B, jac != nullptr);
    const LpHyp Hy = lp_hyp(m);
    double* ks = (double*)(ws + L.off_ks);
    double* y = (double*)(ws + L.off_y);
    double* kpart = (double*)(ws + L.off_kpart);
    double* qpart = (double*)(ws + L.off_qpart);
    double* colpart = (double*)(ws + L.off_colpart);
    double* jpart = (double*)(ws + L.off_jpart);
    double* gbuf = jac ? (double*)(ws + L.off_g) : nullptr;
    const int shared = m->gp_stride == 0;
    const bool vec = ((uintptr_t)m->Kinv % 16 == 0) && m->ld % 2 == 0 && m->gp_stride % 2 == 0;
    for (long c0 = 0; c0 < B; c0 += L.C) {
        const int cn = (int)(B - c0 < L.C ? B - c0 : L.C);
        const int ngroups = shared ? (cn * ds + LPS_COLS - 1) / LPS_COLS : (cn + LPS_COLS - 1) / LPS_COLS;
        LpIn I;
        I.mu = mu_prev + (size_t)c0 * xs; I.var = var_prev + (size_t)c0 * xs; I.U = U_t ? U_t + (size_t)c0 * us : nullptr;
        I.xs = xs; I.us = us;
        const dim3 gv(L.nbk, ds, cn), gq(L.nrb, shared ? 1 : ds, ngroups), gt((unsigned)(((long)cn * ds + 255) / 256));
        hipLaunchKernelGGL(k_lps_kstar, gv, dim3(256), 0, s, n, L.np, D, ds, m->X, I, m->beta, Hy, ks, kpart);
        auto quad = jac ? (vec ? k_lps_quad<true, true> : k_lps_quad<true, false>) : (vec ? k_lps_quad<false, true> : k_lps_quad<false, false>);
        hipLaunchKernelGGL(quad, gq, dim3(256), 0, s, n, L.np, ds, cn, shared, m->Kinv, m->ld, m->gp_stride, (const double*)ks, y, qpart, colpart);
        hipLaunchKernelGGL(k_lps_sums, gt, dim3(256), 0, s, cn, L.nbk, L.nrb, D, ds, Hy, tail, I, (const double*)kpart, (const double*)qpart,
                           out_mu + (size_t)c0 * os, out_var + (size_t)c0 * os, os, gbuf);
        if (jac) {
            hipLaunchKernelGGL(k_lps_grad, gv, dim3(256), 0, s, n, L.np, L.nrb, D, ds, m->X, I, m->beta, Hy, tail, (const double*)ks,
                               (const double*)y, (const double*)colpart, (const double*)gbuf, jpart);
            hipLaunchKernelGGL(k_lps_jac, gt, dim3(256), 0, s, cn, L.nbk, D, ds, (const double*)jpart, (const double*)gbuf,
                               jac + (size_t)c0 * js, js);
        }
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
