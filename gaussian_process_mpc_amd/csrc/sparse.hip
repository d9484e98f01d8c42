// Sparse GP (FITC inducing points) in the whitened form: everything that produces (alpha, Q) for gpmpc_pack_build_beta(X := Z, beta := alpha,
// Ky_inv := Q).  Formulas, layouts and refusals: include/gpmpc.h, "Sparse GP"; why whitened: DESIGN.md section 3h.
//
//   W = chol(k(Z,Z) + jitter I)^-1 (lower triangular, from the caller)       v_n = W k(Z, x_n)       Lambda_n = sigma_f^2 + noise_var - |v_n|^2
//   G = sum_n v_n v_n^T / Lambda_n      r = sum_n v_n y_n^T / Lambda_n        B = I + G, Binv = B^-1 (from the caller)
//   alpha = W^T Binv r                  Q = W^T (I - Binv) W
// and the O(M^2) rank-one steps of one observation: append, remove and replace (remove + append in one pass over G, Binv, Q).
//
// Rules every kernel here keeps: no atomics; every output element is owned by one workgroup, which sums in a fixed order; launch geometry
// depends on sizes only; symmetric outputs are written once per pair (i, j) and mirrored, so they are symmetric bit for bit.
#include <hip/hip_runtime.h>
#include <atomic>
#include "gpmpc_internal.h"
#include "tile_stage.h"    // SP_T, SP_KB, sp_stage<MF>: the 64 x 64 x 16 LDS stage (shared with particles.hip)

#define SP_DEFAULT_CHUNK 4096

struct SparseHyp { double ilam[GPMPC_MAX_D]; double sf2; double kappa; };      // 1 / lambda_d, sigma_f^2, sigma_f^2 + noise_var

static __device__ __forceinline__ double sp_kval(const double* __restrict__ z, const double* __restrict__ x, int D, const SparseHyp& H) {
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) { const double t = z[d] - x[d]; d2 = fma(t * t, H.ilam[d], d2); }
    return H.sf2 * exp(-0.5 * d2);
}
// NaN-propagating minimum (Lambda is a cancelling difference that may come out NaN: it must be seen, not dropped as fmin would)
static __device__ __forceinline__ double sp_min(double a, double b) { return (a < b || a != a) ? a : b; }

// lower-triangular tile p -> (ti, tj), tj <= ti
static __device__ __forceinline__ void sp_tri(int p, int* ti, int* tj) {
    int t = 0;
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    *ti = t; *tj = p - t * (t + 1) / 2;
}

// ---------------------------------------------------------------------------
// accumulate, launch 1: V[i][j] = sum_{l <= i} W[i][l] k(z_l, x_{n0 + j}) for one chunk of rows, kernel values generated on the fly;
// columns j >= cn of the (64-padded) chunk are written as zero.  Workgroup (bj, bi) owns the 64 x 64 tile and also the partial sums
// sq[bi][j] = sum_{i in tile} V[i][j]^2 (a fixed order).  Only l < 64 (bi + 1) is visited: W is lower triangular.
// ---------------------------------------------------------------------------
template <bool MF>
__global__ __launch_bounds__(256) void k_sparse_v(int cn, int D, int M, const double* __restrict__ X, const double* __restrict__ Z,
                                                   const double* __restrict__ W, size_t ld_w, SparseHyp H, double* __restrict__ V, int ldv,
                                                   double* __restrict__ sq) {
    __shared__ double s_w[SP_KB][SP_T + 1], s_k[SP_KB][SP_T + 1], s_x[SP_T][GPMPC_MAX_D];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int j0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T;
    for (int e = t; e < SP_T * D; e += 256) {
        const int j = e / D, d = e - j * D;
        s_x[j][d] = (j0 + j < cn) ? X[(size_t)(j0 + j) * D + d] : 0.0;
    }
    double acc[4][4] = {};
    const int lend = min(M, i0 + SP_T);
    for (int l0 = 0; l0 < lend; l0 += SP_KB) {
        __syncthreads();
        for (int e = t; e < SP_KB * SP_T; e += 256) {
            const int i = e >> 4, k = e & 15;            // W tile: row i0 + i, column l0 + k (k fastest: consecutive addresses)
            const int gi = i0 + i, gl = l0 + k;
            s_w[k][i] = (gi < M && gl <= gi) ? W[(size_t)gi * ld_w + gl] : 0.0;
            const int kk = e >> 6, j = e & 63;           // kernel tile: inducing point l0 + kk, data column j0 + j
            s_k[kk][j] = (l0 + kk < M && j0 + j < cn) ? sp_kval(Z + (size_t)(l0 + kk) * D, s_x[j], D, H) : 0.0;
        }
        __syncthreads();
        sp_stage<MF>(s_w, s_k, tx, ty, acc);
    }
    __syncthreads();                                     // (s_w is free now: it takes the per-thread sums of squares, [ty][column])
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        double p = 0.0;
#pragma unroll
        for (int qa = 0; qa < 4; ++qa) {
            const int i = i0 + sp_row<MF>(ty, qa), j = j0 + tx + 16 * qb;
            const double v = sp_acc<MF>(acc, qa, qb);
            if (i < M) V[(size_t)i * ldv + j] = v;
            p = fma(v, v, p);                            // the thread's four rows of this column (rows >= M hold zero)
        }
        s_w[ty][tx + 16 * qb] = p;
    }
    __syncthreads();
    if (t < SP_T) {
        double s = 0.0;
        for (int y = 0; y < 16; ++y) s += s_w[y][t];
        sq[(size_t)blockIdx.y * ldv + j0 + t] = s;
    }
}

// accumulate, launch 2 (ONE workgroup): Lambda_j = kappa - sum_b sq[b][j] (b ascending), winv[j] = 1 / Lambda_j (0 for the padding columns),
// stats = {rows accumulated, min Lambda}
__global__ __launch_bounds__(256) void k_sparse_lambda(int cn, int cnp, int nbi, int ldv, const double* __restrict__ sq, double kappa,
                                                        double* __restrict__ winv, int fresh, double* __restrict__ stats) {
    __shared__ double s_m[256];
    double m = HUGE_VAL;
    for (int j = threadIdx.x; j < cnp; j += 256) {
        double s = 0.0;
        for (int b = 0; b < nbi; ++b) s += sq[(size_t)b * ldv + j];
        const double lam = kappa - s;
        winv[j] = j < cn ? 1.0 / lam : 0.0;
        if (j < cn) m = sp_min(lam, m);
    }
    s_m[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 256; ++q) m = sp_min(s_m[q], m);
        if (fresh) { stats[0] = (double)cn; stats[1] = m; }
        else { stats[0] += (double)cn; stats[1] = sp_min(m, stats[1]); }
    }
}

// accumulate, launch 3: workgroups [0, ntri) own the lower-triangular 64 x 64 tiles of G (G_new = G_old + sum_j V[i][j] winv[j] V[i'][j], j
// ascending; every pair (i, i') is computed once and written to both places); workgroups ntri + b own rows 64 b ... of r
// (r_new[i][a] = r_old[i][a] + sum_j V[i][j] winv[j] Y[j][a], each column a by itself).
template <bool MF>
__global__ __launch_bounds__(256) void k_sparse_gr(int cn, int cnp, int M, int nt, int ntri, const double* __restrict__ V, int ldv,
                                                    const double* __restrict__ winv, const double* __restrict__ Y, size_t ld_y, int fresh,
                                                    double* __restrict__ G, double* __restrict__ r) {
    __shared__ double s_a[SP_KB][SP_T + 1], s_b[SP_KB][SP_T + 1];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < ntri) {
        int ti, tj;
        sp_tri(blockIdx.x, &ti, &tj);
        const int i0 = ti * SP_T, c0 = tj * SP_T, tx = t & 15, ty = t >> 4;
        double acc[4][4] = {};
        // the next stage's operands travel in registers while this stage is multiplied (with a handful of tiles nothing else hides the loads)
        double pa[4], pb[4];
        auto fetch = [&](int j0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = t + 256 * q, i = e >> 4, k = e & 15;
                const double w = winv[j0 + k];
                pa[q] = (i0 + i < M) ? V[(size_t)(i0 + i) * ldv + j0 + k] * w : 0.0;
                pb[q] = (c0 + i < M) ? V[(size_t)(c0 + i) * ldv + j0 + k] : 0.0;
            }
        };
        fetch(0);
        for (int j0 = 0; j0 < cnp; j0 += SP_KB) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = t + 256 * q, i = e >> 4, k = e & 15;
                s_a[k][i] = pa[q];
                s_b[k][i] = pb[q];
            }
            __syncthreads();
            if (j0 + SP_KB < cnp) fetch(j0 + SP_KB);
            sp_stage<MF>(s_a, s_b, tx, ty, acc);
        }
#pragma unroll
        for (int qa = 0; qa < 4; ++qa)
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) {
                const int i = i0 + sp_row<MF>(ty, qa), c = c0 + tx + 16 * qb;
                if (i < M && c <= i) {
                    const double g = fresh ? sp_acc<MF>(acc, qa, qb) : G[(size_t)i * M + c] + sp_acc<MF>(acc, qa, qb);
                    G[(size_t)i * M + c] = g;
                    G[(size_t)c * M + i] = g;
                }
            }
        return;
    }
    // rows of r: thread (i = t & 63, q = t >> 6) sums the columns j = 16 q ... 16 q + 15 of every 64-column stage
    __shared__ double s_v[SP_T][SP_T + 1], s_y[SP_T][GPMPC_MAX_DS];
    const int i0 = ((int)blockIdx.x - ntri) * SP_T, il = t & 63, q = t >> 6;
    double acc[GPMPC_MAX_DS] = {};
    for (int j0 = 0; j0 < cnp; j0 += SP_T) {
        __syncthreads();
        for (int e = t; e < SP_T * SP_T; e += 256) {
            const int i = e >> 6, j = e & 63;
            s_v[i][j] = (i0 + i < M) ? V[(size_t)(i0 + i) * ldv + j0 + j] : 0.0;
        }
        for (int e = t; e < SP_T * GPMPC_MAX_DS; e += 256) {
            const int j = e >> 3, a = e & 7;
            s_y[j][a] = (a < nt && j0 + j < cn) ? winv[j0 + j] * Y[(size_t)(j0 + j) * ld_y + a] : 0.0;
        }
        __syncthreads();
        for (int j = 16 * q; j < 16 * q + 16; ++j) {
            const double v = s_v[il][j];
#pragma unroll
            for (int a = 0; a < GPMPC_MAX_DS; ++a) acc[a] = fma(v, s_y[j][a], acc[a]);
        }
    }
    __syncthreads();
    double (*s_p)[SP_T][GPMPC_MAX_DS] = (double (*)[SP_T][GPMPC_MAX_DS])&s_v[0][0];      // [4][64][8] = 2048 doubles of the 4160
#pragma unroll
    for (int a = 0; a < GPMPC_MAX_DS; ++a) s_p[q][il][a] = acc[a];
    __syncthreads();
    for (int e = t; e < SP_T * nt; e += 256) {
        const int i = e / nt, a = e - i * nt;
        if (i0 + i < M) {
            const double s = (s_p[0][i][a] + s_p[1][i][a]) + (s_p[2][i][a] + s_p[3][i][a]);
            r[(size_t)(i0 + i) * nt + a] = fresh ? s : r[(size_t)(i0 + i) * nt + a] + s;
        }
    }
}

static int sp_chunk(int chunk) { return chunk == 0 ? SP_DEFAULT_CHUNK : chunk; }

static int sp_check_dims(const char* who, int D, int M, int nt) {
    const char* why = nullptr;
    if (M < 1 || M > GPMPC_SPARSE_MAX_M) why = "M (inducing points) outside 1...GPMPC_SPARSE_MAX_M";
    else if (D < 1 || D > GPMPC_MAX_D) why = "D outside 1...GPMPC_MAX_D";
    else if (nt < 1 || nt > GPMPC_MAX_DS) why = "n_targets outside 1...GPMPC_MAX_DS";
    return why ? gpmpc_refuse(who, "%s", why) : GPMPC_OK;
}

static void sp_hyp(SparseHyp* h, int D, const double* lambdas_host, double sigma_f, double noise_var) {
    memset(h, 0, sizeof(*h));
    for (int d = 0; d < D; ++d) h->ilam[d] = 1.0 / lambdas_host[d];
    h->sf2 = sigma_f * sigma_f;
    h->kappa = h->sf2 + noise_var;
}

// which form of the two N M^2 products gpmpc_sparse_accumulate launches (process-wide; the default is the measured choice)
static std::atomic<int> g_sparse_form{GPMPC_SPARSE_FORM_DEFAULT};

extern "C" int gpmpc_sparse_set_form(int form) {
    if (form != GPMPC_SPARSE_FORM_FMA && form != GPMPC_SPARSE_FORM_MFMA) {
        if (form == -1) return g_sparse_form.load();
        return gpmpc_refuse("gpmpc_sparse_set_form", "form must be GPMPC_SPARSE_FORM_FMA, GPMPC_SPARSE_FORM_MFMA or -1 (query)");
    }
    return g_sparse_form.exchange(form);
}

extern "C" size_t gpmpc_sparse_accumulate_workspace_bytes(int n, int D, int M, int n_targets, int chunk) {
    (void)n; (void)D; (void)n_targets;
    if (M < 1 || M > GPMPC_SPARSE_MAX_M || chunk < 0 || chunk % 64) return 0;
    const size_t c = (size_t)sp_chunk(chunk), nbi = (size_t)(M + SP_T - 1) / SP_T;
    return gpmpc_align256(sizeof(double) * M * c) + gpmpc_align256(sizeof(double) * nbi * c) + gpmpc_align256(sizeof(double) * c);
}

extern "C" int gpmpc_sparse_accumulate(int n, int D, int M, int n_targets, const double* X_dev, const double* Y_dev, size_t ld_y,
                                       const double* Z_dev, const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f,
                                       double noise_var, int chunk, int accumulate, double* G_dev, double* r_dev, double* stats_dev,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1) return gpmpc_refuse("gpmpc_sparse_accumulate", "n < 1");
    if (int rc = sp_check_dims("gpmpc_sparse_accumulate", D, M, n_targets)) return rc;
    if (chunk < 0 || chunk % 64) return gpmpc_refuse("gpmpc_sparse_accumulate", "chunk must be 0 or a positive multiple of 64");
    if (ld_y < (size_t)n_targets) return gpmpc_refuse("gpmpc_sparse_accumulate", "ld_y < n_targets");
    if (ld_w < (size_t)M) return gpmpc_refuse("gpmpc_sparse_accumulate", "ld_w < M");
    if (!X_dev || !Y_dev || !Z_dev || !W_dev || !lambdas_host || !G_dev || !r_dev || !stats_dev || !workspace)
        return gpmpc_refuse("gpmpc_sparse_accumulate", "NULL pointer");
    if (workspace_bytes < gpmpc_sparse_accumulate_workspace_bytes(n, D, M, n_targets, chunk)) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int c = sp_chunk(chunk), nbi = (M + SP_T - 1) / SP_T, ntri = nbi * (nbi + 1) / 2;
    double* V = (double*)workspace;
    double* sq = (double*)((char*)workspace + gpmpc_align256(sizeof(double) * (size_t)M * c));
    double* winv = (double*)((char*)sq + gpmpc_align256(sizeof(double) * (size_t)nbi * c));
    SparseHyp hyp;
    sp_hyp(&hyp, D, lambdas_host, sigma_f, noise_var);
    const bool mfma = g_sparse_form.load() == GPMPC_SPARSE_FORM_MFMA;
    for (int n0 = 0; n0 < n; n0 += c) {
        const int cn = (n - n0 < c) ? n - n0 : c, cnp = (cn + SP_T - 1) / SP_T * SP_T;      // cnp <= c: c is a multiple of 64
        const int fresh = (n0 == 0 && !accumulate) ? 1 : 0;
        if (mfma)
            hipLaunchKernelGGL(k_sparse_v<true>, dim3(cnp / SP_T, nbi), dim3(256), 0, s, cn, D, M, X_dev + (size_t)n0 * D, Z_dev, W_dev, ld_w, hyp, V, c, sq);
        else
            hipLaunchKernelGGL(k_sparse_v<false>, dim3(cnp / SP_T, nbi), dim3(256), 0, s, cn, D, M, X_dev + (size_t)n0 * D, Z_dev, W_dev, ld_w, hyp, V, c, sq);
        hipLaunchKernelGGL(k_sparse_lambda, dim3(1), dim3(256), 0, s, cn, cnp, nbi, c, (const double*)sq, hyp.kappa, winv, fresh, stats_dev);
        if (mfma)
            hipLaunchKernelGGL(k_sparse_gr<true>, dim3(ntri + nbi), dim3(256), 0, s, cn, cnp, M, n_targets, ntri, (const double*)V, c,
                               (const double*)winv, Y_dev + (size_t)n0 * ld_y, ld_y, fresh, G_dev, r_dev);
        else
            hipLaunchKernelGGL(k_sparse_gr<false>, dim3(ntri + nbi), dim3(256), 0, s, cn, cnp, M, n_targets, ntri, (const double*)V, c,
                               (const double*)winv, Y_dev + (size_t)n0 * ld_y, ld_y, fresh, G_dev, r_dev);
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// finish: alpha = W^T (Binv r), Q = W^T (I - Binv) W.  Binv is SYMMETRIC by contract: only its lower triangle is read.
// ---------------------------------------------------------------------------
static __device__ __forceinline__ double sp_binv(const double* __restrict__ Binv, int M, int i, int j) {
    return i >= j ? Binv[(size_t)i * M + j] : Binv[(size_t)j * M + i];
}

// C = (I - Binv) W, all 64 x 64 tiles (i, l); C[i][l] = sum_{i' >= l} (delta_ii' - Binv[i][i']) W[i'][l], i' ascending from the tile's first column
__global__ __launch_bounds__(256) void k_sparse_c(int M, const double* __restrict__ Binv, const double* __restrict__ W, size_t ld_w,
                                                   double* __restrict__ C) {
    __shared__ double s_a[SP_KB][SP_T + 1], s_b[SP_KB][SP_T + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int l0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T;
    double acc[4][4] = {};
    for (int k0 = l0; k0 < M; k0 += SP_KB) {
        __syncthreads();
        for (int e = t; e < SP_KB * SP_T; e += 256) {
            const int i = e >> 4, k = e & 15;
            const int gi = i0 + i, gk = k0 + k;
            s_a[k][i] = (gi < M && gk < M) ? (gi == gk ? 1.0 : 0.0) - sp_binv(Binv, M, gi, gk) : 0.0;
            const int kk = e >> 6, l = e & 63;
            const int g2 = k0 + kk, gl = l0 + l;
            s_b[kk][l] = (g2 < M && gl <= g2) ? W[(size_t)g2 * ld_w + gl] : 0.0;
        }
        __syncthreads();
        sp_stage<false>(s_a, s_b, tx, ty, acc);
    }
#pragma unroll
    for (int qa = 0; qa < 4; ++qa)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const int i = i0 + ty + 16 * qa, l = l0 + tx + 16 * qb;
            if (i < M && l < M) C[(size_t)i * M + l] = acc[qa][qb];
        }
}

// Q[l][l'] = sum_{i >= l} W[i][l] C[i][l'] over the lower-triangular tiles (l >= l'), mirrored
__global__ __launch_bounds__(256) void k_sparse_q(int M, const double* __restrict__ W, size_t ld_w, const double* __restrict__ C,
                                                   double* __restrict__ Q) {
    __shared__ double s_a[SP_KB][SP_T + 1], s_b[SP_KB][SP_T + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    int ti, tj;
    sp_tri(blockIdx.x, &ti, &tj);
    const int l0 = ti * SP_T, c0 = tj * SP_T;
    double acc[4][4] = {};
    for (int k0 = l0; k0 < M; k0 += SP_KB) {
        __syncthreads();
        for (int e = t; e < SP_KB * SP_T; e += 256) {
            const int kk = e >> 6, l = e & 63;
            const int gi = k0 + kk;
            s_a[kk][l] = (gi < M && l0 + l <= gi) ? W[(size_t)gi * ld_w + l0 + l] : 0.0;
            s_b[kk][l] = (gi < M && c0 + l < M) ? C[(size_t)gi * M + c0 + l] : 0.0;
        }
        __syncthreads();
        sp_stage<false>(s_a, s_b, tx, ty, acc);
    }
#pragma unroll
    for (int qa = 0; qa < 4; ++qa)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const int l = l0 + ty + 16 * qa, c = c0 + tx + 16 * qb;
            if (l < M && c <= l) { Q[(size_t)l * M + c] = acc[qa][qb]; Q[(size_t)c * M + l] = acc[qa][qb]; }
        }
}

// T[i][a] = sum_i' Binv[i][i'] r[i'][a]   (one workgroup per row i; every column a by itself)
__global__ __launch_bounds__(256) void k_sparse_t(int M, int nt, const double* __restrict__ Binv, const double* __restrict__ r, double* __restrict__ T) {
    __shared__ double s_scr[16 * GPMPC_MAX_DS], s_out[GPMPC_MAX_DS];
    const int i = blockIdx.x;
    double acc[GPMPC_MAX_DS] = {};
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        const double b = sp_binv(Binv, M, i, k);
#pragma unroll
        for (int a = 0; a < GPMPC_MAX_DS; ++a) acc[a] = fma(b, a < nt ? r[(size_t)k * nt + a] : 0.0, acc[a]);
    }
    block_sum<GPMPC_MAX_DS>(acc, s_scr, s_out);
    if ((int)threadIdx.x < nt) T[(size_t)i * nt + threadIdx.x] = s_out[threadIdx.x];
}

// alpha[l][a] = sum_{i >= l} W[i][l] T[i][a]   (one workgroup per column l of W)
__global__ __launch_bounds__(256) void k_sparse_alpha(int M, int nt, const double* __restrict__ W, size_t ld_w, const double* __restrict__ T,
                                                       double* __restrict__ alpha) {
    __shared__ double s_scr[16 * GPMPC_MAX_DS], s_out[GPMPC_MAX_DS];
    const int l = blockIdx.x;
    double acc[GPMPC_MAX_DS] = {};
    for (int i = l + threadIdx.x; i < M; i += blockDim.x) {
        const double w = W[(size_t)i * ld_w + l];
#pragma unroll
        for (int a = 0; a < GPMPC_MAX_DS; ++a) acc[a] = fma(w, a < nt ? T[(size_t)i * nt + a] : 0.0, acc[a]);
    }
    block_sum<GPMPC_MAX_DS>(acc, s_scr, s_out);
    if ((int)threadIdx.x < nt) alpha[(size_t)l * nt + threadIdx.x] = s_out[threadIdx.x];
}

extern "C" size_t gpmpc_sparse_finish_workspace_bytes(int M, int n_targets) {
    if (M < 1 || M > GPMPC_SPARSE_MAX_M || n_targets < 1 || n_targets > GPMPC_MAX_DS) return 0;
    return gpmpc_align256(sizeof(double) * (size_t)M * M) + gpmpc_align256(sizeof(double) * (size_t)M * n_targets);
}

extern "C" int gpmpc_sparse_finish(int M, int n_targets, const double* W_dev, size_t ld_w, const double* Binv_dev, const double* r_dev,
                                   double* alpha_dev, double* Q_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = sp_check_dims("gpmpc_sparse_finish", 1, M, n_targets)) return rc;
    if (ld_w < (size_t)M) return gpmpc_refuse("gpmpc_sparse_finish", "ld_w < M");
    if (!W_dev || !Binv_dev || !r_dev || !alpha_dev || !Q_dev || !workspace) return gpmpc_refuse("gpmpc_sparse_finish", "NULL pointer");
    if (workspace_bytes < gpmpc_sparse_finish_workspace_bytes(M, n_targets)) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nb = (M + SP_T - 1) / SP_T;
    double* C = (double*)workspace;
    double* T = (double*)((char*)workspace + gpmpc_align256(sizeof(double) * (size_t)M * M));
    hipLaunchKernelGGL(k_sparse_c, dim3(nb, nb), dim3(256), 0, s, M, Binv_dev, W_dev, ld_w, C);
    hipLaunchKernelGGL(k_sparse_q, dim3(nb * (nb + 1) / 2), dim3(256), 0, s, M, W_dev, ld_w, (const double*)C, Q_dev);
    hipLaunchKernelGGL(k_sparse_t, dim3(M), dim3(256), 0, s, M, n_targets, Binv_dev, r_dev, T);
    hipLaunchKernelGGL(k_sparse_alpha, dim3(M), dim3(256), 0, s, M, n_targets, W_dev, ld_w, (const double*)T, alpha_dev);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// append of ONE observation (x, y), O(M^2):
//   k = k(Z, x); v = W k; Lambda = kappa - |v|^2; t = Binv v; den = Lambda + v . t; u = W^T t
//   G += v v^T / Lambda; r += v y^T / Lambda; Binv -= t t^T / den; Q += u u^T / den; alpha = W^T (Binv r)
// Six dependent launches: v | t | u | the M x M streams and r | Binv r | alpha.  Scalars (Lambda, den) are re-evaluated by every workgroup
// that needs them, from the same vectors in the same order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sparse_app_v(int D, int M, const double* __restrict__ xnew, const double* __restrict__ Z,
                                                       const double* __restrict__ W, size_t ld_w, SparseHyp H, double* __restrict__ v) {
    __shared__ double s_scr[16], s_out[1];
    const int i = blockIdx.x;
    double acc[1] = {0.0};
    for (int l = threadIdx.x; l <= i; l += blockDim.x) acc[0] = fma(W[(size_t)i * ld_w + l], sp_kval(Z + (size_t)l * D, xnew, D, H), acc[0]);
    block_sum<1>(acc, s_scr, s_out);
    if (threadIdx.x == 0) v[i] = s_out[0];
}

__global__ __launch_bounds__(256) void k_sparse_app_t(int M, const double* __restrict__ Binv, const double* __restrict__ v, double* __restrict__ tv) {
    __shared__ double s_scr[16], s_out[1];
    const int i = blockIdx.x;
    double acc[1] = {0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) acc[0] = fma(sp_binv(Binv, M, i, k), v[k], acc[0]);
    block_sum<1>(acc, s_scr, s_out);
    if (threadIdx.x == 0) tv[i] = s_out[0];
}

__global__ __launch_bounds__(256) void k_sparse_app_u(int M, const double* __restrict__ W, size_t ld_w, const double* __restrict__ tv, double* __restrict__ u) {
    __shared__ double s_scr[16], s_out[1];
    const int l = blockIdx.x;
    double acc[1] = {0.0};
    for (int i = l + threadIdx.x; i < M; i += blockDim.x) acc[0] = fma(W[(size_t)i * ld_w + l], tv[i], acc[0]);
    block_sum<1>(acc, s_scr, s_out);
    if (threadIdx.x == 0) u[l] = s_out[0];
}

// grid ((M + 255) / 256, M): row i, columns j.  The products v_i v_j, t_i t_j, u_i u_j commute exactly, so the updated matrices stay symmetric bit
// for bit.  Column block 0 of row i also owns r[i][:]; workgroup (0, 0) the stats.
__global__ __launch_bounds__(256) void k_sparse_app_fill(int M, int nt, const double* __restrict__ v, const double* __restrict__ tv,
                                                          const double* __restrict__ u, const double* __restrict__ ynew, double kappa,
                                                          double* __restrict__ G, double* __restrict__ r, double* __restrict__ Binv,
                                                          double* __restrict__ Q, double* __restrict__ stats) {
    __shared__ double s_scr[32], s_out[2];
    double acc[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) { acc[0] = fma(v[k], v[k], acc[0]); acc[1] = fma(v[k], tv[k], acc[1]); }
    block_sum<2>(acc, s_scr, s_out);
    const double lam = kappa - s_out[0], den = lam + s_out[1];
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (blockIdx.x == 0 && (int)threadIdx.x < nt) {
        const int a = threadIdx.x;
        r[(size_t)i * nt + a] += v[i] * ynew[a] / lam;
    }
    if (blockIdx.x == 0 && i == 0 && threadIdx.x == 0) { stats[0] += 1.0; stats[1] = sp_min(lam, stats[1]); }
    if (j >= M) return;
    const size_t o = (size_t)i * M + j;
    G[o] += (v[i] * v[j]) / lam;
    Binv[o] -= (tv[i] * tv[j]) / den;
    Q[o] += (u[i] * u[j]) / den;
}

extern "C" size_t gpmpc_sparse_append_workspace_bytes(int M, int n_targets) {
    if (M < 1 || M > GPMPC_SPARSE_MAX_M || n_targets < 1 || n_targets > GPMPC_MAX_DS) return 0;
    return gpmpc_align256(sizeof(double) * 3 * (size_t)M) + gpmpc_align256(sizeof(double) * (size_t)M * n_targets);
}

extern "C" int gpmpc_sparse_append(int D, int M, int n_targets, const double* x_new_dev, const double* y_new_dev, const double* Z_dev,
                                   const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f, double noise_var,
                                   double* G_dev, double* r_dev, double* Binv_dev, double* Q_dev, double* alpha_dev, double* stats_dev,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = sp_check_dims("gpmpc_sparse_append", D, M, n_targets)) return rc;
    if (ld_w < (size_t)M) return gpmpc_refuse("gpmpc_sparse_append", "ld_w < M");
    if (!x_new_dev || !y_new_dev || !Z_dev || !W_dev || !lambdas_host || !G_dev || !r_dev || !Binv_dev || !Q_dev || !alpha_dev || !stats_dev ||
        !workspace)
        return gpmpc_refuse("gpmpc_sparse_append", "NULL pointer");
    if (workspace_bytes < gpmpc_sparse_append_workspace_bytes(M, n_targets)) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* v = (double*)workspace; double* tv = v + M; double* u = tv + M;
    double* T = (double*)((char*)workspace + gpmpc_align256(sizeof(double) * 3 * (size_t)M));
    SparseHyp hyp;
    sp_hyp(&hyp, D, lambdas_host, sigma_f, noise_var);
    hipLaunchKernelGGL(k_sparse_app_v, dim3(M), dim3(256), 0, s, D, M, x_new_dev, Z_dev, W_dev, ld_w, hyp, v);
    hipLaunchKernelGGL(k_sparse_app_t, dim3(M), dim3(256), 0, s, M, (const double*)Binv_dev, (const double*)v, tv);
    hipLaunchKernelGGL(k_sparse_app_u, dim3(M), dim3(256), 0, s, M, W_dev, ld_w, (const double*)tv, u);
    hipLaunchKernelGGL(k_sparse_app_fill, dim3((M + 255) / 256, M), dim3(256), 0, s, M, n_targets, (const double*)v, (const double*)tv,
                       (const double*)u, y_new_dev, hyp.kappa, G_dev, r_dev, Binv_dev, Q_dev, stats_dev);
    hipLaunchKernelGGL(k_sparse_t, dim3(M), dim3(256), 0, s, M, n_targets, (const double*)Binv_dev, (const double*)r_dev, T);
    hipLaunchKernelGGL(k_sparse_alpha, dim3(M), dim3(256), 0, s, M, n_targets, W_dev, ld_w, (const double*)T, alpha_dev);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// removal of ONE observation (x, y) the state holds, O(M^2): the inverse of the append.
//   v = W k(Z, x); Lambda = kappa - |v|^2; t = Binv v; den = Lambda - v . t; u = W^T t
//   G -= v v^T / Lambda; r -= v y^T / Lambda; Binv += t t^T / den; Q -= u u^T / den; alpha = W^T (Binv r); stats[0] -= 1
// den cancels (den / Lambda = 1 - v . t / Lambda is small when the row carries much of what the state knows); nothing is clamped.
// The launches are the append's with another fill: v | t | u | the M x M streams and r | Binv r | alpha.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sparse_rem_fill(int M, int nt, const double* __restrict__ v, const double* __restrict__ tv,
                                                          const double* __restrict__ u, const double* __restrict__ yold, double kappa,
                                                          double* __restrict__ G, double* __restrict__ r, double* __restrict__ Binv,
                                                          double* __restrict__ Q, double* __restrict__ stats) {
    __shared__ double s_scr[32], s_out[2];
    double acc[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) { acc[0] = fma(v[k], v[k], acc[0]); acc[1] = fma(v[k], tv[k], acc[1]); }
    block_sum<2>(acc, s_scr, s_out);
    const double lam = kappa - s_out[0], den = lam - s_out[1];
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (blockIdx.x == 0 && (int)threadIdx.x < nt) {
        const int a = threadIdx.x;
        r[(size_t)i * nt + a] -= v[i] * yold[a] / lam;
    }
    if (blockIdx.x == 0 && i == 0 && threadIdx.x == 0) stats[0] -= 1.0;      // (stats[1] stays: a lower bound on the held rows' Lambda from here on)
    if (j >= M) return;
    const size_t o = (size_t)i * M + j;
    G[o] -= (v[i] * v[j]) / lam;
    Binv[o] += (tv[i] * tv[j]) / den;
    Q[o] -= (u[i] * u[j]) / den;
}

// the argument checks the rank-one entry points share (after sp_check_dims)
static int sp_check_rank_one(const char* who, int M, size_t ld_w, bool pointers) {
    if (ld_w < (size_t)M) return gpmpc_refuse(who, "ld_w < M");
    if (!pointers) return gpmpc_refuse(who, "NULL pointer");
    return GPMPC_OK;
}

extern "C" size_t gpmpc_sparse_remove_workspace_bytes(int M, int n_targets) { return gpmpc_sparse_append_workspace_bytes(M, n_targets); }

extern "C" int gpmpc_sparse_remove(int D, int M, int n_targets, const double* x_old_dev, const double* y_old_dev, const double* Z_dev,
                                   const double* W_dev, size_t ld_w, const double* lambdas_host, double sigma_f, double noise_var,
                                   double* G_dev, double* r_dev, double* Binv_dev, double* Q_dev, double* alpha_dev, double* stats_dev,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = sp_check_dims("gpmpc_sparse_remove", D, M, n_targets)) return rc;
    if (int rc = sp_check_rank_one("gpmpc_sparse_remove", M, ld_w, x_old_dev && y_old_dev && Z_dev && W_dev && lambdas_host && G_dev && r_dev &&
                                   Binv_dev && Q_dev && alpha_dev && stats_dev && workspace))
        return rc;
    if (workspace_bytes < gpmpc_sparse_remove_workspace_bytes(M, n_targets)) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* v = (double*)workspace; double* tv = v + M; double* u = tv + M;
    double* T = (double*)((char*)workspace + gpmpc_align256(sizeof(double) * 3 * (size_t)M));
    SparseHyp hyp;
    sp_hyp(&hyp, D, lambdas_host, sigma_f, noise_var);
    hipLaunchKernelGGL(k_sparse_app_v, dim3(M), dim3(256), 0, s, D, M, x_old_dev, Z_dev, W_dev, ld_w, hyp, v);
    hipLaunchKernelGGL(k_sparse_app_t, dim3(M), dim3(256), 0, s, M, (const double*)Binv_dev, (const double*)v, tv);
    hipLaunchKernelGGL(k_sparse_app_u, dim3(M), dim3(256), 0, s, M, W_dev, ld_w, (const double*)tv, u);
    hipLaunchKernelGGL(k_sparse_rem_fill, dim3((M + 255) / 256, M), dim3(256), 0, s, M, n_targets, (const double*)v, (const double*)tv,
                       (const double*)u, y_old_dev, hyp.kappa, G_dev, r_dev, Binv_dev, Q_dev, stats_dev);
    hipLaunchKernelGGL(k_sparse_t, dim3(M), dim3(256), 0, s, M, n_targets, (const double*)Binv_dev, (const double*)r_dev, T);
    hipLaunchKernelGGL(k_sparse_alpha, dim3(M), dim3(256), 0, s, M, n_targets, W_dev, ld_w, (const double*)T, alpha_dev);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// replacement of one held observation (x_o, y_o) by (x_n, y_n) in ONE pass over G, Binv, Q (the hot path of a full window).  The removed
// state is never formed: with t_o = Binv v_o, s_n = Binv v_n and den_o = Lambda_o - v_o . t_o, the removed state's Binv' v_n is
//   t_n = s_n + c t_o,  c = (t_o . v_n) / den_o,  den_n = Lambda_n + v_n . t_n,  u_o = W^T t_o,  u_n = W^T t_n
//   G = (G - v_o v_o^T / Lambda_o) + v_n v_n^T / Lambda_n            r likewise with y_o, y_n
//   Binv = (Binv + t_o t_o^T / den_o) - t_n t_n^T / den_n            Q = (Q - u_o u_o^T / den_o) + u_n u_n^T / den_n
// Six dependent launches: v_o, v_n | t_o, s_n (one pass over Binv) | t_n, u_o, u_n (one pass over W) | the streams, r, stats | Binv r | alpha.
// G and r come out as gpmpc_sparse_remove followed by gpmpc_sparse_append give them, bit for bit: v_o, v_n, Lambda_o, Lambda_n are the
// same sums in the same order and the two corrections are applied in that order.  Binv, Q and alpha agree with the two calls to rounding.
// Workspace: v_o | v_n | t_o | s_n | t_n | u_o | u_n, M doubles each, then T [M][n_targets].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sparse_rep_v(int D, int M, const double* __restrict__ xold, const double* __restrict__ xnew,
                                                       const double* __restrict__ Z, const double* __restrict__ W, size_t ld_w, SparseHyp H,
                                                       double* __restrict__ vo, double* __restrict__ vn) {
    __shared__ double s_scr[16], s_out[1];
    const int i = blockIdx.x;
    const double* __restrict__ x = blockIdx.y ? xnew : xold;
    double acc[1] = {0.0};
    for (int l = threadIdx.x; l <= i; l += blockDim.x) acc[0] = fma(W[(size_t)i * ld_w + l], sp_kval(Z + (size_t)l * D, x, D, H), acc[0]);
    block_sum<1>(acc, s_scr, s_out);
    if (threadIdx.x == 0) (blockIdx.y ? vn : vo)[i] = s_out[0];
}

__global__ __launch_bounds__(256) void k_sparse_rep_t(int M, const double* __restrict__ Binv, const double* __restrict__ vo,
                                                       const double* __restrict__ vn, double* __restrict__ to, double* __restrict__ sn) {
    __shared__ double s_scr[32], s_out[2];
    const int i = blockIdx.x;
    double acc[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        const double b = sp_binv(Binv, M, i, k);
        acc[0] = fma(b, vo[k], acc[0]);
        acc[1] = fma(b, vn[k], acc[1]);
    }
    block_sum<2>(acc, s_scr, s_out);
    if (threadIdx.x == 0) { to[i] = s_out[0]; sn[i] = s_out[1]; }
}

// c of the block comment above, from the vectors alone: every workgroup of k_sparse_rep_u evaluates it in this order
static __device__ __forceinline__ double sp_rep_c(int M, const double* __restrict__ vo, const double* __restrict__ vn,
                                                   const double* __restrict__ to, double kappa, double* s_scr, double* s_out) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        acc[0] = fma(vo[k], vo[k], acc[0]);
        acc[1] = fma(vo[k], to[k], acc[1]);
        acc[2] = fma(to[k], vn[k], acc[2]);
    }
    block_sum<3>(acc, s_scr, s_out);
    const double lam_o = kappa - s_out[0], den_o = lam_o - s_out[1];
    return s_out[2] / den_o;
}

// one workgroup per column l of W: u_o[l], u_n[l]; it also owns t_n[l]
__global__ __launch_bounds__(256) void k_sparse_rep_u(int M, const double* __restrict__ W, size_t ld_w, const double* __restrict__ vo,
                                                       const double* __restrict__ vn, const double* __restrict__ to,
                                                       const double* __restrict__ sn, double kappa, double* __restrict__ tn,
                                                       double* __restrict__ uo, double* __restrict__ un) {
    __shared__ double s_scr[48], s_out[3];
    const double c = sp_rep_c(M, vo, vn, to, kappa, s_scr, s_out);
    __syncthreads();                                     // (s_out is read above by every thread and written again below)
    const int l = blockIdx.x;
    double acc[2] = {0.0, 0.0};
    for (int i = l + threadIdx.x; i < M; i += blockDim.x) {
        const double w = W[(size_t)i * ld_w + l];
        acc[0] = fma(w, to[i], acc[0]);
        acc[1] = fma(w, sn[i] + c * to[i], acc[1]);
    }
    block_sum<2>(acc, s_scr, s_out);
    if (threadIdx.x == 0) { uo[l] = s_out[0]; un[l] = s_out[1]; tn[l] = sn[l] + c * to[l]; }
}

// grid ((M + 255) / 256, M) as k_sparse_app_fill: row i, columns j; column block 0 of row i owns r[i][:], workgroup (0, 0) the stats
__global__ __launch_bounds__(256) void k_sparse_rep_fill(int M, int nt, const double* __restrict__ vo, const double* __restrict__ vn,
                                                          const double* __restrict__ to, const double* __restrict__ tn,
                                                          const double* __restrict__ uo, const double* __restrict__ un,
                                                          const double* __restrict__ yold, const double* __restrict__ ynew, double kappa,
                                                          double* __restrict__ G, double* __restrict__ r, double* __restrict__ Binv,
                                                          double* __restrict__ Q, double* __restrict__ stats) {
    __shared__ double s_scr[64], s_out[4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        acc[0] = fma(vo[k], vo[k], acc[0]);
        acc[1] = fma(vo[k], to[k], acc[1]);
        acc[2] = fma(vn[k], vn[k], acc[2]);
        acc[3] = fma(vn[k], tn[k], acc[3]);
    }
    block_sum<4>(acc, s_scr, s_out);
    const double lam_o = kappa - s_out[0], den_o = lam_o - s_out[1], lam_n = kappa - s_out[2], den_n = lam_n + s_out[3];
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (blockIdx.x == 0 && (int)threadIdx.x < nt) {
        const int a = threadIdx.x;
        const double ra = r[(size_t)i * nt + a] - vo[i] * yold[a] / lam_o;
        r[(size_t)i * nt + a] = ra + vn[i] * ynew[a] / lam_n;
    }
    if (blockIdx.x == 0 && i == 0 && threadIdx.x == 0) stats[1] = sp_min(lam_n, stats[1]);
    if (j >= M) return;
    const size_t o = (size_t)i * M + j;
    const double g = G[o] - (vo[i] * vo[j]) / lam_o;
    G[o] = g + (vn[i] * vn[j]) / lam_n;
    const double b = Binv[o] + (to[i] * to[j]) / den_o;
    Binv[o] = b - (tn[i] * tn[j]) / den_n;
    const double q = Q[o] - (uo[i] * uo[j]) / den_o;
    Q[o] = q + (un[i] * un[j]) / den_n;
}

extern "C" size_t gpmpc_sparse_replace_workspace_bytes(int M, int n_targets) {
    if (M < 1 || M > GPMPC_SPARSE_MAX_M || n_targets < 1 || n_targets > GPMPC_MAX_DS) return 0;
    return gpmpc_align256(sizeof(double) * 7 * (size_t)M) + gpmpc_align256(sizeof(double) * (size_t)M * n_targets);
}

extern "C" int gpmpc_sparse_replace(int D, int M, int n_targets, const double* x_old_dev, const double* y_old_dev, const double* x_new_dev,
                                    const double* y_new_dev, const double* Z_dev, const double* W_dev, size_t ld_w,
                                    const double* lambdas_host, double sigma_f, double noise_var, double* G_dev, double* r_dev,
                                    double* Binv_dev, double* Q_dev, double* alpha_dev, double* stats_dev, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (int rc = sp_check_dims("gpmpc_sparse_replace", D, M, n_targets)) return rc;
    if (int rc = sp_check_rank_one("gpmpc_sparse_replace", M, ld_w, x_old_dev && y_old_dev && x_new_dev && y_new_dev && Z_dev && W_dev &&
                                   lambdas_host && G_dev && r_dev && Binv_dev && Q_dev && alpha_dev && stats_dev && workspace))
        return rc;
    if (workspace_bytes < gpmpc_sparse_replace_workspace_bytes(M, n_targets)) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* vo = (double*)workspace; double* vn = vo + M; double* to = vn + M; double* sn = to + M; double* tn = sn + M;
    double* uo = tn + M; double* un = uo + M;
    double* T = (double*)((char*)workspace + gpmpc_align256(sizeof(double) * 7 * (size_t)M));
    SparseHyp hyp;
    sp_hyp(&hyp, D, lambdas_host, sigma_f, noise_var);
    hipLaunchKernelGGL(k_sparse_rep_v, dim3(M, 2), dim3(256), 0, s, D, M, x_old_dev, x_new_dev, Z_dev, W_dev, ld_w, hyp, vo, vn);
    hipLaunchKernelGGL(k_sparse_rep_t, dim3(M), dim3(256), 0, s, M, (const double*)Binv_dev, (const double*)vo, (const double*)vn, to, sn);
    hipLaunchKernelGGL(k_sparse_rep_u, dim3(M), dim3(256), 0, s, M, W_dev, ld_w, (const double*)vo, (const double*)vn, (const double*)to,
                       (const double*)sn, hyp.kappa, tn, uo, un);
    hipLaunchKernelGGL(k_sparse_rep_fill, dim3((M + 255) / 256, M), dim3(256), 0, s, M, n_targets, (const double*)vo, (const double*)vn,
                       (const double*)to, (const double*)tn, (const double*)uo, (const double*)un, y_old_dev, y_new_dev, hyp.kappa, G_dev,
                       r_dev, Binv_dev, Q_dev, stats_dev);
    hipLaunchKernelGGL(k_sparse_t, dim3(M), dim3(256), 0, s, M, n_targets, (const double*)Binv_dev, (const double*)r_dev, T);
    hipLaunchKernelGGL(k_sparse_alpha, dim3(M), dim3(256), 0, s, M, n_targets, W_dev, ld_w, (const double*)T, alpha_dev);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
