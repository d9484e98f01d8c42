// GP state ("pack") construction kernels: everything that depends only on the training data and
// the hyper-parameters, hoisted out of the per-call path of the reference
// (src/tools/uncertainty_prop.py:324-327 beta, :392-394 Lambda_part, :399 Ky_inv - beta beta^T;
// src/gpr.py:163-170 Kf / Ky).  The pack's lifecycle and its index data: pack.hip.
#include "gpmpc_internal.h"

// X [N][D] -> Xp [Np][D] (zero rows appended) and XT [D][Np]
__global__ void k_pack_points(const double* __restrict__ X, int N, int Np, int D,
                              double* __restrict__ Xp, double* __restrict__ XT) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Np) return;
    for (int k = 0; k < D; ++k) {
        const double v = i < N ? X[(size_t)i * D + k] : 0.0;
        Xp[(size_t)i * D + k] = v;
        XT[(size_t)k * Np + i] = v;
    }
}

// beta_a = Ky_inv_a @ y_a  (src/tools/uncertainty_prop.py:327); one wave per row.
__global__ __launch_bounds__(256) void k_pack_beta(const double* __restrict__ Kinv, size_t ld, size_t gstride, const double* __restrict__ Y,
                                                    int N, int Np, int ds, double* __restrict__ beta) {
    const int a = blockIdx.y;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= Np) return;
    double s = 0.0;
    if (row < N) {
        const double* __restrict__ r = Kinv + (size_t)a * gstride + (size_t)row * ld;
        for (int j = lane; j < N; j += 64) s = fma(r[j], Y[(size_t)j * ds + a], s);
        s = wave_sum(s);
    }
    if (lane == 0) beta[(size_t)a * Np + row] = s;
}

// M_a: element (i,j), i <= j, stored at [j*Np + i]:
//   w_ij * ( (Kinv[i][j] + Kinv[j][i])/2 - beta_i beta_j ) * sigma_f^4 * exp(-1/4 sum_k (x_ik - x_jk)^2 / lambda_k)
// with w = 1 on the diagonal and 2 above it; everything else (lower triangle, padding) is zero.
// 32x32 tiles staged through LDS so that both Kinv[i][j] and Kinv[j][i] are read coalesced.
__global__ __launch_bounds__(256) void k_pack_weights(const double* __restrict__ Kinv, size_t ld, size_t gstride, const double* __restrict__ beta,
                                                       const double* __restrict__ XT, const double* __restrict__ lam,
                                                       const double* __restrict__ sf, int N, int Np, int D,
                                                       double* __restrict__ M) {
    __shared__ double s_t[32][33];
    const int a = blockIdx.z;
    const int ti = blockIdx.x * 32, tj = blockIdx.y * 32;   // tile origin: rows i in [ti,ti+32), cols j in [tj,tj+32)
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const double* __restrict__ Ka = Kinv + (size_t)a * gstride;
    double* __restrict__ Ma = M + (size_t)a * Np * Np;
    if (tj + 31 < ti) {   // strictly below the diagonal
        for (int r = ty; r < 32; r += 8) {
            const int j = tj + r, i = ti + tx;
            if (j < Np && i < Np) Ma[(size_t)j * Np + i] = 0.0;
        }
        return;
    }
    // s_t[r][c] = Kinv[ti + r][tj + c]  (row-major read, coalesced over c)
    for (int r = ty; r < 32; r += 8) {
        const int i = ti + r, j = tj + tx;
        s_t[r][tx] = (i < N && j < N) ? Ka[(size_t)i * ld + j] : 0.0;
    }
    __syncthreads();
    const double sf2 = sf[a] * sf[a], sf4 = sf2 * sf2;
    for (int r = ty; r < 32; r += 8) {
        const int j = tj + r, i = ti + tx;                   // write M[j][i], coalesced over i
        if (j >= Np || i >= Np) continue;
        double out = 0.0;
        if (i <= j && j < N) {
            const double kji = Ka[(size_t)j * ld + i];       // coalesced over i
            const double kij = s_t[tx][r];
            double d2 = 0.0;
            for (int k = 0; k < D; ++k) {
                const double d = XT[(size_t)k * Np + i] - XT[(size_t)k * Np + j];
                d2 = fma(d * d, 1.0 / lam[a * D + k], d2);
            }
            const double wsym = 0.5 * (kij + kji) - beta[(size_t)a * Np + i] * beta[(size_t)a * Np + j];
            out = (i == j ? 1.0 : 2.0) * wsym * sf4 * exp(-0.25 * d2);
        }
        Ma[(size_t)j * Np + i] = out;
    }
}

// Step-1 weights (pair_kernel_q1.h).  At horizon step 1 the input variances s_k are those of the pack's noise model, so the scales of the pair
// transform, sc_k^2 = 1/8 / (lambda_k / 2 + s_k), are constants of the pack, and
//   M_ij exp(-|h_i + h_j|^2) = M1_ij kappa_i kappa_j,   kappa_i = exp(-2 |h_i|^2),   M1_ij = M_ij exp(+sum_k sc_k^2 (x_ik - x_jk)^2)
// (|h_i + h_j|^2 = 2 |h_i|^2 + 2 |h_j|^2 - |h_i - h_j|^2, and h_i - h_j = sc o (x_j - x_i) does not depend on the trajectory).  With M's own factor
// exp(-1/4 sum_k d_k^2 / lambda_k) that leaves M1_ij = bracket_ij exp(-sum_k d_k^2 s_k / (2 lambda_k (lambda_k + 2 s_k))): no decay with the distance
// when s is small.  The bracket needs Ky_inv, which a pack does not keep, and M1 has to follow a gpmpc_pack_set_noise that brings none: so M1 is
// formed from M.  What that costs: an entry whose M_ij has underflowed (1/4 sum d^2 / lambda > ~690) is dropped although M1_ij itself would be of
// the bracket's size -- its term M1_ij kappa_i kappa_j <= |M_ij| < 1e-300 is far below anything the sum resolves --, and exp(e) is taken as
// exp(e / 2)^2 so that no intermediate overflows while the product is finite.
__global__ __launch_bounds__(256) void k_pack_weights1(const double* __restrict__ M, const double* __restrict__ XT, const double* __restrict__ lam,
                                                        const double* __restrict__ noise, int Np, int D, int ds, double* __restrict__ M1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, a = blockIdx.z;
    if (i >= Np) return;
    const size_t at = ((size_t)a * Np + j) * Np + i;
    const double m = M[at];
    double out = 0.0;
    if (i <= j && fabs(m) >= 0x1p-1000) {
        double e = 0.0;
        for (int k = 0; k < D; ++k) {
            const double sk = k < ds ? noise[k * (ds + 1)] : noise[gpmpc_noise_off_action(ds) + (k - ds)];
            const double d = XT[(size_t)k * Np + i] - XT[(size_t)k * Np + j];
            e = fma(d * d, 0.125 / (0.5 * lam[a * D + k] + sk), e);
        }
        const double f = exp(0.5 * e);
        out = (m * f) * f;
    }
    M1[at] = out;
}

int gpmpc_pack_step1_refresh(gpmpc_pack* p, hipStream_t s) {
    if (!p || !p->built) return GPMPC_E_STATE;
    if (p->M1 && !p->m1_stale) {
        // current, or still being filled on whichever stream found it stale: behind the fill's event (a wait on the stream's own event is free)
        GPMPC_HIP(hipStreamWaitEvent(s, (hipEvent_t)p->m1_event, 0));
        return GPMPC_OK;
    }
    if (!p->M1) {                                            // weights and event: the pack has both or neither
        if (p->m1_failed) return GPMPC_E_ALLOC;
        double* m1 = nullptr; hipEvent_t ev = nullptr;
        hipError_t e = hipMalloc(&m1, sizeof(double) * (size_t)p->Np * p->Np * p->ds);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (m1) (void)hipFree(m1);
            (void)hipGetLastError();                         // the call goes on with the FIRST variant: no sticky error left behind
            gpmpc_set_error("gpmpc_rollout: step-1 weights not allocated, horizon step 1 keeps the pair kernel's FIRST variant", e);
            p->m1_failed = 1;
            return GPMPC_E_ALLOC;
        }
        p->M1 = m1; p->m1_event = ev;
        p->m1_stale = 1;
    }
    hipLaunchKernelGGL(k_pack_weights1, dim3((p->Np + 255) / 256, p->Np, p->ds), dim3(256), 0, s, p->M, p->XT, p->lam, p->noise_dev, p->Np, p->D,
                       p->ds, p->M1);
    GPMPC_HIP(hipGetLastError());
    GPMPC_HIP(hipEventRecord((hipEvent_t)p->m1_event, s));
    p->m1_stale = 0;
    return GPMPC_OK;
}

// Residual targets of a pack with a linear nominal model: R[i][a] = Y[i][a] - sum_k X[i][k] n_ak - c_a (the GPs learn the residual)
__global__ void k_pack_residual(const double* __restrict__ X, const double* __restrict__ Y, const double* __restrict__ nom,
                                int N, int D, int ds, double* __restrict__ R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
    if (i >= N) return;
    double m = nom[ds * D + a];
    for (int k = 0; k < D; ++k) m = fma(X[(size_t)i * D + k], nom[a * D + k], m);
    R[(size_t)i * ds + a] = Y[(size_t)i * ds + a] - m;
}

struct gpmpc_small_payload { unsigned w[128]; };
__global__ void k_upload_small(gpmpc_small_payload p, unsigned* __restrict__ dst, int nwords) {
    const int i = threadIdx.x;
    if (i < nwords) dst[i] = p.w[i];
}
int gpmpc_upload_small(void* dst_dev, const void* src_host, size_t bytes, hipStream_t s) {
    if (!dst_dev || !src_host || bytes == 0 || bytes > sizeof(gpmpc_small_payload) || (bytes & 3)) return GPMPC_E_ARG;
    gpmpc_small_payload p;
    memset(&p, 0, sizeof(p));
    memcpy(&p, src_host, bytes);
    hipLaunchKernelGGL(k_upload_small, dim3(1), dim3(128), 0, s, p, (unsigned*)dst_dev, (int)(bytes / 4));
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_store_host(void* dst_dev, const void* src_host, size_t bytes, void* stream) {
    return gpmpc_upload_small(dst_dev, src_host, bytes, (hipStream_t)stream);
}

// Kf = sigma_f^2 exp(-1/2 d2), Ky = Kf + noise_var I   (src/gpr.py:163-170)
__global__ void k_build_ky(const double* __restrict__ X, int n, int D, const double* __restrict__ lam,
                           double sf2, double noise_var, double* __restrict__ Kf, double* __restrict__ Ky) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    double d2 = 0.0;
    for (int k = 0; k < D; ++k) {
        const double d = X[(size_t)i * D + k] - X[(size_t)j * D + k];
        d2 = fma(d * d, 1.0 / lam[k], d2);
    }
    const double kf = sf2 * exp(-0.5 * d2);
    if (Kf) Kf[(size_t)i * n + j] = kf;
    Ky[(size_t)i * n + j] = kf + (i == j ? noise_var : 0.0);
}

// One lambda for all GPs, full-covariance rollout (pair_kernel_sbfx.h): the constant part of a column j of every cross unit,
//   rows[j] = [x_jk (D) | (N/ln2)/4 sum_k x_jk^2 / lambda_k | beta_c,j (c < ds) | pad],   beta = 0 for padded columns
__global__ void k_pack_fcs_rows(const double* __restrict__ beta, const double* __restrict__ XT, const double* __restrict__ lam,
                                int N, int Np, int D, int ds, int rw, double* __restrict__ rows) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Np) return;
    double* r = rows + (size_t)j * rw;
    double e = 0.0;
    for (int k = 0; k < D; ++k) { const double x = XT[(size_t)k * Np + j]; r[k] = x; e = fma(x * x, 1.0 / lam[k], e); }
    r[D] = (0.25 * 0x1.71547652b82fep+11) * e;               // (GPMPC_EXP_NEG_INV_C: the exponent travels scaled, fast_exp.h)
    for (int c = 0; c < ds; ++c) r[D + 1 + c] = j < N ? beta[(size_t)c * Np + j] : 0.0;
    for (int k = D + 1 + ds; k < rw; ++k) r[k] = 0.0;
}

// The rows exist from the first build or enable_fullcov at which the pack serves the full-covariance rollout with one lambda (its tile
// tables are part of the pack's index data from creation on: pack.hip); every build refreshes them while it does.
static bool fcs_serves(const gpmpc_pack* p, int shared_lambda) { return p->fullcov && shared_lambda && gpmpc_fcs_shape(p->ds, p->da); }
static int fcs_rows_alloc(gpmpc_pack* p, int shared_lambda) {
    if (p->fcs_rows || !fcs_serves(p, shared_lambda)) return GPMPC_OK;
    double* rows = nullptr;
    if (hipError_t e = hipMalloc(&rows, sizeof(double) * (size_t)p->Np * p->fcs_rw); e != hipSuccess) { gpmpc_set_error("gpmpc_pack_build: hipMalloc of the one-lambda column rows", e); return GPMPC_E_ALLOC; }
    p->fcs_rows = rows;
    return GPMPC_OK;
}
static int fcs_refresh(gpmpc_pack* p, hipStream_t s) {
    if (!p->fcs_rows || !fcs_serves(p, p->shared_lambda)) return GPMPC_OK;
    hipLaunchKernelGGL(k_pack_fcs_rows, dim3((p->Np + 255) / 256), dim3(256), 0, s, p->beta, p->XT, p->lam, p->N, p->Np, p->D, p->ds,
                       p->fcs_rw, p->fcs_rows);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// Cross-covariance weights of the GP pair (a, b), a < b:  element (i,j) at [j*Np + i]
//   beta_a[i] beta_b[j] sfa^2 sfb^2 exp(-1/2 sum_k (x_ik - x_jk)^2 / (lambda_ak + lambda_bk))
// (the x-independent factor of k_a(x,x_i) k_b(x,x_j), src/tools/uncertainty_prop.py:448-460 as a Gaussian product).
__global__ void k_pack_cross(const double* __restrict__ beta, const double* __restrict__ XT, const double* __restrict__ lam,
                             const double* __restrict__ sf, const int* __restrict__ pair_ab, int N, int Np, int D, int ds,
                             double* __restrict__ Mx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, pr = blockIdx.z;
    if (i >= Np) return;
    const int a = pair_ab[2 * pr], b = pair_ab[2 * pr + 1];
    double out = 0.0;
    if (i < N && j < N) {
        double d2 = 0.0;
        for (int k = 0; k < D; ++k) {
            const double d = XT[(size_t)k * Np + i] - XT[(size_t)k * Np + j];
            d2 = fma(d * d, 1.0 / (lam[a * D + k] + lam[b * D + k]), d2);
        }
        const double s2 = sf[a] * sf[a] * sf[b] * sf[b];
        out = beta[(size_t)a * Np + i] * beta[(size_t)b * Np + j] * s2 * exp(-0.5 * d2);
    }
    Mx[((size_t)pr * Np + j) * Np + i] = out;
}

// beta given directly: [N][ds] -> [ds][Np] zero padded
__global__ void k_pack_copy_beta(const double* __restrict__ Bsrc, int N, int Np, int ds, double* __restrict__ beta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
    if (i < Np) beta[(size_t)a * Np + i] = i < N ? Bsrc[(size_t)i * ds + a] : 0.0;
}

// ld / gstride: row stride of a Ky_inv matrix and the stride from one GP's matrix to the next, in doubles (0, 0 = packed [ds][N][N];
// gstride 0 with ld > 0: ONE matrix for every GP -- GPs with identical hyper-parameters and inputs share Ky_inv, src/gpr.py:159-171)
static int pack_build_impl(gpmpc_pack* p, const double* X_dev, const double* Y_dev, bool y_is_beta,
                           const double* Ky_inv_dev, const double* lambdas_host, const double* sigma_f_host,
                           void* stream, size_t ld = 0, size_t gstride = 0) {
    if (!p || !X_dev || !Y_dev || !lambdas_host || !sigma_f_host) return GPMPC_E_ARG;
    if (ld == 0) { ld = (size_t)p->N; gstride = (size_t)p->N * p->N; }
    if (ld < (size_t)p->N) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    if (!Ky_inv_dev && !y_is_beta) return GPMPC_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    for (int e = 0; e < p->ds * p->D; ++e) if (!(lambdas_host[e] > 0.0)) return GPMPC_E_ARG;
    // every GP with bit-identical length-scales (the reference's experiments): the rollout may share exponent and exp
    // across the GPs of a pair (pair_kernel_sbs.h)
    int shared = p->sh_ng > 0 ? 1 : 0;
    for (int a = 1; a < p->ds && shared; ++a)
        if (memcmp(lambdas_host + a * p->D, lambdas_host, sizeof(double) * p->D) != 0) shared = 0;
    if (int rca = fcs_rows_alloc(p, shared)) return rca;     // the one allocation a build can need: before the pack is touched
    p->m1_stale = 1; p->m1_failed = 0;                       // M, X, lambda and sigma_f change below: the step-1 weights follow on their next use
    for (int a = 0; a < p->ds; ++a) {
        p->sf_host[a] = sigma_f_host[a];
        for (int k = 0; k < p->D; ++k) p->lam_host[a][k] = lambdas_host[a * p->D + k];
    }
    // a captured launch sequence carries the kernel choice of the build it was captured under: the shared-lambda kernel
    // replayed on a pack whose lambdas have since become distinct would be WRONG (not just slow)
    if (shared != p->shared_lambda) {
        gpmpc_graph_cache_invalidate(p->graph_cache);
        gpmpc_cb_cache_invalidate(p->cb_cache);
        gpmpc_tuned_clear(p->tuned);                         // measured plans name the kernel family too
    }
    p->shared_lambda = shared;
    // hyper-parameters are tiny: as kernel arguments (consumed before this call returns, gpmpc_upload_small)
    if (int rcu = gpmpc_upload_small(p->lam, lambdas_host, sizeof(double) * p->ds * p->D, s)) return rcu;
    if (int rcu = gpmpc_upload_small(p->sf, sigma_f_host, sizeof(double) * p->ds, s)) return rcu;
    hipLaunchKernelGGL(k_pack_points, dim3((p->Np + 255) / 256), dim3(256), 0, s, X_dev, p->N, p->Np, p->D, p->X, p->XT);
    if (p->nominal && !y_is_beta) {                          // raw targets: the GPs are trained on what the nominal model leaves
        hipLaunchKernelGGL(k_pack_residual, dim3((p->N + 255) / 256, p->ds), dim3(256), 0, s, X_dev, Y_dev, p->nom_dev, p->N, p->D, p->ds, p->resid_dev);
        Y_dev = p->resid_dev;
    }
    if (y_is_beta)
        hipLaunchKernelGGL(k_pack_copy_beta, dim3((p->Np + 255) / 256, p->ds), dim3(256), 0, s, Y_dev, p->N, p->Np, p->ds, p->beta);
    else
        hipLaunchKernelGGL(k_pack_beta, dim3((p->Np + 3) / 4, p->ds), dim3(256), 0, s, Ky_inv_dev, ld, gstride, Y_dev, p->N, p->Np, p->ds, p->beta);
    if (Ky_inv_dev)
        hipLaunchKernelGGL(k_pack_weights, dim3(p->Np / 32, p->Np / 32, p->ds), dim3(256), 0, s,
                           Ky_inv_dev, ld, gstride, p->beta, p->XT, p->lam, p->sf, p->N, p->Np, p->D, p->M);
    else
        GPMPC_HIP(hipMemsetAsync(p->M, 0, sizeof(double) * (size_t)p->Np * p->Np * p->ds, s));
    if (p->fullcov && p->npairs > 0)
        hipLaunchKernelGGL(k_pack_cross, dim3((p->Np + 255) / 256, p->Np, p->npairs), dim3(256), 0, s, p->beta, p->XT, p->lam,
                           p->sf, p->pair_ab_dev, p->N, p->Np, p->D, p->ds, p->M + (size_t)p->ds * p->Np * p->Np);
    if (int rcf = fcs_refresh(p, s)) return rcf;
    {   // the column count that carries weight (traj_persist.h): re-sent when it changes (every 8th observation of a growing set)
        int nc = ((p->N + 7) / 8) * 8;
        if (nc > p->Np) nc = p->Np;
        if (nc != p->ncol_host) {
            if (int rcu = gpmpc_upload_small(p->ncol_dev, &nc, sizeof(int), s)) return rcu;
            p->ncol_host = nc;
        }
    }
    GPMPC_HIP(hipGetLastError());
    p->built = 1;
    return GPMPC_OK;
}

// Allocate and fill the cross-covariance weight matrices (needed by the full-covariance rollout and by the
// analytic cross-covariance Jacobians of gpmpc_moment_match).  Later gpmpc_pack_build* calls keep them current.
// Everything that can fail comes first, into locals: a failed call leaves the pack as it was.
extern "C" int gpmpc_pack_enable_fullcov(gpmpc_pack* p, void* stream) {
    if (!p) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    if (p->fullcov || p->npairs == 0) { p->fullcov = 1; return GPMPC_OK; }
    hipStream_t s = (hipStream_t)stream;
    const size_t mat = sizeof(double) * (size_t)p->Np * p->Np;
    const bool want_rows = p->built && p->shared_lambda && gpmpc_fcs_shape(p->ds, p->da) && !p->fcs_rows;
    double* Mnew = nullptr; double* rows = nullptr;
    const char* what = "gpmpc_pack_enable_fullcov: hipMalloc of the cross-covariance weights";
    int rc = GPMPC_E_ALLOC;
    hipError_t e = hipMalloc(&Mnew, mat * (p->ds + p->npairs));
    if (e == hipSuccess && want_rows) { what = "gpmpc_pack_enable_fullcov: hipMalloc of the one-lambda column rows"; e = hipMalloc(&rows, sizeof(double) * (size_t)p->Np * p->fcs_rw); }
    if (e == hipSuccess) { what = "gpmpc_pack_enable_fullcov: copy of the variance weights"; rc = GPMPC_E_LAUNCH; e = hipMemcpyAsync(Mnew, p->M, mat * p->ds, hipMemcpyDeviceToDevice, s); }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        gpmpc_set_error(what, e);
        if (Mnew) (void)hipFree(Mnew);
        if (rows) (void)hipFree(rows);
        return rc;
    }
    (void)hipFree(p->M);
    p->M = Mnew;
    if (rows) p->fcs_rows = rows;
    p->fullcov = 1;
    gpmpc_graph_cache_free(p->graph_cache); p->graph_cache = nullptr;    // p->M moved
    gpmpc_cb_cache_free(p->cb_cache); p->cb_cache = nullptr;
    if (p->built) {
        hipLaunchKernelGGL(k_pack_cross, dim3((p->Np + 255) / 256, p->Np, p->npairs), dim3(256), 0, s, p->beta, p->XT, p->lam,
                           p->sf, p->pair_ab_dev, p->N, p->Np, p->D, p->ds, p->M + (size_t)p->ds * p->Np * p->Np);
        GPMPC_HIP(hipGetLastError());
        if (int rcf = fcs_refresh(p, s)) return rcf;
    }
    return GPMPC_OK;
}

extern "C" int gpmpc_pack_build(gpmpc_pack* p, const double* X_dev, const double* Y_dev, const double* Ky_inv_dev,
                                const double* lambdas_host, const double* sigma_f_host, void* stream) {
    return pack_build_impl(p, X_dev, Y_dev, false, Ky_inv_dev, lambdas_host, sigma_f_host, stream);
}

extern "C" int gpmpc_pack_build_strided(gpmpc_pack* p, const double* X_dev, const double* Y_dev, const double* Ky_inv_dev,
                                        size_t ld, size_t gp_stride, const double* lambdas_host, const double* sigma_f_host, void* stream) {
    if (!Ky_inv_dev || ld == 0) return GPMPC_E_ARG;
    return pack_build_impl(p, X_dev, Y_dev, false, Ky_inv_dev, lambdas_host, sigma_f_host, stream, ld, gp_stride);
}

extern "C" int gpmpc_pack_build_beta(gpmpc_pack* p, const double* X_dev, const double* beta_dev, const double* Ky_inv_dev,
                                     const double* lambdas_host, const double* sigma_f_host, void* stream) {
    return pack_build_impl(p, X_dev, beta_dev, true, Ky_inv_dev, lambdas_host, sigma_f_host, stream);
}

extern "C" int gpmpc_pack_export(const gpmpc_pack* p, double* beta_out, double* weights_out, void* stream) {
    if (!p) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    hipStream_t s = (hipStream_t)stream;
    const size_t Np = p->Np;
    if (beta_out) GPMPC_HIP(hipMemcpyAsync(beta_out, p->beta, sizeof(double) * Np * p->ds, hipMemcpyDeviceToDevice, s));
    if (weights_out) GPMPC_HIP(hipMemcpyAsync(weights_out, p->M, sizeof(double) * Np * Np * p->ds, hipMemcpyDeviceToDevice, s));   // variance units only
    return GPMPC_OK;
}

extern "C" int gpmpc_build_ky(int n, int D, const double* X_dev, const double* lambdas_host, double sigma_f,
                              double noise_var, double* Kf_dev, double* Ky_dev, void* stream) {
    if (n < 1 || D < 1 || D > GPMPC_MAX_D || !X_dev || !lambdas_host || !Ky_dev) return GPMPC_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* lam = nullptr;
    GPMPC_HIP(hipMallocAsync((void**)&lam, sizeof(double) * D, s));
    if (int rcu = gpmpc_upload_small(lam, lambdas_host, sizeof(double) * D, s)) { (void)hipFreeAsync(lam, s); return rcu; }
    hipLaunchKernelGGL(k_build_ky, dim3((n + 255) / 256, n), dim3(256), 0, s, X_dev, n, D, lam, sigma_f * sigma_f,
                       noise_var, Kf_dev, Ky_dev);
    GPMPC_HIP(hipGetLastError());
    GPMPC_HIP(hipFreeAsync(lam, s));
    return GPMPC_OK;
}
