// Particles: the pointwise posterior of all GPs at many points, and Monte-Carlo rollouts through it.  Formulas, layouts, the noise
// addressing and the refusals: include/gpmpc.h, "Particles"; the why and the measurements: DESIGN.md section 3i.
//
// Per chunk of C columns (points) and per group of GPs with bit-identical (lambda, sigma_f) (GpGroup, model_frame.h):
//   k_pt_kstar   Ks[i][c] = k(X_i, z_c), c fastest, zero-padded to multiples of 64 both ways, and the partial sums of the means
//                mpart[bi][slot][c] = sum_{i in row block bi} beta_{i, gp(slot)} Ks[i][c]
//   k_pt_quad    workgroup (bc, bi, matrix): T = Kinv[64 bi ...][:] Ks[:][64 bc ...] by MFMA stages (tile_stage.h), contracted in the
//                epilogue with the matching rows of Ks: part[matrix][bi][c] = sum_{i in tile} Ks[i][c] T[i][c].  T is never written.
//   k_pt_finish  q = sum_bi part (ascending), m = sum_bi mpart (ascending) + the nominal term, s2 = sf^2 - q + process_var, the draw
// Rules: no atomics; every output element is owned by one thread or one workgroup, which sums in a fixed order; launch geometry depends
// on sizes only.
#include <cmath>
#include "model_frame.h"     // the model checks, GpGroup, the chunk rule, the pivots of init_cov
#include "tile_stage.h"
#include "philox.h"
#include "particles_internal.h"

static_assert(SP_T == GPMPC_MODEL_TILE, "the chunk rule of model_frame.h rounds to the tile of tile_stage.h");
#define PT_KEY_XOR 0x50415254u      // "PART": keeps the particle streams apart from the MPPI streams of the same seed
#define PT_MAX_NORMALS (GPMPC_MAX_D + GPMPC_MAX_DS)

struct PtTail {                     // what k_pt_finish needs of the model besides the group
    double nom_w[GPMPC_MAX_DS * GPMPC_MAX_D], nom_b[GPMPC_MAX_DS], process_var[GPMPC_MAX_DS];
    int has_nominal;
};
struct PtVec { double v[GPMPC_MAX_DS * GPMPC_MAX_DS]; };

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// grid (cnp / 64, np / 64).  Thread (c = t & 63, q = t >> 6) owns column c0 + c and the rows i0 + 16 q ... + 15 (ascending).
__global__ __launch_bounds__(256) void k_pt_kstar(int n, int cn, int D, int ds, const double* __restrict__ X, const double* __restrict__ Z,
                                                   const double* __restrict__ beta, GpGroup G, double* __restrict__ Ks, int ldk,
                                                   double* __restrict__ mpart) {
    __shared__ double s_x[SP_T][GPMPC_MAX_D], s_b[SP_T][GPMPC_MAX_DS], s_p[4][GPMPC_MAX_DS][SP_T];
    const int t = threadIdx.x, c = t & 63, q = t >> 6;
    const int c0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T;
    for (int e = t; e < SP_T * GPMPC_MAX_D; e += 256) {
        const int i = e >> 3, d = e & 7;
        s_x[i][d] = (i0 + i < n && d < D) ? X[(size_t)(i0 + i) * D + d] : 0.0;
        s_b[i][d] = (i0 + i < n && d < G.ng) ? beta[(size_t)(i0 + i) * ds + G.gp[d]] : 0.0;
    }
    double z[GPMPC_MAX_D];
#pragma unroll
    for (int d = 0; d < GPMPC_MAX_D; ++d) z[d] = (c0 + c < cn && d < D) ? Z[(size_t)(c0 + c) * D + d] : 0.0;
    __syncthreads();
    double m[GPMPC_MAX_DS] = {};
    for (int r = 0; r < 16; ++r) {
        const int il = 16 * q + r;
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < GPMPC_MAX_D; ++d) { const double u = s_x[il][d] - z[d]; d2 = fma(u * u, G.ilam[d], d2); }
        const double k = (i0 + il < n && c0 + c < cn) ? G.sf2 * exp(-0.5 * d2) : 0.0;
        Ks[(size_t)(i0 + il) * ldk + c0 + c] = k;
#pragma unroll
        for (int a = 0; a < GPMPC_MAX_DS; ++a) m[a] = fma(s_b[il][a], k, m[a]);
    }
#pragma unroll
    for (int a = 0; a < GPMPC_MAX_DS; ++a) s_p[q][a][c] = m[a];
    __syncthreads();
    for (int e = t; e < G.ng * SP_T; e += 256) {
        const int a = e >> 6, cc = e & 63;
        mpart[((size_t)blockIdx.y * GPMPC_MAX_DS + a) * ldk + c0 + cc] = (s_p[0][a][cc] + s_p[1][a][cc]) + (s_p[2][a][cc] + s_p[3][a][cc]);
    }
}

// grid (cnp / 64, np / 64, matrices).  Matrix z is GP G.gp[z]'s (gp_stride != 0) or the one matrix of all GPs.
__global__ __launch_bounds__(256) void k_pt_quad(int n, int np, const double* __restrict__ Kinv, size_t ld, size_t gp_stride, GpGroup G,
                                                  const double* __restrict__ Ks, int ldk, double* __restrict__ part) {
    __shared__ double s_a[SP_KB][SP_T + 1], s_b[SP_KB][SP_T + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int c0 = blockIdx.x * SP_T, i0 = blockIdx.y * SP_T, nbi = gridDim.y;
    const double* __restrict__ K = Kinv + (size_t)G.gp[blockIdx.z] * gp_stride;
    double acc[4][4] = {};
    // the next stage's operands travel in registers while this stage is multiplied
    double pa[4], pb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q;
            const int i = e >> 4, k = e & 15;            // Kinv tile: row i0 + i, column k0 + k (k fastest: consecutive addresses)
            pa[q] = (i0 + i < n && k0 + k < n) ? K[(size_t)(i0 + i) * ld + k0 + k] : 0.0;
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
    __syncthreads();                                     // (s_a is free now: it takes the per-thread sums, [ty][column])
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        double p = 0.0;
#pragma unroll
        for (int qa = 0; qa < 4; ++qa) {                 // the thread's four rows of this column, ascending
            const int i = i0 + sp_row<true>(ty, qa), c = c0 + tx + 16 * qb;
            p = fma(Ks[(size_t)i * ldk + c], sp_acc<true>(acc, qa, qb), p);
        }
        s_a[ty][tx + 16 * qb] = p;
    }
    __syncthreads();
    if (t < SP_T) {
        double s = 0.0;
        for (int y = 0; y < 16; ++y) s += s_a[y][t];
        part[((size_t)blockIdx.z * nbi + blockIdx.y) * ldk + c0 + t] = s;
    }
}

// one thread per (column, GP of the group).  col0: index of the chunk's first column in the whole call (p = column % P addresses eps).
__global__ __launch_bounds__(256) void k_pt_finish(int cn, int nbi, int D, int ds, int da, int shared_mat, GpGroup G, PtTail M,
                                                    const double* __restrict__ Z, const double* __restrict__ mpart,
                                                    const double* __restrict__ part, int ldk, double* __restrict__ out_mean,
                                                    double* __restrict__ out_var, const double* __restrict__ eps, int P, long col0,
                                                    double* __restrict__ out_next) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cn * G.ng) return;
    const int c = (int)(e / G.ng), slot = (int)(e - (long)c * G.ng), a = G.gp[slot], mat = shared_mat ? 0 : slot;
    double q = 0.0, m = 0.0;
    for (int b = 0; b < nbi; ++b) q += part[((size_t)mat * nbi + b) * ldk + c];
    for (int b = 0; b < nbi; ++b) m += mpart[((size_t)b * GPMPC_MAX_DS + slot) * ldk + c];
    if (M.has_nominal) {
        double lin = M.nom_b[a];
        for (int d = 0; d < D; ++d) lin = fma(M.nom_w[a * D + d], Z[(size_t)c * D + d], lin);
        m += lin;
    }
    const double s2 = (G.sf2 - q) + M.process_var[a];
    const size_t o = (size_t)c * ds + a;
    if (out_mean) out_mean[o] = m;
    if (out_var) out_var[o] = s2;
    if (out_next) {
        const int p = (int)((col0 + c) % P);
        out_next[o] = m + sqrt(s2 > 0.0 ? s2 : 0.0) * eps[(size_t)p * (da + ds) + da + a];
    }
}

// one thread per (particle, pair): two normals
__global__ __launch_bounds__(256) void k_pt_noise(int P, int nn, unsigned t, unsigned seed_lo, unsigned seed_hi, unsigned call_index,
                                                   double* __restrict__ out) {
    const int npair = (nn + 1) / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)P * npair) return;
    const int p = (int)(e / npair), j = (int)(e - (long)p * npair);
    const Philox4 r = philox4x32_10((unsigned)p, (unsigned)j, t, call_index, seed_lo, seed_hi ^ PT_KEY_XOR);
    const double u1 = mppi_uniform(r.w[0], r.w[1]), u2 = mppi_uniform(r.w[2], r.w[3]);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    out[(size_t)p * nn + 2 * j] = rad * cs;
    if (2 * j + 1 < nn) out[(size_t)p * nn + 2 * j + 1] = rad * sn;
}

// x_0[b P + p][a] = x0[b][a] + sum_{k <= a} L[a][k] eps[p][k], k ascending
__global__ __launch_bounds__(256) void k_pt_init(int B, int P, int ds, const double* __restrict__ x0, const double* __restrict__ eps, PtVec L,
                                                  double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * P * ds) return;
    const int a = (int)(e % ds);
    const long c = e / ds;
    const int p = (int)(c % P), b = (int)(c / P);
    double s = 0.0;
    for (int k = 0; k <= a; ++k) s = fma(L.v[a * ds + k], eps[(size_t)p * ds + k], s);
    out[e] = x0[(size_t)b * ds + a] + s;
}

// z[c] = (x_prev[c], U_t[b] + sqrt(action_var) eps_u[p]); sd = sqrt(action_var) from the host
__global__ __launch_bounds__(256) void k_pt_assemble(int B, int P, int ds, int da, const double* __restrict__ x_prev, const double* __restrict__ U,
                                                      size_t u_stride, const double* __restrict__ eps, PtVec sd, double* __restrict__ z) {
    const int D = ds + da;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * P * D) return;
    const int d = (int)(e % D);
    const long c = e / D;
    const int p = (int)(c % P), b = (int)(c / P);
    z[e] = d < ds ? x_prev[(size_t)c * ds + d] : U[(size_t)b * u_stride + (d - ds)] + sd.v[d - ds] * eps[(size_t)p * D + (d - ds)];
}

// grid (T, B).  Thread i adds the particles i, i + 256, ... in ascending order; the 256 partial sums are folded in halves.
// t0v: first step `var` covers (the rollout keeps s2 of the steps 1 ... H only); out_clamped is [B][T - t0v].
__global__ __launch_bounds__(MPPI_THREADS) void k_pt_stats(int B, int P, int T, int ds, const double* __restrict__ X, const double* __restrict__ var,
                                                           int t0v, int n_rows, gpmpc_state_constraints cons, double* __restrict__ out_mean,
                                                           double* __restrict__ out_cov, int* __restrict__ out_clamped,
                                                           double* __restrict__ out_viol) {
    __shared__ double red[MPPI_THREADS];
    __shared__ int redi[MPPI_THREADS];
    const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    const double* __restrict__ x = X + ((size_t)t * B + b) * P * ds;
    double mean[GPMPC_MAX_DS];
#pragma unroll
    for (int e = 0; e < GPMPC_MAX_DS; ++e) {
        mean[e] = 0.0;
        if (e < ds) {
            double s = 0.0;
            for (int p = tid; p < P; p += MPPI_THREADS) s = s + x[(size_t)p * ds + e];
            mean[e] = mppi_fold_sum(s, red) / (double)P;
            if (out_mean && tid == 0) out_mean[((size_t)b * T + t) * ds + e] = mean[e];
        }
    }
    if (out_cov) {
#pragma unroll
        for (int e = 0; e < GPMPC_MAX_DS; ++e)
#pragma unroll
            for (int f = e; f < GPMPC_MAX_DS; ++f) {
                if (f >= ds) continue;
                double s = 0.0;
                for (int p = tid; p < P; p += MPPI_THREADS) s = s + (x[(size_t)p * ds + e] - mean[e]) * (x[(size_t)p * ds + f] - mean[f]);
                const double cv = mppi_fold_sum(s, red) / (double)(P - 1);
                if (tid == 0) {
                    double* o = out_cov + ((size_t)b * T + t) * ds * ds;
                    o[e * ds + f] = cv;
                    o[f * ds + e] = cv;
                }
            }
    }
    if (out_clamped && t >= t0v) {
        const double* __restrict__ v = var + ((size_t)(t - t0v) * B + b) * P * ds;
        int cnt = 0;
        for (int p = tid; p < P; p += MPPI_THREADS) {
            bool neg = false;
            for (int e = 0; e < ds; ++e) neg |= v[(size_t)p * ds + e] < 0.0;
            cnt += neg ? 1 : 0;
        }
        cnt = mppi_fold_count(cnt, redi);
        if (tid == 0) out_clamped[(size_t)b * (T - t0v) + (t - t0v)] = cnt;
    }
    for (int r = 0; r < n_rows; ++r) {
        int cnt = 0;
        for (int p = tid; p < P; p += MPPI_THREADS) {
            double g = 0.0;
            for (int e = 0; e < ds; ++e) g = g + cons.A[r * ds + e] * x[(size_t)p * ds + e];
            cnt += g > cons.b[r] ? 1 : 0;
        }
        cnt = mppi_fold_count(cnt, redi);
        if (tid == 0) out_viol[((size_t)b * T + t) * n_rows + r] = (double)cnt / (double)P;
    }
}

// grid (B): the fraction of particles that violate some row at some step t >= 1
__global__ __launch_bounds__(MPPI_THREADS) void k_pt_joint(int B, int P, int T, int ds, const double* __restrict__ X, int n_rows,
                                                           gpmpc_state_constraints cons, double* __restrict__ out_joint) {
    __shared__ int redi[MPPI_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    int cnt = 0;
    for (int p = tid; p < P; p += MPPI_THREADS) {
        bool any = false;
        for (int t = 1; t < T; ++t) {
            const double* __restrict__ x = X + (((size_t)t * B + b) * P + p) * ds;
            for (int r = 0; r < n_rows; ++r) {
                double g = 0.0;
                for (int e = 0; e < ds; ++e) g = g + cons.A[r * ds + e] * x[e];
                any |= g > cons.b[r];
            }
        }
        cnt += any ? 1 : 0;
    }
    cnt = mppi_fold_count(cnt, redi);
    if (tid == 0) out_joint[b] = (double)cnt / (double)P;
}

// ---------------------------------------------------------------------------
// host: checks
// ---------------------------------------------------------------------------
struct PtNoise { double L[GPMPC_MAX_DS * GPMPC_MAX_DS], action_sd[GPMPC_MAX_D], process_var[GPMPC_MAX_DS]; };

// The noise model of `m` (or the defaults): the lower Cholesky factor of init_cov, sqrt(action_var), process_var.
static int pt_noise(const char* who, const gpmpc_gp_model* m, PtNoise* out) {
    const int ds = m->state_dim, da = m->action_dim;
    memset(out, 0, sizeof(*out));
    double Pm[GPMPC_MAX_DS * GPMPC_MAX_DS] = {};
    for (int a = 0; a < ds; ++a) Pm[a * ds + a] = GPMPC_INIT_VAR;
    for (int j = 0; j < da; ++j) out->action_sd[j] = sqrt(GPMPC_ACTION_VAR);
    if (m->has_noise) {
        double big = 0.0;
        for (int k = 0; k < ds * ds; ++k) {
            if (!gpmpc_finite(m->init_cov[k])) return gpmpc_refuse(who, "init_cov holds a non-finite value");
            big = fmax(big, fabs(m->init_cov[k]));
        }
        for (int a = 0; a < ds; ++a)
            for (int b = 0; b < a; ++b)
                if (fabs(m->init_cov[a * ds + b] - m->init_cov[b * ds + a]) > 1e-12 * big) return gpmpc_refuse(who, "init_cov is not symmetric");
        for (int a = 0; a < ds; ++a)
            for (int b = 0; b < ds; ++b) Pm[a * ds + b] = 0.5 * (m->init_cov[a * ds + b] + m->init_cov[b * ds + a]);
        for (int j = 0; j < da; ++j) {
            if (!gpmpc_finite(m->action_var[j]) || m->action_var[j] < 0.0) return gpmpc_refuse(who, "action_var[%d] = %g is negative or not finite", j, m->action_var[j]);
            out->action_sd[j] = sqrt(m->action_var[j]);
        }
        for (int a = 0; a < ds; ++a) {
            if (!gpmpc_finite(m->process_var[a]) || m->process_var[a] < 0.0) return gpmpc_refuse(who, "process_var[%d] = %g is negative or not finite", a, m->process_var[a]);
            out->process_var[a] = m->process_var[a];
        }
    }
    double big = 0.0, d = 0.0;
    for (int k = 0; k < ds * ds; ++k) big = fmax(big, fabs(Pm[k]));
    int j = 0;
    if (!gpmpc_psd_pivots(Pm, ds, big, out->L, &d, &j))
        return gpmpc_refuse(who, "init_cov has a negative pivot (%g at %d): it is not positive semi-definite", d, j);
    return GPMPC_OK;
}

// the core (model_frame.h), then the whole noise model
static int pt_check_model(const char* who, const gpmpc_gp_model* m, PtNoise* noise) {
    if (int rc = gpmpc_model_check_core(who, m)) return rc;
    return pt_noise(who, m, noise);
}

static int pt_check_count(const char* who, long cols, int width) {
    return cols * width > 0x7fffffffL ? gpmpc_refuse(who, "more than 2^31 - 1 elements in one array") : GPMPC_OK;
}

// workspace of the posterior: Ks [np][C] | mpart [nbi][GPMPC_MAX_DS][C] | part [ds][nbi][C]
struct PtLayout { size_t off_ks, off_mpart, off_part, total; int np, nbi, C; };
static PtLayout pt_layout(int n, int ds, int chunk, long ncols, gpmpc_carver& c) {
    PtLayout L;
    L.nbi = (n + SP_T - 1) / SP_T;
    L.np = L.nbi * SP_T;
    L.C = gpmpc_chunk_cols(ncols, chunk);
    const size_t d = sizeof(double);
    L.off_ks = c.take(d * L.np * L.C);
    L.off_mpart = c.take(d * L.nbi * GPMPC_MAX_DS * L.C);
    L.off_part = c.take(d * ds * L.nbi * L.C);
    L.total = c.total();
    return L;
}

// the three passes over all chunks; eps / out_next as k_pt_finish
static int pt_posterior(const gpmpc_gp_model* m, const PtNoise& noise, long nq, const double* z, double* out_mean, double* out_var,
                        const double* eps, int P, double* out_next, const PtLayout& L, char* ws, hipStream_t s) {
    const int ds = m->state_dim, da = m->action_dim, D = ds + da;
    GpGroup groups[GPMPC_MAX_DS];
    const int ngroups = gpmpc_model_groups(m, groups);
    PtTail tail;
    memset(&tail, 0, sizeof(tail));
    tail.has_nominal = m->has_nominal;
    if (m->has_nominal) { memcpy(tail.nom_w, m->nom_w, sizeof(double) * ds * D); memcpy(tail.nom_b, m->nom_b, sizeof(double) * ds); }
    memcpy(tail.process_var, noise.process_var, sizeof(tail.process_var));
    double* Ks = (double*)(ws + L.off_ks);
    double* mpart = (double*)(ws + L.off_mpart);
    double* part = (double*)(ws + L.off_part);
    const int shared_mat = m->gp_stride == 0;
    for (long c0 = 0; c0 < nq; c0 += L.C) {
        const int cn = (int)(nq - c0 < L.C ? nq - c0 : L.C), cnp = (cn + SP_T - 1) / SP_T * SP_T;
        const double* zc = z + (size_t)c0 * D;
        for (int g = 0; g < ngroups; ++g) {
            const GpGroup& G = groups[g];
            hipLaunchKernelGGL(k_pt_kstar, dim3(cnp / SP_T, L.nbi), dim3(256), 0, s, m->n, cn, D, ds, m->X, zc, m->beta, G, Ks, L.C, mpart);
            hipLaunchKernelGGL(k_pt_quad, dim3(cnp / SP_T, L.nbi, shared_mat ? 1 : G.ng), dim3(256), 0, s, m->n, L.np, m->Kinv, m->ld,
                               m->gp_stride, G, (const double*)Ks, L.C, part);
            hipLaunchKernelGGL(k_pt_finish, dim3(gpmpc_blocks256((long)cn * G.ng)), dim3(256), 0, s, cn, L.nbi, D, ds, da, shared_mat, G, tail, zc,
                               (const double*)mpart, (const double*)part, L.C, out_mean ? out_mean + (size_t)c0 * ds : nullptr,
                               out_var ? out_var + (size_t)c0 * ds : nullptr, eps, P, c0, out_next ? out_next + (size_t)c0 * ds : nullptr);
        }
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// host: entries
// ---------------------------------------------------------------------------
// for particle_cost.hip (particles_internal.h)
int gpmpc_pt_check_model(const char* who, const gpmpc_gp_model* m) {
    PtNoise noise;
    return pt_check_model(who, m, &noise);
}

extern "C" size_t gpmpc_gp_posterior_workspace_bytes(const gpmpc_gp_model* m, int nq, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || nq < 1 || !gpmpc_chunk_ok(chunk)) return 0;
    gpmpc_carver c;
    return pt_layout(m->n, m->state_dim, chunk, nq, c).total;
}

extern "C" int gpmpc_gp_posterior(const gpmpc_gp_model* m, int nq, const double* z_dev, double* out_mean, double* out_var, int chunk,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_gp_posterior";
    PtNoise noise;
    if (int rc = pt_check_model(who, m, &noise)) return rc;
    if (nq < 1) return gpmpc_refuse(who, "nq < 1");
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (int rc = pt_check_count(who, nq, GPMPC_MAX_D)) return rc;
    if (!z_dev || !out_mean || !out_var || !workspace) return gpmpc_refuse(who, "NULL pointer");
    gpmpc_carver c;
    const PtLayout L = pt_layout(m->n, m->state_dim, chunk, nq, c);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    return pt_posterior(m, noise, nq, z_dev, out_mean, out_var, nullptr, 1, nullptr, L, (char*)workspace, (hipStream_t)stream);
}

static int pt_launch_noise(int P, int nn, int t, unsigned long long seed, unsigned call_index, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_pt_noise, dim3(gpmpc_blocks256((long)P * ((nn + 1) / 2))), dim3(256), 0, s, P, nn, (unsigned)t, (unsigned)seed,
                       (unsigned)(seed >> 32), call_index, out);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_particle_noise(int P, int n_normals, int t, unsigned long long seed, unsigned call_index, double* out_eps, void* stream) {
    const char* who = "gpmpc_particle_noise";
    if (P < 1) return gpmpc_refuse(who, "P < 1");
    if (n_normals < 1 || n_normals > PT_MAX_NORMALS) return gpmpc_refuse(who, "n_normals = %d outside 1...%d", n_normals, PT_MAX_NORMALS);
    if (t < 0) return gpmpc_refuse(who, "t < 0");
    if (int rc = pt_check_count(who, P, PT_MAX_NORMALS)) return rc;
    if (!out_eps) return gpmpc_refuse(who, "NULL pointer");
    return pt_launch_noise(P, n_normals, t, seed, call_index, out_eps, (hipStream_t)stream);
}

// workspace of a step: z [B P][D] | the posterior's
struct PtStepLayout { size_t off_z; PtLayout post; size_t total; };
static PtStepLayout pt_step_layout(const gpmpc_gp_model* m, int B, int P, int chunk, gpmpc_carver& c) {
    PtStepLayout S;
    const int D = m->state_dim + m->action_dim;
    S.off_z = c.take(sizeof(double) * (size_t)B * P * D);
    S.post = pt_layout(m->n, m->state_dim, chunk, (long)B * P, c);
    S.total = c.total();
    return S;
}

int gpmpc_pt_check_bp(const char* who, int B, int P) {
    if (B < 1) return gpmpc_refuse(who, "B < 1");
    if (P < 1) return gpmpc_refuse(who, "P < 1");
    return pt_check_count(who, (long)B * P, GPMPC_MAX_D);
}

int gpmpc_pt_initial(const gpmpc_gp_model* m, int B, int P, const double* x0, const double* eps, double* out, hipStream_t s) {
    PtNoise noise;
    if (int rc = pt_noise("gpmpc_pt_initial", m, &noise)) return rc;
    PtVec L;
    memcpy(L.v, noise.L, sizeof(L.v));
    hipLaunchKernelGGL(k_pt_init, dim3(gpmpc_blocks256((long)B * P * m->state_dim)), dim3(256), 0, s, B, P, m->state_dim, x0, eps, L, out);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// U_p (or null): an input per particle, dev [B P][da], in the place of U_t / u_stride (the assemble kernel of linprop_inputs.hip)
static int pt_step(const gpmpc_gp_model* m, const PtNoise& noise, int B, int P, const double* x_prev, const double* U_t, size_t u_stride,
                   const double* eps, double* out_next, double* out_mean, double* out_var, const PtStepLayout& S, char* ws, hipStream_t s,
                   const double* U_p = nullptr) {
    const int ds = m->state_dim, da = m->action_dim, D = ds + da;
    double* z = (double*)(ws + S.off_z);
    if (U_p) {
        if (int rc = gpmpc_lpi_assemble(B, P, ds, da, x_prev, U_p, eps, noise.action_sd, z, s)) return rc;
    } else {
        PtVec sd;
        memset(&sd, 0, sizeof(sd));
        memcpy(sd.v, noise.action_sd, sizeof(double) * GPMPC_MAX_D);
        hipLaunchKernelGGL(k_pt_assemble, dim3(gpmpc_blocks256((long)B * P * D)), dim3(256), 0, s, B, P, ds, da, x_prev, U_t, u_stride, eps, sd, z);
    }
    return pt_posterior(m, noise, (long)B * P, z, out_mean, out_var, eps, P, out_next, S.post, ws, s);
}

extern "C" size_t gpmpc_particle_step_workspace_bytes(const gpmpc_gp_model* m, int B, int P, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || B < 1 || P < 1 || (long)B * P * GPMPC_MAX_D > 0x7fffffffL || !gpmpc_chunk_ok(chunk)) return 0;
    gpmpc_carver c;
    return pt_step_layout(m, B, P, chunk, c).total;
}

extern "C" int gpmpc_particle_step(const gpmpc_gp_model* m, int B, int P, const double* x_prev, const double* U_t, size_t u_stride,
                                   const double* eps, double* out_next, double* out_mean, double* out_var, int chunk, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_particle_step";
    PtNoise noise;
    if (int rc = pt_check_model(who, m, &noise)) return rc;
    if (int rc = gpmpc_pt_check_bp(who, B, P)) return rc;
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!x_prev || !eps || !out_next || !workspace || (m->action_dim > 0 && !U_t)) return gpmpc_refuse(who, "NULL pointer");
    if (u_stride < (size_t)m->action_dim && B > 1) return gpmpc_refuse(who, "u_stride < action_dim");
    gpmpc_carver c;
    const PtStepLayout S = pt_step_layout(m, B, P, chunk, c);
    if (workspace_bytes < S.total) return GPMPC_E_WORKSPACE;
    return pt_step(m, noise, B, P, x_prev, U_t, u_stride, eps, out_next, out_mean, out_var, S, (char*)workspace, (hipStream_t)stream);
}

// gpmpc_particle_step with an input per particle, U_p dev [B P][da] (gpmpc_particle_inputs makes them), in the place of U_t / u_stride
extern "C" size_t gpmpc_particle_step_inputs_workspace_bytes(const gpmpc_gp_model* m, int B, int P, int chunk) {
    if (!m || m->action_dim < 1) return 0;
    return gpmpc_particle_step_workspace_bytes(m, B, P, chunk);
}

extern "C" int gpmpc_particle_step_inputs(const gpmpc_gp_model* m, int B, int P, const double* x_prev, const double* U_p, const double* eps,
                                          double* out_next, double* out_mean, double* out_var, int chunk, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_particle_step_inputs";
    PtNoise noise;
    if (int rc = pt_check_model(who, m, &noise)) return rc;
    if (m->action_dim < 1) return gpmpc_refuse(who, "an input per particle needs action_dim >= 1");
    if (int rc = gpmpc_pt_check_bp(who, B, P)) return rc;
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!x_prev || !U_p || !eps || !out_next || !workspace) return gpmpc_refuse(who, "NULL pointer");
    gpmpc_carver c;
    const PtStepLayout S = pt_step_layout(m, B, P, chunk, c);
    if (workspace_bytes < S.total) return GPMPC_E_WORKSPACE;
    return pt_step(m, noise, B, P, x_prev, nullptr, 0, eps, out_next, out_mean, out_var, S, (char*)workspace, (hipStream_t)stream, U_p);
}

static int pt_stats(int B, int P, int T, int ds, const double* particles, const double* var, int t0v, const gpmpc_state_constraints* cons,
                    double* out_mean, double* out_cov, int* out_clamped, double* out_viol, double* out_joint, hipStream_t s) {
    gpmpc_state_constraints cz;
    memset(&cz, 0, sizeof(cz));
    const int n_rows = cons ? cons->n_rows : 0;
    hipLaunchKernelGGL(k_pt_stats, dim3(T, B), dim3(MPPI_THREADS), 0, s, B, P, T, ds, particles, var, t0v, n_rows, cons ? *cons : cz, out_mean,
                       out_cov, var ? out_clamped : nullptr, out_viol);
    if (cons) hipLaunchKernelGGL(k_pt_joint, dim3(B), dim3(MPPI_THREADS), 0, s, B, P, T, ds, particles, n_rows, *cons, out_joint);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

static int pt_check_stats_args(const char* who, int B, int P, int T, const gpmpc_state_constraints* cons, const double* out_viol,
                               const double* out_joint) {
    if (int rc = gpmpc_pt_check_bp(who, B, P)) return rc;
    if (T < 1 || T > 65535) return gpmpc_refuse(who, "T (steps) outside 1...65535");
    if (B > 65535) return gpmpc_refuse(who, "B > 65535");
    if ((long)B * P * GPMPC_MAX_DS * T > (1L << 40)) return gpmpc_refuse(who, "more than 2^40 particle values");
    if (cons) { if (int rc = gpmpc_check_constraints(cons, who)) return rc; }
    if ((cons != nullptr) != (out_viol != nullptr) || (cons != nullptr) != (out_joint != nullptr))
        return gpmpc_refuse(who, "out_viol and out_joint are given exactly when constraint rows are");
    return GPMPC_OK;
}

extern "C" int gpmpc_particle_stats(int B, int P, int T, int ds, const double* particles, const double* var,
                                    const gpmpc_state_constraints* cons, double* out_mean, double* out_cov, int* out_clamped,
                                    double* out_viol, double* out_joint, void* stream) {
    const char* who = "gpmpc_particle_stats";
    if (ds < 1 || ds > GPMPC_MAX_DS) return gpmpc_refuse(who, "state_dim = %d outside 1...GPMPC_MAX_DS", ds);
    if (int rc = pt_check_stats_args(who, B, P, T, cons, out_viol, out_joint)) return rc;
    if (!particles) return gpmpc_refuse(who, "NULL pointer");
    if ((var != nullptr) != (out_clamped != nullptr)) return gpmpc_refuse(who, "var and out_clamped are given together");
    return pt_stats(B, P, T, ds, particles, var, 0, cons, out_mean, out_cov, out_clamped, out_viol, out_joint, (hipStream_t)stream);
}

// workspace of a rollout: eps [P][da + ds] | var [H][B P][ds] | a step's
// under feedback without out_inputs: | inputs [H][B P][da]
struct PtRollLayout { size_t off_eps, off_var; PtStepLayout step; size_t off_u, total; };
static PtRollLayout pt_roll_layout(const gpmpc_gp_model* m, int B, int P, int H, int chunk, bool ubuf = false) {
    PtRollLayout R;
    gpmpc_carver c;
    R.off_eps = c.take(sizeof(double) * (size_t)P * PT_MAX_NORMALS);
    R.off_var = c.take(sizeof(double) * (size_t)H * B * P * m->state_dim);
    R.step = pt_step_layout(m, B, P, chunk, c);
    R.off_u = c.take(ubuf ? sizeof(double) * (size_t)H * B * P * m->action_dim : 0);
    R.total = c.total();
    return R;
}

// what gpmpc_particle_rollout_feedback adds to gpmpc_particle_rollout
struct PtFeedback {
    const double* K; size_t kss; const double* mu_ref; const gpmpc_input_constraints* ucons;
    double *out_inputs, *out_umean, *out_ucov, *out_uviol, *out_ujoint;
};
static int pt_rollout(const char* who, const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U, unsigned long long seed,
                      unsigned call_index, const gpmpc_state_constraints* cons, double* out_particles, double* out_mean, double* out_cov,
                      int* out_clamped, double* out_viol, double* out_joint, int chunk, void* workspace, size_t workspace_bytes, void* stream,
                      const PtFeedback* fb);

extern "C" size_t gpmpc_particle_rollout_workspace_bytes(const gpmpc_gp_model* m, int B, int P, int H, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || B < 1 || P < 1 || H < 1 || H > 65534 || (long)B * P * GPMPC_MAX_D > 0x7fffffffL || !gpmpc_chunk_ok(chunk)) return 0;
    return pt_roll_layout(m, B, P, H, chunk).total;
}

extern "C" int gpmpc_particle_rollout(const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U,
                                      unsigned long long seed, unsigned call_index, const gpmpc_state_constraints* cons,
                                      double* out_particles, double* out_mean, double* out_cov, int* out_clamped, double* out_viol,
                                      double* out_joint, int chunk, void* workspace, size_t workspace_bytes, void* stream) {
    return pt_rollout("gpmpc_particle_rollout", m, B, P, H, x0, U, seed, call_index, cons, out_particles, out_mean, out_cov, out_clamped, out_viol,
                      out_joint, chunk, workspace, workspace_bytes, stream, nullptr);
}

// The particle rollout under u^p_t = v_t + K_t (x^p_t - mu_ref_t): the arguments of gpmpc_particle_rollout, the same noise addressing (no new
// normals are drawn), each step the chain gpmpc_particle_noise -> gpmpc_particle_inputs -> gpmpc_particle_step_inputs.
extern "C" size_t gpmpc_particle_rollout_feedback_workspace_bytes(const gpmpc_gp_model* m, int B, int P, int H, int chunk, int want_inputs) {
    if (!m || m->action_dim < 1 || gpmpc_particle_rollout_workspace_bytes(m, B, P, H, chunk) == 0) return 0;
    return pt_roll_layout(m, B, P, H, chunk, want_inputs == 0).total;
}

extern "C" int gpmpc_particle_rollout_feedback(const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U,
                                               unsigned long long seed, unsigned call_index, const gpmpc_state_constraints* cons,
                                               double* out_particles, double* out_mean, double* out_cov, int* out_clamped, double* out_viol,
                                               double* out_joint, const double* K_dev, size_t k_step_stride, const double* mu_ref,
                                               const gpmpc_input_constraints* ucons, double* out_inputs, double* out_umean, double* out_ucov,
                                               double* out_uviol, double* out_ujoint, int chunk, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    const PtFeedback fb = {K_dev, k_step_stride, mu_ref, ucons, out_inputs, out_umean, out_ucov, out_uviol, out_ujoint};
    return pt_rollout("gpmpc_particle_rollout_feedback", m, B, P, H, x0, U, seed, call_index, cons, out_particles, out_mean, out_cov, out_clamped,
                      out_viol, out_joint, chunk, workspace, workspace_bytes, stream, &fb);
}

static int pt_rollout(const char* who, const gpmpc_gp_model* m, int B, int P, int H, const double* x0, const double* U, unsigned long long seed,
                      unsigned call_index, const gpmpc_state_constraints* cons, double* out_particles, double* out_mean, double* out_cov,
                      int* out_clamped, double* out_viol, double* out_joint, int chunk, void* workspace, size_t workspace_bytes, void* stream,
                      const PtFeedback* fb) {
    PtNoise noise;
    if (int rc = pt_check_model(who, m, &noise)) return rc;
    if (H < 1) return gpmpc_refuse(who, "H < 1");
    if (int rc = pt_check_stats_args(who, B, P, H + 1, cons, out_viol, out_joint)) return rc;
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!x0 || !out_particles || !out_mean || !out_cov || !out_clamped || !workspace || (m->action_dim > 0 && !U))
        return gpmpc_refuse(who, "NULL pointer");
    if (fb) {
        const size_t full = (size_t)m->action_dim * m->state_dim;
        if (m->action_dim < 1) return gpmpc_refuse(who, "a state feedback needs action_dim >= 1");
        if (fb->kss != 0 && fb->kss != full) return gpmpc_refuse(who, "k_step_stride must be 0 or action_dim state_dim");
        if (fb->K && !fb->mu_ref) return gpmpc_refuse(who, "a gain needs the mean trajectory it acts around (mu_ref is NULL)");
        if (!fb->out_umean || !fb->out_ucov) return gpmpc_refuse(who, "NULL pointer (out_umean, out_ucov)");
        if (fb->ucons) { if (int rc = gpmpc_lpi_check_rows(who, fb->ucons)) return rc; }
        if ((fb->ucons != nullptr) != (fb->out_uviol != nullptr) || (fb->ucons != nullptr) != (fb->out_ujoint != nullptr))
            return gpmpc_refuse(who, "out_uviol and out_ujoint are given exactly when input rows are");
    }
    const PtRollLayout R = pt_roll_layout(m, B, P, H, chunk, fb && !fb->out_inputs);
    if (workspace_bytes < R.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int ds = m->state_dim, da = m->action_dim;
    const size_t slab = (size_t)B * P * ds;
    double* eps = (double*)(ws + R.off_eps);
    double* var = (double*)(ws + R.off_var);
    if (int rc = pt_launch_noise(P, ds, 0, seed, call_index, eps, s)) return rc;
    PtVec L;
    memcpy(L.v, noise.L, sizeof(L.v));
    hipLaunchKernelGGL(k_pt_init, dim3(gpmpc_blocks256((long)slab)), dim3(256), 0, s, B, P, ds, x0, (const double*)eps, L, out_particles);
    double* inputs = fb ? (fb->out_inputs ? fb->out_inputs : (double*)(ws + R.off_u)) : nullptr;
    const size_t uslab = (size_t)B * P * da;
    for (int t = 1; t <= H; ++t) {
        if (int rc = pt_launch_noise(P, da + ds, t, seed, call_index, eps, s)) return rc;
        double* u_t = fb ? inputs + (size_t)(t - 1) * uslab : nullptr;
        if (fb)
            if (int rc = gpmpc_lpi_particle_inputs(B, P, ds, da, out_particles + (size_t)(t - 1) * slab, U + (size_t)(t - 1) * da, (size_t)H * da,
                                                   fb->K ? fb->K + (size_t)(t - 1) * fb->kss : nullptr,
                                                   fb->mu_ref ? fb->mu_ref + (size_t)(t - 1) * ds : nullptr, (size_t)(H + 1) * ds, u_t, s))
                return rc;
        if (int rc = pt_step(m, noise, B, P, out_particles + (size_t)(t - 1) * slab, U ? U + (size_t)(t - 1) * da : nullptr, (size_t)H * da, eps,
                             out_particles + (size_t)t * slab, nullptr, var + (size_t)(t - 1) * slab, R.step, ws, s, u_t))
            return rc;
    }
    if (int rc = pt_stats(B, P, H + 1, ds, out_particles, var, 1, cons, out_mean, out_cov, out_clamped, out_viol, out_joint, s)) return rc;
    if (fb) return gpmpc_lpi_input_stats(B, P, H, da, inputs, fb->ucons, fb->out_umean, fb->out_ucov, fb->out_uviol, fb->out_ujoint, s);
    return GPMPC_OK;
}
