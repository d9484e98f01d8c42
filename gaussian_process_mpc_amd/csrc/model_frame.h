// The frame the entries that take a gpmpc_gp_model share (particles.hip, particle_cost.hip, linprop.hip, linprop_stream.hip,
// linprop_fc.hip), the sibling of solver_frame.h: the size, chunk and model checks, the grouping of the GPs, the hyper-parameters by GP and
// the pivots of init_cov.  The ORDER of the checks is behaviour -- a call with two faults is refused for the earlier one -- and the shared
// prefix of it is written down once, here (tests/test_host_model_frame.py holds every entry to it).  Host only.
#pragma once
#include <cfloat>
#include <cmath>
#include "gpmpc_internal.h"

#define GPMPC_MODEL_TILE 64                 // columns of one tile of the kernels behind these entries (SP_T of tile_stage.h: asserted where both are seen)
#define GPMPC_MODEL_DEFAULT_CHUNK 4096      // columns per set of launches where the caller passes chunk = 0

static inline bool gpmpc_finite(double v) { return v - v == 0.0; }
static inline unsigned gpmpc_blocks256(long threads) { return (unsigned)((threads + 255) / 256); }

// what the gpmpc_*_workspace_bytes entries accept of a model, and of a chunk
static inline bool gpmpc_model_sizes_ok(const gpmpc_gp_model* m) {
    return m && m->state_dim >= 1 && m->state_dim <= GPMPC_MAX_DS && m->action_dim >= 0 && m->state_dim + m->action_dim <= GPMPC_MAX_D && m->n >= 1;
}
static inline bool gpmpc_chunk_ok(int chunk) { return chunk >= 0 && chunk % GPMPC_MODEL_TILE == 0; }
static inline int gpmpc_check_chunk(const char* who, int chunk) {
    return gpmpc_chunk_ok(chunk) ? GPMPC_OK : gpmpc_refuse(who, "chunk must be 0 or a positive multiple of 64");
}
// the columns of one set of launches: `chunk` (0: the default), but no more than the call has, rounded up to whole tiles
static inline int gpmpc_chunk_cols(long ncols, int chunk) {
    const long colsp = (ncols + GPMPC_MODEL_TILE - 1) / GPMPC_MODEL_TILE * GPMPC_MODEL_TILE, ch = chunk == 0 ? GPMPC_MODEL_DEFAULT_CHUNK : chunk;
    return (int)(colsp < ch ? colsp : ch);
}

// What every entry refuses of a model before it looks at the noise model: sizes, n, ld, arrays, sigma_f / lambdas GP by GP, a non-finite
// nominal model.
static inline int gpmpc_model_check_core(const char* who, const gpmpc_gp_model* m) {
    if (!m) return gpmpc_refuse(who, "NULL pointer (model)");
    const int ds = m->state_dim, da = m->action_dim, D = ds + da;
    if (ds < 1 || ds > GPMPC_MAX_DS) return gpmpc_refuse(who, "state_dim = %d outside 1...GPMPC_MAX_DS", ds);
    if (da < 0 || D > GPMPC_MAX_D) return gpmpc_refuse(who, "action_dim = %d: D = state_dim + action_dim outside 1...GPMPC_MAX_D", da);
    if (m->n < 1) return gpmpc_refuse(who, "n < 1");
    if (m->ld < (size_t)m->n) return gpmpc_refuse(who, "ld < n");
    if (!m->X || !m->beta || !m->Kinv) return gpmpc_refuse(who, "NULL pointer (model arrays)");
    for (int a = 0; a < ds; ++a) {
        if (!(m->sigma_f[a] > 0.0) || !gpmpc_finite(m->sigma_f[a])) return gpmpc_refuse(who, "sigma_f[%d] = %g is not positive and finite", a, m->sigma_f[a]);
        for (int d = 0; d < D; ++d)
            if (!(m->lambdas[a * D + d] > 0.0) || !gpmpc_finite(m->lambdas[a * D + d]))
                return gpmpc_refuse(who, "lambdas[%d][%d] = %g is not positive and finite", a, d, m->lambdas[a * D + d]);
    }
    if (m->has_nominal)
        for (int a = 0; a < ds; ++a) {
            if (!gpmpc_finite(m->nom_b[a])) return gpmpc_refuse(who, "the nominal model holds a non-finite value");
            for (int d = 0; d < D; ++d)
                if (!gpmpc_finite(m->nom_w[a * D + d])) return gpmpc_refuse(who, "the nominal model holds a non-finite value");
        }
    return GPMPC_OK;
}

// A group of GPs with bit-identical (lambda, sigma_f): a kernel argument of the TILE kernels of particles.hip and linprop.hip
struct GpGroup {
    double ilam[GPMPC_MAX_D];       // 1 / lambda_d
    double sf2;
    int ng;                         // GPs of the group
    int gp[GPMPC_MAX_DS];           // their indices, ascending
};
// the groups of a checked model, in order of their first GP; returns their number
static inline int gpmpc_model_groups(const gpmpc_gp_model* m, GpGroup* g) {
    const int ds = m->state_dim, D = ds + m->action_dim;
    int ngroups = 0;
    bool done[GPMPC_MAX_DS] = {};
    for (int a = 0; a < ds; ++a) {
        if (done[a]) continue;
        GpGroup& G = g[ngroups++];
        memset(&G, 0, sizeof(G));
        for (int d = 0; d < D; ++d) G.ilam[d] = 1.0 / m->lambdas[a * D + d];
        G.sf2 = m->sigma_f[a] * m->sigma_f[a];
        for (int b = a; b < ds; ++b)
            if (!done[b] && memcmp(&m->lambdas[a * D], &m->lambdas[b * D], sizeof(double) * D) == 0 &&
                memcmp(&m->sigma_f[a], &m->sigma_f[b], sizeof(double)) == 0) {
                done[b] = true;
                G.gp[G.ng++] = b;
            }
    }
    return ngroups;
}

// The lower Cholesky factor L (ds x ds, zeroed by the caller) of the symmetric P, column by column.  A pivot within rounding of zero (16 ulp
// of the diagonal entry it is left of) gives a zero column: zero variances are legal.  One below -1e-12 `big` (the caller's max |P|) is not:
// false, with the pivot and its index for the caller's refusal.
static inline bool gpmpc_psd_pivots(const double* P, int ds, double big, double* L, double* bad_pivot, int* bad_index) {
    for (int j = 0; j < ds; ++j) {
        double d = P[j * ds + j];
        for (int k = 0; k < j; ++k) d -= L[j * ds + k] * L[j * ds + k];
        if (d < -1e-12 * big) { *bad_pivot = d; *bad_index = j; return false; }
        if (d <= 16.0 * DBL_EPSILON * P[j * ds + j]) continue;      // (also d <= 0 with a zero diagonal entry)
        const double r = sqrt(d);
        L[j * ds + j] = r;
        for (int i = j + 1; i < ds; ++i) {
            double s = P[i * ds + j];
            for (int k = 0; k < j; ++k) s -= L[i * ds + k] * L[j * ds + k];
            L[i * ds + j] = s / r;
        }
    }
    return true;
}
