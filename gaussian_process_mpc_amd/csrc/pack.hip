// The pack's lifecycle: creation (every device buffer, and all index data -- work lists, pair table, one-lambda tile tables -- in ONE
// arena), resize, destruction; the GPMPC_* tuning reader; the nominal and noise models.  What a build computes: pack_build.hip; how the
// lists are ordered: worklist.h.
#include "gpmpc_internal.h"
#include "worklist.h"
#include <cstdlib>
#include <memory>
#include <new>
#include <utility>

// Host-side views of launch geometry, for tests that run without a GPU (include/gpmpc.h, "launch geometry")
static int copy_out(const std::vector<int>& src, int per_item, int* dst, int capacity, int* n_items) {
    const int k = (int)(src.size() / per_item);
    *n_items = k;
    if (k > 0 && k <= capacity) memcpy(dst, src.data(), sizeof(int) * src.size());
    return (k > capacity && capacity > 0) ? GPMPC_E_ARG : GPMPC_OK;
}
extern "C" int gpmpc_debug_run_list(int n_padded, int state_dim, int slots, int* items_out, int capacity, int* n_items) try {
    if (n_padded < 64 || n_padded % 64 || state_dim < 1 || state_dim > GPMPC_MAX_DS || !n_items || capacity < 0 || (capacity > 0 && !items_out)) return GPMPC_E_ARG;
    return copy_out(gpmpc_build_run_list(n_padded, state_dim, slots).items, 4, items_out, capacity, n_items);
} catch (const std::bad_alloc&) { return GPMPC_E_ALLOC; }
extern "C" int gpmpc_debug_work_list(int n_padded, int rows_per_tile, int cols_per_tile, int n_tri_units, int n_cross_units, int xcd_sort, int tile_slot,
                                     int* items_out, int capacity, int* n_items, int* perm_out, int* ustart_out) try {
    if (n_padded < 64 || n_padded % 64 || rows_per_tile < 64 || rows_per_tile % 64 || cols_per_tile < 8 || cols_per_tile % 8 || n_tri_units < 0 ||
        n_tri_units > GPMPC_MAX_DS || n_cross_units < 0 || n_cross_units > GPMPC_MAX_PAIRS || n_tri_units + n_cross_units < 1 || !n_items ||
        capacity < 0 || (capacity > 0 && (!items_out || !perm_out || !ustart_out))) return GPMPC_E_ARG;
    const gpmpc_tile_list t = gpmpc_build_tile_list(n_padded, rows_per_tile, cols_per_tile, n_tri_units, n_cross_units, xcd_sort != 0, tile_slot != 0);
    const int rc = copy_out(t.items, 4, items_out, capacity, n_items);
    if (rc == GPMPC_OK && capacity > 0) {
        std::copy(t.perm.begin(), t.perm.end(), perm_out);
        std::copy(t.ustart.begin(), t.ustart.end(), ustart_out);
    }
    return rc;
} catch (const std::bad_alloc&) { return GPMPC_E_ALLOC; }
extern "C" int gpmpc_debug_fcs_tables(int n_padded, int state_dim, int cols_per_tile, int* ntile_out, int* tiles_out, int capacity, int* n_tiles,
                                      int* ustart_out) try {
    if (n_padded < 64 || n_padded % 64 || state_dim < 2 || state_dim > 4 || cols_per_tile < 64 || cols_per_tile % 64 || !ntile_out || !n_tiles ||
        capacity < 0 || (capacity > 0 && (!tiles_out || !ustart_out))) return GPMPC_E_ARG;
    const int npairs = state_dim * (state_dim - 1) / 2;
    const gpmpc_fcs_tiles f = gpmpc_build_fcs_tiles(n_padded);
    std::copy(f.ntile, f.ntile + 3, ntile_out);
    const int rc = copy_out(f.tiles256, 3, tiles_out, capacity, n_tiles);
    if (rc == GPMPC_OK && capacity > 0) {
        const std::vector<int> ust = gpmpc_build_tile_list(n_padded, 256, cols_per_tile, state_dim, npairs, false, false).ustart;
        for (int q = 0; q < 3; ++q) {
            const std::vector<int> u = gpmpc_fcs_ustart(ust, state_dim, npairs, f.ntile[q]);
            std::copy(u.begin(), u.end(), ustart_out + q * (state_dim + npairs + 1));
        }
    }
    return rc;
} catch (const std::bad_alloc&) { return GPMPC_E_ALLOC; }
extern "C" int gpmpc_debug_xcd_order(int linear_id, int grid_x, int n_tile, int n_traj, int* traj, int* column) {
    if (!traj || !column || grid_x < 1 || n_tile < 1 || n_tile > grid_x || n_traj < 1 || linear_id < 0 || (long)linear_id >= (long)grid_x * n_traj) return GPMPC_E_ARG;
    unsigned bx = 0;
    gpmpc_xcd_remap(linear_id, grid_x, n_tile, n_traj, traj, &bx);
    *column = (int)bx;
    return GPMPC_OK;
}

void gpmpc_read_tuning(gpmpc_tuning* t) {
    auto geti = [](const char* name, int unset) { const char* ev = getenv(name); return ev ? atoi(ev) : unset; };
    t->pair_sb = geti("GPMPC_PAIR_SB", -1);
    t->tiling = geti("GPMPC_TILING", -1);
    t->tb = geti("GPMPC_PAIR_TB", 0);
    t->rgroup = geti("GPMPC_RGROUP", 0);
    t->no_first = getenv("GPMPC_NO_FIRST") ? 1 : 0;
    t->fused = geti("GPMPC_FUSED", -1);
    t->no_xcd_sort = getenv("GPMPC_NO_XCD_SORT") ? 1 : 0;
    t->hchunks = geti("GPMPC_HEAD_CHUNKS", -1);
    t->sbf_min = geti("GPMPC_SBF_MIN", 0);
    t->shared = geti("GPMPC_SHARED", -1);
    t->colunroll = geti("GPMPC_SB_UNROLL", -1);
    t->split = geti("GPMPC_SPLIT", -1);
    t->fused_sb = geti("GPMPC_FUSED_SB", -1);
    t->persist = geti("GPMPC_PERSIST", -1);
    t->xcdmap = geti("GPMPC_XCDMAP", -1);
    t->fc_shared = geti("GPMPC_FC_SHARED", -1);
    t->fc_form = geti("GPMPC_FC_FORM", -1);
    t->fc_tiling = geti("GPMPC_FC_TILING", -1);
    t->fc_rsplit = geti("GPMPC_FC_RSPLIT", 0);
    t->fc_cu = geti("GPMPC_FC_CU", 0);
    t->step1_quad = geti("GPMPC_STEP1_QUAD", -1);
    t->step1_t = geti("GPMPC_STEP1_T", 0);
}

extern "C" int gpmpc_pack_reload_tuning(gpmpc_pack* p) {
    if (!p) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;   // the caches below hold streams / buffers of the pack's device
    const int keep = p->tune.no_xcd_sort;             // baked into the work list at creation
    gpmpc_read_tuning(&p->tune);
    p->tune.no_xcd_sort = keep;
    if (p->graph_cache) { gpmpc_graph_cache_free(p->graph_cache); p->graph_cache = nullptr; }   // captured under the old plan
    if (p->cb_cache) { gpmpc_cb_cache_free(p->cb_cache); p->cb_cache = nullptr; }
    gpmpc_tuned_clear(p->tuned);
    return GPMPC_OK;
}

// The defaults of the noise model (the reference's constants), written into the parts asked for of a [GPMPC_NOISE_MAX] host image
static void noise_defaults(int ds, int da, double* img, bool init, bool action, bool process) {
    if (init) for (int k = 0; k < ds; ++k) for (int l = 0; l < ds; ++l) img[k * ds + l] = k == l ? GPMPC_INIT_VAR : 0.0;
    if (action) for (int j = 0; j < da; ++j) img[gpmpc_noise_off_action(ds) + j] = GPMPC_ACTION_VAR;
    if (process) for (int a = 0; a < ds; ++a) img[gpmpc_noise_off_process(ds, da) + a] = 0.0;
}

// The pack's index data on the host: sections, each with the pointer field of the pack it is known by.  image() lays them out, every section
// on a 256-byte boundary, for the ONE upload; point() then sets the fields into the arena (gpmpc_pack::index_dev).  A section that is not
// built leaves its field null.
struct IndexImage {
    struct Section { int** field; std::vector<int> data; size_t at; };
    std::vector<Section> sections;
    static size_t padded(size_t n) { return (n + 63) & ~(size_t)63; }
    void add(int** field, std::vector<int> v) { if (!v.empty()) sections.push_back({field, std::move(v), 0}); }
    void add(gpmpc_worklist* w, gpmpc_tile_list t, int it, int jt) {
        w->it = it; w->waves = it / 64 > 0 ? it / 64 : 1; w->jt = jt; w->nunits = (int)t.ustart.size() - 1; w->nwork = t.n();
        w->contiguous = t.perm.empty() ? 1 : 0;
        std::copy(t.ustart.begin(), t.ustart.end(), w->ustart_host);
        add(&w->work_dev, std::move(t.items)); add(&w->perm_dev, std::move(t.perm)); add(&w->ustart_dev, std::move(t.ustart));
    }
    std::vector<int> image() {
        size_t total = 0;
        for (Section& sec : sections) { sec.at = total; total += padded(sec.data.size()); }
        std::vector<int> host;
        host.reserve(total);
        for (const Section& sec : sections) { host.insert(host.end(), sec.data.begin(), sec.data.end()); host.resize(sec.at + padded(sec.data.size())); }
        return host;
    }
    void point(int* arena) const { for (const Section& sec : sections) *sec.field = arena + sec.at; }
};

// Every device buffer a pack owns: the ONE table that creation allocates from and destruction frees by.  bytes 0: allocated on first use
// (gpmpc_pack_set_nominal; the first build or enable_fullcov that serves the one-lambda full-covariance form, pack_build.hip).
struct PackBuffer { void** ptr; size_t bytes; const char* name; };
static std::array<PackBuffer, 12> pack_buffers(gpmpc_pack* p, size_t index_ints = 0) {
    const size_t Np = p->Np, ds = p->ds, D = p->D, dbl = sizeof(double);
    return {{{(void**)&p->X, dbl * Np * D, "X"}, {(void**)&p->XT, dbl * Np * D, "XT"}, {(void**)&p->beta, dbl * Np * ds, "beta"},
             {(void**)&p->M, dbl * Np * Np * ds, "the weight matrices"}, {(void**)&p->lam, dbl * ds * D, "lambda"}, {(void**)&p->sf, dbl * ds, "sigma_f"},
             {(void**)&p->noise_dev, dbl * GPMPC_NOISE_MAX, "the noise model"}, {(void**)&p->index_dev, sizeof(int) * index_ints, "the index data"},
             {(void**)&p->nom_dev, 0, "the nominal model"}, {(void**)&p->resid_dev, 0, "the residual targets"}, {(void**)&p->fcs_rows, 0, "the one-lambda column rows"},
             {(void**)&p->M1, 0, "the step-1 weights"}}};
}

extern "C" int gpmpc_pack_destroy(gpmpc_pack* p) {
    if (!p) return GPMPC_OK;
    for (const PackBuffer& b : pack_buffers(p)) if (*b.ptr) (void)hipFree(*b.ptr);
    if (p->m1_event) (void)hipEventDestroy((hipEvent_t)p->m1_event);
    gpmpc_graph_cache_free(p->graph_cache);
    gpmpc_cb_cache_free(p->cb_cache);
    gpmpc_tuned_free(p->tuned);
    gpmpc_lock_destroy(p->lock);
    delete p;
    return GPMPC_OK;
}

struct PackDestroy { void operator()(gpmpc_pack* p) const { gpmpc_pack_destroy(p); } };

extern "C" int gpmpc_pack_create(gpmpc_pack** out, int n_train, int state_dim, int action_dim) try {
    if (!out || n_train < 1 || state_dim < 1 || action_dim < 0) return GPMPC_E_ARG;
    const int D = state_dim + action_dim;
    if (D > GPMPC_MAX_D || state_dim > GPMPC_MAX_DS || D < 1) return GPMPC_E_ARG;
    std::unique_ptr<gpmpc_pack, PackDestroy> pk(new gpmpc_pack());       // (zeroed; whatever exists of it is destroyed on every early return)
    gpmpc_pack* p = pk.get();
    p->N = n_train; p->Np = ((n_train + 63) / 64) * 64; p->ds = state_dim; p->da = action_dim; p->D = D;
    gpmpc_read_tuning(&p->tune);
    p->lock = gpmpc_lock_create();
    if (!p->lock) { gpmpc_set_error_text("gpmpc_pack_create: out of host memory"); return GPMPC_E_ALLOC; }
    if (hipError_t ed = hipGetDevice(&p->device); ed != hipSuccess) { gpmpc_set_error("gpmpc_pack_create: hipGetDevice", ed); return GPMPC_E_LAUNCH; }
    if (hipDeviceGetAttribute(&p->num_cu, hipDeviceAttributeMultiprocessorCount, p->device) != hipSuccess || p->num_cu < 1) p->num_cu = 256;
    IndexImage img;
    const int nc0 = p->Np;
    p->ncol_host = nc0;
    img.add(&p->ncol_dev, {nc0});
    std::vector<int> hab;
    for (int a = 0; a < state_dim; ++a)
        for (int b = a + 1; b < state_dim; ++b) { p->pair_a[p->npairs] = a; p->pair_b[p->npairs] = b; ++p->npairs; hab.insert(hab.end(), {a, b}); }
    img.add(&p->pair_ab_dev, std::move(hab));
    // 256-row workgroups: 512 / 1024 rows would cut the G-row re-reads 2x / 4x but ran 8 % / 46 % slower on C3 (C4: -1 %).
    // 256x64: scalar-broadcast kernel for small batches of a large N (enough workgroups to fill the chip at B = 1).
    // 64x128: staged kernel for B = 1 of a large N (fewer partial sums to reduce per step: N = 2048 1.30 -> 1.18 ms per
    // rollout; N <= 512 is 10 % slower on it and stays on 64x64).
    // 256x128: between the 256x64 and the 256x256 shapes, two trajectories per wave (round 3: N = 2048, B = 24 / 32 +19 / +21 %
    // against 256x64, N = 1024, B = 96 / 128 +10 / +14 %; -3...-4 % against 256x256 from ~5 generations of workgroups on).
    // 256x32 / 256x16: the one-launch-per-step form (step_fused.h) on launches that would leave most of the chip without a workgroup
    // (B = 1...4 of a large N): narrower tiles, more and shorter-lived tile workgroups.
    int cfg[7][2] = {{256, 256}, {64, 64}, {256, 64}, {64, 128}, {256, 128}, {256, 32}, {256, 16}};
    if (const char* ev = getenv("GPMPC_JT0")) { const int v = atoi(ev); if (v >= 64 && v % 64 == 0) cfg[0][1] = v; }   // A/B: column extent of the large tiles
    const bool xcd = !p->tune.no_xcd_sort;
    for (int mode = 0; mode < 2; ++mode)
        for (int k = 0; k < 7; ++k) {
            if (mode == 1 && k >= 2 && k != 2 && k != 4) continue;      // full-covariance units: 256x256, 64x64, and 256x64 / 256x128 for small batches (fullcov.hip)
            img.add(&p->wl[mode][k], gpmpc_build_tile_list(p->Np, cfg[k][0], cfg[k][1], state_dim, mode ? p->npairs : 0, mode == 0 && (k == 0 || k == 4) && xcd, false),
                    cfg[k][0], cfg[k][1]);
        }
    // Measured (tools/lib_ab.py, profiles/r05/ab17_runs.txt; ms per rollout of ONE trajectory, 256x64 tiles | runs): N = 4096, ds = 6, da = 1, H = 30
    // 3.63 | 3.34; N = 3584, ds = 5, da = 1, H = 20 1.48 | 1.35; N = 4096, ds = 4, da = 2 1.44 | 1.37; but ds = 4, da = 1 (D = 5, five waves per
    // SIMD) 1.25 | 1.35: there the plain list already streams the weights at 4.3 TB/s, the rate of the full-covariance pair kernel (the
    // practical ceiling of this access pattern), and longer workgroups only lose its overlap of prologues with loops.  From D = 6.
    if (D >= 6 && !getenv("GPMPC_NO_RUNS")) {
        // (workgroup slots of the one-launch form on 256-row tiles: 4 waves per SIMD from D = 6, 5 below -- step_fused.h's launch bounds)
        const int occ = 4;
        // (the launch carries 2 ds more workgroups behind the tiles -- mean sums and finish, step_fused.h --: they need slots of the same generation)
        gpmpc_tile_list runs = gpmpc_build_run_list(p->Np, state_dim, p->num_cu * occ - 2 * state_dim);
        if (runs.n() > 0) img.add(&p->wl[0][7], std::move(runs), 256, 256);
    }
    // shared-lambda work lists (pair_kernel_sbs.h): "units" are groups of sh_ng GPs
    if (state_dim >= 2 && action_dim >= 1 && action_dim <= 2) {
        p->sh_ng = gpmpc_sbs_group(state_dim, D);
        if (const char* ev = getenv("GPMPC_SHARED_NG")) { const int v = atoi(ev); if (v >= 2 && v <= 4 && v <= state_dim) p->sh_ng = v; }   // A/B (at pack creation)
        const int groups = (state_dim + p->sh_ng - 1) / p->sh_ng;
        const int sh_cfg[3][2] = {{cfg[0][1], xcd}, {64, false}, {128, xcd}};
        for (int k = 0; k < 3; ++k) {
            gpmpc_tile_list t = gpmpc_build_tile_list(p->Np, 256, sh_cfg[k][0], groups, 0, sh_cfg[k][1] != 0, true);
            p->sh_tiles[k] = t.tiles;
            img.add(&p->wl_sh[k], std::move(t), 256, sh_cfg[k][0]);
        }
        if (p->sh_ng > 2 && state_dim % 2 == 0) img.add(&p->wl_sh[3], gpmpc_build_tile_list(p->Np, 256, 64, state_dim / 2, 0, false, true), 256, 64);
    }
    // one lambda for all GPs, full-covariance rollout: the tables of every shape that can ever take that path (fullcov.hip needs the column
    // rows too, which the first build that serves it allocates: pack_build.hip)
    if (gpmpc_fcs_shape(state_dim, action_dim)) {
        gpmpc_fcs_tiles f = gpmpc_build_fcs_tiles(p->Np);
        p->fcs_rw = (D + 1 + state_dim + 1) & ~1;
        p->fcs_tj = p->Np / 64;
        std::copy(f.ntile, f.ntile + 3, p->fcs_ntile);
        img.add(&p->fcs_tiles256_dev, std::move(f.tiles256));
        for (int k : {0, 2, 4}) {
            const gpmpc_worklist& w = p->wl[1][k];
            const std::vector<int> ust(w.ustart_host, w.ustart_host + w.nunits + 1);
            p->fcs_base[k] = ust[state_dim];
            for (int q = 0; q < 3; ++q) {
                std::vector<int> u = gpmpc_fcs_ustart(ust, state_dim, p->npairs, f.ntile[q]);
                p->fcs_total[k][q] = u.back();
                img.add(&p->fcs_ustart_dev[k][q], std::move(u));
            }
        }
    }
    noise_defaults(p->ds, p->da, p->noise_host, true, true, true);
    const std::vector<int> index = img.image();
    hipError_t e = hipSuccess;
    const char* what = nullptr;
    for (const PackBuffer& b : pack_buffers(p, index.size())) {
        if (e != hipSuccess || b.bytes == 0) continue;
        what = b.name;
        if ((e = hipMalloc(b.ptr, b.bytes)) != hipSuccess) *b.ptr = nullptr;
    }
    if (e == hipSuccess) { what = "the upload of the noise model"; e = hipMemcpy(p->noise_dev, p->noise_host, sizeof(double) * GPMPC_NOISE_MAX, hipMemcpyHostToDevice); }
    if (e == hipSuccess) { what = "the upload of the index data"; e = hipMemcpy(p->index_dev, index.data(), sizeof(int) * index.size(), hipMemcpyHostToDevice); }
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gpmpc_pack_create: %s", what);
        gpmpc_set_error(msg, e);
        return GPMPC_E_ALLOC;
    }
    img.point(p->index_dev);
    *out = pk.release();
    return GPMPC_OK;
} catch (const std::bad_alloc&) {
    gpmpc_set_error_text("gpmpc_pack_create: out of host memory");
    return GPMPC_E_ALLOC;
}

// Re-use a pack for a training set of a different size with the SAME padded size (the closed loop grows the set by one
// observation per step, src/simulator.py:55: the padded size changes every 64 steps only).  Everything allocated at creation
// depends on the padded size alone, and so do the rollout's launches (rows >= N carry zero weights; no rollout kernel reads
// N): the captured launch sequences of the pack stay valid and are replayed on the refilled buffers.
extern "C" int gpmpc_pack_resize(gpmpc_pack* p, int n_train) {
    if (!p || n_train < 1) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    if (((n_train + 63) / 64) * 64 != p->Np) return GPMPC_E_ARG;
    p->N = n_train;
    p->built = 0;
    return GPMPC_OK;
}

// Linear nominal model of the rollout: GP a corrects m_a(z) = weights[a] . z + bias[a].  Both NULL clears it.
extern "C" int gpmpc_pack_set_nominal(gpmpc_pack* p, const double* weights_host, const double* bias_host, void* stream) {
    if (!p || ((weights_host == nullptr) != (bias_host == nullptr))) return GPMPC_E_ARG;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    const int on = weights_host ? 1 : 0, nw = p->ds * p->D;
    if (on) {
        if (!p->nom_dev) {                                   // the first model: both buffers or neither
            double* nom = nullptr; double* resid = nullptr;
            hipError_t e = hipMalloc(&nom, sizeof(double) * (nw + p->ds));
            if (e == hipSuccess) e = hipMalloc(&resid, sizeof(double) * (size_t)p->Np * p->ds);
            if (e != hipSuccess) { if (nom) (void)hipFree(nom); gpmpc_set_error("gpmpc_pack_set_nominal: hipMalloc", e); return GPMPC_E_ALLOC; }
            p->nom_dev = nom; p->resid_dev = resid;
        }
        // (two uploads: ds D + ds doubles can exceed the 512 bytes one carries)
        if (int rcu = gpmpc_upload_small(p->nom_dev, weights_host, sizeof(double) * nw, (hipStream_t)stream)) return rcu;
        if (int rcu = gpmpc_upload_small(p->nom_dev + nw, bias_host, sizeof(double) * p->ds, (hipStream_t)stream)) return rcu;
        memcpy(p->nom_host, weights_host, sizeof(double) * nw);
        memcpy(p->nom_host + nw, bias_host, sizeof(double) * p->ds);
    }
    // a nominal pack runs other kernel instances under another plan: what was captured or measured for the other state is dropped
    // (new VALUES of a model that stays on change neither: the kernels read them from device memory)
    if (on != p->nominal) {
        gpmpc_graph_cache_invalidate(p->graph_cache);
        gpmpc_cb_cache_invalidate(p->cb_cache);
        gpmpc_tuned_clear(p->tuned);
    }
    p->nominal = on;
    p->built = 0;                                            // beta belongs to the targets minus the OLD model
    return GPMPC_OK;
}

// 1: a nominal model is set (weights_host [ds][D] / bias_host [ds] are filled where not NULL), 0: none
extern "C" int gpmpc_pack_get_nominal(const gpmpc_pack* p, double* weights_host, double* bias_host) {
    if (!p) return GPMPC_E_ARG;
    if (!p->nominal) return 0;
    const int nw = p->ds * p->D;
    if (weights_host) memcpy(weights_host, p->nom_host, sizeof(double) * nw);
    if (bias_host) memcpy(bias_host, p->nom_host + nw, sizeof(double) * p->ds);
    return 1;
}

// Noise model of the rollout (layout and defaults: gpmpc_internal.h).  A NULL part is reset to its default.  Everything is checked on the
// host image first: a refused set has touched neither the pack nor the device.
extern "C" int gpmpc_pack_set_noise(gpmpc_pack* p, const double* init_cov_host, const double* action_var_host, const double* process_var_host,
                                    void* stream) {
    if (!p) return GPMPC_E_ARG;
    const int ds = p->ds, da = p->da, oa = gpmpc_noise_off_action(ds), ow = gpmpc_noise_off_process(ds, da), n = ow + ds;
    double img[GPMPC_NOISE_MAX];
    memset(img, 0, sizeof(img));
    noise_defaults(ds, da, img, !init_cov_host, !action_var_host, !process_var_host);
    const char* who = "gpmpc_pack_set_noise";
    if (init_cov_host) {
        double pmax = 0.0;
        for (int e = 0; e < ds * ds; ++e) {
            const double v = init_cov_host[e];
            if (!(v - v == 0.0)) return gpmpc_refuse(who, "init_cov[%d][%d] is not finite", e / ds, e % ds);
            if (fabs(v) > pmax) pmax = fabs(v);
        }
        for (int k = 0; k < ds; ++k) {
            if (init_cov_host[k * ds + k] < 0.0) return gpmpc_refuse(who, "init_cov[%d][%d] is negative", k, k);
            for (int l = 0; l < ds; ++l) {
                const double a = init_cov_host[k * ds + l], b = init_cov_host[l * ds + k];
                if (fabs(a - b) > 1e-12 * pmax) return gpmpc_refuse(who, "init_cov is not symmetric at [%d][%d]", k, l);
                img[k * ds + l] = k == l ? a : 0.5 * (a + b);          // the mean of each off-diagonal pair
            }
        }
    }
    for (int part = 0; part < 2; ++part) {
        const double* src = part ? process_var_host : action_var_host;
        const int cnt = part ? ds : da, off = part ? ow : oa;
        if (!src) continue;
        for (int j = 0; j < cnt; ++j) {
            const double v = src[j];
            if (!(v - v == 0.0) || v < 0.0)
                return gpmpc_refuse(who, "%s[%d] is %s", part ? "process_var" : "action_var", j, v < 0.0 ? "negative" : "not finite");
            img[off + j] = v;
        }
    }
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    // (pieces of 64 doubles: what one upload carries; ds^2 + da + ds <= 80)
    // (the host mirror follows piece by piece: should a launch fail -- a HIP error, not a refusal --, it still says what the device holds)
    p->m1_stale = 1;
    for (int o = 0; o < n; o += 64) {
        const int m = n - o < 64 ? n - o : 64;
        if (int rcu = gpmpc_upload_small(p->noise_dev + o, img + o, sizeof(double) * m, (hipStream_t)stream)) return rcu;
        memcpy(p->noise_host + o, img + o, sizeof(double) * m);
    }
    // nothing is dropped: no kernel instance, plan or captured launch depends on the values (the kernels read them from device memory)
    // (the step-1 weights carry the scales of step 1: marked stale above, refilled by the next call that uses them)
    return GPMPC_OK;
}

// 1: some part differs from its default, 0: none does (the three parts are copied out where not NULL); GPMPC_E_ARG
extern "C" int gpmpc_pack_get_noise(const gpmpc_pack* p, double* init_cov_host, double* action_var_host, double* process_var_host) {
    if (!p) return GPMPC_E_ARG;
    const int ds = p->ds, da = p->da, oa = gpmpc_noise_off_action(ds), ow = gpmpc_noise_off_process(ds, da);
    if (init_cov_host) memcpy(init_cov_host, p->noise_host, sizeof(double) * ds * ds);
    if (action_var_host) memcpy(action_var_host, p->noise_host + oa, sizeof(double) * da);
    if (process_var_host) memcpy(process_var_host, p->noise_host + ow, sizeof(double) * ds);
    double def[GPMPC_NOISE_MAX];
    noise_defaults(ds, da, def, true, true, true);
    for (int e = 0; e < ow + ds; ++e) if (p->noise_host[e] != def[e]) return 1;
    return 0;
}

extern "C" int gpmpc_pack_dims(const gpmpc_pack* p, int* n, int* np, int* ds, int* da) {
    if (!p) return GPMPC_E_ARG;
    if (n) *n = p->N;
    if (np) *np = p->Np;
    if (ds) *ds = p->ds;
    if (da) *da = p->da;
    return GPMPC_OK;
}
extern "C" int gpmpc_pack_shared_lambda(const gpmpc_pack* p) {
    if (!p) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    return p->shared_lambda;
}
