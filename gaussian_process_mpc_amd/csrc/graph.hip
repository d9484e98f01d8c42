// Everything between an entry point of the diagonal rollout and gpmpc_enqueue_rollout (step.hip): the per-pack cache of captured
// rollouts and its replay, the split of one call into concurrent sub-batches, the solver-callback cache (gpmpc_objective_gradient),
// and the entry points that only wrap the enqueue.
#include "rollout.h"
#include <cstdlib>

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

// The pack's private streams / events (graph replay and split launches), created on first use (under the pack's lock).
int gpmpc_ensure_graph_cache(gpmpc_pack* p, gpmpc_graph_cache** out) {
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
        if (ec != hipSuccess) {
            gpmpc_set_error("graph cache: stream / event creation", ec);
            gpmpc_graph_cache_free(g);
            return GPMPC_E_LAUNCH;
        }
        p->graph_cache = g;
    }
    *out = g;
    return GPMPC_OK;
}

size_t gpmpc_split_bytes(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad, int S) {
    RollSlice sl[GPMPC_MAX_SPLIT];
    return gpmpc_split_slices(p, r, B, H, grad, S, sl);
}

// The trajectories of slice sl as a call of their own on stream s, in its slice of the workspace, launched as the whole call is
// (null outputs stay null).
static RollCall roll_sub(const RollCall& c, const RollSlice& sl, hipStream_t s, const RollShape* whole) {
    const size_t b0 = sl.b0, nx = b0 * (c.H + 1) * c.p->ds, nu = b0 * c.H * c.p->da;
    RollCall k = c;
    k.B = sl.b1 - sl.b0; k.x0 += b0 * c.p->ds; k.U += nu; k.out_cost += b0;
    if (k.out_means) k.out_means += nx;
    if (k.out_vars) k.out_vars += nx;
    if (k.out_grad) k.out_grad += nu;
    k.workspace = (char*)c.workspace + sl.ws_off; k.workspace_bytes = sl.lay.total; k.stream = s; k.shape = whole;
    return k;
}

// One rollout call as S sub-batches: sub-batch 0 on c.stream (`origin`), the others on the pack's auxiliary streams, forked from and
// joined back into `origin` with events (inside a stream capture these become parallel branches of the graph).  The
// caller holds the pack's lock (PackGuard): two host threads sharing a pack must not interleave their fork / join pairs.
int gpmpc_enqueue_split(gpmpc_graph_cache* g, int S, const RollShape& whole, const RollCall& c) {
    const hipStream_t origin = c.stream;
    int rc = GPMPC_OK;
    hipError_t ef = hipEventRecord(g->ev_fork, origin);
    RollSlice sl[GPMPC_MAX_SPLIT];
    gpmpc_split_slices(c.p, whole, c.B, c.H, (c.flags & GPMPC_WANT_GRAD) != 0, S, sl);
    for (int k = S - 1; k >= 0 && rc == GPMPC_OK && ef == hipSuccess; --k) {
        hipStream_t sk = k == 0 ? origin : g->aux[k - 1];
        if (k > 0) ef = hipStreamWaitEvent(sk, g->ev_fork, 0);
        if (ef != hipSuccess) break;
        rc = gpmpc_enqueue_rollout(roll_sub(c, sl[k], sk, &whole));
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

static void graph_key_fill(gpmpc_graph_key* k, const RollCall& c) {
    memset(k, 0, sizeof(*k));                               // (compared with memcmp: padding included)
    k->B = c.B; k->H = c.H; k->flags = c.flags; k->x0 = c.x0; k->U = c.U; k->means = c.out_means; k->vars = c.out_vars;
    k->cost_out = c.out_cost; k->grad = c.out_grad; k->ws = c.workspace; k->ws_bytes = c.workspace_bytes; k->cost = *c.cost;
}

// Replay the launches of a rollout as ONE hipGraph on a stream owned by the pack (the caller's stream, c.stream, may be the
// legacy default stream, which cannot be captured); ordered against the caller's stream with two events.
static int graph_rollout(gpmpc_pack* p, const RollCall& c) {
    PackGuard lock(p);                                      // cache creation, capture (begin ... end) and replay: one host thread at a time
    gpmpc_graph_cache* g = nullptr;
    if (int rcg = gpmpc_ensure_graph_cache(p, &g)) return rcg;
    gpmpc_graph_key k;
    graph_key_fill(&k, c);
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
        const bool grad = (c.flags & GPMPC_WANT_GRAD) != 0, lowprec = (c.flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
        const RollShape whole = gpmpc_choose_shape(p, c.B, c.H, grad, lowprec);
        const int S = gpmpc_split_count(p, whole, c.B, lowprec, false, 0, c.H, grad ? 1 : 0);
        if (S > 1 && gpmpc_split_bytes(p, whole, c.B, c.H, grad, S) > c.workspace_bytes) return GPMPC_E_WORKSPACE;
        RollCall cc = c;
        cc.stream = g->stream;
        const int rc = gpmpc_capture(g->stream, [&] { return S <= 1 ? gpmpc_enqueue_rollout(cc) : gpmpc_enqueue_split(g, S, whole, cc); },
                                     &g->exec[slot]);
        if (rc != GPMPC_OK) return rc;
        g->key[slot] = k; g->valid[slot] = 1; ++g->captures;
    }
    g->used[slot] = ++g->tick;
    GPMPC_HIP(hipEventRecord(g->ev_in, c.stream));
    GPMPC_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
    GPMPC_HIP(hipGraphLaunch(g->exec[slot], g->stream));
    GPMPC_HIP(hipEventRecord(g->ev_out, g->stream));
    GPMPC_HIP(hipStreamWaitEvent(c.stream, g->ev_out, 0));
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

// the captured graph is stale (or about to lose its buffers): wait for its last replay, drop it
static void cb_drop_exec(gpmpc_cb_cache* g) {
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    g->valid = 0;
}
static void cb_free_staging(gpmpc_cb_cache* g) {
    if (g->h_in) (void)hipHostFree(g->h_in);
    if (g->h_out) (void)hipHostFree(g->h_out);
    if (g->d_in) (void)hipFree(g->d_in);
    if (g->d_out) (void)hipFree(g->d_out);
    if (g->ws) (void)hipFree(g->ws);
    g->h_in = g->h_out = g->d_in = g->d_out = nullptr; g->ws = nullptr; g->cap_H = 0;
}

void gpmpc_cb_cache_free(void* c) {
    gpmpc_cb_cache* g = (gpmpc_cb_cache*)c;
    if (!g) return;
    cb_drop_exec(g);
    if (g->ev_in) (void)hipEventDestroy(g->ev_in);
    cb_free_staging(g);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    free(g);
}

void gpmpc_cb_cache_invalidate(void* c) {
    if (c) cb_drop_exec((gpmpc_cb_cache*)c);
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
    {   // a cost schedule is looked up on EVERY call, before a replay: the captured launches hold its buffer, not its state
        gpmpc_sched_ref sched;
        if (int rcs = gpmpc_schedule_resolve(cost, p->ds, p->da, H, "gpmpc_objective_gradient", &sched)) return rcs;
    }
    PackGuard lock(p);                                      // the entry owns per-pack staging buffers and is synchronous: one caller at a time
    // per-kernel events cannot be recorded inside a captured graph: with timing on the same work is enqueued uncaptured
    const bool eager = gpmpc_timing_on();
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
        if (e != hipSuccess) {
            gpmpc_set_error("gpmpc_objective_gradient: stream / event creation", e);
            gpmpc_cb_cache_free(g);
            return GPMPC_E_LAUNCH;
        }
        p->cb_cache = g;
    }
    if (H > g->cap_H) {                                   // (re)allocate for the longer horizon
        cb_drop_exec(g);
        cb_free_staging(g);
        const size_t bin = sizeof(double) * (p->ds + (size_t)H * p->da), bout = sizeof(double) * (1 + (size_t)H * p->da);
        hipError_t ea = hipHostMalloc((void**)&g->h_in, bin, hipHostMallocDefault);
        if (ea == hipSuccess) ea = hipHostMalloc((void**)&g->h_out, bout, hipHostMallocDefault);
        if (ea == hipSuccess) ea = hipMalloc((void**)&g->d_in, bin);
        if (ea == hipSuccess) ea = hipMalloc((void**)&g->d_out, bout);
        g->ws_bytes = gpmpc_rollout_workspace_bytes(p, 1, H, GPMPC_WANT_GRAD);
        if (ea == hipSuccess) ea = hipMalloc(&g->ws, g->ws_bytes);
        if (ea != hipSuccess) {                           // cap_H stays 0: retried next call
            gpmpc_set_error("gpmpc_objective_gradient: staging allocation", ea);
            return GPMPC_E_ALLOC;
        }
        g->cap_H = H;
    }
    {   // the pack may have been refilled under a plan that needs more scratch (e.g. lambdas no longer shared: G rows per GP);
        // checked on EVERY call -- a plan is a few hundred host instructions -- so that neither the captured nor the timed
        // (uncaptured) path ever runs with a stale size
        const size_t need = gpmpc_rollout_workspace_bytes(p, 1, H, GPMPC_WANT_GRAD);
        if (need > g->ws_bytes) {
            cb_drop_exec(g);
            if (g->ws) (void)hipFree(g->ws);
            g->ws = nullptr; g->ws_bytes = 0;
            if (hipError_t ea = hipMalloc(&g->ws, need); ea != hipSuccess) {
                gpmpc_set_error("gpmpc_objective_gradient: workspace", ea);
                g->cap_H = 0;
                return GPMPC_E_ALLOC;
            }
            g->ws_bytes = need;
        }
    }
    const RollCall call{p, 1, H, g->d_in, g->d_in + p->ds, cost, flags, nullptr, nullptr, g->d_out, grad ? g->d_out + 1 : nullptr,
                        g->ws, g->ws_bytes, g->stream};
    if (eager) {                                          // timing on: upload, the H + 1 launches, download -- uncaptured
        memcpy(g->h_in, x0_host, sizeof(double) * p->ds);
        memcpy(g->h_in + p->ds, U_host, sizeof(double) * (size_t)H * p->da);
        GPMPC_HIP(hipEventRecord(g->ev_in, (hipStream_t)stream));
        GPMPC_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
        GPMPC_HIP(hipMemcpyAsync(g->d_in, g->h_in, sizeof(double) * nin, hipMemcpyHostToDevice, g->stream));
        if (int rc = gpmpc_enqueue_rollout(call)) return rc;
        GPMPC_HIP(hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, g->stream));
        GPMPC_HIP(hipStreamSynchronize(g->stream));
        memcpy(out_host, g->h_out, sizeof(double) * nout);
        return GPMPC_OK;
    }
    if (!g->valid || g->H != H || g->flags != flags || memcmp(&g->cost, cost, sizeof(*cost)) != 0) {
        cb_drop_exec(g);
        const int rc = gpmpc_capture(g->stream, [&] {      // the two copies are nodes of the graph; their errors count as the capture's
            const hipError_t e1 = hipMemcpyAsync(g->d_in, g->h_in, sizeof(double) * nin, hipMemcpyHostToDevice, g->stream);
            const int rcr = gpmpc_enqueue_rollout(call);
            const hipError_t e2 = hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, g->stream);
            if (rcr != GPMPC_OK || (e1 == hipSuccess && e2 == hipSuccess)) return rcr;
            gpmpc_set_error("gpmpc_objective_gradient capture", e1 != hipSuccess ? e1 : e2);
            return (int)GPMPC_E_LAUNCH;
        }, &g->exec);
        if (rc != GPMPC_OK) return rc;
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
    {   // (as in gpmpc_objective_gradient: before a replay)
        gpmpc_sched_ref sched;
        if (int rcs = gpmpc_schedule_resolve(cost, p->ds, p->da, H, "gpmpc_rollout", &sched)) return rcs;
    }
    const bool graph = (flags & GPMPC_USE_GRAPH) && !gpmpc_timing_on();
    GraphModeGuard mode(graph ? 1 : 0);
    RollCall c{p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace, workspace_bytes, (hipStream_t)stream};
    if (p->built && x0 && U && out_cost && workspace && B >= 1 && H >= 1) {
        // Horizon step 1 as a quadratic form (pair_kernel_q1.h), decided HERE for the whole call: its weights are allocated on first use and
        // refilled when a build or gpmpc_pack_set_noise has made them stale -- on the caller's stream, ahead of every launch and of every replay
        // of a graph that was captured with the kernel in it (a replay reads the same buffer; neither event drops a captured graph).  A call on
        // another stream than the one that filled them waits there for the fill's event: rollouts stay re-entrant across streams.
        const bool lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
        const RollShape whole = gpmpc_choose_shape(p, B, H, (flags & GPMPC_WANT_GRAD) != 0, lowprec);
        if (gpmpc_step1_quad_plan(p, whole, B, lowprec)) {
            PackGuard lock(p);
            const int rc1 = gpmpc_pack_step1_refresh(const_cast<gpmpc_pack*>(p), (hipStream_t)stream);
            if (rc1 != GPMPC_OK && rc1 != GPMPC_E_ALLOC) return rc1;
            c.step1_quad = rc1 == GPMPC_OK;                 // (no memory for the weights: the FIRST variant, as before)
        }
    }
    if (graph && p->built && x0 && U && out_cost && workspace && B >= 1 && H >= 1) return graph_rollout(const_cast<gpmpc_pack*>(p), c);
    if (p->built && x0 && U && out_cost && workspace && B >= 4 && H >= 1 && !(flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) &&
        (!(flags & GPMPC_WANT_GRAD) || out_grad)) {
        // mid-size batch launched plainly: the same split into concurrent sub-batches as under graph replay, on the pack's
        // auxiliary streams, forked from / joined into the caller's stream
        const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
        const RollShape whole = gpmpc_choose_shape(p, B, H, grad, false);
        const int S = gpmpc_split_count(p, whole, B, false, true, 0, H, grad ? 1 : 0);
        if (S > 1 && gpmpc_split_bytes(p, whole, B, H, grad, S) <= workspace_bytes) {
            PackGuard lock(p);                              // the pack's auxiliary streams / events (shared with graph_rollout's captures)
            gpmpc_graph_cache* g = nullptr;
            if (int rcg = gpmpc_ensure_graph_cache(const_cast<gpmpc_pack*>(p), &g)) return rcg;
            return gpmpc_enqueue_split(g, S, whole, c);
        }
    }
    return gpmpc_enqueue_rollout(c);
}

// ---------------------------------------------------------------------------
// Differentiable propagation: trajectory + step Jacobians, and their vector-Jacobian product
// ---------------------------------------------------------------------------
static inline size_t jac_scratch_bytes(const gpmpc_pack* p, int B, int H) {     // [cost | grad] of the (zero-cost) tail kernel
    return gpmpc_align256(sizeof(double) * (size_t)B * (1 + (size_t)H * p->da));
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
    return gpmpc_enqueue_rollout({p, B, H, x0, U, &zero, GPMPC_WANT_GRAD, out_means, out_vars, scratch, scratch + B, workspace, base,
                                  (hipStream_t)stream, out_jac, true});
}

// ---------------------------------------------------------------------------
// Rollout + state chance constraints in one device pass (kernel: constraints.hip)
// ---------------------------------------------------------------------------
static int constrained_flags_ok(unsigned flags) {
    if (flags & ~GPMPC_WANT_GRAD) {
        gpmpc_set_error_text("gpmpc_rollout_constrained: only GPMPC_WANT_GRAD is accepted (no GPMPC_USE_GRAPH, no GPMPC_FP32_* mode in this "
                             "version)");
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
    // the layout gpmpc_enqueue_rollout takes for this call: where it keeps J_t, means, variances
    const RollLayout L = gpmpc_layout_for(p, gpmpc_choose_shape(p, B, H, grad, false), B, H, grad);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    if (int rc = gpmpc_enqueue_rollout({p, B, H, x0, U, cost, flags, out_means, out_vars, out_cost, out_grad, workspace, workspace_bytes,
                                        (hipStream_t)stream}))
        return rc;
    char* ws = (char*)workspace;
    return gpmpc_rollout_constraints(B, H, p->ds, p->da, cons, out_means ? out_means : (const double*)(ws + L.off_means),
                                     out_vars ? out_vars : (const double*)(ws + L.off_vars),
                                     grad ? (const double*)(ws + L.off_jac) : nullptr, out_g, grad ? out_gjac : nullptr, stream);
}
