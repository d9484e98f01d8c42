// Host side of the diagonal rollout, shared by step.hip (kernels + enqueue), graph.hip (graph cache, split launch, callback cache, the
// rollout entry points), autotune.hip and runtime.hip (error text, timing record, per-pack lock).  Host only: no device code here.
// (gpmpc_dispatch_dim, which the timed launchers use, lives in gpmpc_internal.h with the rest of the plumbing every unit shares.)
#pragma once
#include "gpmpc_internal.h"
#include "plan.h"
#include <mutex>

// One rollout call: what the entry points, the split launch, the graph capture and the autotuner hand to the enqueue.
struct RollCall {
    const gpmpc_pack* p; int B, H;
    const double* x0; const double* U; const gpmpc_cost_params* cost; unsigned flags;
    double* out_means; double* out_vars; double* out_cost; double* out_grad;
    void* workspace; size_t workspace_bytes; hipStream_t stream;
    double* ext_jac = nullptr;          // caller-owned [B][H][2ds][2ds+da] buffer for the step Jacobians instead of the workspace's (gpmpc_rollout_jac)
    bool full_first = false;            // horizon step 1 keeps the derivatives w.r.t. its state inputs (needed for d/dx0)
    const RollShape* shape = nullptr;   // the launches of a larger batch this one is a sub-batch of, or of a candidate of gpmpc_pack_autotune;
                                        // null: chosen by the enqueue
    bool step1_quad = false;            // horizon step 1 through pair_kernel_q1.h: set by gpmpc_rollout alone, for the WHOLE call (its sub-batches inherit it), after
                                        // it has brought the pack's step-1 weights up to date on the caller's stream (gpmpc_step1_quad_plan, plan.h)
};
int gpmpc_enqueue_rollout(const RollCall& c);                          // step.hip: validates, plans (unless c.shape), launches on c.stream

// Per-pack host lock (gpmpc_pack::lock, created with the pack: runtime.hip).  It serialises, per pack, everything that touches the pack's OWN
// streams, events and caches: the lazy creation of graph_cache / cb_cache, a stream capture from hipStreamBeginCapture to
// hipStreamEndCapture (the auxiliary streams are in capture state meanwhile: a plain split launch of another host thread on them
// would be recorded into that capture instead of executing), the fork / join of a split launch, and the solver-callback entry.
// Calls that use only the caller's stream and workspace (unsplit plain launches) do not take it.
struct PackGuard {
    std::recursive_mutex* m;
    explicit PackGuard(const gpmpc_pack* p) : m((std::recursive_mutex*)p->lock) { if (m) m->lock(); }
    ~PackGuard() { if (m) m->unlock(); }
    PackGuard(const PackGuard&) = delete; PackGuard& operator=(const PackGuard&) = delete;
};

// runtime.hip: the timing record (per-kernel events cannot be recorded inside a capture: entry points ask before they capture), and a
// timed launcher for every kernel form between the head and the tail
bool gpmpc_timing_on();
int gpmpc_timed_pair(int D, bool diag, bool grad, int tb, int waves, const PairArgs& a, hipStream_t s);
int gpmpc_timed_pair_sb(int D, bool grad, int tb, int ns2, int waves, const PairSbArgs& a, hipStream_t s);
int gpmpc_timed_pair_sbs(int D, bool grad, int ng, int ns2, const PairSbsArgs& a, hipStream_t s);
int gpmpc_timed_pair_q1(int D, int da, const PairQ1Args& a, hipStream_t s);
int gpmpc_timed_pair_sbf(int D, bool grad, int ns2, int waves, const PairSbfArgs& a, hipStream_t s);
int gpmpc_timed_persist(int D, bool grad, int ns2, int waves, int ng, const PersistArgs& a, hipStream_t s);
int gpmpc_timed_step_fused(int D, bool grad, int ns2, int q, int ng, const FusedArgs& a, int t, hipStream_t s);

// graph.hip: the pack's private streams / events, and one call as S concurrent sub-batches on them (caller holds the PackGuard)
struct gpmpc_graph_cache;
int gpmpc_ensure_graph_cache(gpmpc_pack* p, gpmpc_graph_cache** out);
size_t gpmpc_split_bytes(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad, int S);
int gpmpc_enqueue_split(gpmpc_graph_cache* g, int S, const RollShape& whole, const RollCall& c);

// Capture what enqueue() puts on s (thread-local capture mode) into an instantiated graph.  The hipGraph_t is destroyed on every path;
// returns the enqueue's code first, then GPMPC_E_LAUNCH with the error text set.
template <class Enqueue>
static int gpmpc_capture(hipStream_t s, Enqueue&& enqueue, hipGraphExec_t* out) {
    GPMPC_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipGraph_t graph = nullptr;
    const int rc = enqueue();
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc == GPMPC_OK && e != hipSuccess) gpmpc_set_error("hipStreamEndCapture", e);
    if (rc == GPMPC_OK && e == hipSuccess) {
        e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) gpmpc_set_error("hipGraphInstantiate", e);
    }
    if (graph) (void)hipGraphDestroy(graph);
    return rc != GPMPC_OK ? rc : (e == hipSuccess ? GPMPC_OK : GPMPC_E_LAUNCH);
}
