// Process-wide state of the library that is not a kernel: the error text of the calling thread, version / device count, the opt-in
// timing record of the pair kernels with the timed launchers of every kernel form, and the per-pack host lock.
#include "rollout.h"
#include <cstdarg>
#include <new>
#include <vector>

static thread_local char g_err[256] = "";
void gpmpc_set_error(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
}
void gpmpc_set_error_text(const char* text) { snprintf(g_err, sizeof(g_err), "%s", text); }
int gpmpc_refuse(const char* who, const char* fmt, ...) {
    const int n = snprintf(g_err, sizeof(g_err), "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (n >= 0 && n < (int)sizeof(g_err)) vsnprintf(g_err + n, sizeof(g_err) - n, fmt, ap);
    va_end(ap);
    return GPMPC_E_ARG;
}
extern "C" const char* gpmpc_last_error(void) { return g_err; }
extern "C" const char* gpmpc_version(void) { return "gpmpc-hip 0.1 (gfx950)"; }
extern "C" int gpmpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Opt-in timing of the pair kernel (bench.py): HIP events around every pair launch on the launch stream, accumulated
// per class (full kernel / horizon-step-1 variant).  One process-wide record behind a mutex: concurrent rollouts on
// different streams or host threads may all run with timing on.
struct EvPair { hipEvent_t a, b; int cls; };
static struct {
    std::mutex mu;
    int on = 0;
    double ms[GPMPC_TIME_CLASSES] = {0.0, 0.0, 0.0};
    long long n[GPMPC_TIME_CLASSES] = {0, 0, 0};
    std::vector<EvPair> pending;
} g_time;

static void drain_events_locked() {
    for (const EvPair& ev : g_time.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            g_time.ms[ev.cls] += ms; ++g_time.n[ev.cls];
        }
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
    }
    g_time.pending.clear();
}
bool gpmpc_timing_on() { std::lock_guard<std::mutex> lk(g_time.mu); return g_time.on != 0; }
extern "C" int gpmpc_timing_enable(int on) { std::lock_guard<std::mutex> lk(g_time.mu); g_time.on = on; return GPMPC_OK; }
extern "C" int gpmpc_pair_kernel_time(double* total_ms, long long* launches, int reset) {
    std::lock_guard<std::mutex> lk(g_time.mu);
    drain_events_locked();
    if (total_ms) *total_ms = g_time.ms[0] + g_time.ms[1] + g_time.ms[2];
    if (launches) *launches = g_time.n[0] + g_time.n[1] + g_time.n[2];
    if (reset) for (int c = 0; c < GPMPC_TIME_CLASSES; ++c) { g_time.ms[c] = 0.0; g_time.n[c] = 0; }
    return GPMPC_OK;
}
extern "C" int gpmpc_pair_kernel_time_class(int cls, double* total_ms, long long* launches) {
    if (cls < 0 || cls >= GPMPC_TIME_CLASSES) return GPMPC_E_ARG;
    std::lock_guard<std::mutex> lk(g_time.mu);
    drain_events_locked();
    if (total_ms) *total_ms = g_time.ms[cls];
    if (launches) *launches = g_time.n[cls];
    return GPMPC_OK;
}

// Bracket one launch with events when timing is on.  `launch` enqueues the kernel on s and returns its status.
template <class F>
static int timed_launch(int cls, hipStream_t s, F launch) {
    if (!gpmpc_timing_on()) return launch();
    EvPair ev; ev.cls = cls;
    GPMPC_HIP(hipEventCreate(&ev.a));
    GPMPC_HIP(hipEventCreate(&ev.b));
    GPMPC_HIP(hipEventRecord(ev.a, s));
    const int rc = launch();
    GPMPC_HIP(hipEventRecord(ev.b, s));
    std::lock_guard<std::mutex> lk(g_time.mu);
    if (g_time.pending.size() >= 4096) drain_events_locked();
    g_time.pending.push_back(ev);
    return rc;
}

int gpmpc_timed_pair(int D, bool diag, bool grad, int tb, int waves, const PairArgs& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FULL, s, [&] { return gpmpc_launch_pair(D, diag, grad, tb, waves, a, s); });
}
int gpmpc_timed_pair_sb(int D, bool grad, int tb, int ns2, int waves, const PairSbArgs& a, hipStream_t s) {
    return timed_launch(a.first_step ? GPMPC_TIME_FIRST : GPMPC_TIME_FULL, s,
                        [&] { return gpmpc_launch_pair_sb(D, grad, tb, ns2, waves, a, s); });
}
int gpmpc_timed_pair_sbs(int D, bool grad, int ng, int ns2, const PairSbsArgs& a, hipStream_t s) {
    return timed_launch(a.first_step ? GPMPC_TIME_FIRST : GPMPC_TIME_FULL, s,
                        [&] { return gpmpc_launch_pair_sbs(D, grad, ng, ns2, a, s); });
}
// (always horizon step 1: timed in the class of the FIRST variant it replaces)
int gpmpc_timed_pair_q1(int D, int da, const PairQ1Args& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FIRST, s, [&] { return gpmpc_launch_pair_q1(D, da, a, s); });
}
int gpmpc_timed_pair_sbf(int D, bool grad, int ns2, int waves, const PairSbfArgs& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FULL, s, [&] { return gpmpc_launch_pair_sbf(D, grad, ns2, waves, a, s); });
}

// the forms whose per-D instances are translation units of their own (persist_d*.o from D = 2, fused_d*.o)
int gpmpc_timed_persist(int D, bool grad, int ns2, int waves, int ng, const PersistArgs& a, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FUSED, s, [&] {
        return gpmpc_dispatch_dim<2>(D, [&](auto d) { return gpmpc_launch_persist_D<decltype(d)::value>(grad, ns2, waves, ng, a, s); });
    });
}
int gpmpc_timed_step_fused(int D, bool grad, int ns2, int q, int ng, const FusedArgs& a, int t, hipStream_t s) {
    return timed_launch(GPMPC_TIME_FUSED, s, [&] {
        return gpmpc_dispatch_dim<1>(D, [&](auto d) { return gpmpc_launch_step_fused_D<decltype(d)::value>(grad, ns2, q, ng, a, t, s); });
    });
}

// the lock of a pack (gpmpc_pack::lock, created with the pack): what it serialises is said at PackGuard, rollout.h
void* gpmpc_lock_create() { return new (std::nothrow) std::recursive_mutex(); }
void gpmpc_lock_destroy(void* l) { delete (std::recursive_mutex*)l; }
