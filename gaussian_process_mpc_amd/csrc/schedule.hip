// Cost schedules (include/gpmpc.h): time-varying references x_ref[t], u_ref[t] and a terminal weight Q_f in ONE device buffer per id,
// read by the schedule variants of the three cost kernels (step_tail.hip, fullcov.hip, cost.hip).  The table of ids is process-wide
// behind a mutex; the contents of a buffer are written in stream order and are never kernel arguments of a cost kernel, so a captured
// launch sequence does not depend on them (the idiom of gpmpc_pack_set_nominal).
#include "gpmpc_internal.h"
#include <cmath>
#include <mutex>
#include <vector>

namespace {
struct Schedule {
    int id, H_max, ds, da, H, has_Qf, device;
    double* dev;
};
std::mutex g_mu;
std::vector<Schedule> g_table;      // live schedules (a handful per process: a linear search)
int g_next_id = 1;                  // ids are not reused

Schedule* find_locked(int id) {
    for (Schedule& s : g_table) if (s.id == id) return &s;
    return nullptr;
}
size_t total_doubles(const Schedule& s) { return gpmpc_sched_off_flags(s.H_max, s.ds, s.da) + 2; }

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}
}  // namespace

// dst[i] = src[i], or 0 where src is null
__global__ void k_sched_write(double* __restrict__ dst, const double* __restrict__ src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src ? src[i] : 0.0;
}
static int sched_write(double* dst, const double* src, size_t n, hipStream_t s) {
    if (n == 0) return GPMPC_OK;
    hipLaunchKernelGGL(k_sched_write, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, (int)n);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
// host values as kernel arguments, 64 doubles per launch (gpmpc_upload_small): consumed before the call returns
static int sched_upload(double* dst, const double* src_host, size_t n, hipStream_t s) {
    for (size_t o = 0; o < n; o += 64) {
        const size_t m = n - o < 64 ? n - o : 64;
        if (int rc = gpmpc_upload_small(dst + o, src_host + o, sizeof(double) * m, s)) return rc;
    }
    return GPMPC_OK;
}

int gpmpc_schedule_resolve(const gpmpc_cost_params* cost, int ds, int da, int H, const char* who, gpmpc_sched_ref* out) {
    out->dev = nullptr; out->H_max = 0;
    if (!cost || cost->schedule_id == 0) return GPMPC_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    const Schedule* s = find_locked(cost->schedule_id);
    if (!s) return gpmpc_refuse(who, "cost schedule %d is unknown or destroyed", cost->schedule_id);
    if (s->ds != ds || s->da != da)
        return gpmpc_refuse(who, "cost schedule of state_dim %d, action_dim %d in a call of state_dim %d, action_dim %d", s->ds, s->da, ds, da);
    if (H > s->H) return gpmpc_refuse(who, "horizon %d exceeds the horizon %d the cost schedule was last set for", H, s->H);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return GPMPC_E_LAUNCH;
    if (dev != s->device) return GPMPC_E_DEVICE;
    out->dev = s->dev; out->H_max = s->H_max;
    return GPMPC_OK;
}

extern "C" int gpmpc_cost_schedule_create(int H_max, int ds, int da, int* id_out) {
    if (!id_out || H_max < 1 || H_max > (1 << 20) || ds < 1 || ds > GPMPC_MAX_DS || da < 0 || da > GPMPC_MAX_D) return GPMPC_E_ARG;
    Schedule s{0, H_max, ds, da, 0, 0, -1, nullptr};
    GPMPC_HIP(hipGetDevice(&s.device));
    const size_t bytes = sizeof(double) * total_doubles(s);
    if (hipError_t e = hipMalloc((void**)&s.dev, bytes); e != hipSuccess) { gpmpc_set_error("gpmpc_cost_schedule_create", e); return GPMPC_E_ALLOC; }
    if (hipError_t e = hipMemset(s.dev, 0, bytes); e != hipSuccess) {
        gpmpc_set_error("gpmpc_cost_schedule_create", e);
        (void)hipFree(s.dev);
        return GPMPC_E_LAUNCH;
    }
    std::lock_guard<std::mutex> lock(g_mu);
    s.id = g_next_id++;
    g_table.push_back(s);
    *id_out = s.id;
    return GPMPC_OK;
}

extern "C" int gpmpc_cost_schedule_destroy(int id) {
    double* dev = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Schedule* s = find_locked(id);
        if (!s) return gpmpc_refuse("gpmpc_cost_schedule_destroy", "cost schedule %d is unknown or destroyed", id);
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) return GPMPC_E_LAUNCH;
        if (cur != s->device) return GPMPC_E_DEVICE;         // (the wait below must be for the device the buffer lives on)
        dev = s->dev;
        g_table.erase(g_table.begin() + (s - g_table.data()));
    }
    (void)hipDeviceSynchronize();       // a rollout that reads the buffer may still be running
    (void)hipFree(dev);
    return GPMPC_OK;
}

// What both forms of set share.  ONE critical section from the lookup to the bookkeeping: a concurrent set of the same id cannot
// interleave, and the table takes the new H / has_Qf only after the last launch was enqueued -- a refused or failed set leaves the table
// as it was.  upload: host values as kernel arguments (sched_upload); else device arrays (sched_write).
static int sched_set(int id, int H, const double* x_ref, const double* u_ref, const double* Qf, bool upload, hipStream_t st, const char* who) {
    if (!x_ref) return gpmpc_refuse(who, "cost schedule: x_ref is NULL");
    std::lock_guard<std::mutex> lock(g_mu);
    Schedule* s = find_locked(id);
    if (!s) return gpmpc_refuse(who, "cost schedule %d is unknown or destroyed", id);
    if (H < 1 || H > s->H_max) return gpmpc_refuse(who, "cost schedule: horizon %d outside 1..H_max = %d", H, s->H_max);
    const size_t nx = (size_t)(H + 1) * s->ds, nu = (size_t)H * s->da, nq = (size_t)s->ds * s->ds;
    if (upload) {
        if (!all_finite(x_ref, nx)) return gpmpc_refuse(who, "cost schedule: x_ref has a non-finite value");
        if (u_ref && !all_finite(u_ref, nu)) return gpmpc_refuse(who, "cost schedule: u_ref has a non-finite value");
        if (Qf && !all_finite(Qf, nq)) return gpmpc_refuse(who, "cost schedule: Q_terminal has a non-finite value");
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return GPMPC_E_LAUNCH;
    if (dev != s->device) return GPMPC_E_DEVICE;
    auto put = [&](double* dst, const double* src, size_t n) { return upload && src ? sched_upload(dst, src, n, st) : sched_write(dst, src, n, st); };
    if (int rc = put(s->dev, x_ref, nx)) return rc;
    if (int rc = put(s->dev + gpmpc_sched_off_u(s->H_max, s->ds), u_ref, nu)) return rc;       // (null: zeros)
    if (Qf) if (int rc = put(s->dev + gpmpc_sched_off_q(s->H_max, s->ds, s->da), Qf, nq)) return rc;
    const double flags[2] = {Qf ? 1.0 : 0.0, (double)H};
    if (int rc = gpmpc_upload_small(s->dev + gpmpc_sched_off_flags(s->H_max, s->ds, s->da), flags, sizeof(flags), st)) return rc;
    s->H = H; s->has_Qf = Qf ? 1 : 0;
    return GPMPC_OK;
}

extern "C" int gpmpc_cost_schedule_set(int id, int H, const double* x_ref, const double* u_ref, const double* Qf, void* stream) {
    return sched_set(id, H, x_ref, u_ref, Qf, true, (hipStream_t)stream, "gpmpc_cost_schedule_set");
}

extern "C" int gpmpc_cost_schedule_set_dev(int id, int H, const double* x_ref, const double* u_ref, const double* Qf, void* stream) {
    return sched_set(id, H, x_ref, u_ref, Qf, false, (hipStream_t)stream, "gpmpc_cost_schedule_set_dev");
}

extern "C" int gpmpc_cost_schedule_get(int id, int* H_max, int* ds, int* da, int* H, int* has_Qf, const double** dev_out) {
    std::lock_guard<std::mutex> lock(g_mu);
    const Schedule* s = find_locked(id);
    if (!s) return gpmpc_refuse("gpmpc_cost_schedule_get", "cost schedule %d is unknown or destroyed", id);
    if (H_max) *H_max = s->H_max;
    if (ds) *ds = s->ds;
    if (da) *da = s->da;
    if (H) *H = s->H;
    if (has_Qf) *has_Qf = s->has_Qf;
    if (dev_out) *dev_out = s->dev;
    return GPMPC_OK;
}
