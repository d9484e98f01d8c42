// Planning of the diagonal rollout (plan.hip): WHAT a call launches -- a RollShape -- and WHERE its buffers lie in the workspace -- a
// RollLayout.  step.hip::gpmpc_enqueue_rollout (rollout.h) enqueues from the two; moment.hip::plan_mom and the full-covariance plan
// (fullcov.hip) are separate.
#pragma once
#include "gpmpc_internal.h"

// doubles per (trajectory, GP) of the head kernel's scalars `sp`, without / with a linear nominal model (the layouts: roll_dev.h)
__host__ __device__ static inline int sps_of(int D) { return 3 + 4 * D; }
__host__ __device__ static inline int sps_nominal(int D) { return sps_of(D) + 2 + 3 * D; }

// Every decision about the launches of one call; none is a size.  A shape chosen for a call is what EVERY sub-batch of that call launches
// (gpmpc_split_slices), so split calls are bit-identical to unsplit ones, and what gpmpc_pack_autotune measures and stores.
struct RollShape {
    int tiling, tb, waves, nwork, sb, rgroup, fused, fq, shared, sh_list;
    int colunroll;   // columns per iteration of the sb kernel
    int fng;         // GPs per tile workgroup of the one-launch form with one lambda
    int xcdmap;      // one-launch form, several trajectories: XCD-aware dispatch order 0 | 1 | -1 by the size of the launch
    int pwaves;      // waves per workgroup of the whole-horizon kernel (fused = 3)
    int png;         // GPs per unit there: 1, or 2 (all of them where that instance exists) with one lambda for all GPs
    int hchunks, hrows;
};
// Record sizes and workspace offsets of a shape at one batch size: a pure function of (pack, shape, B, H, grad).
struct RollLayout {
    int nm, pps, sps, gw;
    size_t off_pp, off_sp, off_part, off_partz, off_mpart, off_jac, off_G, off_means, off_vars, total;
};

// The only reader of the pack's tuned table and of the measured thresholds.  tn_over (optional): GPMPC_* overrides to plan under
// instead of the pack's (gpmpc_pack_autotune enumerates candidates with it).
RollShape gpmpc_choose_shape(const gpmpc_pack* p, int B, int H, bool grad, bool lowprec, const gpmpc_tuning* tn_over = nullptr);
// The only place that sizes the buffers of a rollout.
RollLayout gpmpc_layout_for(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad);
// the shared work list the one-launch form uses for this shape (one lambda for all GPs): groups of two GPs | of the pack's group size
static inline const gpmpc_worklist& gpmpc_fused_shared_list(const gpmpc_pack* p, const RollShape& r) {
    return p->wl_sh[(r.fng == 2 && p->sh_ng != 2) ? 3 : 1];
}
// Horizon step 1 as a quadratic form (pair_kernel_q1.h) for a call of B trajectories whose launches are r: the two-launch scalar-broadcast form on
// 256-row tiles of a pack with distinct lambdas, fp64, da in {1, 2} (with or without a nominal model: that is the head kernel's business), GPMPC_NO_FIRST unset; B from the measured threshold on, or whatever
// the batch with GPMPC_STEP1_QUAD=1, never with =0.  B = 0 asks about the shape alone (the enqueue of a sub-batch: the whole call's B decided).
bool gpmpc_step1_quad_plan(const gpmpc_pack* p, const RollShape& r, int B, bool lowprec);
// equal as far as the LAUNCHES go (the autotuner's de-duplication)
bool gpmpc_same_shape(const RollShape& a, const RollShape& b);

#define GPMPC_MAX_SPLIT 4
int gpmpc_split_count(const gpmpc_pack* p, const RollShape& r, int B, bool lowprec, bool eager = false, int split_over = 0,
                      int H = 0, int grad = -1);
// Sub-batch k of S: trajectories [b0, b1) = [B k / S, B (k + 1) / S), its layout, and its slice of the workspace at ws_off (prefix sum
// of the layouts before it).  Fills out[0 .. S), S <= GPMPC_MAX_SPLIT; returns the bytes all slices take together.
struct RollSlice { int b0, b1; RollLayout lay; size_t ws_off; };
size_t gpmpc_split_slices(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad, int S, RollSlice* out);

// Shapes MEASURED for this pack (gpmpc_pack_autotune): a call shape found here takes its kernel form from the table instead of
// from the thresholds.  Owned by the pack (gpmpc_pack::tuned), written only by gpmpc_pack_autotune.
#define GPMPC_TUNED_SLOTS 16
struct gpmpc_tuned_entry { int B, H, grad, graph, S, valid; RollShape shape; double ms_default, ms_best; };
struct gpmpc_tuned_table { gpmpc_tuned_entry e[GPMPC_TUNED_SLOTS]; int next; };

// How the calling entry point will launch (captured graph replay = 1, plain launches = 0, unknown = -1): a plan and split count
// measured as graph replays -- launch overhead hidden, up to four parallel branches -- must not be applied to eager calls of the same
// shape, nor the reverse.  Set by the entry points for the duration of their planning (thread-local: the library is re-entrant).
struct GraphModeGuard {
    int prev;
    explicit GraphModeGuard(int m);
    ~GraphModeGuard();
};
