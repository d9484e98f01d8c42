// Plan selection of the diagonal rollout: which kernels a call of a given shape launches (gpmpc_choose_shape: the tuned table and every
// measured threshold), how its workspace is laid out (gpmpc_layout_for), into how many concurrent sub-batches it is split
// (gpmpc_split_count, gpmpc_split_slices), and the two entry points that only plan: gpmpc_rollout_workspace_bytes, gpmpc_plan_describe.
// No kernel lives here; step.hip::gpmpc_enqueue_rollout enqueues what is decided here (graph.hip and autotune.hip call it).
#include "plan.h"
#include <cstdlib>

#define GPMPC_PERSIST_MAXNP_HOST 1024
static thread_local int tl_graph_mode = -1;       // GraphModeGuard (plan.h)
GraphModeGuard::GraphModeGuard(int m) : prev(tl_graph_mode) { tl_graph_mode = m; }
GraphModeGuard::~GraphModeGuard() { tl_graph_mode = prev; }
static const gpmpc_tuned_entry* tuned_lookup(const gpmpc_pack* p, int B, int H, bool grad) {
    const gpmpc_tuned_table* t = (const gpmpc_tuned_table*)p->tuned;
    if (!t) return nullptr;
    for (int k = 0; k < GPMPC_TUNED_SLOTS; ++k)
        if (t->e[k].valid && t->e[k].B == B && t->e[k].H == H && t->e[k].grad == (grad ? 1 : 0) &&
            (tl_graph_mode < 0 || t->e[k].graph == tl_graph_mode)) return &t->e[k];
    return nullptr;
}
void gpmpc_tuned_free(void* t) { free(t); }
void gpmpc_tuned_clear(void* t) { if (t) memset(t, 0, sizeof(gpmpc_tuned_table)); }      // plans measured under another kernel selection (lambdas no longer shared, new GPMPC_* overrides)

RollShape gpmpc_choose_shape(const gpmpc_pack* p, int B, int H, bool grad, bool lowprec, const gpmpc_tuning* tn_over) {
    const int D = p->D;
    if (!tn_over && !lowprec)                                   // a measured plan for this call shape
        if (const gpmpc_tuned_entry* te = tuned_lookup(p, B, H, grad)) return te->shape;
    RollShape shape;
    RollShape* const r = &shape;
    // A pack with a linear nominal model is planned as under GPMPC_FUSED=0 GPMPC_FUSED_SB=0 GPMPC_PERSIST=0, whatever the overrides say:
    // only the head / tail kernels (step.hip, step_tail.hip) know the model (step_fused.h and traj_persist.h keep their own finish code), and their
    // nominal variants run without row chunks (the extra sums E1, E2 are not carried through mpart).
    gpmpc_tuning tn_nom;
    if (p->nominal) { tn_nom = tn_over ? *tn_over : p->tune; tn_nom.fused = 0; tn_nom.fused_sb = 0; tn_nom.persist = 0; tn_nom.hchunks = 1; }
    const gpmpc_tuning& tn = p->nominal ? tn_nom : (tn_over ? *tn_over : p->tune);        // GPMPC_* overrides, read once at pack creation
    // The selection as it stands (diagonal rollout, da <= 2; every threshold is a measured crossover -- its numbers are in the
    // comment at its line, the method in DESIGN.md section 5, the maps in profiles/r02 and r03/batch_size_map.txt):
    //   W64 = B x tiles(256x64) < ~150 (~400 for N < 512), or N < 256           ONE launch per step, 64-row tiles, staged column loop
    //                                                                           (step_fused.h, Q = 1 | 4; the B = 1 solver callbacks)
    //   up to W64 ~4700 (~7000: <= 200 tiles per trajectory, or one lambda),    ONE launch per step, 256x16 / 32 / 64 tiles by the size of the launch,
    //   256 <= N <= ~4300                                                       scalar-broadcast column loop (step_fused.h, Q = 16 / 32 / 0; groups of GPs
    //                                                                           per tile workgroup with one lambda), two concurrent sub-batches
    //   W64 beyond, until a wide tiling fills the chip                          head kernel + pair_kernel_sb.h on 256x64 tiles, one trajectory per
    //                                                                           wave (pair_kernel_sbs.h with one lambda), 2-4 concurrent sub-batches
    //   ceil(B/2) x tiles(256x128) >= 2800, N > 512, D <= 5                     head + pair_kernel_sb.h on 256x128 tiles, two trajectories per wave
    //   ceil(B/2) x tiles(256x256) >= 2800 (1100 for N <= 512); D >= 6:         head + pair_kernel_sb.h on 256x256 tiles (the big batches: C3, C4);
    //   B x tiles(256x256) >= 1500; one lambda: B x tiles >= 1700               XCD-aware dispatch, rgroup 4
    //   full covariance / da > 2 / the fp32 sweep modes                         staged pair_kernel.h (fullcov.hip has its own plan)
    //                                                                           (da > 2: tests/test_gpu_offgrid.py::test_wide_action_ladder_vs_cport)
    const bool sb_ok = p->da <= 2;
    // 256x256 tiles once they give enough workgroups (profiles/r02/batch_size_map.txt): with two trajectories per wave
    // (D <= 5) from ~2800 on -- N = 2048: B = 32 5.28 k rollouts/s vs 5.45 k on 256x64, B = 48 equal, B = 64 6.02 k vs 5.76 k;
    // N = 1024: B = 96 18.5 k vs 19.2 k, B = 128 20.5 k vs 20.0 k --, with one per wave (D >= 6) from ~1500 on -- N = 4096, ds = 6:
    // ahead at every batch size from B = 2 (295 vs 282 rollouts/s) on.
    const bool tb2 = D <= 5 && B >= 2;
    const long wg0 = (long)(tb2 ? (B + 1) / 2 : B) * p->wl[0][0].nwork;
    // Small training sets (Np <= 512: at most 3 tiles per GP) switch earlier, from ~1100 workgroups: their 256x64 workgroups
    // run 64 columns on at most 4 waves behind a full prologue (N = 512, ds = 3, B = 256: 2.82 vs 3.20 ms per batch of 20 steps;
    // N = 300, ds = 2, B = 512: 0.88 vs 1.04 ms; N = 100, B = 2048: 1.30 vs 1.44 ms; below 1100 the 256x64 shape stays ahead).
    const long thr2 = p->Np <= 512 ? 1100 : 2800;
    const bool big = sb_ok ? wg0 >= (tb2 ? thr2 : 1500) : (long)((B + 1) / 2) * p->wl[0][0].nwork >= 1024;
    // (round 2: 2048 instead of 1024 work items -- below that the one-launch-per-step kernel of step_fused.h wins: N = 2048,
    // B = 2: 1.03 vs 1.19 ms per rollout; N = 1536, B = 4: 1.07 vs 1.23; N = 1024, B = 4: 0.67 vs 1.01)
    // (1700 since the head kernel is split over row chunks: N = 2048, B = 3: 1.16 vs 1.33 ms; N = 1536, B = 6: 1.31 vs 1.40)
    // (round 3, with four columns in flight and concurrent sub-batches on the 256x64 path: from 1250 work items for N >= 1024 --
    // N = 1024, B = 8 / 10: 0.92 vs 0.99 / 1.00 vs 1.18 ms; smaller training sets stay at 1700: N = 600, B = 16 0.89 vs 0.86 ms,
    // N = 400, B = 64 0.43 vs 0.38 ms -- profiles/r03/ab_fused_vs_sb_threshold.txt)
    // ... and, where the one-launch-per-step form on these tiles can run (step_fused.h, Q = 0: see r->fused below), from ~400 tile
    // workgroups: against the 64-row fused form N = 2048, B = 1 / 2 x1.19 / 1.43; N = 1024, B = 2 / 3 / 4 / 6 x1.06 / 1.24 / 1.19 / 1.34;
    // N = 512, ds = 3, B = 8 / 12 / 16 / 32 x1.01 / 1.16 / 1.19 / 1.38; N = 300, ds = 2, B = 32 / 64 x1.02 / 1.15; below ~300 workgroups
    // it loses (N = 1024, B = 1 x0.92; N = 512, B = 4 x0.77), and so do training sets of less than one row tile (N = 128, B = 128 x0.89)
    const long wg2 = (long)B * p->wl[0][2].nwork;
    const bool shared_on = p->shared_lambda && tn.shared != 0 && p->sh_ng >= 2;
    const bool fsb_can = sb_ok && !lowprec && p->da >= 1 && tn.fused_sb != 0 && (p->Np >= 256 || tn.fused_sb == 1) &&
                         p->wl[0][2].nwork <= 600 * p->ds;           // (N <= ~4300; measured up to N = 4096: B = 1 / 2 x1.22 / 1.18 at ds = 4, level at ds = 6)
    // ... and with NARROWER tiles (256x32, 256x16: work lists 5, 6) further down for training sets of at least two row tiles: a launch
    // of a few hundred 256x64 workgroups leaves most of the chip empty while each workgroup walks its 64 columns one L2 round trip
    // at a time (N = 2048, B = 1: 24.5 us per launch on 576 workgroups, profiles/r03/kernel_stats_C3_B1.csv); half / quarter tiles
    // give 2x / 4x the workgroups, each living half / a quarter as long (profiles/r03/ab_fused_sb_narrow_tiles.txt, ms per rollout
    // on 64 / 32 / 16 columns: N = 1024, B = 1 0.359 / 0.300 / 0.270 (64-row form 0.330), B = 2 0.409 / 0.359 / 0.359, B = 4
    // 0.561 / 0.484 / 0.514, B = 8 0.673 / 0.661 / 0.825; N = 1536, ds = 3, B = 1 0.391 / 0.330 / 0.308, B = 2 0.503 / 0.417 / 0.502;
    // N = 512, ds = 3, B = 8 0.434 / 0.357 / 0.325, B = 16 0.481 / 0.396 / 0.407; N = 2048, B = 1 0.554 / 0.539 / 0.679 -- every tile
    // workgroup re-reduces its trajectory's partial sums, 2304 of them there on 16 columns; N <= 448: the 64-row form stays ahead
    // until ~400 workgroups, N = 400, ds = 2, B = 16 0.179 vs 0.200 / 0.190)
    const bool narrow_ok = fsb_can && p->Np >= 512;
    const bool mid = !big && sb_ok && (wg2 >= (p->Np >= 1024 ? 1250 : 1700) || (fsb_can && wg2 >= (narrow_ok ? 150 : 400)));
    // 256x128 tiles with two trajectories per wave where they already give the workgroups the 256x256 tiles do not yet
    // (profiles/r03/ab_tiling_256x128.txt: N = 2048, B = 24 / 32 4.02 / 5.07 vs 4.78 / 6.12 ms on 256x64; N = 1024, B = 96 / 128
    // 4.51 / 5.71 vs 4.98 / 6.49 ms; from there on 256x256 is 3-4 % ahead)
    // (re-measured against the plan as it stood at the end of round 3, whose mid-size forms had moved: ahead from ~1600 of its own
    // workgroups -- N = 2048, B = 12 / 14 / 16 / 18 x1.00 / 1.05 / 1.10 / 1.05; N = 1024, B = 44 / 48 / 56 / 64 x1.01 / 1.05 / 1.07 / 1.11;
    // N = 1536, ds = 3, B = 24 / 32 x1.07 / 1.14; N = 2048, B = 10 x0.96)
    // ... but only beyond the reach of the one-launch form, which is ahead of it wherever both apply (N = 1024, B = 40 2.27 vs 2.57 ms;
    // N = 768, B = 72 2.35 vs 2.58; N = 600, B = 96 2.36 vs 2.64)
    const long fsb_max = shared_on ? 7000 : (p->wl[0][2].nwork <= 200 ? 9000 : (D <= 5 ? 7000 : 4700));      // (7000 at D <= 5 with the XCD-aware order: N = 2048, B = 12 two kernels on 256x128 tiles 2.70 | one launch 2.50 ms, B = 16 the other way round)           // (9000: N = 400, ds = 3, da = 2, B = 288 two-kernel form 2.09 | one launch per step 1.86 ms, profiles/r05/autotune_512_verbose.txt)
    const bool fsb_take = fsb_can && wg2 <= fsb_max;
    // (Np = 512 -- two row tiles -- runs its mid range on the 256x128 tiling too: B = 288 / 320 / 384 / 640 x1.14 / 1.10 / 1.09 / 1.15 over 256x256,
    // profiles/r05/autotune_grid_second.txt)
    const bool mid512 = p->Np == 512 && B < 768 && !fsb_take && sb_ok && tb2 && (long)((B + 1) / 2) * p->wl[0][4].nwork >= 1600;
    const bool big128 = (!big || mid512) && !fsb_take && sb_ok && tb2 && (p->Np > 512 || mid512) && (long)((B + 1) / 2) * p->wl[0][4].nwork >= 1600;
    r->sb = (sb_ok && (big || mid)) ? 1 : 0;
    // (round 5: a small training set stays on the one-launch form as far as that reaches -- N = 400, ds = 3, da = 2, B = 288: 256x256 tiles, two
    // kernels per step 2.19 | one launch per step 1.88 ms, profiles/r05/autotune_grid_third.txt)
    const bool big_small_fused = big && p->Np <= 512 && fsb_take && sb_ok && tn.tiling < 0;
    const bool many = (long)p->wl[0][1].nwork > 256L * p->ds;        // > 256 one-wave tiles per GP (N >= 1472)
    r->tiling = big_small_fused ? 2 : ((big && !(mid512 && big128)) ? 0 : (big128 ? 4 : (mid ? 2 : (many ? 3 : 1))));
    if (r->tiling == 2 && narrow_ok && wg2 < 1000)           // 32 columns from ~300 workgroups of 64, 16 below (while the partial sums
        r->tiling = (wg2 >= 300 || p->wl[0][6].nwork > 1300) ? 5 : 6;      // of a trajectory stay within ~1300)
    // A training set whose LAST row tile is a quarter or half tile (Np = 320, 384: N = 257...384): its 256x64 workgroups carry one or
    // two waves of four; on 32 columns there are twice as many, half as long -- measured with gpmpc_pack_autotune (round 4,
    // profiles/r04/autotune_small_n.txt): N = 300, ds = 4, B = 48 / 64 / 96 / 128 / 160 x1.07 / 1.08 / 1.09 / 1.10 / 1.07, ds = 2,
    // B = 128 / 160 x1.06; N = 400 (Np = 448) and N = 512: level, N = 200 (one row tile): level.
    // (not with one lambda for all GPs: there the 64-column tiles are ahead -- round 5 grid, profiles/r05/autotune_grid_first_shared.txt:
    // N = 300, ds = 4, B = 128 0.58 | 0.38 ms, ds = 2, B = 320 0.49 | 0.33)
    // (round 5, with the XCD-aware dispatch order -- on from B = 2 unless switched off --: the 64-column tiles are ahead for distinct
    // lambdas as well: N = 300, ds = 4, B = 64 / 96 / 128 0.298 | 0.274, 0.42 | 0.35, 0.55 | 0.45 ms; ds = 2, B = 64 0.171 | 0.162 --
    // profiles/r05/autotune_xcd_verbose.txt: the rule stays for the natural order only)
    if (r->tiling == 2 && fsb_take && p->Np > 256 && p->Np <= 384 && wg2 >= 1000 && !shared_on && tn.xcdmap == 0) r->tiling = 5;
    if (tn.pair_sb >= 0) {                                   // 0 = staged kernel, 1 = scalar broadcast
        r->sb = (tn.pair_sb != 0 && sb_ok) ? 1 : 0;
        r->tiling = r->sb ? (big ? 0 : (big128 ? 4 : 2)) : (big ? 0 : (many ? 3 : 1));
    }
    if (tn.tiling >= 0) { const int v = tn.tiling; if (v == 0 || ((v == 1 || v == 3) && !r->sb) || ((v == 2 || v == 4) && r->sb) || ((v == 5 || v == 6) && r->sb && fsb_can)) r->tiling = v; }
    const bool wide = r->tiling == 0 || r->tiling == 4;          // 256-row tiles of the XCD-sorted lists
    // scalar-broadcast kernel: two trajectories per wave on the big tiling up to D = 5 (two independent dependency chains per
    // lane, one M_ij load for both: C3 +2.6 %, objective-only +14 %; 82 VGPRs); D = 7 (C4) is 2.5 % faster with one
    r->tb = r->sb ? ((wide && D <= 5 && B >= 2) ? 2 : 1) : (B >= 2 ? 2 : 1);
    if (tn.tb) { const int v = tn.tb; if (v == 1 || v == 2 || (v == 4 && !r->sb)) r->tb = v; }
    // Dispatch interleave of the scalar-broadcast kernel (pair_kernel_sb.h): 4 row tiles per trajectory share each fetch
    // of the G rows (C3 fabric reads per launch 757 -> 418 MB by FETCH_SIZE at the same speed; C4 +0.5 %).
    r->rgroup = 4;
    if (tn.rgroup >= 1 && tn.rgroup <= 16) r->rgroup = tn.rgroup;
    if (!wide) r->rgroup = 1;
    if (lowprec) { r->sb = 0; r->tiling = 0; r->tb = 1; }      // tolerance-sweep kernels: 256x256 work list, one trajectory per workgroup
    // Small batches on the 64-row work lists: ONE launch per horizon step (step_fused.h) instead of head + staged pair
    // kernel -- the B = 1 callbacks of a solver loop are pure dependent latency (GPMPC_FUSED=0 keeps the two-kernel form).
    // (every workgroup of the fused kernel re-reduces the Z0 partials of ALL work items: quadratic in their number, fine up to
    // a few thousand -- N = 2048 has 2112 --, 16x off at the 6336 items of N = 4096, which keeps the two-kernel form)
    r->fused = (!r->sb && !lowprec && (r->tiling == 1 || r->tiling == 3) && p->da <= 2 && tn.fused != 0 &&
                p->wl[0][r->tiling].nwork <= 4096) ? 1 : 0;
    // Mid-size batches on the 256x64 tiling: the same single launch per step with the scalar-broadcast column loop in the tile
    // workgroups (step_fused.h, Q = 0).  Every tile workgroup re-reduces the Z0 partial sums of its trajectory: up to 320 tiles
    // per GP (N <= 2048; 256 of them are prefetched in one round trip).
    // Measured against head + pair kernel with concurrent sub-batches (tools/env_ab.py --var GPMPC_FUSED_SB, synchronising after
    // each call; profiles/r03/ab_fused_sb.txt): N = 1024, B = 8 / 12 / 16 / 24 / 32 / 48 x1.29 / 1.42 / 1.26 / 1.08 / 1.04 / 0.98;
    // N = 2048, B = 4 / 6 / 8 / 12 x1.17 / 1.10 / 1.06 / 0.97; N = 768, B = 24 / 48 x1.36 / 1.13: up to ~4700 tile workgroups per
    // launch (beyond, the longer prologue of every tile workgroup costs more than the head kernel it replaces).
    // (up to 600 tiles per GP, N <= ~4300.  An earlier limit of 320 came from N = 4096, ds = 6, B = 1 at 4.35 vs 3.73 ms -- measured on D = 7
    // instances that spilled 21 registers; compiled for 4 waves per SIMD they are level there, and ds = 4 gains x1.2 at N = 3584 / 4096)
    // With ONE lambda for all GPs the shared-lambda pair kernel (two launches per step) is the alternative: the one-launch form
    // evaluating the exponent per GP is ahead of it up to ~3000 tile workgroups (profiles/r03/ab_fused_sb_vs_shared.txt:
    // N = 1024, B = 8 / 12 / 16 / 24 / 32 x1.52 / 1.45 / 1.20 / 0.99 / 0.75; N = 2048, B = 2 / 4 / 8 x1.37 / 1.29 / 0.85), and with
    // groups of GPs per tile workgroup (r->shared below) up to ~7000.
    // (training sets of up to ~200 tiles per trajectory, N <= 1024 at ds = 4, whose tile workgroups have less to re-reduce: ahead or
    // level up to ~7000 -- N = 1024, B = 32 / 48 1.88 / 2.72 vs 2.17 / 2.91 ms on one box, 1.95 / 2.83 vs 2.02 / 2.77 on another;
    // N = 768, B = 64 2.14 vs 2.44 ms)
    if (r->sb && r->tiling == 2 && r->tb == 1 && fsb_can && (tn.fused_sb == 1 || wg2 <= fsb_max))
        r->fused = 2;
    if (r->sb && (r->tiling == 5 || r->tiling == 6) && r->tb == 1 && fsb_can) r->fused = 2;   // narrower tiles: this form only
    if (r->fused) r->tb = 1;
    // a quarter of a tile's columns per workgroup while whole tiles would leave most SIMDs without a wave
    r->fq = (r->fused == 1 && r->tiling == 1 && (long)B * p->wl[0][1].nwork < 256) ? 4 : 1;
    r->waves = p->wl[0][r->tiling].waves;
    r->nwork = p->wl[0][r->tiling].nwork;
    // Shared length-scales: one exponent / exp per pair for a group of GPs (pair_kernel_sbs.h) wherever the scalar-broadcast
    // kernel would run.  256x256 tiles once they give ~1700 workgroups (one trajectory per workgroup), else 256x64.
    r->shared = 0; r->sh_list = 0;
    // groups of TWO GPs (twice the workgroups of the pack's group size, 17.5 instead of 14.25 instructions per pair and GP at D = 5) while
    // the launch is small: ms per batch, groups of 2 | groups of 4 | one GP per workgroup -- N = 1024, B = 8 0.65 | 0.80 | 0.69, B = 12
    // 0.70 | 0.87 | 0.81, B = 16 0.83 | 0.89 | 0.99, B = 24 1.07 | 1.16 | 1.44; N = 2048, B = 2 0.61 | 0.84 | 0.69, B = 4 0.86 | 0.95 | 1.03,
    // B = 8 1.51 | 1.38 | 1.91; N = 768, B = 16 0.64 | 0.73 | 0.72 (profiles/r03/ab_fused_shared.txt)
    r->fng = p->sh_ng;
    if (p->sh_ng > 2 && p->ds % 2 == 0 && p->wl_sh[3].work_dev && wg2 < 4200) r->fng = 2;
    // (two GPs: from ~700 tile workgroups -- N = 300, ds = 2, B = 64 / 128 0.195 / 0.205 -> 0.155 / 0.183 ms, profiles/r05/autotune_grid_second_shared.txt)
    if (r->sb && r->fused == 2 && r->tiling == 2 && shared_on && (wg2 >= (r->fng == 2 ? (p->ds == 2 ? 700 : 1000) : 2200) || tn.fused_sb == 1)) {
        // one lambda for all GPs AND the one-launch form: its tile workgroups take groups of sh_ng GPs (step_fused.h, NG > 1) on the
        // shared 256x64 list.  Three forms compete for such a pack (profiles/r03/ab_fused_shared.txt, ms per batch: groups of GPs in one
        // launch | one GP per tile workgroup in one launch | shared-lambda pair kernel, two launches): N = 1024, B = 8 0.81 | 0.67 | -,
        // B = 16 0.89 | 0.99 | -, B = 24 1.17 | 1.42 | 1.64, B = 32 1.45 | 1.84 | 1.67, B = 48 1.94 | - | 1.91; N = 2048, B = 2
        // 0.82 | 0.67, B = 4 0.94 | 1.03, B = 8 1.37 | 1.88 | 1.69, B = 12 2.06 | - | 2.05; N = 512, ds = 3, B = 32 0.64 | 0.56, B = 128
        // 1.10 | 1.48 | 1.41: per-GP workgroups (4x as many, narrower tiles) below ~2200 workgroups of 64 columns, groups up to ~7000
        r->shared = 1; r->sh_list = 1;
        r->tb = 1; r->waves = 4;
        r->nwork = p->ds * p->sh_tiles[1];
    } else
    if (r->sb && r->fused != 2 && !lowprec && p->shared_lambda && tn.shared != 0 && p->sh_ng >= 2) {
        r->shared = 1;
        // (round 3: a 256x128 list, wl_sh[2], is built for the A/B only -- GPMPC_TILING=4 --: with one trajectory per workgroup it has
        // nothing to share that the 256x64 tiles under the concurrent sub-batches do not have; N = 2048, B = 16...40 -3...-20 %,
        // N = 1024, B = 128 / 160 +2 / +3 % -- profiles/r03/ab_shared_tiling.txt.  256x256 from 1700 workgroups: N = 2048, B = 40
        // 4.90 (256x64) vs 5.32 ms, B = 48 5.71 vs 5.77; N = 1024, B = 160 5.10 vs 5.19)
        r->sh_list = ((long)B * p->wl_sh[0].nwork >= 1700) ? 0 : 1;
        if (tn.tiling == 0 || tn.tiling == 2 || tn.tiling == 4) r->sh_list = tn.tiling == 0 ? 0 : (tn.tiling == 2 ? 1 : 2);
        r->tb = 1; r->waves = 4;
        r->nwork = p->ds * p->sh_tiles[r->sh_list];           // partial sums per trajectory: [GP][tile]
        r->rgroup = r->sh_list != 1 ? ((tn.rgroup >= 1 && tn.rgroup <= 16) ? tn.rgroup : 4) : 1;
    }
    // One trajectory (or a few) of a training set whose 256x64 tiles would take several workgroup generations: balanced runs of up to 256
    // columns, ONE generation per trajectory (worklist.h, work list 7; step_fused.h, Q = 256)
    if (r->fused == 2 && r->tiling == 2 && !r->shared && tn.tiling < 0 && p->wl[0][7].work_dev) {
        r->tiling = 7;
        r->nwork = p->wl[0][7].nwork;
    }
    // Columns per iteration of the scalar-broadcast kernel: 4 on the 256x64 tiling (mid-size batches: latency tolerance of
    // the partly filled generations, pair_kernel_sb.h), 1 on full launches.
    // (tools/env_ab.py --var GPMPC_SB_UNROLL: +8...14 % up to ~2 generations of workgroups, -4 % from ~4 on)
    r->colunroll = (r->sb && !r->shared && !lowprec && r->tiling == 2 && r->tb == 1 && tn.colunroll != 1 &&
                  ((long)B * r->nwork <= 4096 || tn.colunroll == 4)) ? 4 : 1;
    r->xcdmap = tn.xcdmap;
    // Whole-horizon kernel, one workgroup per trajectory (traj_persist.h): large batches of a small training set -- at least about one
    // trajectory per CU, X within the kernel's LDS budget.  r->fused = 3; r->pwaves = waves per workgroup.
    r->pwaves = 0;
    // Measured against the step-per-launch plan (tools/lib_ab.py, profiles/r04/ab_persist.txt; ms per batch, H = 10, default | 16 waves |
    // 8 waves): N = 300, ds = 4: B = 128 0.70 | 0.92 | 1.29, B = 192 1.34 | 0.95 | 1.48, B = 256 1.31 | 0.99 | 1.56, B = 384 1.72 | 1.83 | 1.77,
    // B = 512 2.11 | 1.93 | 1.80; N = 300, ds = 2, B = 256 0.57 | 0.43 | 0.47; N = 200, ds = 2, B = 1024 0.58 | 0.57 | 0.48; N = 400, ds = 3,
    // da = 2, B = 256 2.11 | 1.68 | 2.54; N = 512, ds = 3, H = 20, B = 256 3.01 | 2.49 | 4.11; N = 640, B = 256 2.75 | 3.03; N = 1024,
    // H = 20, B = 256 10.9 | 14.4 (every workgroup streams all of M from L2 / Infinity Cache each step: 6.5 TB/s at N = 1024).
    // Round 5 (the kernel is x1.3-1.6 faster than the one the round-4 thresholds were fitted to; re-measured with gpmpc_pack_autotune over
    // N = 200 ... 640, B = 64 ... 1024: profiles/r05/autotune_grid_first*.txt, autotune_grid.txt): a COST comparison instead of fill thresholds.
    // One 16-wave workgroup per CU (or two of 8 waves), so the kernel's time goes in generations of num_cu (2 num_cu) trajectories; a partly
    // filled generation is shorter (less contention for the L2: N = 300, ds = 4: B = 128 / 192 / 256 0.56 / 0.59 / 0.69 ms): 0.64 + 0.36 fill of
    // a full one.  In units of a full 16-wave generation: cost16 = generations (last one discounted), cost8 = r8 x the same over 2 num_cu slots,
    // r8 = 1.6 (light trajectories) ... 2.0; the step-per-launch forms cost (B / num_cu) x inv_e(Np), inv_e = how much less efficient per
    // trajectory they are than a full generation of this kernel: 2.15 at Np = 256 (break-even B ~ 96), 1.55 at 320 (~140), 1.36 at 448 (~175),
    // 1.16 at 512 (~200), 1.05 at 640 (full generations only); with one lambda x1.25 (units of 3 / 4 GPs).  Np >= 512 beyond two generations:
    // never (every workgroup streams all of M each step; the 256x128 / 256x256 pair kernels are ahead: N = 512, B = 640 6.2 | 5.4 ms).
    {
        const int cu = p->num_cu > 0 ? p->num_cu : 256;
        auto gens_cost = [](int Bn, int slots) {
            const int full = Bn / slots, rem = Bn - full * slots;
            return (double)full + (rem > 0 ? 0.64 + 0.36 * (double)rem / slots : 0.0);
        };
        const bool pshared = shared_on && p->ds >= 2 && D >= 3 && D <= 6;
        const bool all_in_one = pshared && ((p->ds == 4 && D == 5) || (p->ds == 3 && D <= 5));   // 16-wave workgroups run ALL GPs of the pack in one unit
        const double work = (double)p->ds * p->Np * p->Np;
        // (an EFFECTIVE ratio, fitted on batches that end in a partly filled 8-wave generation; a refit on full generations -- 1.63 at N = 200, ds = 2,
        // 1.93 at 300 / 2 and 200 / 4 -- with its own partial-generation term moved more shapes away from the measured best than it brought back:
        // profiles/r05/autotune_grid_sixth.txt and the run before it)
        double r8 = 1.4 + 4.0e-12 * work * work;                                         // (grid: 1.46 at N = 200, ds = 2; 1.53 at 300 / 2; ~1.7 at 200 / 4; > 2.05 at 300 / 4)
        if (r8 > 2.2) r8 = 2.2;
        if (all_in_one) r8 *= 1.25;                                                      // (8-wave workgroups fall back to units of two GPs)
        const double cost16 = gens_cost(B, cu), cost8 = r8 * gens_cost(B, 2 * cu);
        const int Npq = p->Np;
        double inv_e = Npq <= 256 ? (p->ds <= 2 ? 2.15 : 1.95) : (Npq <= 320 ? 1.50 : (Npq <= 384 ? 1.50 : (Npq <= 448 ? 1.45 : (Npq <= 512 ? 1.16 : (Npq <= 576 ? 1.10 : 1.14)))));      // (640: 1.14 -- B = 224 step-per-launch 2.43 | whole horizon 2.25 ms, B = 192 the other way round)
        if (pshared) inv_e *= p->ds <= 2 ? 1.0 : (Npq <= 448 ? 1.15 : 1.10);
        if (Npq >= 512 && B > 2 * cu && !pshared) inv_e = 0.9;
        const double cost_spl = (double)B / cu * inv_e;
        int pw = 0;
        if ((cost16 <= cost8 ? cost16 : cost8) < 0.97 * cost_spl) pw = cost8 < cost16 ? 8 : 16;
        if (tn.persist == 8 || tn.persist == 16) pw = tn.persist;
        // With ONE lambda for all GPs the step-per-launch forms share exponent and exp across the GPs of a pair, this kernel does not
        // (yet): from three GPs on they are ahead of it (shared packs, ms per batch, step-per-launch | 16 waves | 8 waves: N = 300, ds = 4,
        // B = 256 0.87 | 0.99 | 1.56, B = 512 1.42 | 1.93 | 1.81; N = 512, ds = 3, B = 256 1.97 | 2.49; with two GPs the whole-horizon
        // kernel still wins: N = 300, ds = 2, B = 256 0.49 | 0.43, N = 200, B = 1024 0.70 | 0.56 | 0.47 -- profiles/r04/ab_persist_shared.txt)
        // ... so with one lambda this kernel runs over units of TWO GPs (traj_persist.h, NG = 2; instantiated up to D = 6), and packs it
        // cannot serve that way (D >= 7) keep the step-per-launch forms from three GPs on.  Shared packs, step-per-launch | units of two
        // GPs, 16 waves | 8 waves (profiles/r04/ab_persist_shared_ng2.txt): N = 300, ds = 4, B = 256 0.86 | 0.68 | 0.78, B = 512 1.41 | 1.27 | 1.10;
        // ds = 2, B = 256 0.49 | 0.33; ds = 5, B = 256 1.34 | 1.03; N = 200, ds = 2, B = 1024 0.69 | 0.43 | 0.33; N = 400, ds = 3, da = 2 1.44 | 1.39;
        // N = 512, ds = 3, H = 20 1.94 | 2.06 (not taken: up to Np = 448 with one lambda).  D = 7 loses with distinct lambdas too
        // (N = 300, ds = 6: 2.19 | 2.32; ds = 5, da = 2: 1.69 | 1.98 -- the accumulators leave the column loop one chain and two loads in
        // flight): taken up to D = 6.
        // an explicit kernel-form override (GPMPC_FUSED=0, GPMPC_PAIR_SB, GPMPC_TILING, GPMPC_FUSED_SB) asks for a step-per-launch form: an A/B
        // with those variables must not silently run this kernel instead (GPMPC_PERSIST=8|16 still forces it)
        const bool form_forced = tn.fused == 0 || tn.pair_sb >= 0 || tn.tiling >= 0 || tn.fused_sb >= 0;
        const bool shared_ahead = shared_on && !pshared && p->ds >= 3;
        r->png = 1;
        if (!lowprec && p->da >= 1 && p->da <= 2 && p->Np <= GPMPC_PERSIST_MAXNP_HOST && H * p->da <= 1024 && tn.persist != 0 &&
            pw && (tn.persist > 0 || (p->Np <= 640 && D <= 6 && !shared_ahead && !form_forced))) {
            r->fused = 3; r->sb = 0; r->shared = 0; r->tb = 1; r->rgroup = 1; r->colunroll = 1; r->fq = 1;
            r->pwaves = pw;
            // units of two GPs; ALL GPs of the pack in one unit where that instance exists (traj_persist.h: ds = 4 at D = 5, ds = 3 at D <= 5;
            // 16-wave workgroups only: two 8-wave workgroups per CU do not fit their static LDS)
            r->png = pshared ? ((pw == 16 && all_in_one) ? p->ds : 2) : 1;
            r->nwork = 0;
        }
    }
    // Row chunks of the head kernel (two-kernel form only): about 64 workgroups, at least 512 rows each.  N = 4096, ds = 6,
    // B = 1: the head kernel was 66 us of a 172 us step on 6 workgroups.
    r->hchunks = 0; r->hrows = 0;
    if (!r->fused && !lowprec) {
        int c = 64 / (B * p->ds);
        if (c > p->Np / 512) c = p->Np / 512;
        if (c > 16) c = 16;
        if (tn.hchunks >= 0) c = tn.hchunks;
        if (c > 1) { r->hrows = ((p->Np + c - 1) / c + 255) & ~255; r->hchunks = (p->Np + r->hrows - 1) / r->hrows; if (r->hchunks <= 1) r->hchunks = 0; }
    }
    return shape;
}

// Measured on one MI355X (profiles/step1_quad/threshold.txt; ms of the step-1 pair launch, FIRST variant | this kernel): wherever the plan is the
// two-launch form the kernel is ahead -- N = 2048, ds = 4: B = 13 0.114 | 0.045, B = 32 0.171 | 0.052, B = 256 1.43 | 0.27; N = 1024: B = 64
// 0.109 | 0.048; N = 4096, ds = 6: B = 8 0.48 | 0.11, B = 128 5.67 | 0.68 -- so the rule has no crossover of its own: from one full block of 8
// trajectories, the smallest batch measured.  Blocks of 8 against 16 trajectories: 8 is ahead at every shape but one (N = 2048, B = 96 level).
#define GPMPC_Q1_MIN_B 8
bool gpmpc_step1_quad_plan(const gpmpc_pack* p, const RollShape& r, int B, bool lowprec) {
    const int knob = p->tune.step1_quad;
    if (knob == 0 || lowprec || p->tune.no_first) return false;
    if (r.fused || !r.sb || r.shared || !gpmpc_q1_shape(p->ds, p->da)) return false;
    // A pack with one lambda for all GPs reaches pair_kernel_sb.h only under GPMPC_SHARED=0, the A/B partner of the shared-lambda kernels: those
    // round the exponent of a pair exactly as the FIRST variant does, and tests/test_gpu_offgrid.py holds the two forms to 1e-9 of each other on
    // that ground (an agreement ten times tighter than either form's distance from the long double step).  This kernel rounds differently -- as
    // accurately, profiles/step1_quad/accuracy.txt -- so such a pack keeps the FIRST variant.
    if (p->shared_lambda) return false;
    if (p->wl[0][r.tiling].it != 256) return false;
    return knob == 1 || B == 0 || B >= GPMPC_Q1_MIN_B;
}

RollLayout gpmpc_layout_for(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad) {
    const int D = p->D;
    RollLayout L;
    L.nm = gpmpc_num_moments(D, true, grad);
    L.pps = D + D * D;
    L.sps = p->nominal ? sps_nominal(D) : sps_of(D);
    gpmpc_carver c;
    auto take = [&](size_t n) { return c.take(n * sizeof(double)); };
    L.off_pp = take((size_t)B * p->ds * L.pps);
    L.off_sp = take((size_t)2 * B * p->ds * L.sps);
    L.off_part = take((size_t)(r.fused ? 2 * r.fq : 1) * B * r.nwork * L.nm);     // fused: double-buffered by step parity
    L.off_partz = take(r.fused ? (size_t)2 * r.fq * B * r.nwork : 0);
    L.off_mpart = take(r.hchunks > 1 ? (size_t)2 * B * p->ds * r.hchunks * (1 + 2 * D) : 0);
    L.off_jac = take(grad ? (size_t)B * H * 2 * p->ds * (2 * p->ds + p->da) : 0);
    L.gw = gpmpc_sb_gw(D, p->ds);
    // column rows: [B][GP][Np][gw] written by the head kernel, or one [64][gw] slot per tile workgroup of the mid-size fused form
    L.off_G = take(r.fused == 3 ? (size_t)B * p->ds * p->Np * L.gw : r.fused == 2 ? (size_t)B * (r.shared ? gpmpc_fused_shared_list(p, r).nwork : r.nwork) * p->wl[0][r.tiling].jt * L.gw
                                : (r.sb ? (size_t)B * (r.shared ? 1 : p->ds) * p->Np * L.gw : 0));
    L.off_means = take((size_t)B * (H + 1) * p->ds);
    L.off_vars = take((size_t)B * (H + 1) * p->ds);
    L.total = c.total();
    return L;
}

// A MID-SIZE batch (256x64 tiling) runs as S sub-batches on S streams (parallel branches of the graph under graph replay).
// A horizon step is a serial chain head kernel -> pair kernel, and at these sizes neither fills the chip for long (the head
// kernel runs B ds workgroups, the pair kernel ends in a partly filled generation: tools/sb_stamps.py); two independent chains
// fill each other's gaps.
int gpmpc_split_count(const gpmpc_pack* p, const RollShape& r, int B, bool lowprec, bool eager, int split_over, int H, int grad) {
    if (lowprec || !r.sb) return 1;
    if (!split_over && H > 0 && grad >= 0)
        if (const gpmpc_tuned_entry* te = tuned_lookup(p, B, H, grad != 0)) { int S = te->S; if (eager && S > 2) S = 2; return S < 1 ? 1 : (S > B ? B : S); }
    const bool mid = r.shared ? r.sh_list == 1 : r.tiling == 2;
    // measured (tools/env_ab.py --var GPMPC_SPLIT, profiles/r03/split_ab.txt): N = 1024, B = 16: 11.3 -> 13.8 (2 branches) -> 14.3 k
    // rollouts/s (4); N = 2048, B = 4 / 16: +15 % / +13 %; a branch must keep at least two trajectories, and branches whose
    // pair launch alone fills the chip twice over gain nothing unless they are wide (N = 4096, B = 2 as 1 + 1: -20 %)
    // A caller who needs each result before the next call (a solver loop) sees the latency of ONE call: there every extra
    // branch also costs launch work up front, and a branch must keep ~900 workgroups per pair launch to pay for itself
    // (N = 1024, B = 16, synchronising after every call: 2 branches x1.12, 4 branches x0.93-1.02; B = 32: 4 branches x1.09-1.13;
    // with calls queued back to back 4 branches give x1.27 / x1.24 -- profiles/r03/split_latency_vs_throughput.txt).
    int S = 1;
    if (r.fused == 2) {
        // one launch per step: two branches are ahead everywhere (tools/env_ab.py --var GPMPC_SPLIT, N = 1024, B = 8 / 16 / 24: one branch
        // x1.03 / 0.86 / 0.94, two x1.11 / 1.01 / 1.06, four x1.02 / 0.95 / 1.01 of the two-kernel rule's choice)
        // ... but only from ~800 tile workgroups per launch on (gpmpc_pack_autotune, round 4: N = 200, ds = 2, B = 64 and ds = 4, B = 32
        // -- 512 tile workgroups -- run x1.21 faster unsplit; N = 200, ds = 4, B = 64 and everything larger keeps two), and a pair of
        // trajectories of a large training set splits too (N = 2048, B = 2: x1.04)
        // (groups of GPs per tile workgroup: count the workgroups, not the partial sums -- N = 300, ds = 2 with one lambda, B = 128: 768 workgroups,
        // 0.210 ms in two branches, 0.184 in one)
        const long wgs = (long)B * (r.shared && r.fng > 1 ? r.nwork / r.fng : r.nwork);
        S = ((B >= 4 && wgs >= 800) || (B >= 2 && wgs >= 1000 && wgs <= 2500)) ? 2 : 1;
    } else if (mid && B >= 4) {
        S = B / 2 < GPMPC_MAX_SPLIT ? B / 2 : GPMPC_MAX_SPLIT;
        while (S > 1 && (long)(B / S) * r.nwork >= 4096 && B / S < 8) --S;
        while (S > 1 && (long)(B / S) * r.nwork < 900) --S;
        if (S == 3) S = 2;
    }
    // 256x256 tiling with two trajectories per wave, up to ~8 generations of workgroups: two sub-batches fill each other's partly
    // filled last generation (N = 2048: B = 48 / 64 / 128 +11 / +9 / +4 %, B = 256 +-0; N = 1024, B = 128 / 256 +6 / +5 %;
    // one trajectory per wave (D >= 6, N = 4096): -3...-7 %, not split) -- profiles/r03/split_big_ab.txt
    if (!mid && !r.shared && (r.tiling == 0 || r.tiling == 4) && r.tb == 2 && B >= 16 && (long)((B + 1) / 2) * r.nwork <= 10000) S = 2;
    // Launched plainly (no graph) the branches are streams of the pack, which the runtime maps onto a handful of hardware queues
    // shared with every other stream of the process: four branches then ran from x1.27 to x0.87 of the unsplit call depending on
    // what else the process had created (N = 1024, B = 32 in a fresh process: 1 / 2 / 3 / 4 branches 2.15 / 1.95 / 1.92 / 2.47 ms
    // -- profiles/r03/split_eager_branches.txt); two are ahead in every process measured.
    if (eager && S > 2) S = 2;
    if (p->tune.split >= 1) S = p->tune.split;
    if (split_over >= 1) S = split_over;
    if (S > GPMPC_MAX_SPLIT) S = GPMPC_MAX_SPLIT;
    if (S > B) S = B;
    return S;
}
size_t gpmpc_split_slices(const gpmpc_pack* p, const RollShape& r, int B, int H, bool grad, int S, RollSlice* out) {
    size_t off = 0;
    for (int k = 0; k < S; ++k) {
        RollSlice& s = out[k];
        s.b0 = (int)((long)B * k / S); s.b1 = (int)((long)B * (k + 1) / S);
        s.lay = gpmpc_layout_for(p, r, s.b1 - s.b0, H, grad);
        s.ws_off = off;
        off += s.lay.total;
    }
    return off;
}

extern "C" size_t gpmpc_rollout_workspace_bytes(const gpmpc_pack* p, int B, int H, unsigned flags) {
    if (!p || B < 1 || H < 1) return 0;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
    GraphModeGuard mode((flags & GPMPC_USE_GRAPH) ? 1 : 0);
    const RollShape r = gpmpc_choose_shape(p, B, H, grad, lowprec);
    size_t need = gpmpc_layout_for(p, r, B, H, grad).total;
    const int S = gpmpc_split_count(p, r, B, lowprec, false, 0, H, grad ? 1 : 0);     // mid-size batches run as S concurrent sub-batches, each with its own slice
    if (S > 1) { RollSlice sl[GPMPC_MAX_SPLIT]; const size_t sb = gpmpc_split_slices(p, r, B, H, grad, S, sl); if (sb > need) need = sb; }
    return need;
}

// What a rollout call of this shape launches, as text (bench.py names the dominant kernel with it, the tests check which form a
// shape reaches, tools/ compare plans): "form=<...> kernel=<...> tiling=<rows>x<cols> workgroups=<per step> launches_per_step=<n> split=<S> ..."
extern "C" int gpmpc_plan_describe(const gpmpc_pack* p, int B, int H, unsigned flags, char* out, size_t out_bytes) {
    if (!p || !out || out_bytes < 64 || B < 1 || H < 1) return GPMPC_E_ARG;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, lowprec = (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) != 0;
    GraphModeGuard mode((flags & GPMPC_USE_GRAPH) ? 1 : 0);
    const RollShape r = gpmpc_choose_shape(p, B, H, grad, lowprec);
    const int S = gpmpc_split_count(p, r, B, lowprec, (flags & GPMPC_USE_GRAPH) == 0, 0, H, grad ? 1 : 0);
    static const int cfg[8][2] = {{256, 256}, {64, 64}, {256, 64}, {64, 128}, {256, 128}, {256, 32}, {256, 16}, {256, 256}};
    const int D = p->D, ds = p->ds;
    char kern[160];
    const char* form;
    long wgs;
    if (r.fused == 3) {
        form = "persist";
        snprintf(kern, sizeof(kern), "k_traj_persist<%d,%d,%s,%d>x%dwaves", D, ds, grad ? "true" : "false", r.png, r.pwaves);
        wgs = B;
    } else if (r.fused == 2) {
        const int q = r.tiling == 2 ? 0 : cfg[r.tiling][1], ng = r.shared ? r.fng : 1;
        const gpmpc_worklist& wsh = gpmpc_fused_shared_list(p, r);
        form = r.shared ? "fused_sb_shared" : "fused_sb";
        snprintf(kern, sizeof(kern), "k_step_fused<%d,%d,%s,%d,%d>", D, ds, grad ? "true" : "false", q, ng);
        wgs = (long)B * ((r.shared ? wsh.nwork : r.nwork) + 2 * ds);
    } else if (r.fused == 1) {
        form = "fused_staged";
        snprintf(kern, sizeof(kern), "k_step_fused<%d,%d,%s,%d,1>", D, ds, grad ? "true" : "false", r.fq);
        wgs = (long)B * (r.nwork * r.fq + 2 * ds);
    } else if (lowprec) {
        form = "lowprec"; snprintf(kern, sizeof(kern), "k_pair_lowprec<%d>", D); wgs = (long)B * r.nwork;
    } else if (r.shared) {
        form = "head+pair_sbs";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel_sbs<%d,%d,%d,%s,false>", D, p->sh_ng, ds, grad ? "true" : "false");
        wgs = (long)B * p->wl_sh[r.sh_list].nwork;
    } else if (r.sb) {
        form = "head+pair_sb";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel_sb<%d,%d,%d,%s,false,%d>", D, r.tb, ds, grad ? "true" : "false", r.colunroll == 4 ? 4 : 1);
        wgs = (long)((B + r.tb - 1) / r.tb) * r.nwork;
    } else {
        form = "head+pair_staged";
        snprintf(kern, sizeof(kern), "gpmpc_pair_kernel<%d,true,%s,%d>", D, grad ? "true" : "false", r.tb);
        wgs = (long)((B + r.tb - 1) / r.tb) * r.nwork;
    }
    const int tl = r.shared && r.fused != 2 ? (r.sh_list == 0 ? 0 : (r.sh_list == 1 ? 2 : 4)) : r.tiling;
    // (step1=quad: what gpmpc_rollout launches at horizon step 1 for this shape; the other entry points keep the FIRST variant)
    snprintf(out, out_bytes, "form=%s kernel=%s tiling=%dx%d workgroups=%ld launches_per_step=%d split=%d tb=%d shared=%d hchunks=%d workspace=%zu%s%s",
             form, kern, cfg[tl][0], cfg[tl][1], wgs, r.fused == 3 ? 0 : (r.fused ? 1 : 2), S, r.tb, r.shared, r.hchunks, gpmpc_layout_for(p, r, B, H, grad).total,
             p->nominal ? " nominal=1" : "", gpmpc_step1_quad_plan(p, r, B, lowprec) ? " step1=quad" : "");
    return GPMPC_OK;
}

bool gpmpc_same_shape(const RollShape& a, const RollShape& b) {
    if (a.fused == 3 && b.fused == 3) return a.pwaves == b.pwaves && a.png == b.png;      // the whole-horizon kernel has no tiling
    return a.tiling == b.tiling && a.tb == b.tb && a.sb == b.sb && a.fused == b.fused && a.fq == b.fq && a.shared == b.shared &&
           a.sh_list == b.sh_list && a.fng == b.fng && a.colunroll == b.colunroll && a.hchunks == b.hchunks && a.pwaves == b.pwaves &&
           a.rgroup == b.rgroup && a.nwork == b.nwork && a.xcdmap == b.xcdmap;
}
