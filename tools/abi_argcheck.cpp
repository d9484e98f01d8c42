// CPU sanitizer driver for the HOST side of libgpmpc_hip.so (tools/run_sanitizers.sh): every entry point of include/gpmpc.h
// is called with invalid arguments -- NULL pointers, dimensions out of range, a pack that was never built -- and must come
// back with a negative GPMPC_E_* code without touching memory it does not own.  Built against the host-only
// AddressSanitizer + UBSan build of the library (make -C gaussian_process_mpc_amd/csrc asan-host).  Runs without a GPU:
// anything that would need one returns GPMPC_E_LAUNCH / GPMPC_E_ALLOC from the failing HIP call instead.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/gpmpc.h"

static int failures = 0;
#define EXPECT_NEG(call) do { long long rc_ = (long long)(call); if (rc_ >= 0) { printf("FAIL %s -> %lld (expected a negative code)\n", #call, rc_); ++failures; } } while (0)
#define EXPECT_ZERO(call) do { long long rc_ = (long long)(call); if (rc_ != 0) { printf("FAIL %s -> %lld (expected 0)\n", #call, rc_); ++failures; } } while (0)

int main() {
    printf("%s; devices visible: %d\n", gpmpc_version(), gpmpc_device_count());
    gpmpc_pack* pk = nullptr;
    double dummy[64] = {0};
    gpmpc_cost_params cp;
    memset(&cp, 0, sizeof(cp));
    EXPECT_NEG(gpmpc_pack_create(nullptr, 10, 2, 1));
    EXPECT_NEG(gpmpc_pack_create(&pk, 0, 2, 1));
    EXPECT_NEG(gpmpc_pack_create(&pk, 10, 0, 1));
    EXPECT_NEG(gpmpc_pack_create(&pk, 10, GPMPC_MAX_DS + 1, 1));
    EXPECT_NEG(gpmpc_pack_create(&pk, 10, 4, GPMPC_MAX_D));
    EXPECT_NEG(gpmpc_pack_create(&pk, 10, 2, -1));
    EXPECT_ZERO(gpmpc_pack_destroy(nullptr));
    EXPECT_NEG(gpmpc_pack_reload_tuning(nullptr));
    EXPECT_NEG(gpmpc_pack_resize(nullptr, 10));
    EXPECT_ZERO(gpmpc_pack_graph_captures(nullptr));
    EXPECT_NEG(gpmpc_pack_build(nullptr, dummy, dummy, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_pack_build_beta(nullptr, dummy, dummy, nullptr, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_pack_enable_fullcov(nullptr, nullptr));
    EXPECT_NEG(gpmpc_pack_dims(nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT_NEG(gpmpc_pack_shared_lambda(nullptr));
    EXPECT_NEG(gpmpc_pack_export(nullptr, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_build_ky(0, 3, dummy, dummy, 1.0, 0.0, nullptr, dummy, nullptr));
    EXPECT_NEG(gpmpc_build_ky(8, GPMPC_MAX_D + 1, dummy, dummy, 1.0, 0.0, nullptr, dummy, nullptr));
    EXPECT_NEG(gpmpc_build_ky(8, 3, nullptr, dummy, 1.0, 0.0, nullptr, dummy, nullptr));
    EXPECT_NEG(gpmpc_build_ky(8, 3, dummy, dummy, 1.0, 0.0, nullptr, nullptr, nullptr));
    EXPECT_ZERO(gpmpc_moment_match_workspace_bytes(nullptr, 4));
    EXPECT_NEG(gpmpc_moment_match(nullptr, 1, dummy, dummy, 0, dummy, dummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_cost(0, 3, 2, 1, &cp, dummy, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_cost(1, 0, 2, 1, &cp, dummy, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_cost(1, 3, GPMPC_MAX_DS + 1, 1, &cp, dummy, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_cost(1, 3, 2, 1, nullptr, dummy, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_cost(1, 3, 2, 1, &cp, nullptr, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_cost_grad(1, 3, 2, 1, &cp, dummy, dummy, dummy, dummy, dummy, nullptr, nullptr, nullptr));      // 1 of 3 derivative outputs
    EXPECT_ZERO(gpmpc_rollout_workspace_bytes(nullptr, 1, 3, 0));
    EXPECT_NEG(gpmpc_rollout(nullptr, 1, 3, dummy, dummy, &cp, 0, nullptr, nullptr, dummy, nullptr, dummy, 64, nullptr));
    EXPECT_ZERO(gpmpc_rollout_jac_workspace_bytes(nullptr, 1, 3));
    EXPECT_NEG(gpmpc_rollout_jac(nullptr, 1, 3, dummy, dummy, dummy, dummy, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_rollout_vjp(1, 3, 2, 1, nullptr, dummy, dummy, dummy, nullptr, nullptr));
    EXPECT_NEG(gpmpc_rollout_vjp(1, 3, 2, 1, dummy, dummy, dummy, nullptr, nullptr, nullptr));
    EXPECT_NEG(gpmpc_rollout_vjp(0, 3, 2, 1, dummy, dummy, dummy, dummy, nullptr, nullptr));
    EXPECT_NEG(gpmpc_rollout_vjp(1, 3, GPMPC_MAX_DS + 1, 1, dummy, dummy, dummy, dummy, nullptr, nullptr));
    EXPECT_NEG(gpmpc_rollout_vjp(1, 3, 2, 0, dummy, dummy, dummy, dummy, nullptr, nullptr));
    EXPECT_ZERO(gpmpc_rollout_fullcov_workspace_bytes(nullptr, 1, 3, 0));
    EXPECT_NEG(gpmpc_rollout_fullcov(nullptr, 1, 3, dummy, dummy, &cp, 0, dummy, dummy, dummy, nullptr, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_objective_gradient(nullptr, 3, dummy, dummy, &cp, 1, dummy, nullptr));
    // round-4 entry points
    char text[256];
    EXPECT_NEG(gpmpc_plan_describe(nullptr, 1, 3, 0, text, sizeof(text)));
    EXPECT_NEG(gpmpc_rollout_fullcov_describe(nullptr, 1, 3, 0, text, sizeof(text)));
    EXPECT_NEG(gpmpc_pack_autotune(nullptr, 1, 3, 0, text, sizeof(text)));
    EXPECT_NEG(gpmpc_pack_autotune_clear(nullptr));
    EXPECT_NEG(gpmpc_pack_build_strided(nullptr, dummy, dummy, dummy, 8, 64, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_store_host(nullptr, dummy, 8, nullptr));
    EXPECT_NEG(gpmpc_store_host(dummy, nullptr, 8, nullptr));
    EXPECT_ZERO(gpmpc_gp_append_workspace_bytes(0, 3));
    EXPECT_NEG(gpmpc_gp_append(0, 3, dummy, dummy, dummy, 1.0, 0.0, dummy, dummy, 8, dummy, 8, dummy, dummy, dummy, 8, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_gp_append(4, GPMPC_MAX_D + 1, dummy, dummy, dummy, 1.0, 0.0, dummy, dummy, 8, dummy, 8, dummy, dummy, dummy, 8, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_gp_append(4, 3, nullptr, dummy, dummy, 1.0, 0.0, dummy, dummy, 8, dummy, 8, dummy, dummy, dummy, 8, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_gp_append(4, 3, dummy, dummy, dummy, 1.0, 0.0, dummy, dummy, 2, dummy, 8, dummy, dummy, dummy, 8, dummy, 64, nullptr));     // leading dimension < n
    // fixed-size window: removal and replacement of one training point
    EXPECT_ZERO(gpmpc_pack_callback_captures(nullptr));
    EXPECT_NEG(gpmpc_kinv_remove(1, dummy, 8, 0, dummy + 32, 8, nullptr));                  // n < 2
    EXPECT_NEG(gpmpc_kinv_remove(4, nullptr, 8, 0, dummy, 8, nullptr));
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 8, 0, nullptr, 8, nullptr));
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 8, -1, dummy + 32, 8, nullptr));                 // index out of range
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 8, 4, dummy + 32, 8, nullptr));
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 8, 0, dummy, 8, nullptr));                       // output aliases the input
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 3, 0, dummy + 32, 8, nullptr));                  // leading dimensions
    EXPECT_NEG(gpmpc_kinv_remove(4, dummy, 8, 0, dummy + 32, 2, nullptr));
    EXPECT_ZERO(gpmpc_gp_replace_workspace_bytes(0, 3));
    {
        double in[3][64] = {{0}}, out[3][64] = {{0}}, ws[32];
        EXPECT_NEG(gpmpc_gp_replace(0, 3, 0, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, GPMPC_MAX_D + 1, 0, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, 3, -1, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 4, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 1, nullptr, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 1, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], in[2], 8, ws, sizeof(ws), nullptr));   // aliasing
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 1, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 2, in[2], 8, out[0], out[1], out[2], 8, ws, sizeof(ws), nullptr));  // leading dimension < n
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 1, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 3, ws, sizeof(ws), nullptr));
        EXPECT_NEG(gpmpc_gp_replace(4, 3, 1, dummy, dummy, dummy, 1.0, 0.0, in[0], in[1], 8, in[2], 8, out[0], out[1], out[2], 8, ws, 16, nullptr));          // workspace too small
    }
    EXPECT_ZERO(gpmpc_timing_enable(0));
    {   // launch geometry, host-side views (round 5): valid calls exercise the host code under the sanitizers, invalid ones return error codes
        int n_items = -1, traj = -1, col = -1;
        EXPECT_ZERO(gpmpc_debug_run_list(4096, 6, 1012, nullptr, 0, &n_items));
        if (n_items > 0) {
            int* items = (int*)malloc(sizeof(int) * 4 * (size_t)n_items);
            EXPECT_ZERO(gpmpc_debug_run_list(4096, 6, 1012, items, n_items, &n_items));
            free(items);
        }
        EXPECT_ZERO(gpmpc_debug_run_list(320, 4, 1016, nullptr, 0, &n_items));
        EXPECT_NEG(gpmpc_debug_run_list(100, 4, 1016, nullptr, 0, &n_items));
        EXPECT_NEG(gpmpc_debug_run_list(4096, 0, 1012, nullptr, 0, &n_items));
        EXPECT_NEG(gpmpc_debug_run_list(4096, 6, 1012, nullptr, 0, nullptr));
        // the tile lists and one-lambda tables of a pack (csrc/worklist.h): a re-ordered list whose XCD queues run dry, a ragged one with tile slots
        for (int slot = 0; slot < 2; ++slot) {
            const int np = slot ? 320 : 1024, units = slot ? 2 : 4, jt = slot ? 128 : 256;
            EXPECT_ZERO(gpmpc_debug_work_list(np, 256, jt, units, 0, 1, slot, nullptr, 0, &n_items, nullptr, nullptr));
            std::vector<int> items(4 * (size_t)n_items), perm(n_items, -1), ust(units + 1);
            EXPECT_ZERO(gpmpc_debug_work_list(np, 256, jt, units, 0, 1, slot, items.data(), n_items, &n_items, perm.data(), ust.data()));
            if (ust[units] != n_items) { printf("FAIL gpmpc_debug_work_list: ustart ends at %d of %d items\n", ust[units], n_items); ++failures; }
        }
        {
            int ntile[3], n_tiles = -1;
            EXPECT_ZERO(gpmpc_debug_fcs_tables(320, 3, 64, ntile, nullptr, 0, &n_tiles, nullptr));
            std::vector<int> tiles(3 * (size_t)n_tiles), ust(3 * (3 + 3 + 1));
            EXPECT_ZERO(gpmpc_debug_fcs_tables(320, 3, 64, ntile, tiles.data(), n_tiles, &n_tiles, ust.data()));
            EXPECT_NEG(gpmpc_debug_fcs_tables(320, 3, 64, ntile, tiles.data(), n_tiles - 1, &n_tiles, ust.data()));
            EXPECT_NEG(gpmpc_debug_fcs_tables(320, 5, 64, ntile, nullptr, 0, &n_tiles, nullptr));
            EXPECT_NEG(gpmpc_debug_fcs_tables(320, 3, 64, nullptr, nullptr, 0, &n_tiles, nullptr));
        }
        EXPECT_NEG(gpmpc_debug_work_list(100, 256, 64, 2, 0, 1, 0, nullptr, 0, &n_items, nullptr, nullptr));
        EXPECT_NEG(gpmpc_debug_work_list(128, 256, 64, 0, 0, 1, 0, nullptr, 0, &n_items, nullptr, nullptr));
        EXPECT_NEG(gpmpc_debug_work_list(128, 256, 64, GPMPC_MAX_DS + 1, 0, 1, 0, nullptr, 0, &n_items, nullptr, nullptr));
        EXPECT_NEG(gpmpc_debug_work_list(128, 256, 64, 2, 0, 1, 0, nullptr, 0, nullptr, nullptr, nullptr));
        EXPECT_NEG(gpmpc_debug_work_list(128, 256, 64, 2, 0, 1, 0, &traj, 1, &n_items, &traj, nullptr));
        for (int L = 0; L < (24 + 8) * 5; ++L) EXPECT_ZERO(gpmpc_debug_xcd_order(L, 24 + 8, 24, 5, &traj, &col));
        EXPECT_NEG(gpmpc_debug_xcd_order(-1, 32, 24, 5, &traj, &col));
        EXPECT_NEG(gpmpc_debug_xcd_order(0, 32, 33, 5, &traj, &col));
        EXPECT_NEG(gpmpc_debug_xcd_order(0, 32, 24, 5, nullptr, &col));
    }
    double ms = 0; long long nl = 0;
    EXPECT_ZERO(gpmpc_pair_kernel_time(&ms, &nl, 1));
    EXPECT_NEG(gpmpc_pair_kernel_time_class(-1, &ms, &nl));
    EXPECT_NEG(gpmpc_pair_kernel_time_class(99, &ms, &nl));
    EXPECT_ZERO(gpmpc_pair_kernel_time_class(2, &ms, &nl));
    EXPECT_NEG(gpmpc_matvec(0, 4, dummy, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_matvec(4, 4, nullptr, dummy, dummy, nullptr));
    EXPECT_NEG(gpmpc_predict(0, 3, dummy, dummy, 1.0, dummy, dummy, 0.0, 1, dummy, dummy, dummy, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_predict(4, GPMPC_MAX_D + 1, dummy, dummy, 1.0, dummy, dummy, 0.0, 1, dummy, dummy, dummy, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_predict(4, 3, nullptr, dummy, 1.0, dummy, dummy, 0.0, 1, dummy, dummy, dummy, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_kinv_append(0, dummy, dummy, 1.0, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_kinv_append(4, nullptr, dummy, 1.0, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_ml_grad(0, 3, dummy, dummy, dummy, dummy, dummy, 1.0, 0.0, dummy, dummy, 64, nullptr));
    EXPECT_NEG(gpmpc_ml_grad(4, 3, nullptr, dummy, dummy, dummy, dummy, 1.0, 0.0, dummy, dummy, 64, nullptr));
    {   // the three MPPI solves share one search and their parameter checks (csrc/mppi_internal.h): calls with TWO faults walk the refusal
        // paths, and the earlier check's text must be the one reported.  Nothing is dereferenced: every call is refused on the host.
        gpmpc_gp_model gm;
        memset(&gm, 0, sizeof(gm));
        gm.n = 4; gm.state_dim = 2; gm.action_dim = 1; gm.ld = 4;
        gm.X = gm.beta = gm.Kinv = dummy;
        for (int k = 0; k < GPMPC_MAX_DS * GPMPC_MAX_D; ++k) gm.lambdas[k] = 1.0;
        for (int k = 0; k < GPMPC_MAX_DS; ++k) gm.sigma_f[k] = 1.0;
        gpmpc_mppi_params mp;
        memset(&mp, 0, sizeof(mp));
        mp.n_samples = 8; mp.iterations = 2; mp.sigma_decay = 0.9; mp.beta = 0.1;
        mp.sigma[0] = 0.5; mp.lb[0] = -1.0; mp.ub[0] = 1.0;
        gpmpc_state_constraints sc;
        memset(&sc, 0, sizeof(sc));
        sc.n_rows = 1;
        const gpmpc_pack* fake = (const gpmpc_pack*)dummy;     // (never looked at: the scalar checks come first)
        auto text = [&](const char* want) {
            if (strcmp(gpmpc_last_error(), want)) { printf("FAIL refusal text: \"%s\" (expected \"%s\")\n", gpmpc_last_error(), want); ++failures; }
        };
        gpmpc_mppi_params bad = mp;
        gpmpc_state_constraints rows0 = sc;
        rows0.n_rows = 0;
        bad.sigma_decay = 0.0;                                  // sigma_decay + constraint rows: the scalar first, in all three
        EXPECT_NEG(gpmpc_mppi_solve(fake, 3, dummy, dummy, &cp, &rows0, &bad, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve: sigma_decay = 0 is not positive");
        EXPECT_NEG(gpmpc_mppi_solve_linearised(&gm, 3, dummy, dummy, &cp, &rows0, &bad, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_linearised: sigma_decay = 0 is not positive");
        EXPECT_NEG(gpmpc_mppi_solve_particles(&gm, 3, 16, dummy, dummy, &cp, &rows0, &bad, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_particles: sigma_decay = 0 is not positive");
        gpmpc_gp_model lam = gm;
        lam.lambdas[1] = 0.0;                                   // constraint rows + lambdas: the rows first in the linearised solve, the model in the particle one
        EXPECT_NEG(gpmpc_mppi_solve_linearised(&lam, 3, dummy, dummy, &cp, &rows0, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_linearised: n_rows = 0 outside 1..16");
        EXPECT_NEG(gpmpc_mppi_solve_particles(&lam, 3, 16, dummy, dummy, &cp, &rows0, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_particles: lambdas[0][1] = 0 is not positive and finite");
        bad = mp;
        bad.sigma[0] = 0.0;                                     // sigma + a horizon too long for the cost kernel / too many particles
        EXPECT_NEG(gpmpc_mppi_solve_linearised(&gm, 2000, dummy, dummy, &cp, &sc, &bad, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_linearised: sigma[0] = 0 is not positive");
        EXPECT_NEG(gpmpc_mppi_solve_particles(&gm, 3, GPMPC_PARTICLE_COST_MAX_P + 1, dummy, dummy, &cp, &sc, &bad, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_particles: sigma[0] = 0 is not positive");
        gpmpc_cost_params sched = cp;
        sched.schedule_id = 12345;                              // the horizon + an unknown cost schedule
        EXPECT_NEG(gpmpc_mppi_solve_linearised(&gm, 2000, dummy, dummy, &sched, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_linearised: H = 2000 is too long for the cost kernel");
        EXPECT_NEG(gpmpc_mppi_solve_particles(&gm, 3, 16, dummy, dummy, &sched, &rows0, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        text("gpmpc_mppi_solve_particles: n_rows = 0 outside 1..16");
        // fault-free up to the workspace: the whole entry preamble and the layouts run
        EXPECT_NEG(gpmpc_mppi_solve_linearised(&gm, 3, dummy, dummy, &cp, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        EXPECT_NEG(gpmpc_mppi_solve_particles(&gm, 3, 16, dummy, dummy, &cp, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        EXPECT_NEG(gpmpc_mppi_solve_linearised(nullptr, 3, dummy, dummy, &cp, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        EXPECT_NEG(gpmpc_mppi_solve_particles(nullptr, 3, 16, dummy, dummy, &cp, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
        EXPECT_NEG(gpmpc_mppi_solve(nullptr, 3, dummy, dummy, &cp, &sc, &mp, dummy, dummy, dummy, dummy, 64, nullptr));
    }
    // a pack cannot be created without a device: the failing HIP call must surface as a code, with its text recorded
    int rc = gpmpc_pack_create(&pk, 32, 2, 1);
    if (rc == GPMPC_OK) {                       // (a GPU is present after all: exercise the "not built" state and clean up)
        std::vector<double> ws(1 << 16);
        EXPECT_NEG(gpmpc_rollout(pk, 1, 3, dummy, dummy, &cp, 0, nullptr, nullptr, dummy, nullptr, ws.data(), ws.size() * 8, nullptr));
        EXPECT_NEG(gpmpc_pack_shared_lambda(pk));
        EXPECT_ZERO(gpmpc_pack_destroy(pk));
    } else if (rc >= 0) { printf("FAIL gpmpc_pack_create -> %d\n", rc); ++failures; }
    else printf("gpmpc_pack_create without a device: %d (%s)\n", rc, gpmpc_last_error());
    printf(failures ? "abi_argcheck: %d FAILURES\n" : "abi_argcheck: all argument checks returned error codes (%d failures)\n", failures);
    return failures ? 1 : 0;
}
