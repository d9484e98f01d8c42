// Plan selection that measures: time the candidate plans of ONE call shape on this device and keep the winner in the pack's tuned
// table (plan.h), where gpmpc_choose_shape finds it.
#include "rollout.h"
#include <cstdlib>

extern "C" int gpmpc_pack_autotune(gpmpc_pack* p, int B, int H, unsigned flags, char* report, size_t report_bytes) {
    if (!p || B < 1 || H < 1) return GPMPC_E_ARG;
    if (!p->built) return GPMPC_E_STATE;
    if (int rc_dev = gpmpc_check_device(p)) return rc_dev;
    PackGuard lock(p);
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0, use_graph = (flags & GPMPC_USE_GRAPH) != 0;
    gpmpc_tuned_table* tab = (gpmpc_tuned_table*)p->tuned;
    if (!tab) { tab = (gpmpc_tuned_table*)calloc(1, sizeof(gpmpc_tuned_table)); if (!tab) return GPMPC_E_ALLOC; p->tuned = tab; }
    for (int k = 0; k < GPMPC_TUNED_SLOTS; ++k)                   // re-tuning a shape replaces its entry
        if (tab->e[k].valid && tab->e[k].B == B && tab->e[k].H == H && tab->e[k].grad == (grad ? 1 : 0) &&
            tab->e[k].graph == (use_graph ? 1 : 0))
            tab->e[k].valid = 0;
    // ---- candidates: the default plan, then the plans the GPMPC_* overrides would force, de-duplicated -------------------------
    struct Cand { RollShape r; int S; double ms; const char* why; };
    Cand cand[48]; int nc = 0;
    auto add = [&](const gpmpc_tuning& tn, int split, const char* why) {
        if (nc >= 48) return;
        const RollShape r = gpmpc_choose_shape(p, B, H, grad, false, &tn);
        int S = gpmpc_split_count(p, r, B, false, !use_graph, split);
        if (S > 1 && r.fused == 3) S = 1;
        for (int k = 0; k < nc; ++k) if (gpmpc_same_shape(cand[k].r, r) && cand[k].S == S) return;
        cand[nc].r = r; cand[nc].S = S; cand[nc].ms = 0.0; cand[nc].why = why; ++nc;
    };
    const gpmpc_tuning base = p->tune;
    add(base, 0, "default");
    { gpmpc_tuning t = base; t.fused_sb = 0; add(t, 0, "fused_sb=0"); }
    { gpmpc_tuning t = base; t.fused_sb = 1; add(t, 0, "fused_sb=1"); }
    for (int tl : {0, 2, 4, 5, 6}) {
        gpmpc_tuning t = base; t.tiling = tl; add(t, 0, "tiling");
        t.fused_sb = 1; add(t, 0, "tiling+fused_sb=1");
        t.fused_sb = 0; add(t, 0, "tiling+fused_sb=0");
    }
    for (int xm : {0, 1}) {                                      // (the one-launch forms with the other dispatch order)
        gpmpc_tuning t = base; t.xcdmap = xm; t.persist = 0; add(t, 0, xm ? "xcdmap=1" : "xcdmap=0");
        for (int tl : {2, 5, 6}) { gpmpc_tuning u = t; u.tiling = tl; u.fused_sb = 1; add(u, 0, xm ? "tiling+xcdmap=1" : "tiling+xcdmap=0"); }
    }
    { gpmpc_tuning t = base; t.persist = 16; add(t, 0, "persist=16"); t.persist = 8; add(t, 0, "persist=8"); t.persist = 0; add(t, 0, "persist=0"); }
    { gpmpc_tuning t = base; t.pair_sb = 0; t.persist = 0; add(t, 0, "pair_sb=0"); t.fused = 0; add(t, 0, "pair_sb=0,fused=0"); }
    { gpmpc_tuning t = base; t.fused = 0; t.persist = 0; add(t, 0, "fused=0"); }
    if (p->shared_lambda) { gpmpc_tuning t = base; t.shared = 0; t.persist = 0; add(t, 0, "shared=0"); }
    for (int sp : {1, 2, 4}) { gpmpc_tuning t = base; t.persist = 0; add(t, sp, "split"); }
    // ---- scratch: inputs (zeros: a valid problem), outputs, the largest workspace --------------------------------------------
    size_t wsb = 0;
    for (int k = 0; k < nc; ++k) {
        size_t need = gpmpc_layout_for(p, cand[k].r, B, H, grad).total;
        if (cand[k].S > 1) { const size_t sb = gpmpc_split_bytes(p, cand[k].r, B, H, grad, cand[k].S); if (sb > need) need = sb; }
        if (need > wsb) wsb = need;
    }
    const size_t nU = (size_t)B * H * p->da, nx = (size_t)B * p->ds;
    double *x0 = nullptr, *U = nullptr, *oc = nullptr, *og = nullptr; void* ws = nullptr;
    hipError_t e = hipMalloc((void**)&x0, sizeof(double) * nx);
    if (e == hipSuccess) e = hipMalloc((void**)&U, sizeof(double) * (nU ? nU : 1));
    if (e == hipSuccess) e = hipMalloc((void**)&oc, sizeof(double) * B);
    if (e == hipSuccess) e = hipMalloc((void**)&og, sizeof(double) * (nU ? nU : 1));
    if (e == hipSuccess) e = hipMalloc(&ws, wsb);
    hipStream_t st = nullptr; hipEvent_t ea = nullptr, eb = nullptr;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ea);
    if (e == hipSuccess) e = hipEventCreate(&eb);
    if (e == hipSuccess) e = hipMemsetAsync(x0, 0, sizeof(double) * nx, st);
    if (e == hipSuccess) e = hipMemsetAsync(U, 0, sizeof(double) * (nU ? nU : 1), st);
    gpmpc_graph_cache* gc = nullptr;
    int rc = e == hipSuccess ? gpmpc_ensure_graph_cache(p, &gc) : GPMPC_E_ALLOC;
    gpmpc_cost_params cost;
    memset(&cost, 0, sizeof(cost));
    cost.gamma = 0.0;
    for (int k = 0; k < p->ds; ++k) cost.Q[k * p->ds + k] = 1.0;
    for (int k = 0; k < p->da; ++k) cost.R[k * p->da + k] = 0.01;
    const unsigned fl = grad ? GPMPC_WANT_GRAD : 0;
    hipGraphExec_t execs[48] = {};
    const bool trace = getenv("GPMPC_AUTOTUNE_TRACE") != nullptr;      // diagnostic: names every candidate on stderr before it runs
    const bool was_timing = gpmpc_timing_on();
    if (was_timing) gpmpc_timing_enable(0);                   // per-kernel events cannot be recorded inside the captures below
    // ---- time every candidate: one captured graph (or the plain launches), one warm-up, then replays for >= ~2 ms or 3 times ----
    for (int pass = 0; pass < 2; ++pass)                          // two passes, the better time of each candidate: the first launches of a
    for (int kk = 0; kk <= nc && rc == GPMPC_OK; ++kk) {          // process (code upload, cold caches) must not be charged to the default plan
        // (the default plan is timed AGAIN at the end of each pass: measured first only, it came out 4 ... 8 % behind candidates that
        // launch exactly the same kernels -- profiles/r05/autotune_grid_mid.txt, N = 2048, B = 6 / 8 --, whatever the position effect is)
        const int k = kk == nc ? 0 : kk;
        if ((pass == 1 || kk == nc) && cand[k].ms < 0.0) continue;              // failed to enqueue before
        const Cand& c = cand[k];
        if (trace)
            fprintf(stderr, "[autotune] pass %d candidate %d (%s): fused=%d tiling=%d sb=%d tb=%d shared=%d pwaves=%d colunroll=%d split=%d\n",
                    pass, k, c.why, c.r.fused, c.r.tiling, c.r.sb, c.r.tb, c.r.shared, c.r.pwaves, c.r.colunroll, c.S);
        const RollCall call{p, B, H, x0, U, &cost, fl, nullptr, nullptr, oc, og, ws, wsb, st, nullptr, false, &c.r};
        auto enqueue = [&] { return c.S <= 1 ? gpmpc_enqueue_rollout(call) : gpmpc_enqueue_split(gc, c.S, c.r, call); };
        // One captured graph per candidate, kept for both passes and destroyed together after the last replay: capturing, instantiating
        // and destroying ~25 graphs (some with two or four parallel branches) back to back crashed intermittently inside
        // hipGraphLaunch (native backtrace: the replay of the re-captured default plan in pass 1; 1 run in ~10, round 4).
        hipGraphExec_t& exec = execs[k];
        if (use_graph && !exec) {
            // (every candidate also runs once as plain launches before it is captured: warm caches, and nothing is launched for the
            // first time in the process inside a capture)
            if (pass == 0) {
                if (enqueue() != GPMPC_OK || hipStreamSynchronize(st) != hipSuccess) { cand[k].ms = -1.0; continue; }
            }
            if (gpmpc_capture(st, enqueue, &exec) != GPMPC_OK) { cand[k].ms = -1.0; continue; }      // this candidate is out, the others go on
        }
        auto run = [&]() { return use_graph ? (hipGraphLaunch(exec, st) == hipSuccess ? GPMPC_OK : GPMPC_E_LAUNCH) : enqueue(); };
        int r2 = run();
        if (r2 == GPMPC_OK && hipStreamSynchronize(st) != hipSuccess) r2 = GPMPC_E_LAUNCH;
        double best = -1.0;
        for (int rep = 0; rep < 3 && r2 == GPMPC_OK; ++rep) {     // best of three blocks
            int n = 1;
            (void)hipEventRecord(ea, st);
            r2 = run();
            (void)hipEventRecord(eb, st);
            if (hipEventSynchronize(eb) != hipSuccess) { r2 = GPMPC_E_LAUNCH; break; }
            float ms1 = 0.f; (void)hipEventElapsedTime(&ms1, ea, eb);
            if (ms1 < 0.7f) {                                     // short call: a block of replays instead of one
                n = ms1 > 0.f ? (int)(2.0f / ms1) + 1 : 20; if (n > 200) n = 200;
                (void)hipEventRecord(ea, st);
                for (int q = 0; q < n && r2 == GPMPC_OK; ++q) r2 = run();
                (void)hipEventRecord(eb, st);
                if (hipEventSynchronize(eb) != hipSuccess) { r2 = GPMPC_E_LAUNCH; break; }
                (void)hipEventElapsedTime(&ms1, ea, eb);
            }
            const double per = (double)ms1 / n;
            if (best < 0.0 || per < best) best = per;
        }
        if (r2 != GPMPC_OK) cand[k].ms = -1.0;
        else if ((pass == 0 && kk < nc) || best < cand[k].ms) cand[k].ms = best;
    }
    (void)hipStreamSynchronize(st);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < nc; ++k) if (execs[k]) (void)hipGraphExecDestroy(execs[k]);
    if (was_timing) gpmpc_timing_enable(1);
    int win = -1;
    for (int k = 0; k < nc; ++k) if (cand[k].ms > 0.0 && (win < 0 || cand[k].ms < cand[win].ms)) win = k;
    // the default keeps its place unless a candidate beats it by more than the noise of this measurement (2 %)
    if (win > 0 && cand[0].ms > 0.0 && cand[win].ms > 0.98 * cand[0].ms) win = 0;
    if (rc == GPMPC_OK && win >= 0) {
        gpmpc_tuned_entry& te = tab->e[tab->next % GPMPC_TUNED_SLOTS];
        tab->next = (tab->next + 1) % GPMPC_TUNED_SLOTS;
        te.B = B; te.H = H; te.grad = grad ? 1 : 0; te.graph = use_graph ? 1 : 0; te.S = cand[win].S; te.shape = cand[win].r;
        te.ms_default = cand[0].ms; te.ms_best = cand[win].ms; te.valid = 1;
        gpmpc_graph_cache_invalidate(p->graph_cache);           // captured under the plan the thresholds chose
        gpmpc_cb_cache_invalidate(p->cb_cache);
    }
    if (report && report_bytes > 0) {
        size_t off = 0;
        report[0] = 0;
        for (int k = 0; k < nc && off + 96 < report_bytes; ++k)
            off += snprintf(report + off, report_bytes - off, "%s%s%s:fused=%d,tiling=%d,sb=%d,tb=%d,shared=%d,pwaves=%d,xcdmap=%d,split=%d:%.5f",
                            k ? ";" : "", k == win ? "*" : "", cand[k].why, cand[k].r.fused, cand[k].r.tiling, cand[k].r.sb, cand[k].r.tb,
                            cand[k].r.shared, cand[k].r.pwaves, cand[k].r.xcdmap, cand[k].S, cand[k].ms);
    }
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (st) (void)hipStreamDestroy(st);
    if (x0) (void)hipFree(x0);
    if (U) (void)hipFree(U);
    if (oc) (void)hipFree(oc);
    if (og) (void)hipFree(og);
    if (ws) (void)hipFree(ws);
    if (e != hipSuccess) { gpmpc_set_error("gpmpc_pack_autotune: scratch", e); return GPMPC_E_ALLOC; }
    if (rc != GPMPC_OK) return rc;
    return win < 0 ? GPMPC_E_LAUNCH : nc;
}

extern "C" int gpmpc_pack_autotune_clear(gpmpc_pack* p) {
    if (!p) return GPMPC_E_ARG;
    PackGuard lock(p);
    gpmpc_tuned_clear(p->tuned);
    gpmpc_graph_cache_invalidate(p->graph_cache);
    gpmpc_cb_cache_invalidate(p->cb_cache);
    return GPMPC_OK;
}
