// Work lists of the pair kernels and the tile tables of the one-lambda full-covariance form, as plain host C++: pure functions of the
// padded size and the unit counts, no HIP in here (pack.hip uploads the results in one arena; tools/worklist_check.cpp walks them under
// the host sanitizers; include/gpmpc.h, "launch geometry", shows them to tests).  The ORDER of every list is part of the contract:
// kernels, plans and captured graphs index by it.
#pragma once
#include <algorithm>
#include <array>
#include <vector>

struct gpmpc_tile_list {
    std::vector<int> items;    // [n][4] = {unit, i0, j0, j1 | tile index within its unit}
    std::vector<int> perm;     // [n] item indices grouped by unit: re-ordered (XCD-sorted) lists only, else empty
    std::vector<int> ustart;   // [nunits + 1]: unit u owns items (natural order) / perm entries (re-ordered) [ustart[u], ustart[u + 1])
    int tiles = 0;             // tiles of the last unit (= of every unit of a list without cross units)
    int n() const { return (int)(items.size() / 4); }
};

// Units x row tiles x column tiles; units < ntri keep the tiles that reach the diagonal only (variance units: upper triangle).
// tile_slot: the 4th entry of an item is the tile's index within its unit instead of j1 (the shared-lambda kernel computes j1 from j0
// and writes its partial sums by (GP, tile)).
inline gpmpc_tile_list gpmpc_build_tile_list(int Np, int it, int jt, int ntri, int ncross, bool xcd_sort, bool tile_slot) {
    gpmpc_tile_list w;
    const int ti = (Np + it - 1) / it, tj = (Np + jt - 1) / jt, nunits = ntri + ncross;
    std::vector<int>& h = w.items;
    h.reserve(4 * (size_t)ti * tj * nunits);
    for (int u = 0; u < nunits; ++u) {
        w.ustart.push_back(w.n());
        for (int i0 = 0; i0 < Np; i0 += it)
            for (int j0 = 0; j0 < Np; j0 += jt) {
                const int j1 = std::min(j0 + jt, Np);
                if (u < ntri && j1 <= i0) continue;          // variance unit: tile wholly below the diagonal
                h.insert(h.end(), {u, i0, j0, tile_slot ? w.n() - w.ustart[u] : j1});
            }
        w.tiles = w.n() - w.ustart[u];
    }
    const int n = w.n();
    w.ustart.push_back(n);
    if (xcd_sort && n >= 16) {
        // Re-order so that the list position p (the pair kernel maps p % 8 to an XCD) groups tiles that share a COLUMN
        // range: they read the same G rows and, per unit, the same column block of M.  Odd units use the mirrored
        // column index so that the triangular tile counts (1..T per column block) balance across the 8 XCDs.
        typedef std::array<int, 4> item;
        std::vector<item> q[8];
        for (int k = 0; k < n; ++k) {
            const int u = h[4 * k], tjx = h[4 * k + 2] / jt;
            q[((u & 1) ? (tj - 1 - tjx) : tjx) & 7].push_back({u, h[4 * k + 1], h[4 * k + 2], h[4 * k + 3]});
        }
        // within an XCD: column block major, then row tile (consecutive items share their G rows, see pair_kernel_sb.h)
        for (auto& qx : q)
            std::sort(qx.begin(), qx.end(), [](const item& a, const item& b) {
                return a[0] != b[0] ? a[0] < b[0] : (a[2] != b[2] ? a[2] < b[2] : a[1] < b[1]);
            });
        size_t pos[8] = {0};
        for (int p = 0; p < n; ++p) {
            int x = p & 7;
            if (pos[x] >= q[x].size()) {                     // this XCD's queue ran dry: take from the fullest one
                int best = 0;
                for (int y = 1; y < 8; ++y) if (q[y].size() - pos[y] > q[best].size() - pos[best]) best = y;
                x = best;
            }
            std::copy(q[x][pos[x]].begin(), q[x][pos[x]].end(), &h[4 * (size_t)p]);
            ++pos[x];
        }
        // per-unit index of the re-ordered list (finish_step, roll_dev.h)
        std::vector<int> fill(w.ustart);
        w.perm.resize(n);
        for (int k = 0; k < n; ++k) w.perm[fill[h[4 * (size_t)k]]++] = k;
    }
    return w;
}

// Work list 7, "balanced runs" (round 5): one trajectory of a large training set (the B = 1 solver callbacks) on 256x64 tiles launches
// n equal workgroups on `slots` workgroup slots -- N = 4096, ds = 6: 3264 on 1024, i.e. 3.19 generations of 30 us workgroups, the last one
// a fifth full (30 of 120 us, profiles/r04/fused_stamps_c4_b1.txt), and every workgroup pays a 7 us prologue for 23 us of columns.
// Here every 256-row tile row of every GP is cut into RUNS of up to 256 columns -- the longest run length L for which the whole
// list still fits ONE generation: sum over (GP, tile row) of ceil(span / L) <= slots -- each run its own work item {unit, i0, j0, j1}
// (multiples of 8 columns; step_fused.h, Q = 256, reads a run's length from its item): one generation per trajectory, a third of the
// prologues.  (A first attempt that only split the LAST partial generation into 256x16 tiles was slower: 3.65 -> 4.23 ms,
// profiles/r05/ab15_split_tail.txt.)  An EMPTY list when it is not worth building (the plain list is about one generation already, or more
// than one generation even with the longest runs).
inline gpmpc_tile_list gpmpc_build_run_list(int Np, int ds, int slots) {
    gpmpc_tile_list w;
    const int it = 256;
    int n64 = 0;
    for (int i0 = 0; i0 < Np; i0 += it) n64 += (Np - (i0 / 64) * 64 + 63) / 64;
    n64 *= ds;
    if (slots < 64 || n64 <= slots + slots / 10) return w;
    auto count = [&](int L) { int c = 0; for (int i0 = 0; i0 < Np; i0 += it) { const int span = Np - i0; c += (span + L - 1) / L; } return c * ds; };
    int L = 8;
    while (L < 256 && count(L) > slots) L += 8;
    if (count(L) > slots) return w;
    for (int u = 0; u < ds; ++u) {
        w.ustart.push_back(w.n());
        for (int i0 = 0; i0 < Np; i0 += it) {
            const int span = Np - i0, runs = (span + L - 1) / L;
            int j = i0;
            for (int q = 0; q < runs; ++q) {                            // equal runs, multiples of 8 columns, the remainder spread over the first ones
                int len = ((span / runs) / 8) * 8;
                const int extra = (span - len * runs) / 8;              // runs that take 8 more columns
                if (q < extra) len += 8;
                if (q == runs - 1) len = Np - j;
                w.items.insert(w.items.end(), {u, i0, j, j + len});
                j += len;
            }
        }
    }
    w.ustart.push_back(w.n());
    return w;
}

// One lambda for all GPs, full-covariance rollout (pair_kernel_sbfx.h): the cross units' tiles per trajectory in three widths, and the
// table of the widest.  They depend on the padded size alone.
struct gpmpc_fcs_tiles {
    int ntile[3];                  // [0] 64 x 64 | [1] 64 x 16 tiles of the upper triangle, [2] 64 x (up to) 256 (listed in tiles256)
    std::vector<int> tiles256;     // [ntile[2]][3] = {64-row block, first column, columns}: row block ti's columns from its diagonal block on
                                   // in chunks of 256 (launches that fill the chip: a third of a 64-column wave's time is prologue and row sums)
};
inline gpmpc_fcs_tiles gpmpc_build_fcs_tiles(int Np) {
    gpmpc_fcs_tiles f;
    const int T = Np / 64;
    f.ntile[0] = T * (T + 1) / 2; f.ntile[1] = 4 * f.ntile[0];
    for (int ti = 0; ti < T; ++ti)
        for (int j0 = 64 * ti; j0 < Np; j0 += 256) f.tiles256.insert(f.tiles256.end(), {ti, j0, std::min(Np - j0, 256)});
    f.ntile[2] = (int)(f.tiles256.size() / 3);
    return f;
}
// ... and the unit offsets into a trajectory's partial-sum slots for one tiling of the variance units (ustart of that full-covariance work
// list) and one width: the variance units as in the work list, cross unit pr at ustart[ds] + pr * ntile.  [ds + npairs + 1]; the last
// entry is the slot count.
inline std::vector<int> gpmpc_fcs_ustart(const std::vector<int>& ustart, int ds, int npairs, int ntile) {
    std::vector<int> u(ustart.begin(), ustart.begin() + ds + 1);
    for (int pr = 1; pr <= npairs; ++pr) u.push_back(ustart[ds] + pr * ntile);
    return u;
}
