// Stand-alone walk over csrc/worklist.h (pure host code: no HIP, no library) for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/worklist_check.cpp -o worklist_check && ./worklist_check
// Every list of the grid of tests/test_host_cpu.py, the one-lambda tables and the balanced-run lists are built and read back once; the
// structural invariants are checked on the way (the item-for-item order is held by the digests of that test).  Exit status 1 on a violation.
#include <cstdio>
#include <set>
#include <tuple>
#include "../gaussian_process_mpc_amd/csrc/worklist.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); ++failures; } } while (0)

int main() {
    const int nps[] = {64, 128, 192, 320, 1024, 2048};
    const int tilings[][3] = {{256, 256, 0}, {64, 64, 0}, {256, 64, 0}, {64, 128, 0}, {256, 128, 0}, {256, 32, 0}, {256, 16, 0}, {256, 64, 1}, {256, 128, 1}, {256, 256, 1}};
    const int units[][2] = {{1, 0}, {2, 0}, {2, 1}, {4, 0}, {4, 6}, {6, 0}};
    long lists = 0, items = 0;
    for (int Np : nps)
        for (const auto& tl : tilings)
            for (const auto& un : units)
                for (int sort = 0; sort < 2; ++sort) {
                    const int it = tl[0], jt = tl[1], nu = un[0] + un[1];
                    const gpmpc_tile_list w = gpmpc_build_tile_list(Np, it, jt, un[0], un[1], sort != 0, tl[2] != 0);
                    const int n = w.n();
                    ++lists; items += n;
                    CHECK((int)w.ustart.size() == nu + 1 && w.ustart[0] == 0 && w.ustart[nu] == n, "Np %d %dx%d units %d+%d", Np, it, jt, un[0], un[1]);
                    CHECK(w.perm.empty() == !(sort && n >= 16), "Np %d %dx%d: perm of %zu for %d items", Np, it, jt, w.perm.size(), n);
                    std::set<std::tuple<int, int, int>> seen;
                    std::vector<int> count(nu, 0);
                    for (int k = 0; k < n; ++k) {
                        const int* t = &w.items[4 * (size_t)k];
                        CHECK(t[0] >= 0 && t[0] < nu && t[1] % it == 0 && t[1] < Np && t[2] % jt == 0 && t[2] < Np, "item %d", k);
                        const int j1 = t[2] + jt < Np ? t[2] + jt : Np;
                        CHECK(t[0] >= un[0] || j1 > t[1], "item %d of a variance unit lies below the diagonal", k);
                        CHECK(tl[2] ? (t[3] >= 0 && t[3] < w.ustart[t[0] + 1] - w.ustart[t[0]]) : t[3] == j1, "item %d: 4th entry %d", k, t[3]);
                        CHECK(seen.insert({t[0], t[1], t[2]}).second, "item %d twice", k);
                        ++count[t[0]];
                    }
                    for (int u = 0; u < nu; ++u) {
                        CHECK(count[u] == w.ustart[u + 1] - w.ustart[u], "unit %d: %d items", u, count[u]);
                        for (int q = w.ustart[u]; q < w.ustart[u + 1] && !w.perm.empty(); ++q)
                            CHECK(w.perm[q] >= 0 && w.perm[q] < n && w.items[4 * (size_t)w.perm[q]] == u, "perm[%d]", q);
                    }
                }
    for (int Np : nps) {
        const gpmpc_fcs_tiles f = gpmpc_build_fcs_tiles(Np);
        CHECK(f.ntile[2] * 3 == (int)f.tiles256.size() && f.ntile[1] == 4 * f.ntile[0], "Np %d", Np);
        for (int ds = 2; ds <= 4; ++ds)
            for (int jt : {256, 64, 128}) {
                const int npairs = ds * (ds - 1) / 2;
                const gpmpc_tile_list w = gpmpc_build_tile_list(Np, 256, jt, ds, npairs, false, false);
                for (int q = 0; q < 3; ++q) {
                    const std::vector<int> u = gpmpc_fcs_ustart(w.ustart, ds, npairs, f.ntile[q]);
                    CHECK((int)u.size() == ds + npairs + 1 && u.back() == w.ustart[ds] + npairs * f.ntile[q], "Np %d ds %d", Np, ds);
                }
            }
    }
    const int runs[][3] = {{4096, 6, 1012}, {2560, 6, 1012}, {3072, 5, 1014}, {2752, 5, 1014}, {4096, 7, 1010}, {4032, 6, 1012}, {2048, 4, 1016}, {320, 4, 1016}, {8192, 8, 1008}, {64, 1, 0}};
    for (const auto& r : runs) {
        const gpmpc_tile_list w = gpmpc_build_run_list(r[0], r[1], r[2]);
        ++lists; items += w.n();
        CHECK(w.n() <= r[2] && (w.n() == 0 || ((int)w.ustart.size() == r[1] + 1 && w.ustart[r[1]] == w.n())), "runs %d %d %d: %d items", r[0], r[1], r[2], w.n());
        for (int k = 0; k < w.n(); ++k) {
            const int* t = &w.items[4 * (size_t)k];
            CHECK(t[3] > t[2] && t[3] - t[2] <= 256 && t[2] >= t[1] && t[3] <= r[0], "run %d", k);
        }
    }
    printf("worklist_check: %ld lists, %ld items, %d failures\n", lists, items, failures);
    return failures ? 1 : 0;
}
