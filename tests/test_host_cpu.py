"""CPU-only tests: the C-ABI library loads and exports everything include/gpmpc.h declares, host
logic (marshalling, sharding, collectives over gloo, synthetic generator), and the rule that the
product never routes through the oracle or a CPU fallback.  No GPU compute calls."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian_process_mpc_amd")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


def test_library_exports_every_declared_symbol(built):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpmpc_[a-z_]+)\s*\(", hdr))
    assert len(declared) >= 20
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(h, name) is not None
    assert b"gfx950" in built.lib().gpmpc_version()


def test_cost_params_struct_layout_matches_header(built, tmp_path):
    from gaussian_process_mpc_amd._lib import CostParamsC
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu %zu %zu %zu",'
                   'sizeof(gpmpc_cost_params), offsetof(gpmpc_cost_params,R), offsetof(gpmpc_cost_params,x_ref),'
                   'offsetof(gpmpc_cost_params,has_R_delta));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_R, off_xref, off_flag = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(CostParamsC)
    assert off_R == CostParamsC.R.offset and off_xref == CostParamsC.x_ref.offset
    assert off_flag == CostParamsC.has_R_delta.offset


def test_no_gpu_means_loud_failure_not_fallback(built):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    g = built
    with pytest.raises(g.GpmpcError):
        g.require_gpu()
    with pytest.raises(g.GpmpcError):
        g.GaussianProcessRegression(3)
    with pytest.raises(g.GpmpcError):
        g.RiskSensitiveMPC(-1.0, 5, 2, 1, np.eye(2), np.eye(1))
    with pytest.raises(g.GpmpcError):
        g.GPPack(np.zeros((4, 3)), np.zeros((4, 2)), np.zeros((2, 4, 4)), np.ones((2, 3)), np.ones(2))


def test_abi_argument_validation_without_device(built):
    lib = built.lib()
    h = ctypes.c_void_p()
    assert lib.gpmpc_pack_create(ctypes.byref(h), 0, 2, 1) == -1          # n_train < 1
    assert lib.gpmpc_pack_create(ctypes.byref(h), 10, 9, 1) == -1         # state_dim > GPMPC_MAX_DS
    assert lib.gpmpc_pack_create(ctypes.byref(h), 10, 4, 5) == -1         # D > GPMPC_MAX_D
    assert lib.gpmpc_pack_create(None, 10, 2, 1) == -1
    assert lib.gpmpc_pack_destroy(None) == 0
    assert lib.gpmpc_rollout(None, 1, 1, None, None, None, 0, None, None, None, None, None, 0, None) == -1
    assert lib.gpmpc_moment_match(None, 1, None, None, 0, *([None] * 10), None, 0, None) == -1
    assert lib.gpmpc_rollout_workspace_bytes(None, 1, 1, 0) == 0
    assert lib.gpmpc_predict_workspace_bytes(100, 3, 7) >= 2 * 7 * 100 * 8
    assert lib.gpmpc_matvec(0, 1, None, None, None, None) == -1
    assert lib.gpmpc_device_count() >= 0


def test_xcd_aware_dispatch_order_is_a_bijection_and_keeps_a_tile_on_its_xcd(built):
    """step_fused.h re-derives (trajectory, grid column) from the linear workgroup id (gpmpc_internal.h::gpmpc_xcd_remap, the same inline
    function on host and device).  Every (trajectory, column) must be visited exactly once -- a hole or a double visit is a missing or a
    twice-written partial sum --, and tile k of EVERY trajectory must sit on XCD k mod 8 (linear id mod 8) as long as k is within the last
    multiple of 8: that is what the order is for."""
    lib = built.lib()
    b, c = ctypes.c_int(), ctypes.c_int()
    for nt, ds, B in [(576, 4, 8), (577, 4, 3), (7, 2, 5), (8, 2, 2), (24, 4, 64), (163, 6, 2), (1, 1, 4), (40, 3, 33)]:
        gx = nt + 2 * ds
        seen = set()
        for L in range(gx * B):
            assert lib.gpmpc_debug_xcd_order(L, gx, nt, B, ctypes.byref(b), ctypes.byref(c)) == 0
            assert 0 <= b.value < B and 0 <= c.value < gx
            seen.add((b.value, c.value))
            if c.value < (nt & ~7):
                assert L % 8 == c.value % 8, (nt, B, L, b.value, c.value)
            if c.value >= nt:                                       # role workgroups come after every tile workgroup
                assert L >= nt * B
        assert len(seen) == gx * B, (nt, ds, B)
    assert lib.gpmpc_debug_xcd_order(10, 8, 9, 2, ctypes.byref(b), ctypes.byref(c)) == -1       # more tile columns than columns
    assert lib.gpmpc_debug_xcd_order(16, 8, 4, 2, ctypes.byref(b), ctypes.byref(c)) == -1       # id beyond the grid


def test_balanced_run_list_covers_every_column_once_within_one_generation(built):
    """worklist.h::gpmpc_build_run_list: for ONE trajectory of a large training set every 256-row tile row of every GP is cut into
    runs of at most 256 columns, multiples of 8, contiguous from the tile row's first column to the padded size, and the whole list fits the
    workgroup slots it was built for; small training sets get no list."""
    lib = built.lib()
    n = ctypes.c_int()
    for Np, ds, slots in [(4096, 6, 1024 - 12), (2560, 6, 1012), (3072, 5, 1014), (2752, 5, 1014), (4096, 7, 1010), (4032, 6, 1012)]:
        assert lib.gpmpc_debug_run_list(Np, ds, slots, None, 0, ctypes.byref(n)) == 0
        k = n.value
        assert 0 < k <= slots, (Np, ds, slots, k)
        items = (ctypes.c_int * (4 * k))()
        assert lib.gpmpc_debug_run_list(Np, ds, slots, items, k, ctypes.byref(n)) == 0 and n.value == k
        it = np.array(items[:]).reshape(k, 4)
        assert (np.diff(it[:, 0]) >= 0).all() and set(it[:, 0]) == set(range(ds))            # unit-contiguous, every GP present
        for u in range(ds):
            for i0 in range(0, Np, 256):
                runs = it[(it[:, 0] == u) & (it[:, 1] == i0)]
                assert len(runs) >= 1 and runs[0, 2] == i0 and runs[-1, 3] == Np
                assert (runs[1:, 2] == runs[:-1, 3]).all()                                    # contiguous, no overlap
                lens = runs[:, 3] - runs[:, 2]
                assert (lens > 0).all() and (lens <= 256).all() and (lens % 8 == 0).all()
        lens = it[:, 3] - it[:, 2]
        assert lens.max() - np.median(lens) <= 16                                             # balanced: equal runs up to the 8-column grain
    assert lib.gpmpc_debug_run_list(2048, 4, 1016, None, 0, ctypes.byref(n)) == 0 and n.value == 0      # about one generation already
    assert lib.gpmpc_debug_run_list(320, 4, 1016, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.gpmpc_debug_run_list(100, 4, 1016, None, 0, ctypes.byref(n)) == -1                       # not a padded size
    assert lib.gpmpc_debug_run_list(8192, 8, 1008, None, 0, ctypes.byref(n)) == 0 and n.value == 0      # more than one generation even at 256 columns


# ----------------------------------------------------------------------------------------------------------------------
# work lists of a pack (csrc/worklist.h): kernels, plans and captured graphs index by their ORDER
# ----------------------------------------------------------------------------------------------------------------------
WL_NP = (64, 128, 192, 320, 1024, 2048)     # 64: one tile, never re-ordered (n < 16); 192 / 320: ragged last tiles; 1024 x 4 units: XCD queues run dry
WL_TILINGS = [(256, 256, 0), (64, 64, 0), (256, 64, 0), (64, 128, 0), (256, 128, 0), (256, 32, 0), (256, 16, 0),   # the seven tilings of a pack
              (256, 64, 1), (256, 128, 1), (256, 256, 1)]                                                            # shared-lambda lists: tile slots
WL_UNITS = [(1, 0), (2, 0), (2, 1), (4, 0), (4, 6), (6, 0)]                                                          # (variance, cross) units
WL_RUNS = [(4096, 6, 1012), (2560, 6, 1012), (3072, 5, 1014), (2752, 5, 1014), (4096, 7, 1010), (4032, 6, 1012)]


def _work_list(lib, Np, it, jt, ntri, ncross, sort, slot):
    """(items (n, 4), perm (n,) -- all -1 for a list in natural order, which has none --, ustart (units + 1,)) of gpmpc_debug_work_list."""
    n = ctypes.c_int()
    ust = (ctypes.c_int * (ntri + ncross + 1))()
    assert lib.gpmpc_debug_work_list(Np, it, jt, ntri, ncross, sort, slot, None, 0, ctypes.byref(n), None, None) == 0
    k = n.value
    items, perm = (ctypes.c_int * (4 * k))(), (ctypes.c_int * k)(*([-1] * k))
    assert lib.gpmpc_debug_work_list(Np, it, jt, ntri, ncross, sort, slot, items, k, ctypes.byref(n), perm, ust) == 0 and n.value == k
    return np.array(items[:], dtype="<i4").reshape(k, 4), np.array(perm[:], dtype="<i4"), np.array(ust[:], dtype="<i4")


def _fcs_tables(lib, Np, ds, jt):
    """(ntile (3,), tiles (n, 3), ustart (3, units + 1)) of gpmpc_debug_fcs_tables."""
    nu = ds + ds * (ds - 1) // 2 + 1
    ntile, ust, n = (ctypes.c_int * 3)(), (ctypes.c_int * (3 * nu))(), ctypes.c_int()
    assert lib.gpmpc_debug_fcs_tables(Np, ds, jt, ntile, None, 0, ctypes.byref(n), None) == 0 and n.value == ntile[2]
    tiles = (ctypes.c_int * (3 * n.value))()
    assert lib.gpmpc_debug_fcs_tables(Np, ds, jt, ntile, tiles, n.value, ctypes.byref(n), ust) == 0
    return np.array(ntile[:], dtype="<i4"), np.array(tiles[:], dtype="<i4").reshape(-1, 3), np.array(ust[:], dtype="<i4").reshape(3, nu)


def _run_list(lib, Np, ds, slots):
    n = ctypes.c_int()
    assert lib.gpmpc_debug_run_list(Np, ds, slots, None, 0, ctypes.byref(n)) == 0
    items = (ctypes.c_int * (4 * n.value))()
    assert lib.gpmpc_debug_run_list(Np, ds, slots, items, n.value, ctypes.byref(n)) == 0
    return np.array(items[:], dtype="<i4").reshape(-1, 4)


def _digest(arrays):
    import hashlib
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype="<i4").tobytes() for a in arrays)).hexdigest()


def test_every_work_list_is_item_for_item_what_it_was(built):
    """SHA-256 over items | perm | ustart (little-endian int32) of every list of the grid, over ntile | tiles | ustart of the one-lambda tables
    and over the items of the balanced-run lists, against WORK_LIST_DIGESTS (end of this file)."""
    lib = built.lib()
    got = {}
    for Np in WL_NP:
        for it, jt, slot in WL_TILINGS:
            for ntri, ncross in WL_UNITS:
                for sort in (0, 1):
                    got["%d %d %d %d %d %d %d" % (Np, it, jt, slot, ntri, ncross, sort)] = _digest(_work_list(lib, Np, it, jt, ntri, ncross, sort, slot))
        for ds in (2, 3, 4):
            for jt in (256, 64, 128):
                got["fcs %d %d %d" % (Np, ds, jt)] = _digest(_fcs_tables(lib, Np, ds, jt))
    for Np, ds, slots in WL_RUNS:
        got["runs %d %d %d" % (Np, ds, slots)] = _digest([_run_list(lib, Np, ds, slots)])
    want = dict(line.rsplit(" ", 1) for line in WORK_LIST_DIGESTS.strip().splitlines())
    assert len(want) == 6 * 10 * 6 * 2 + 6 * 3 * 3 + 6 and set(got) == set(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong[:10]


def test_work_list_invariants(built):
    """Independently of the recorded digests: every (unit, row tile, column tile) that should exist appears exactly once -- for a variance unit
    the tiles that reach the diagonal, for a cross unit all --, the 4th entry is the end column (or the tile's slot within its unit), ustart
    partitions the list by unit, and a re-ordered list carries a perm that is a bijection and groups the positions by unit."""
    lib = built.lib()
    reordered = 0
    for Np in (64, 128, 192, 320):
        for it, jt, slot in WL_TILINGS:
            for ntri, ncross in WL_UNITS:
                for sort in (0, 1):
                    items, perm, ust = _work_list(lib, Np, it, jt, ntri, ncross, sort, slot)
                    what, n = (Np, it, jt, slot, ntri, ncross, sort), len(items)
                    expect = [(u, i0, j0) for u in range(ntri + ncross) for i0 in range(0, Np, it) for j0 in range(0, Np, jt)
                              if u >= ntri or min(j0 + jt, Np) > i0]
                    assert sorted(map(tuple, items[:, :3])) == expect, what                   # exactly once, nothing wholly below the diagonal
                    assert (np.diff(ust) >= 0).all() and ust[0] == 0 and ust[-1] == n, what
                    assert (np.bincount(items[:, 0], minlength=ntri + ncross) == np.diff(ust)).all(), what
                    if slot:                                                                  # the tile's index within its unit, in (i0, j0) order
                        for u in range(ntri + ncross):
                            mine = items[items[:, 0] == u]
                            assert [tuple(r) for r in mine[np.argsort(mine[:, 3])][:, 1:3]] == [e[1:] for e in expect if e[0] == u], what
                    else:
                        assert (items[:, 3] == np.minimum(items[:, 2] + jt, Np)).all(), what
                    if (perm < 0).all():                                                      # natural order: unit-contiguous, no perm
                        assert not (sort and n >= 16), what
                        assert [tuple(r) for r in items[:, :3]] == expect, what
                    else:
                        assert sort and n >= 16, what
                        reordered += 1
                        assert sorted(perm) == list(range(n)), what
                        for u in range(ntri + ncross):
                            assert sorted(perm[ust[u]:ust[u + 1]]) == list(np.flatnonzero(items[:, 0] == u)), what
    assert reordered >= 40
    # the one-lambda tables: row block ti's columns from its diagonal block on in chunks of 256; unit offsets = the variance units of the
    # 256 x jt full-covariance list, then one block of ntile slots per pair
    for Np in (64, 128, 192, 320):
        for ds in (2, 3, 4):
            npairs = ds * (ds - 1) // 2
            for jt in (256, 64, 128):
                ntile, tiles, ust = _fcs_tables(lib, Np, ds, jt)
                T = Np // 64
                assert ntile[0] == T * (T + 1) // 2 and ntile[1] == 4 * ntile[0] and ntile[2] == len(tiles)
                assert [tuple(t) for t in tiles] == [(ti, j0, min(256, Np - j0)) for ti in range(T) for j0 in range(64 * ti, Np, 256)]
                tri = _work_list(lib, Np, 256, jt, ds, npairs, 0, 0)[2]
                for q in range(3):
                    assert (ust[q, :ds + 1] == tri[:ds + 1]).all() and (np.diff(ust[q, ds:]) == ntile[q]).all()
    # refused: sizes that are no padded size / tile size / unit count, a capacity below the count
    n = ctypes.c_int()
    buf = (ctypes.c_int * 64)()
    for bad in [(100, 256, 64, 2, 0), (128, 100, 64, 2, 0), (128, 256, 0, 2, 0), (128, 256, 64, 0, 0), (128, 256, 64, 9, 0), (128, 256, 64, 2, 29), (128, 256, 64, -1, 3)]:
        assert lib.gpmpc_debug_work_list(*bad, 1, 0, None, 0, ctypes.byref(n), None, None) == -1, bad
    assert lib.gpmpc_debug_work_list(128, 256, 64, 2, 0, 1, 0, None, 0, None, None, None) == -1
    assert lib.gpmpc_debug_work_list(128, 256, 64, 2, 0, 1, 0, buf, 2, ctypes.byref(n), buf, buf) == -1 and n.value == 4      # capacity below the count
    assert lib.gpmpc_debug_work_list(128, 256, 64, 2, 0, 1, 0, buf, 4, ctypes.byref(n), None, buf) == -1
    assert lib.gpmpc_debug_fcs_tables(128, 1, 64, buf, None, 0, ctypes.byref(n), None) == -1
    assert lib.gpmpc_debug_fcs_tables(128, 5, 64, buf, None, 0, ctypes.byref(n), None) == -1
    assert lib.gpmpc_debug_fcs_tables(100, 2, 64, buf, None, 0, ctypes.byref(n), None) == -1
    assert lib.gpmpc_debug_fcs_tables(128, 2, 64, buf, buf, 1, ctypes.byref(n), buf) == -1 and n.value == 2


def test_product_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import oracle/."""
    pat = re.compile(r"^\s*(from|import)\s+oracle\b", re.M)
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not pat.search(txt), f
                assert "oracle" not in txt.lower() or f == "__init__.py" or "the oracle is pinned" in txt or \
                    all("import" not in ln for ln in txt.splitlines() if "oracle" in ln.lower()), f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    hits = [m.start() for m in pat.finditer(bench)]
    start = bench.index("def cpu_baseline")
    end = bench.index("def main")
    assert 1 <= len(hits) <= 2 and all(start < h < end for h in hits)      # torch oracle + its C port, both inside cpu_baseline


def test_cost_params_marshalling(built):
    g = built
    Q = np.array([[2.0, 0.5], [0.25, 3.0]])
    R = np.array([[1.5]])
    c = g.CostParams(-1.0, Q, R, R_delta=np.array([[0.7]]), x_ref=[0.1, 0.2], u_ref=[0.3], last_u=np.array([9.0, 8.0]))
    assert c.c.gamma == -1.0 and c.c.has_R_delta == 1
    assert list(c.c.Q[:4]) == [2.0, 0.5, 0.25, 3.0] and c.c.R[0] == 1.5 and c.c.R_delta[0] == 0.7
    assert list(c.c.x_ref[:2]) == [0.1, 0.2] and c.c.u_ref[0] == 0.3 and c.c.last_u[0] == 9.0
    assert g.CostParams(0.0, np.eye(3), np.eye(2)).c.has_R_delta == 0
    with pytest.raises(ValueError):
        g.CostParams(1.0, np.eye(9), np.eye(1))


def test_synth_problem_is_seeded_and_shaped(built):
    from gaussian_process_mpc_amd.synth import CONFIGS, synth_problem
    a = synth_problem(3, 64, 4, 1, 5, 3)
    b = synth_problem(3, 64, 4, 1, 5, 3)
    for k in ("X", "Y", "lambdas", "x0", "U"):
        assert np.array_equal(a[k], b[k])
    assert a["X"].shape == (64, 5) and a["Y"].shape == (64, 4) and a["U"].shape == (3, 5, 1)
    assert not np.array_equal(a["X"], synth_problem(4, 64, 4, 1, 5, 3)["X"])
    assert CONFIGS["C3"] == dict(N=2048, ds=4, da=1, H=20, B=256, gamma=-1.0)
    assert CONFIGS["C4"]["N"] == 4096 and CONFIGS["C2"]["B"] == 1


def test_shard_ranges_partition(built):
    from gaussian_process_mpc_amd.parallel import shard_range, shard_sizes
    for n, w in ((256, 8), (1024, 8), (10, 3), (5, 8), (1, 2)):
        covered = []
        for r in range(w):
            lo, hi = shard_range(n, w, r)
            covered += list(range(lo, hi))
        assert covered == list(range(n))
        assert sum(shard_sizes(n, w)) == n and max(shard_sizes(n, w)) - min(shard_sizes(n, w)) <= 1


def _gloo_worker(rank, world, port, ragged, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from gaussian_process_mpc_amd.parallel import gather_results, shard_range, shard_sizes, broadcast_kinv
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = 7 if ragged else 8
    H, da = 3, 2
    cost_all = torch.arange(n, dtype=torch.float64) * 1.5
    grad_all = torch.arange(n * H * da, dtype=torch.float64).reshape(n, H, da)
    lo, hi = shard_range(n, world, rank)
    sizes = shard_sizes(n, world)
    c, g = gather_results(cost_all[lo:hi].clone(), grad_all[lo:hi].clone(), dist, sizes if ragged else None)
    c2, g2 = gather_results(cost_all[lo:hi].clone(), None, dist, sizes if ragged else None)
    from gaussian_process_mpc_amd.parallel import sharded_rollout
    fake = lambda x0b, Ub: {"cost": Ub.sum(dim=(1, 2)), "grad": 2.0 * Ub}      # stands in for the device rollout  # noqa: E731
    Uall = torch.arange(n * H * da, dtype=torch.float64).reshape(n, H, da) / 7.0
    cs, gs = sharded_rollout(fake, torch.zeros(3), Uall, dist)
    ok_sharded = bool(torch.equal(cs, Uall.sum(dim=(1, 2))) and torch.equal(gs, 2.0 * Uall))
    kinv = torch.full((2, 4, 4), float(rank + 1), dtype=torch.float64)
    broadcast_kinv(kinv, dist, src=0)
    ok = bool(torch.equal(c, cost_all) and torch.equal(g, grad_all) and torch.equal(c2, cost_all) and g2 is None
              and torch.all(kinv == 1.0) and ok_sharded)
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.parametrize("ragged", [False, True])
def test_gather_results_gloo_world2(ragged):
    """The N>1 path of bench.py / the sharded batch API: fused all_gather of [cost | grad] and the
    pack broadcast, world_size 2 over gloo on CPU."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 400) + (50 if ragged else 0)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, ragged, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]


def _gloo_worker_more_ranks_than_items(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from gaussian_process_mpc_amd.parallel import sharded_rollout
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    H, da = 3, 2
    fake = lambda x0b, Ub: {"cost": Ub.sum(dim=(1, 2)), "grad": 2.0 * Ub}      # noqa: E731
    ok = True
    for n in (1, 2):                                    # fewer trajectories than ranks: some ranks own an empty block
        Uall = torch.arange(n * H * da, dtype=torch.float64).reshape(n, H, da) / 3.0
        cs, gs = sharded_rollout(fake, torch.zeros(3), Uall, dist)
        ok = ok and bool(torch.equal(cs, Uall.sum(dim=(1, 2))) and torch.equal(gs, 2.0 * Uall))
        cs, gs = sharded_rollout(fake, torch.zeros(3), Uall, dist, want_grad=False)
        ok = ok and bool(torch.equal(cs, Uall.sum(dim=(1, 2))) and gs is None)
    q.put((rank, ok))
    dist.destroy_process_group()


def test_sharded_rollout_more_ranks_than_trajectories_gloo_world3():
    """world > B: the ranks without a trajectory contribute an empty block and must still enter the collective (an
    ambiguous reshape of the (0, H, da) gradient used to raise on them while the others hung in all_gather)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 400) + 120
    procs = [ctx.Process(target=_gloo_worker_more_ranks_than_items, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(3))
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True), (2, True)]


def test_bench_refuses_to_mislabel_the_rank_count():
    """bench.py --gpus N must run N ranks or fail: (i) with WORLD_SIZE already set to something else it exits non-zero
    before touching a device; (ii) with no WORLD_SIZE and fewer visible GPUs than N the launcher exits non-zero (here:
    zero GPUs) instead of printing a 1-GPU line -- the round-1 behaviour the driver would have recorded as `n_gpus: 1`."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=dict(env, WORLD_SIZE="1", RANK="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '"n_gpus"' not in r.stdout


def test_bench_launcher_notices_a_dead_rank_within_seconds():
    """bench.py's launcher polls every child: when rank 1 dies while rank 0 would sit in a collective for minutes, the job
    ends non-zero in well under 30 s (it used to block on rank 0's stdout until the process-group timeout)."""
    import time
    import types
    sys.path.insert(0, ROOT)
    import bench
    worker = ("import os, sys, time\n"
              "r = int(os.environ['RANK'])\n"
              "assert os.environ['WORLD_SIZE'] == '3' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
              "if r == 1:\n    time.sleep(1.0); sys.exit(7)\n"
              "print('{\"rank\": %d}' % r, flush=True)\n"
              "time.sleep(600)\n")
    t0 = time.time()
    rc = bench.spawn_ranks(types.SimpleNamespace(gpus=3, oversubscribe=True), argv=[sys.executable, "-c", worker])
    assert rc == 7 and time.time() - t0 < 30.0
    ok = "import os\nprint('{\"n\": %s}' % os.environ['RANK'], flush=True)\n"
    assert bench.spawn_ranks(types.SimpleNamespace(gpus=2, oversubscribe=True), argv=[sys.executable, "-c", ok]) == 0


def test_plants_match_the_reference_environments(golden):
    """the plant updates either side of the path, as plain classes, against the reference's own
    environment classes run by tests/golden/gen_golden.py (g9): cart-pole stepPhysics / step
    (src/environments/continuous_cartpole.py:71-101) and pendulum step_static / step
    (src/environments/adjustable_pendulum.py:135-178), bit for bit (same operations in the same order)."""
    from gaussian_process_mpc_amd.simulator import CartPolePlant, PendulumPlant
    z = golden("g9_closed_loop.npz")
    cp = CartPolePlant()
    assert [cp.gravity, cp.masscart, cp.masspole, cp.length, cp.force_mag, cp.tau] == list(z["cp_params"])
    nxt = np.array([cp.stepPhysics(float(f), tuple(s)) for s, f in zip(z["cp_states"], z["cp_forces"])])
    assert np.array_equal(nxt, z["cp_next"])
    cp = CartPolePlant(init_state=z["cp_chain_x0"])
    cp.reset()
    chain = []
    for a in z["cp_chain_actions"]:
        obs, rew, term, trunc, _ = cp.step(np.array([a]))
        assert rew == 1 and not term and not trunc
        chain.append(obs)
    assert np.array_equal(np.array(chain), z["cp_chain"])
    with pytest.raises(AssertionError):
        cp.step(np.array([1.0]))                                  # the reference asserts -1 < action < 1
    s0, _ = CartPolePlant(seed=3).reset()
    assert s0.shape == (4,) and np.all(np.abs(s0) <= 0.2)
    opts = dict(zip(("g", "m", "l", "dt", "max_torque", "max_speed"), z["pd_opts"]))
    st = np.array([PendulumPlant.step_static(s, u, opts) for s, u in zip(z["pd_states"], z["pd_u"])])
    assert np.array_equal(st, z["pd_static_next"])
    pd = PendulumPlant(g=10.0, max_speed=8, max_torque=2.0, init_state=(np.pi, 0.0))
    obs, _ = pd.reset()
    states, rewards = [obs], []
    for u in z["pd_chain_actions"]:
        obs, r, _, _, _ = pd.step(u)
        states.append(obs); rewards.append(r)
    assert np.array_equal(np.array(states), z["pd_chain"])
    np.testing.assert_allclose(rewards, z["pd_chain_reward"], rtol=1e-15)
    assert np.array_equal(PendulumPlant.step_static(z["pd_chain"][3], z["pd_chain_actions"][3], pd.options()), z["pd_chain"][4])


# ------------------------------------------------------------------------------------------------------------------
# round 5: lock-step multi-start driver (host logic; the GPU variant is tests/test_gpu_api.py::test_closed_loop_simulator_multistart)
# ------------------------------------------------------------------------------------------------------------------
def _rosen_batch(X):
    f = np.sum(100 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1)
    g = np.zeros_like(X)
    g[:, :-1] += -400 * X[:, :-1] * (X[:, 1:] - X[:, :-1] ** 2) - 2 * (1 - X[:, :-1])
    g[:, 1:] += 200 * (X[:, 1:] - X[:, :-1] ** 2)
    return f, g


def test_lockstep_multistart_reaches_the_bounded_optima_scipy_finds():
    """K projected L-BFGS searches advanced together, ONE batched evaluation per tick (multistart.py: the consumer of the
    trajectory batch inside a solve, src/mpc.py:269-330): on a bounded Rosenbrock every start ends where scipy's L-BFGS-B ends from
    the same point; evaluations = ticks + 1 (never one call per start); a region that returns NaN (the risk-sensitive cost's
    log det of a non-positive matrix, src/mpc.py:183) rejects trial points and drops starts that begin inside it."""
    from scipy.optimize import minimize
    from gaussian_process_mpc_amd.multistart import lockstep_lbfgs, make_starts
    n = 8
    lb, ub = -2 * np.ones(n), 0.8 * np.ones(n)
    X0 = make_starts(12, n, lb, ub, np.random.default_rng(1), warm=np.full(n, 0.5))
    assert np.array_equal(X0[0], np.zeros(n)) and np.array_equal(X0[1], np.full(n, 0.5)) and (X0 >= lb).all() and (X0 <= ub).all()
    calls = []

    def ev(X):
        calls.append(X.shape)
        return _rosen_batch(X)
    x, info = lockstep_lbfgs(ev, X0, lb, ub, max_ticks=2000, gtol=1e-6)
    assert info["converged"].all() and len(calls) == info["evaluations"] == info["ticks"] + 1
    assert all(c == (12, n) for c in calls)
    for k in (0, 1, 5):
        r = minimize(lambda v: _rosen_batch(v[None])[0][0], X0[k], jac=lambda v: _rosen_batch(v[None])[1][0], method="L-BFGS-B",
                     bounds=list(zip(lb, ub)), options={"gtol": 1e-6, "ftol": 1e-14})
        assert abs(info["f"][k] - r.fun) <= 1e-6 * max(1.0, abs(r.fun))
    assert np.isclose(_rosen_batch(x[None])[0][0], info["f"].min()) and (x <= ub + 1e-15).all()
    x2, info2 = lockstep_lbfgs(_rosen_batch, X0, lb, ub, max_ticks=2000, gtol=1e-6)      # deterministic: same bits
    assert np.array_equal(x, x2) and np.array_equal(info["f"], info2["f"])
    # four step lengths per start and tick (the line-search evaluations of an iteration as ONE batch of 4 K plans): fewer ticks, same optima
    shapes = []

    def ev4(X):
        shapes.append(X.shape)
        return _rosen_batch(X)
    x4, info4 = lockstep_lbfgs(ev4, X0, lb, ub, max_ticks=2000, gtol=1e-6, line_points=4)
    assert info4["converged"].all() and info4["ticks"] < info["ticks"] and set(shapes[1:]) == {(48, n)} and shapes[0] == (12, n)
    np.testing.assert_allclose(info4["f"], info["f"], rtol=1e-6)

    def with_nan(X):
        f, g = np.sum((X - 0.3) ** 2, axis=1), 2 * (X - 0.3)
        return np.where(X[:, 0] > 0.9, np.nan, f), g
    x, info = lockstep_lbfgs(with_nan, np.array([[0.95, 0, 0], [0.0, 0, 0], [-1, 1, 1.0]]), -np.ones(3), np.ones(3))
    assert list(info["alive"]) == [False, True, True] and np.allclose(x, 0.3) and info["best"] in (1, 2)


def _gloo_multistart_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from gaussian_process_mpc_amd.multistart import lockstep_lbfgs, make_starts
    from gaussian_process_mpc_amd.parallel import sharded_rollout
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    K, H, da = 5, 4, 2                                   # ragged: 3 + 2 starts
    n = H * da
    lb, ub = -2 * np.ones(n), 0.8 * np.ones(n)
    X0 = make_starts(K, n, lb, ub, np.random.default_rng(7))
    blocks = []

    def fake_rollout(x0b, Ub):                            # stands in for the device rollout of this rank's block of plans
        blocks.append(Ub.shape[0])
        f, g = _rosen_batch(Ub.reshape(Ub.shape[0], n).numpy())
        return {"cost": torch.as_tensor(f), "grad": torch.as_tensor(g).reshape(-1, H, da)}

    def evaluate(X):
        c, g = sharded_rollout(fake_rollout, torch.zeros(3), torch.as_tensor(X.reshape(K, H, da)), dist)
        return c.numpy(), g.numpy().reshape(K, n)
    x, info = lockstep_lbfgs(evaluate, X0, lb, ub, max_ticks=1500, gtol=1e-6)
    xs, infos = lockstep_lbfgs(_rosen_batch, X0, lb, ub, max_ticks=1500, gtol=1e-6)          # the same solve in one process
    ok = bool(np.array_equal(x, xs) and np.array_equal(info["f"], infos["f"]) and info["ticks"] == infos["ticks"]
              and set(blocks) == {3 if rank == 0 else 2})
    q.put((rank, ok, x.tobytes()))
    dist.destroy_process_group()


def test_lockstep_multistart_sharded_over_two_gloo_ranks():
    """The sharded variant of the multi-start solve (RiskSensitiveMPC._solve_multistart with torch.distributed initialised): each rank
    evaluates ITS block of the K trial plans, one fused all_gather returns every [cost | grad] to every rank, and both ranks run
    the same deterministic host loop -- identical plans on both ranks, bit-equal to the single-process solve."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 400) + 170
    procs = [ctx.Process(target=_gloo_multistart_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert [(r, ok) for r, ok, _ in res] == [(0, True), (1, True)] and res[0][2] == res[1][2]


# ------------------------------------------------------------------------------------------------------------------
# round 5: build-time spill guard, compact bench record
# ------------------------------------------------------------------------------------------------------------------
def test_spill_guard_passes_on_the_shipped_build_and_fails_on_a_new_spill(built, tmp_path):
    """`make check` (tools/spill_guard.py over the <object>.res files the build writes): every shipped kernel within its VGPR-spill /
    scratch budget -- the whole-horizon instances for D <= 7 at ZERO spills --, and a kernel that starts to spill fails the check."""
    import subprocess
    build = os.path.join(PKG, "csrc", "build")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spill_guard.py"), build, "--all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("k_traj_persist<")]
    assert len(rows) >= 40
    for ln in rows:
        if not re.match(r"k_traj_persist<8, ", ln):
            assert " spill v  0 " in ln and ln.rstrip().endswith(" ok"), ln
    bad = tmp_path / "b"
    bad.mkdir()
    (bad / "x.o.res").write_text(
        "f.h:1:1: remark: Function Name: _Z14k_traj_persistILi5ELi4ELb1ELi1EEv11PersistArgs [-Rpass-analysis=kernel-resource-usage]\n"
        "f.h:1:1: remark:     VGPRs: 128 [-Rpass-analysis=kernel-resource-usage]\n"
        "f.h:1:1: remark:     ScratchSize [bytes/lane]: 48 [-Rpass-analysis=kernel-resource-usage]\n"
        "f.h:1:1: remark:     VGPRs Spill: 11 [-Rpass-analysis=kernel-resource-usage]\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spill_guard.py"), str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "OVER BUDGET" in r.stderr


def test_bench_stdout_record_is_compact():
    """The driver keeps an 8 KB tail of stdout: the default line (headline + roofline + cpu_baseline + every leg) must fit in 6 KB,
    each leg in ~250 bytes with value / ms_per_step / kernel / bound / frac / avg_launch_ms."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04", "bench_C3.json")))      # a full record of the previous format
    legs = {}
    for name, _ in bench.LEGS:
        legs[name] = {"value": 12345.678, "unit": "rollouts/s", "ms_per_step": 1.2345678, "kernel": "gpmpc_pair_kernel_sbs<5,4,4,true,false>",
                      "bound": "valu_fp64", "frac": 0.5021, "avg_launch_ms": 1.30712}
    full["extras"] = legs
    full["extras_full"] = {"x": "y" * 5000}
    line = json.dumps(bench.compact_record(full), separators=(",", ":"))
    assert len(line) < 6000, len(line)
    d = json.loads(line)
    assert "extras_full" not in d and set(d["extras"]) == {n for n, _ in bench.LEGS}
    assert all(len(json.dumps(v, separators=(",", ":"))) <= 250 for v in d["extras"].values())
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"]
    assert bench.short_kernel("k_step_fused<5,4,true,32,1> (one launch per horizon step: ...)") == "k_step_fused<5,4,true,32,1>"


def test_bench_dump_outputs_keeps_small_outputs_and_samples_large_ones(tmp_path, monkeypatch):
    """--dump-outputs: under the limit every array is written as float64, unchanged; over it, the files stay within the
    limit, cost and grad keep the SAME seeded rows, sample_rows.npy names them, and a second call writes identical files."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    cost = rng.standard_normal(300)
    grad = cost[:, None, None] * np.arange(1, 7)[None, :, None]          # row i of grad is a function of cost[i]
    bench.dump_outputs(str(tmp_path / "small"), {"cost": cost, "grad": grad})
    assert sorted(os.listdir(tmp_path / "small")) == ["cost.npy", "grad.npy"]
    for name, a in (("cost", cost), ("grad", grad)):
        b = np.load(tmp_path / "small" / f"{name}.npy")
        assert b.dtype == np.float64 and np.array_equal(a, b)
    assert bench.dump_outputs(str(tmp_path / "none"), {"cost": cost, "grad": None}) is None
    assert sorted(os.listdir(tmp_path / "none")) == ["cost.npy"]
    limit = bench.NPY_HEADER_SLACK + 4000                               # ~70 of the 300 rows (8 + 48 + 8 bytes each) fit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    files = []
    for run in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / run), {"cost": cost.astype(np.float32), "grad": grad})
        names = sorted(os.listdir(tmp_path / run))
        assert names == ["cost.npy", "grad.npy", "sample_rows.npy"]
        assert sum(os.path.getsize(tmp_path / run / n) for n in names) <= limit
        files.append({n: open(tmp_path / run / n, "rb").read() for n in names})
    assert files[0] == files[1]
    c, g, rows = (np.load(tmp_path / "big1" / n) for n in ("cost.npy", "grad.npy", "sample_rows.npy"))
    assert c.dtype == g.dtype == rows.dtype == np.float64
    idx = rows.astype(np.int64)
    assert 1 < len(idx) < len(cost) and np.all(np.diff(idx) > 0) and np.array_equal(rows, idx)
    assert np.array_equal(c, cost.astype(np.float32).astype(np.float64)[idx]) and np.array_equal(g, grad[idx])


def test_split_golden_fixture_round_trip(tmp_path):
    """oracle/golden.py: a fixture written in parts with a nearly symmetric matrix stored as triangle + residual comes back
    bit for bit under its own names; the split g10 fixture has both noise levels' inverses; a whole fixture loads as np.load."""
    sys.path.insert(0, ROOT)
    from oracle import golden
    rng = np.random.default_rng(11)
    a = rng.standard_normal((37, 37))
    m = np.linalg.inv(a @ a.T + 37 * np.eye(37))                        # an LU inverse: symmetric up to round-off
    parts = [{"m": m, "v": np.arange(5.0)}, {"w": rng.standard_normal((2, 3))}]
    golden.save_split(str(tmp_path / "f.npz"), parts, nearly_symmetric=("m",))
    assert sorted(os.listdir(tmp_path)) == ["f.npz", "f_part2.npz"] and "m" not in np.load(tmp_path / "f.npz").files
    d = golden.load("f.npz", str(tmp_path))
    assert set(d) == {"m", "v", "w"}
    for k, v in (("m", m), ("v", parts[0]["v"]), ("w", parts[1]["w"])):
        assert d[k].dtype == v.dtype and d[k].shape == v.shape and d[k].tobytes() == v.tobytes()
    z = golden.load("g10_readme_regime.npz")
    N = int(z["dims"][0])
    assert z["s0_Ky_inv"].shape == z["s1_Ky_inv"].shape == (N, N) and z["s1_vars"].shape == z["s0_vars"].shape
    assert isinstance(golden.load("g3_rollout_c1.npz"), type(np.load(os.path.join(golden.GOLDEN, "g3_rollout_c1.npz"))))


# Recorded from the parent of the commit that moved the list construction into csrc/worklist.h (dcfe28d), whose build_worklist / runs_host /
# fcs_refresh were given copy-out entries in a scratch build: "Np rows cols tile_slot variance_units cross_units xcd_sort", "fcs Np ds cols" and
# "runs Np ds slots", then the digest.
WORK_LIST_DIGESTS = """
64 256 256 0 1 0 0 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 256 0 1 0 1 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 256 0 2 0 0 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 256 0 2 0 1 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 256 0 2 1 0 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 256 0 2 1 1 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 256 0 4 0 0 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 256 0 4 0 1 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 256 0 4 6 0 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 256 0 4 6 1 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 256 0 6 0 0 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 256 0 6 0 1 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 64 64 0 1 0 0 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 64 64 0 1 0 1 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 64 64 0 2 0 0 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 64 64 0 2 0 1 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 64 64 0 2 1 0 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 64 64 0 2 1 1 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 64 64 0 4 0 0 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 64 64 0 4 0 1 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 64 64 0 4 6 0 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 64 64 0 4 6 1 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 64 64 0 6 0 0 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 64 64 0 6 0 1 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 64 0 1 0 0 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 64 0 1 0 1 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 64 0 2 0 0 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 64 0 2 0 1 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 64 0 2 1 0 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 64 0 2 1 1 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 64 0 4 0 0 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 64 0 4 0 1 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 64 0 4 6 0 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 64 0 4 6 1 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 64 0 6 0 0 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 64 0 6 0 1 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 64 128 0 1 0 0 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 64 128 0 1 0 1 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 64 128 0 2 0 0 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 64 128 0 2 0 1 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 64 128 0 2 1 0 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 64 128 0 2 1 1 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 64 128 0 4 0 0 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 64 128 0 4 0 1 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 64 128 0 4 6 0 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 64 128 0 4 6 1 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 64 128 0 6 0 0 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 64 128 0 6 0 1 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 128 0 1 0 0 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 128 0 1 0 1 ff7ee299c0c763dd923cc2707321b7c9815a3e3d872b7e1b0988b7472c760883
64 256 128 0 2 0 0 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 128 0 2 0 1 6ccb2bb093c58d4af267dd2b294526d4aca0a1dc4b6cd02e424079aae0713634
64 256 128 0 2 1 0 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 128 0 2 1 1 58286e173ff522f0b1f6454641aad6f09ca69cb4720fcf9f112d287551e7d43d
64 256 128 0 4 0 0 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 128 0 4 0 1 7abe108b720acd632755e6a7469a9a663c9a537e48c40be62b7ac346644ee4df
64 256 128 0 4 6 0 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 128 0 4 6 1 1a8a5483cf0babe2c5108fa2fc959a20cfee3f7a8748fcc824bf971654485199
64 256 128 0 6 0 0 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 128 0 6 0 1 d8bcf82de4c480b32c654b4f07b98aad517e4223cb7df95a2afa5c6a7732d546
64 256 32 0 1 0 0 9f2f295cd1311fbf1e9093d63cee8cf2257ebf30e71ed1500d7fdfd0d49d5806
64 256 32 0 1 0 1 9f2f295cd1311fbf1e9093d63cee8cf2257ebf30e71ed1500d7fdfd0d49d5806
64 256 32 0 2 0 0 b2110734c82696fff0f139ba72c4807daa210499f402bab0fa7fd23cd121cd19
64 256 32 0 2 0 1 b2110734c82696fff0f139ba72c4807daa210499f402bab0fa7fd23cd121cd19
64 256 32 0 2 1 0 78b909a1b8fa2af2c8b7879b55b080e22173e6a2a9320362ce7e4b83b618e2d0
64 256 32 0 2 1 1 78b909a1b8fa2af2c8b7879b55b080e22173e6a2a9320362ce7e4b83b618e2d0
64 256 32 0 4 0 0 cc0ceaa1cb66f51a4a8011b8e063eda7a5cede2279ebe84bbecb5a6d24d9ac03
64 256 32 0 4 0 1 cc0ceaa1cb66f51a4a8011b8e063eda7a5cede2279ebe84bbecb5a6d24d9ac03
64 256 32 0 4 6 0 877dcee9ab68c1a3c69b9cba918a421f05a4894f7819ec244a0691ea15ada507
64 256 32 0 4 6 1 1cb6446e97b3c071cbfff93cd77887aa32c7372e4b929979e6af5827ff2ef697
64 256 32 0 6 0 0 727a9ac196b2aa57f2f5793c93f7894fa81d730970622dc36299ff6203c69c67
64 256 32 0 6 0 1 727a9ac196b2aa57f2f5793c93f7894fa81d730970622dc36299ff6203c69c67
64 256 16 0 1 0 0 d36d5e9a4876c7e82610d015628c886b9a31cc1af570a44939587f3272c5c13a
64 256 16 0 1 0 1 d36d5e9a4876c7e82610d015628c886b9a31cc1af570a44939587f3272c5c13a
64 256 16 0 2 0 0 775eb872ff40f56dea55a6f596294f84b94321d496351c2d780e46ca44d6c206
64 256 16 0 2 0 1 775eb872ff40f56dea55a6f596294f84b94321d496351c2d780e46ca44d6c206
64 256 16 0 2 1 0 41be694a61d9635e96680c15ef7355fa57ed3b85d63b240159febbb2691dc694
64 256 16 0 2 1 1 41be694a61d9635e96680c15ef7355fa57ed3b85d63b240159febbb2691dc694
64 256 16 0 4 0 0 228c0782f888f8f1c0a1f60beb38f98936bcadccd432664e8b253f695d49ee6f
64 256 16 0 4 0 1 bc80f256695b9ce3bb3db29c76419d362df1903d1aa39da9b6988e0004cd0e63
64 256 16 0 4 6 0 5bee9d366e174b792d998b2bcb8b4187d9e7f014b36713e38f1c65a471472eb3
64 256 16 0 4 6 1 bce1cb5bd63ca1c5112a27f19ce64fc2d55500274d0616826c0b2f576b04034d
64 256 16 0 6 0 0 dbfdd181b63d11f5ea14e0a4d7c0a55fa36ff394ddd64f4fe1b9942b48066e34
64 256 16 0 6 0 1 eff2f5102b6ff37999d7b5751a2e0ce954335ead6fa75165fcbc3f6e6218264f
64 256 64 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 64 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 64 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 64 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 64 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 64 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 64 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 64 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 64 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 64 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 64 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
64 256 64 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
64 256 128 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 128 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 128 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 128 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 128 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 128 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 128 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 128 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 128 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 128 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 128 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
64 256 128 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
64 256 256 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 256 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
64 256 256 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 256 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
64 256 256 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 256 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
64 256 256 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 256 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
64 256 256 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 256 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
64 256 256 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
64 256 256 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
128 256 256 0 1 0 0 72499965592fc20517d3ac848d2b9fe5a803ae49f31ccce6faf5ed18dffd9810
128 256 256 0 1 0 1 72499965592fc20517d3ac848d2b9fe5a803ae49f31ccce6faf5ed18dffd9810
128 256 256 0 2 0 0 daecd11ca30c3c3023d0cce9b4f3ad87acb4293a478bec8fa57005921d33fea1
128 256 256 0 2 0 1 daecd11ca30c3c3023d0cce9b4f3ad87acb4293a478bec8fa57005921d33fea1
128 256 256 0 2 1 0 21e97fe4e4a00d74c96cd9201b6b19ecbbe40c471f74edbef4472969a5fbdc47
128 256 256 0 2 1 1 21e97fe4e4a00d74c96cd9201b6b19ecbbe40c471f74edbef4472969a5fbdc47
128 256 256 0 4 0 0 6496b5377dcd2d580905559da1e65084b19e05ddeeb5e6ce3220d1fb34edc4a2
128 256 256 0 4 0 1 6496b5377dcd2d580905559da1e65084b19e05ddeeb5e6ce3220d1fb34edc4a2
128 256 256 0 4 6 0 cc8a62d7ab8ff7ca8de84c18ba9f89faee2e60e6f7e387b034af571f14303c49
128 256 256 0 4 6 1 cc8a62d7ab8ff7ca8de84c18ba9f89faee2e60e6f7e387b034af571f14303c49
128 256 256 0 6 0 0 3cb3caaf39feeac08fee7e20219f55dbe3d4e66e795a76ef30d4dfeca97b651a
128 256 256 0 6 0 1 3cb3caaf39feeac08fee7e20219f55dbe3d4e66e795a76ef30d4dfeca97b651a
128 64 64 0 1 0 0 384fd09bb22def10dc8d3581f43302a0293c9bd4dad412c8b355d07254622338
128 64 64 0 1 0 1 384fd09bb22def10dc8d3581f43302a0293c9bd4dad412c8b355d07254622338
128 64 64 0 2 0 0 3adc12bea428048eac7263f30b5ba4dfcf1ae44548fe4c3129d5d6f5f110e5da
128 64 64 0 2 0 1 3adc12bea428048eac7263f30b5ba4dfcf1ae44548fe4c3129d5d6f5f110e5da
128 64 64 0 2 1 0 b5173e88c1f03295781530023479b696e070afa1a61a763ef5674477091dd7f4
128 64 64 0 2 1 1 b5173e88c1f03295781530023479b696e070afa1a61a763ef5674477091dd7f4
128 64 64 0 4 0 0 d35e99a8170b5c0a53fc1ac2c4368b19ea9a9b1beb90aa3e336b42eb3310f2ec
128 64 64 0 4 0 1 d35e99a8170b5c0a53fc1ac2c4368b19ea9a9b1beb90aa3e336b42eb3310f2ec
128 64 64 0 4 6 0 294b00492c9ef16353ef7ed80c54e3cc02fba4760172e4764407650c73816ab6
128 64 64 0 4 6 1 bac15b0016042b3f3e64722fcc837a354680c626227391236d257569ff63b1fb
128 64 64 0 6 0 0 66ee9e08ddba0f31b4397e152b32c4c39742714735c67b753d03af7caa9f261a
128 64 64 0 6 0 1 63fb4b340b093f5fa7507718a5073257059127b5ecb4b8a0bc77390aad0df8af
128 256 64 0 1 0 0 d00e5f8a852e3320a2d5791220436543fe255869e7d9c15d07feb99f259929c3
128 256 64 0 1 0 1 d00e5f8a852e3320a2d5791220436543fe255869e7d9c15d07feb99f259929c3
128 256 64 0 2 0 0 aa3e831df4a17de606598793f37b456bd62fd19de394e33684ca06fc0b77f3c7
128 256 64 0 2 0 1 aa3e831df4a17de606598793f37b456bd62fd19de394e33684ca06fc0b77f3c7
128 256 64 0 2 1 0 8c5d1bb6457e67d1a10c5a0ee685d742a915c4919779ef12b59795a7d2fac774
128 256 64 0 2 1 1 8c5d1bb6457e67d1a10c5a0ee685d742a915c4919779ef12b59795a7d2fac774
128 256 64 0 4 0 0 34798b22aa1893d7db44c315441feecfb22dfbed1f245362519d1e70a9b9299e
128 256 64 0 4 0 1 34798b22aa1893d7db44c315441feecfb22dfbed1f245362519d1e70a9b9299e
128 256 64 0 4 6 0 701e33e050a92c039b6a07a228cfda642ebf2ebf23f28eb85883f469374aa378
128 256 64 0 4 6 1 168cf9b96badaf7ce2294c339cb5fccd295b533dfd6c51cb85721bda9ae03a3f
128 256 64 0 6 0 0 8237d50059afc5a9ac4af9d8d1a1fd306716a234360251a2046906c0513581ae
128 256 64 0 6 0 1 8237d50059afc5a9ac4af9d8d1a1fd306716a234360251a2046906c0513581ae
128 64 128 0 1 0 0 84b2ecdf53d5690d8d0fc82ae251fe3722925f4ad88db2229df65f01da9a6ff3
128 64 128 0 1 0 1 84b2ecdf53d5690d8d0fc82ae251fe3722925f4ad88db2229df65f01da9a6ff3
128 64 128 0 2 0 0 c34fa4914df2b9e78c4719966cf6ad8d4a8e34238bf2daebc8aeea72a6a91f83
128 64 128 0 2 0 1 c34fa4914df2b9e78c4719966cf6ad8d4a8e34238bf2daebc8aeea72a6a91f83
128 64 128 0 2 1 0 9ecb99e4f132ac43e9b912e8eddb19b08d077902b7bdfc6267dc6b08e854fc55
128 64 128 0 2 1 1 9ecb99e4f132ac43e9b912e8eddb19b08d077902b7bdfc6267dc6b08e854fc55
128 64 128 0 4 0 0 c649ede65c25248e2a038c470ed796e1b325299d3dafbe84b36a4b1e46273149
128 64 128 0 4 0 1 c649ede65c25248e2a038c470ed796e1b325299d3dafbe84b36a4b1e46273149
128 64 128 0 4 6 0 aef394515e4c75b69c888471c92e43f761717c0b502308fac7e157be3b286f4e
128 64 128 0 4 6 1 c30e85b81cd22b9cb36251b86f5e243627adeafdcc4eab1418b614e179bb3596
128 64 128 0 6 0 0 31d172351ea9896fa40f66d0db0830bd1f06dbc16ddadea04b18b696be812bbb
128 64 128 0 6 0 1 31d172351ea9896fa40f66d0db0830bd1f06dbc16ddadea04b18b696be812bbb
128 256 128 0 1 0 0 72499965592fc20517d3ac848d2b9fe5a803ae49f31ccce6faf5ed18dffd9810
128 256 128 0 1 0 1 72499965592fc20517d3ac848d2b9fe5a803ae49f31ccce6faf5ed18dffd9810
128 256 128 0 2 0 0 daecd11ca30c3c3023d0cce9b4f3ad87acb4293a478bec8fa57005921d33fea1
128 256 128 0 2 0 1 daecd11ca30c3c3023d0cce9b4f3ad87acb4293a478bec8fa57005921d33fea1
128 256 128 0 2 1 0 21e97fe4e4a00d74c96cd9201b6b19ecbbe40c471f74edbef4472969a5fbdc47
128 256 128 0 2 1 1 21e97fe4e4a00d74c96cd9201b6b19ecbbe40c471f74edbef4472969a5fbdc47
128 256 128 0 4 0 0 6496b5377dcd2d580905559da1e65084b19e05ddeeb5e6ce3220d1fb34edc4a2
128 256 128 0 4 0 1 6496b5377dcd2d580905559da1e65084b19e05ddeeb5e6ce3220d1fb34edc4a2
128 256 128 0 4 6 0 cc8a62d7ab8ff7ca8de84c18ba9f89faee2e60e6f7e387b034af571f14303c49
128 256 128 0 4 6 1 cc8a62d7ab8ff7ca8de84c18ba9f89faee2e60e6f7e387b034af571f14303c49
128 256 128 0 6 0 0 3cb3caaf39feeac08fee7e20219f55dbe3d4e66e795a76ef30d4dfeca97b651a
128 256 128 0 6 0 1 3cb3caaf39feeac08fee7e20219f55dbe3d4e66e795a76ef30d4dfeca97b651a
128 256 32 0 1 0 0 776c9828e6c9474f3223d13854fb3613fe2866933638645c4ebea73a1db75bc8
128 256 32 0 1 0 1 776c9828e6c9474f3223d13854fb3613fe2866933638645c4ebea73a1db75bc8
128 256 32 0 2 0 0 04eccd8d0af0b562002aeeb45badce548a0eee0c0b50abf12c648fc557e2c0fd
128 256 32 0 2 0 1 04eccd8d0af0b562002aeeb45badce548a0eee0c0b50abf12c648fc557e2c0fd
128 256 32 0 2 1 0 0e82822c7df34df058c8535719044f644d5ada1474ed551043c9c0e60f1c21e1
128 256 32 0 2 1 1 0e82822c7df34df058c8535719044f644d5ada1474ed551043c9c0e60f1c21e1
128 256 32 0 4 0 0 f58f54ceb9a9921a1ccb9dfeab1633507e49516a838acacbcd77f2007ce0b5b0
128 256 32 0 4 0 1 7702cbd1a8adbc759e8b20d3513ac9821402e229cce5a2e5e82502c18955fd85
128 256 32 0 4 6 0 a401c9115f0d6484d1494e11c983a25911b7c03f8899fb477561167c81ba34f5
128 256 32 0 4 6 1 96d522646de395f90c8cd5e187d6d531c5c9bc7583f5eab77ee14ecbb89fb7df
128 256 32 0 6 0 0 3a323b8477f01b976c56d5c1b221ce8caf04188870c60f250de304d4e9f05272
128 256 32 0 6 0 1 485ff1d664cb4483db7be294c4c512effa73b79b1791b0916b5d5635abaaebd7
128 256 16 0 1 0 0 af97498408ec06fc7203ed6ee175b26f184e47181f6d17be95a17a1e06793df3
128 256 16 0 1 0 1 af97498408ec06fc7203ed6ee175b26f184e47181f6d17be95a17a1e06793df3
128 256 16 0 2 0 0 1d8ef7925a6a2e02a6830fe281656a4527c74c3f693bd834a873daf6e9b20858
128 256 16 0 2 0 1 5f6b61ea59c00b90ed73048bbb4d34044495d2741ada63d359eefeb0448d180a
128 256 16 0 2 1 0 630e6a851c6f7187b2cf6ea330da16c4f6d0033bfda2d482692dfb5d8c74c202
128 256 16 0 2 1 1 1c2a20af7610175604148d325d258e1c504d5613c3be0300ca3f58df7028279f
128 256 16 0 4 0 0 e1a369943568a878f248092680c22c069df71ae145de3b3a33dc3c8b733744d2
128 256 16 0 4 0 1 6b878cb79d993fc6788ab63013d7e72374fd7c68017c402478fa6ef5b948f142
128 256 16 0 4 6 0 1f41f3e2c3e35f142d5fcc49299eb3c70c204aaf01e25976a96af0d98e139881
128 256 16 0 4 6 1 c0bc1f448640aec2286b511697163234996d3f4f13e830411061f2212e18dba0
128 256 16 0 6 0 0 ca4076268eef9839063926ba5e4fd931c704e6269d4d02ed92ef70f6158a230b
128 256 16 0 6 0 1 9585ebac6738408ce059e66f0ce880c3e8578a62e568db85bd42b2ba1d5fadaa
128 256 64 1 1 0 0 c9bdc4b623fad601db24d4bce34e19e1820728b0671ba7c8a9c94a5f6ea0e436
128 256 64 1 1 0 1 c9bdc4b623fad601db24d4bce34e19e1820728b0671ba7c8a9c94a5f6ea0e436
128 256 64 1 2 0 0 083539c19e51da409b4f653221369ae3ba37b3d6300867c35032ad3c96187ad2
128 256 64 1 2 0 1 083539c19e51da409b4f653221369ae3ba37b3d6300867c35032ad3c96187ad2
128 256 64 1 2 1 0 3013d543ffee204ae35a3d9747802b53fa58ea9882f8d57e2edb0cee07273171
128 256 64 1 2 1 1 3013d543ffee204ae35a3d9747802b53fa58ea9882f8d57e2edb0cee07273171
128 256 64 1 4 0 0 55fd6cce8bcd50994d95cacc9ca290f23247bd7cdab86ceda3bce0eed142e888
128 256 64 1 4 0 1 55fd6cce8bcd50994d95cacc9ca290f23247bd7cdab86ceda3bce0eed142e888
128 256 64 1 4 6 0 d40c37eb28003377f89ddab71263bc78b6cec35d13c7e1ed08f81b70b9bb5c4d
128 256 64 1 4 6 1 d16b5e17b4e3291601afa7755dab4d005c6fb924132733dcf2cea02f4e2d1efc
128 256 64 1 6 0 0 9636189a78d828cfcba1af35949dfc3b67efb59757d6874141fa16b33f816d01
128 256 64 1 6 0 1 9636189a78d828cfcba1af35949dfc3b67efb59757d6874141fa16b33f816d01
128 256 128 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
128 256 128 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
128 256 128 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
128 256 128 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
128 256 128 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
128 256 128 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
128 256 128 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
128 256 128 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
128 256 128 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
128 256 128 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
128 256 128 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
128 256 128 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
128 256 256 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
128 256 256 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
128 256 256 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
128 256 256 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
128 256 256 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
128 256 256 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
128 256 256 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
128 256 256 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
128 256 256 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
128 256 256 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
128 256 256 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
128 256 256 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
192 256 256 0 1 0 0 6e3fb0f5d86c3ca0541122a282266123949d9660e026c27a5b1df087e8aa7693
192 256 256 0 1 0 1 6e3fb0f5d86c3ca0541122a282266123949d9660e026c27a5b1df087e8aa7693
192 256 256 0 2 0 0 c76d41b7e0d9015d7b40458e23dbb3371b41e4087cf9f2b94440bdcf8fe82ff9
192 256 256 0 2 0 1 c76d41b7e0d9015d7b40458e23dbb3371b41e4087cf9f2b94440bdcf8fe82ff9
192 256 256 0 2 1 0 b0af19ee6a6f32d496b947b64e535f7c7d6ff99f3d0f58c58563d1942127aa3a
192 256 256 0 2 1 1 b0af19ee6a6f32d496b947b64e535f7c7d6ff99f3d0f58c58563d1942127aa3a
192 256 256 0 4 0 0 2bbfd090acb43b1ab3f17ba72976f5d9c833d4d09a280618e0d6bd44d56f2e97
192 256 256 0 4 0 1 2bbfd090acb43b1ab3f17ba72976f5d9c833d4d09a280618e0d6bd44d56f2e97
192 256 256 0 4 6 0 90f1f7d6e91d4830ad3b1274ab69781f528674616a06f9aa84b2a227193170fd
192 256 256 0 4 6 1 90f1f7d6e91d4830ad3b1274ab69781f528674616a06f9aa84b2a227193170fd
192 256 256 0 6 0 0 043a0c9cb3e210f28231e57103ca4d07c2a0b536658f71a0e23542531c49f263
192 256 256 0 6 0 1 043a0c9cb3e210f28231e57103ca4d07c2a0b536658f71a0e23542531c49f263
192 64 64 0 1 0 0 471e516b2263ef50f25e94db908c33240ead6ffb0f6a96e839c7b10a1679dea4
192 64 64 0 1 0 1 471e516b2263ef50f25e94db908c33240ead6ffb0f6a96e839c7b10a1679dea4
192 64 64 0 2 0 0 859596162113a3d8a61f7eb2eed7f89ac701a2b0fd8fc49c9eccc5978caca780
192 64 64 0 2 0 1 859596162113a3d8a61f7eb2eed7f89ac701a2b0fd8fc49c9eccc5978caca780
192 64 64 0 2 1 0 1c4362515fc6e1778f9bd1f1dc5d45e642c8a376574d7d42d5831e0ba0d16734
192 64 64 0 2 1 1 5e1f665e7086f115597650727296ca2e0cc4eaeb1b294d4b8f5c8ff78f3b1f1a
192 64 64 0 4 0 0 583b2f0fa2f6ddec333d020c50d5c3e829cb6e073ca6da81e5fc98c29d1c2bf8
192 64 64 0 4 0 1 0f92ac46c394adba62f3a5a831cc9a941fac26815032c2304844983c2cf786c3
192 64 64 0 4 6 0 9df7c9e7d5c2584ecddb2d65a774a0720a59b38add3b68135282556020358031
192 64 64 0 4 6 1 3c026f2b1cf6766baf0b24ade4f61cb4a622a6460127e6f29c348fb82a755d17
192 64 64 0 6 0 0 eb2be9cc21285e53a080e9ba7d83c8457c523c7aba73fb9e74a6c9ac9d2088f3
192 64 64 0 6 0 1 6475891b2113b1889d0ba5398a6947fefd7fc2e4f91689ccfbd02b7a2c2cab4b
192 256 64 0 1 0 0 74fc1a74ff11e94a05a10e5bc2151d9cb5b2c98979ffa8694774496b9cf5542d
192 256 64 0 1 0 1 74fc1a74ff11e94a05a10e5bc2151d9cb5b2c98979ffa8694774496b9cf5542d
192 256 64 0 2 0 0 6f596521f396099f0dc513a7ce4d6259433a81a335a96cb1d214b86cfdec6277
192 256 64 0 2 0 1 6f596521f396099f0dc513a7ce4d6259433a81a335a96cb1d214b86cfdec6277
192 256 64 0 2 1 0 63101689db15bbf306ef96a3899e0e5a1a898cd92ddcc3cb9e2db956dad1aed9
192 256 64 0 2 1 1 63101689db15bbf306ef96a3899e0e5a1a898cd92ddcc3cb9e2db956dad1aed9
192 256 64 0 4 0 0 fa06839ac7a337af9464564268b5dfd9ea96b3951f1c711eb517558d2329d91d
192 256 64 0 4 0 1 fa06839ac7a337af9464564268b5dfd9ea96b3951f1c711eb517558d2329d91d
192 256 64 0 4 6 0 1a6ff372d55b6cfa0ee826d0161d1bfcd22a05c218a4b478f545a4caaf4911b7
192 256 64 0 4 6 1 0b049d160e401b6db0702979f0d62f1286c44ed0ea8187e76741491c81b147aa
192 256 64 0 6 0 0 fd3bc78b681f09582b60574152febbbd2e044e95e6a8dd3d6cd1411f7e07ae8e
192 256 64 0 6 0 1 41a78d61fbe40d333dbbbf4686019b08ae2312e3d078961410a7cf0da4cdd806
192 64 128 0 1 0 0 bada9f986cf7fd1d5c65ab7f7da777bedb0768db4968ca724dbe062ae57c25d3
192 64 128 0 1 0 1 bada9f986cf7fd1d5c65ab7f7da777bedb0768db4968ca724dbe062ae57c25d3
192 64 128 0 2 0 0 5417b229c3bdbdf480822e79a38e7f7ea61a0b35ccfc37a05968df3d145b7ad2
192 64 128 0 2 0 1 5417b229c3bdbdf480822e79a38e7f7ea61a0b35ccfc37a05968df3d145b7ad2
192 64 128 0 2 1 0 512e1191396e7fd1b73983eb7d528c36761fe3175a8d88c64f0c7da21662faac
192 64 128 0 2 1 1 984d98eb6f0b12a8cc14f49628e56a9915915fe55d3155f044d6fa713b23fcc8
192 64 128 0 4 0 0 5ebffa29919d9c4aa73229517fffc91191c74f87435b1bdbb63c07d98b0683fe
192 64 128 0 4 0 1 406cfe7124a0bbf0ac48860defb51be83e899a7141dd64c2d4c9810e73359e54
192 64 128 0 4 6 0 7414abb92b459f7925085142474d442d77be03916b239c50763757458614d2a5
192 64 128 0 4 6 1 eaeb4c9eac378d77c81529c8fee8dd093a1af878386764ca0e028b78e73c33fb
192 64 128 0 6 0 0 1149e07784bbae60228e1cfc0ec038c5b1f700025f25ce80db46a787a4827109
192 64 128 0 6 0 1 36f733ad777f104c7403e1d1c3e9a1dc319a0ed828b92b2944a80d3dbe953bbd
192 256 128 0 1 0 0 29377dfae8580bd2f0f5dc25901acc7216a8d76a3e1f9eb4f89c5e05a61043fe
192 256 128 0 1 0 1 29377dfae8580bd2f0f5dc25901acc7216a8d76a3e1f9eb4f89c5e05a61043fe
192 256 128 0 2 0 0 17f107852812f47ea159d720b9e1b1ddb62aba3f1fed834bdf89c43ac3d77c55
192 256 128 0 2 0 1 17f107852812f47ea159d720b9e1b1ddb62aba3f1fed834bdf89c43ac3d77c55
192 256 128 0 2 1 0 5699d526b80642e88d40632578949bac8656652b75122bfea5d956b0c10da18f
192 256 128 0 2 1 1 5699d526b80642e88d40632578949bac8656652b75122bfea5d956b0c10da18f
192 256 128 0 4 0 0 e5b9e74bedb4d69f61d2f64f71092c587a4ec530f24bde5cb9ca058a4ba93554
192 256 128 0 4 0 1 e5b9e74bedb4d69f61d2f64f71092c587a4ec530f24bde5cb9ca058a4ba93554
192 256 128 0 4 6 0 63ae677312a46f5fc70997cc2bd93750b116d6e391fcc607f474648e5eb6c2b5
192 256 128 0 4 6 1 caa95ef26aa03d7ea039cdaeb483a389906af1b2ba53ea9bf875e3cf7da83d5b
192 256 128 0 6 0 0 a0530e99e6df50cc0b6d7f772e680be7b508b312e3a35fe64d580ed48d8854b7
192 256 128 0 6 0 1 a0530e99e6df50cc0b6d7f772e680be7b508b312e3a35fe64d580ed48d8854b7
192 256 32 0 1 0 0 7320149308f532bc5c9a1db32739418bb76e1a30ff7de341b88c8bf596dc8d75
192 256 32 0 1 0 1 7320149308f532bc5c9a1db32739418bb76e1a30ff7de341b88c8bf596dc8d75
192 256 32 0 2 0 0 a59d80263a3ca95d37184c8217d361fc130e51b1a55d03e76cdab378238a12ab
192 256 32 0 2 0 1 a59d80263a3ca95d37184c8217d361fc130e51b1a55d03e76cdab378238a12ab
192 256 32 0 2 1 0 675189133bf461726be79ca70684d1b88150ac7fa44892d87109a61ec41857b2
192 256 32 0 2 1 1 d7784c55a60c5404a9c39bdd51cf2a27469d0bacd421dcdf76d06c2a05f99f4c
192 256 32 0 4 0 0 c474674028628ae6f180bd63ac0af10f150dfb935c8637aa4d5086bd2e7f6709
192 256 32 0 4 0 1 e50abe6454c49e68f38a371b25e64eedd069cc6a63140069128d6c329728d269
192 256 32 0 4 6 0 ae6808a9f8e132681b2651c93e0f5842385e5623c9781cbe7f0a7b014d6edf18
192 256 32 0 4 6 1 69e8d03b566042d1cf2a12507f7beb23d5fb34397bd0257843967d0c29213e8e
192 256 32 0 6 0 0 1d0a7d10f87bd2888e6633c9b6f3021d6ae9d35fb04b0528b08b7a62be6e7e3f
192 256 32 0 6 0 1 bb32c5ac193e24affb469cb0a20f4bc54cbe2aee944e19a8367835f251b2f0a7
192 256 16 0 1 0 0 39b4974f42e4d48767a137e7108953d3e506487b76d6ef412bd89bb18072bc4b
192 256 16 0 1 0 1 39b4974f42e4d48767a137e7108953d3e506487b76d6ef412bd89bb18072bc4b
192 256 16 0 2 0 0 f08855b0955acdd9b007a86f90ad1b873814d83ffd6badee2d1f706d0c6654ce
192 256 16 0 2 0 1 d17db13a9a6b1acef33224fa4b7ff2ec653674c3fe88474f8a04ce33f35a32ea
192 256 16 0 2 1 0 ee997c2e0848ec5edf4aa51fbfc4a4d92605b00d2fa7194a693511bff1582e9f
192 256 16 0 2 1 1 25327201b96ba7d30dcb726c7507e8406455f4f14a217013d03287ba1f56eec0
192 256 16 0 4 0 0 59ded83d29dce5b4baa68a7be7c9f6e459a184aca73bec47d8ac8a252401a9d3
192 256 16 0 4 0 1 1cc71f21501f3bdb1869a65c254798f7cfc8d7126f985ce9a832c3ca950f157b
192 256 16 0 4 6 0 c75c458cf2183a6f3c80b43e173a30526864d3c30b5a5a6da03f1098c4e8454c
192 256 16 0 4 6 1 37ca33284ec076aa03e29af4c0b725f145a24e4dc46cd92d0cb872c2c1ab9ed3
192 256 16 0 6 0 0 16f37a2ebe554d44ec9193cb4209a794d83e7a528c170be70aab621c83cea30e
192 256 16 0 6 0 1 3a939af02b08d1cfa50eac1a0b641aa0d0e4f30052800d6c5d13acd326585d0e
192 256 64 1 1 0 0 c31fda143f28de371367ed75236977050269e7a2f18b9c7715ac81038886c21a
192 256 64 1 1 0 1 c31fda143f28de371367ed75236977050269e7a2f18b9c7715ac81038886c21a
192 256 64 1 2 0 0 6b359a923efc1778c046a9ed020aab5143729e50c02c2c25c828f7b741befb4e
192 256 64 1 2 0 1 6b359a923efc1778c046a9ed020aab5143729e50c02c2c25c828f7b741befb4e
192 256 64 1 2 1 0 07bd121d9b66718e6603c31bcb1f8e236da8a2c5dedc7eae15440493ab67b58f
192 256 64 1 2 1 1 07bd121d9b66718e6603c31bcb1f8e236da8a2c5dedc7eae15440493ab67b58f
192 256 64 1 4 0 0 3331b36e3bbece835c7dd117a2668a14a395f36ed3ad547110672f1c7204517d
192 256 64 1 4 0 1 3331b36e3bbece835c7dd117a2668a14a395f36ed3ad547110672f1c7204517d
192 256 64 1 4 6 0 edd83d96894331b1c5d2a5c8d1f80188652bd5c6dfafa6ab21514fddef3c7971
192 256 64 1 4 6 1 fe949ee4afc54f31e994aa59471f131d04baf1381429fae81f18e24b14ef7db3
192 256 64 1 6 0 0 4f735c63a35ecb85ac596f30e8f17b57be02b095b7bf11d8d1a6f79498af2157
192 256 64 1 6 0 1 7a685310fedd9112b4a0429cab70bf9f37e21691b943b10b0564cebc077af67e
192 256 128 1 1 0 0 e7e18fef1797647da5138682c2a9c46fa5fe9acee31f8b05c8ba381dffc75885
192 256 128 1 1 0 1 e7e18fef1797647da5138682c2a9c46fa5fe9acee31f8b05c8ba381dffc75885
192 256 128 1 2 0 0 f086f222939c1affe6c4f75b4b576b5f9b28ea2a998565a81741fedbe90d181a
192 256 128 1 2 0 1 f086f222939c1affe6c4f75b4b576b5f9b28ea2a998565a81741fedbe90d181a
192 256 128 1 2 1 0 2b59dd4ef3490f197faef530ad1c3323af14cf750f4775429f6ab3f001c11c2d
192 256 128 1 2 1 1 2b59dd4ef3490f197faef530ad1c3323af14cf750f4775429f6ab3f001c11c2d
192 256 128 1 4 0 0 7652f5c730f5c312313dd8dd05c5b8aa5eef99d0c559e323042a54d91df7c393
192 256 128 1 4 0 1 7652f5c730f5c312313dd8dd05c5b8aa5eef99d0c559e323042a54d91df7c393
192 256 128 1 4 6 0 ba5a69f8a35be12ed859b8b9ed0b607a3efe2cce5e7d96743b581f6a3b9dad57
192 256 128 1 4 6 1 24ee1fd32494e9d46ecdf7eb33c17516c1686ca5b29b45dd9fa81cdaea7067b9
192 256 128 1 6 0 0 5a7af9fe277247e85ad93d597f9089159cc5d18717c0fc98d8d65884fa519ba4
192 256 128 1 6 0 1 5a7af9fe277247e85ad93d597f9089159cc5d18717c0fc98d8d65884fa519ba4
192 256 256 1 1 0 0 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
192 256 256 1 1 0 1 6397b86b4e7e529c04f66db1e3f6ee34c441900e12c59f809e48216cbde707ba
192 256 256 1 2 0 0 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
192 256 256 1 2 0 1 2e637168e737801db2a1700122d65071c042d23fb7f30aa5ec772a83be181b6f
192 256 256 1 2 1 0 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
192 256 256 1 2 1 1 ccd28ba419e660459758fd6849082564006ebbccd24105a3b71fb00a0b0473ad
192 256 256 1 4 0 0 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
192 256 256 1 4 0 1 5a53f7535e898a8df7008088f38d810da60c202a497542d364ba2183d475a276
192 256 256 1 4 6 0 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
192 256 256 1 4 6 1 4d3bcd258b62b4f20609b2a7e706b51e2b9f8ff220a6078ee99555e3a1a02288
192 256 256 1 6 0 0 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
192 256 256 1 6 0 1 c3bcf25f430f6eb1fbcab979f6fc0b9d7dc87e4140fa3631ecbb1e34596fa067
320 256 256 0 1 0 0 5e5069bc2fb7728502a306c4b8dae29b0b9d8d06f3243498a27bd951c3fb81c4
320 256 256 0 1 0 1 5e5069bc2fb7728502a306c4b8dae29b0b9d8d06f3243498a27bd951c3fb81c4
320 256 256 0 2 0 0 bd1f0cee5570105f3030f2103f40a53c5b6df1cbe02ed929afd8b31e3e4a0147
320 256 256 0 2 0 1 bd1f0cee5570105f3030f2103f40a53c5b6df1cbe02ed929afd8b31e3e4a0147
320 256 256 0 2 1 0 fd5a516c88ce521a5239b6d279c7eaa2cb24de34facf2dfae00efa948cee496a
320 256 256 0 2 1 1 fd5a516c88ce521a5239b6d279c7eaa2cb24de34facf2dfae00efa948cee496a
320 256 256 0 4 0 0 f04f76f3065850e1dc816d74790823cfa0be0e4d88b9d22e1c3b4826952442d3
320 256 256 0 4 0 1 f04f76f3065850e1dc816d74790823cfa0be0e4d88b9d22e1c3b4826952442d3
320 256 256 0 4 6 0 8b26bb21777d67131e1311dc4e288f524f96d156732b3a98053c016fcdd78b1d
320 256 256 0 4 6 1 a077e2325d3f4782ce6d2e075bcba7223a53728a4187a66379e518eec3dc4043
320 256 256 0 6 0 0 b32094bd0593a1a2af73de631f08e0c878675453906edcbbfe3ac51f0ca8adad
320 256 256 0 6 0 1 8a3ab1ea07405526a64aefd82f313657e305c83a874215102d6d1c97a7b9c069
320 64 64 0 1 0 0 9e10e4546f577c405b7368e258f7e41c9c03c169adea22cdaa4149f8a109c0d1
320 64 64 0 1 0 1 9e10e4546f577c405b7368e258f7e41c9c03c169adea22cdaa4149f8a109c0d1
320 64 64 0 2 0 0 4ad11a21f7b3e008c0ce2d1e389968ff3fac8a74cae7b6033e825b122b8beea8
320 64 64 0 2 0 1 79864852a66010ada0084fa8256fbe01133ce41bebb88cda9e3b435f02848040
320 64 64 0 2 1 0 87759eca581f64851819139e50f1aab5c8b36e9e89d4146648df1a08c3c1f56d
320 64 64 0 2 1 1 d42426bd2cb2a92b4723ee4281f550f9578ab365b7b25d45d017132de426a7e5
320 64 64 0 4 0 0 026ee503a7a4ffba6b17613202112442e45bb49c725071edf62d96d333671197
320 64 64 0 4 0 1 e42cae9e09b20f420977c80982bb3a57a4a19cf7c52ace2234adff8142c79563
320 64 64 0 4 6 0 957270cb7d465436272fa11269f031f98d86b31e986e54ae7c6397e706bb1086
320 64 64 0 4 6 1 a81f07ec4168ada3c5a8de672e41e563c370f64d7065678b62a9ede08e3ddd94
320 64 64 0 6 0 0 43575b4375a73545ff0044d5018c21e2aaa8d5c3d6e51c07e6c3f59c896f7620
320 64 64 0 6 0 1 4bd34ec19ccad1fd5c6316ac2f14c78e9b532c92263656e810993a9b7323da71
320 256 64 0 1 0 0 742ad72b9d46b1159a8368d45a6496b77db56969ba0de784626ce0942a497e7c
320 256 64 0 1 0 1 742ad72b9d46b1159a8368d45a6496b77db56969ba0de784626ce0942a497e7c
320 256 64 0 2 0 0 3073ad6ccfe8676ac2ec97efdfcc05776da2a5d1c1a31d0d535736f48bc9e0f1
320 256 64 0 2 0 1 3073ad6ccfe8676ac2ec97efdfcc05776da2a5d1c1a31d0d535736f48bc9e0f1
320 256 64 0 2 1 0 eac7b9c3f1a95e96d7f28722e0442365037168ff17d0c34dd26c69da54a7435c
320 256 64 0 2 1 1 6cdcc8e0566e100b6ecf679151b187a80135b349bf7cc14b66af041badb0e35e
320 256 64 0 4 0 0 5cee1b1044a153bec03b08199ee36382a62063de35a63b7743a3e43046bedc45
320 256 64 0 4 0 1 397da817af54f40c1b06eaa1101b16c8fe0ff5eb59b569603c939355a6e1483b
320 256 64 0 4 6 0 8ca171cc948c167931f5f53c4c7627b667a57957afb69d79f385c67999a4c2b8
320 256 64 0 4 6 1 2f9726e23cfdf5569a6a29dc05bc1586ba6fa163fafa29460dbd4b46c06a65dc
320 256 64 0 6 0 0 97e1d13a1f61be2b624a2b57906cbd54c970e237f24444e1e237f9337326644f
320 256 64 0 6 0 1 3a42dfad3607efe971238cc483127beded12863a63628e6545d2925eb397b874
320 64 128 0 1 0 0 5ff6d7bfe7bc05735f976dece68db4c6d6b9b9448d1eb5767f49ba37ee4fc74d
320 64 128 0 1 0 1 5ff6d7bfe7bc05735f976dece68db4c6d6b9b9448d1eb5767f49ba37ee4fc74d
320 64 128 0 2 0 0 9bd342e77caccd79515e2fb751d06911a0757e93170ed9defce6c164b6f1ebf5
320 64 128 0 2 0 1 2c21dad96be4bac44bc91e9f41fda6f6015c78eb8f11bb8dd6ebb3ad3c0756bc
320 64 128 0 2 1 0 bef6865a4d3c275ea9d3ac9aa32dd11a78b60610c62013a8446423a8f756150b
320 64 128 0 2 1 1 cbd2b7db91ee72dac4ab838b8a23b6aa2ba3a2b2c77d2310eb7dc37ed81c9977
320 64 128 0 4 0 0 d188fd85ed04c412fbf8dc85f1e4928f074d41237c564f61a58c08bb84e0759a
320 64 128 0 4 0 1 514d88a1f4cd9007c24a07d82a9a6ce18825f022724fd7706055f769e41e6aa5
320 64 128 0 4 6 0 11373f4e8445808877271e7cee1e14e192cedfbc4ff1ce5e6d8e17cec5c32a8a
320 64 128 0 4 6 1 be497e143d44a5a9b4b6e27b6dfb6c2c32575573228f918d54fa82f74336bfa7
320 64 128 0 6 0 0 32a6ebb32066779ac4e08d87922e9aaa67b3bf6f21f4c6e43dc25309283e61ba
320 64 128 0 6 0 1 d121115975ea3e4ca71bf10a37e102972875d6cb74c630da182d5b169d8b3be1
320 256 128 0 1 0 0 e2a3a942dacaaa1e1f00395bd292b649604e130180fc38e17fcd60545b0e9bc5
320 256 128 0 1 0 1 e2a3a942dacaaa1e1f00395bd292b649604e130180fc38e17fcd60545b0e9bc5
320 256 128 0 2 0 0 443e3b0b66676f1a854451f00de1c55259d8c0c6ac902aa5f7b36e7adaa36ae3
320 256 128 0 2 0 1 443e3b0b66676f1a854451f00de1c55259d8c0c6ac902aa5f7b36e7adaa36ae3
320 256 128 0 2 1 0 e15d0788211618adf576f6e6fb38ead378075a9fcf01d8d6b560e45b6985c1ac
320 256 128 0 2 1 1 e15d0788211618adf576f6e6fb38ead378075a9fcf01d8d6b560e45b6985c1ac
320 256 128 0 4 0 0 3e984181a3038d18eed0cdec38849a7cdc4d2fadcc2bcdee1f380887d098e7c6
320 256 128 0 4 0 1 14614e73af74ea9752c535f990d25d653c75e19175c944ed7b01604442b8c2fb
320 256 128 0 4 6 0 f54074e995e835e1e4068c38f546e94aa987d99f2bcec572fec1891227f47ba0
320 256 128 0 4 6 1 db5d03a87a80700a7e0f69f9c1c3ddb1dd569784a6ca13392ad99ac4ad576f41
320 256 128 0 6 0 0 9af52db9a378b842c68ba76b8fd6b7bc62d0e099b4ec59f5807dc2a917b8d05b
320 256 128 0 6 0 1 1984e71204ab0a1011feb3a08803d8210fa1fcdcbbc6110aa422f9ac2e56f651
320 256 32 0 1 0 0 238a87189583d35c2acc5980239db0c09b4550e939966d7232e6871244a179af
320 256 32 0 1 0 1 238a87189583d35c2acc5980239db0c09b4550e939966d7232e6871244a179af
320 256 32 0 2 0 0 d14895ce31e6a3f41bc7ccf6cfe8de5d1877f447a2b67ee0d21dc454f315a468
320 256 32 0 2 0 1 0baddfdd49471cfaf3d7115a92b5bd1b24bb930f23701ac01ce66b82f1badd41
320 256 32 0 2 1 0 0648995b26e2c4cce9041a505a98b23a0f569b0463da39ca51832570313897a0
320 256 32 0 2 1 1 0641954a0ff52494937757a06b4d12daf66a2932f09369afc4929aad0272c4c5
320 256 32 0 4 0 0 c5859a90396fd553ead28b257f38625b1532474599c067f249bb0f4244126821
320 256 32 0 4 0 1 d7ab7e4d87a28a24d06b52dee5060dedf1d603f1b24736ccce08db2bd8c9bb4c
320 256 32 0 4 6 0 4b83a08669e3ab9238ea9ad3e977206d08a145cc0da89199059c319be682b340
320 256 32 0 4 6 1 443382e6abcbad187a92b026b4efbf9191655a59ea2990ee8eb5fde39a23cbb5
320 256 32 0 6 0 0 1ec469e6707622ebcbf04f76694fb9082dd27f3439a5fde84d3a834df186d524
320 256 32 0 6 0 1 314de64c9478cc3d0ec6c5d186a45b3eaffaaba323eb2991146f4dd0ba96f87c
320 256 16 0 1 0 0 b8905f03a2ddb0fea432fa8e684b1702155764374c9ce73d74bb95130b6dfc3e
320 256 16 0 1 0 1 b249a6b6573fb350cf0ff372460c3e4fdad88d1d00afc6ac1b20306a53e07c4a
320 256 16 0 2 0 0 a2e6c9f245197543e5a48ff3155bd72f667bf5a6fd653e7085dcfa1cadd8ea9f
320 256 16 0 2 0 1 cac183413baaccd112a0b4832434e8e8bcae6e77175e4ec8ef6718f9d5fcbef1
320 256 16 0 2 1 0 6fa10b01db205a5720b8a62f64ad4d32fd849f7c7e6d6a2c5a9ef1c2079dd7d9
320 256 16 0 2 1 1 8494e5f89c90ba3ce0933fc4db49c3fd6c007a0d7ef83a1e16b93e898e1f45b7
320 256 16 0 4 0 0 f5fd1411de8d6f3a5118a33d34237ac5408f6274a324c0fbda7db932dca6ea9b
320 256 16 0 4 0 1 1987beb99bf3364d5d173858c3cd0873f8adb598c44aef966aecce0a90672a6f
320 256 16 0 4 6 0 a5e7e06b52f4975d6ba3214cf15df61ed4913a85c7a084dd41e289d91c68b760
320 256 16 0 4 6 1 71817aee16f6e800b14cf5d7025182ef2cdd528fd8432da6aaa03761ebeb7dec
320 256 16 0 6 0 0 39bce6e28ef48596e0c43392d38ce967862650440e88c82681555b6baa4f0537
320 256 16 0 6 0 1 31f65fa67fe521d7371f79adea316d2c769f0ebfc3ce559deef080fbf0cbea3f
320 256 64 1 1 0 0 b0606691a85b0611bedf9af87ca43e19bdc69de9e448eae0d97c4643178e04c6
320 256 64 1 1 0 1 b0606691a85b0611bedf9af87ca43e19bdc69de9e448eae0d97c4643178e04c6
320 256 64 1 2 0 0 3000d0fa900b28a58e04a840535ba1ae11c37e33d6120f3d46a260f7cb90afda
320 256 64 1 2 0 1 3000d0fa900b28a58e04a840535ba1ae11c37e33d6120f3d46a260f7cb90afda
320 256 64 1 2 1 0 43be495cf5db6982efa293fdc3f3126d4c4d85f32023c6dce6c7b334e1d7dbab
320 256 64 1 2 1 1 bcf72c4e43cb8cd26ef21591302ad526841c80d1e1be52c58be7b4958ac7fe77
320 256 64 1 4 0 0 7d83e2088b5bee6791c67abb6ea948f2c1ad6135afe414ca23acadece26a5613
320 256 64 1 4 0 1 066a7700fbb3d5c0c6ad83afea3822b1782b10fdd209672b70dff85279d9c307
320 256 64 1 4 6 0 c5abd04be8fe8e7b4af691678bb04dba3cff72b05237ef96f9f8cac0e8a5a515
320 256 64 1 4 6 1 2ba31c7a1ac0f165f0e906b0164a8e1cfdddf03888e643777a1f4471f115de16
320 256 64 1 6 0 0 8c9e2c2e9bb3ec0296e5df9156b3da60eda84a5d057985f309c4f4a518885bde
320 256 64 1 6 0 1 1b1065bf1e13d1f4b955657d8344e1c974565c01849d4ee7d7b80c1370e8a40c
320 256 128 1 1 0 0 5a63d93a91b0de33f959e80532d066fe58f139fc0152a30ee1c9a488b1b3ae7a
320 256 128 1 1 0 1 5a63d93a91b0de33f959e80532d066fe58f139fc0152a30ee1c9a488b1b3ae7a
320 256 128 1 2 0 0 2db4bb90688a2667a468768f156bc5a6b033abca4cceefd20a5dd0de5ecdf6b3
320 256 128 1 2 0 1 2db4bb90688a2667a468768f156bc5a6b033abca4cceefd20a5dd0de5ecdf6b3
320 256 128 1 2 1 0 c5701f25ee85c01e07d8e6b9f13e847b612adc405e3a16b4437df12c75b9ee98
320 256 128 1 2 1 1 c5701f25ee85c01e07d8e6b9f13e847b612adc405e3a16b4437df12c75b9ee98
320 256 128 1 4 0 0 75f9c2598ae3dc63deebf648a3615638a3780d2bce6ff9d93a98f3db57759f0b
320 256 128 1 4 0 1 ad1db5062e35edb2376fff1dcee53c1000a775037993e398e2145ac5a469043e
320 256 128 1 4 6 0 36f02a53316ffbeff87799b0a26f0907ac0ec791f57b7e6af4f6ee9bcd5e25b3
320 256 128 1 4 6 1 d4a4f7a484228f36ac458a14529d7ef7aa600503431f2c24ff1c4eb3ae9e12f6
320 256 128 1 6 0 0 6e3d14edad62af4475f8266b8b54fa0c2da6e943a39d04f31569fa9a2ac8db4a
320 256 128 1 6 0 1 910c8f12543f004948a9d2860461932bdfdce88b20394eaab13dc2dcff452eda
320 256 256 1 1 0 0 8f9e446173c9027981098631b8383d60fd4d9e24a9f00f7bd1fe05927c5091a9
320 256 256 1 1 0 1 8f9e446173c9027981098631b8383d60fd4d9e24a9f00f7bd1fe05927c5091a9
320 256 256 1 2 0 0 3fce66431bbced83f3943376da01427135bcc4f5bef6442cc8509a21aa09319f
320 256 256 1 2 0 1 3fce66431bbced83f3943376da01427135bcc4f5bef6442cc8509a21aa09319f
320 256 256 1 2 1 0 6fc49717b4d12e79bbf32895516334c3ec9af43d3c7a9356b042b61f33ec8e78
320 256 256 1 2 1 1 6fc49717b4d12e79bbf32895516334c3ec9af43d3c7a9356b042b61f33ec8e78
320 256 256 1 4 0 0 74a5f12c77bfa0bc25d9ee6b9f0663617c09dc2a160609fdda0111d542969710
320 256 256 1 4 0 1 74a5f12c77bfa0bc25d9ee6b9f0663617c09dc2a160609fdda0111d542969710
320 256 256 1 4 6 0 a2d0f56dce15ecd086a93187196ba313847d78e3008654b28ee1fda45146eb59
320 256 256 1 4 6 1 7500fb7ad35d409c8c99365694295565f930a6dd28309e9b87fe1f861f691559
320 256 256 1 6 0 0 1aaac8f0cf72436cb19ebc204078478c696fe438f9815ae11d40b2c9848371dc
320 256 256 1 6 0 1 b3ab46d4fa712abc80f2f8f28205e541368bfaf6eb7b0af208456c1acf7c2df5
1024 256 256 0 1 0 0 7d6295cef43e92abc020dedd4233720ae93b59af22928f1787fcb635b25c965d
1024 256 256 0 1 0 1 7d6295cef43e92abc020dedd4233720ae93b59af22928f1787fcb635b25c965d
1024 256 256 0 2 0 0 d0f41d47a2c83bd1e3bfcddd4a60b7e3b578e884c7a6e512a023fdb9484a0592
1024 256 256 0 2 0 1 fd06f2f1bbfb216c551e8a8514b5832fa8fa53444c07a81b26ae3f37331a463f
1024 256 256 0 2 1 0 de30a527851931d409adc424294c13cf64b8fcad5e6527c1befb1017540aaab6
1024 256 256 0 2 1 1 9f99e1df349f563f4be741d2d454e47222b6cfc978dc9c53a9a0a67f0d5c5a09
1024 256 256 0 4 0 0 84cd67fa5a1714146441b4f52dde777eaccba932f9598f5c561f927a4100cc77
1024 256 256 0 4 0 1 06a8269dcf332e2167ca0f1578ddd9ecfe4e7a5d7061e427f143d57c58b5bd5d
1024 256 256 0 4 6 0 8e42e8e23198d7ba6f0405dbad1bffccdb7a687df1975808adcefb803c524bb7
1024 256 256 0 4 6 1 4d49afe91aabffca0d9c758008becfc82e3e4dbad80366107035871ab49585c0
1024 256 256 0 6 0 0 86deaab349bbf7bd1329363bde85dc7342606e3600dba52d4347232e7a92c3c6
1024 256 256 0 6 0 1 2d176ea4737928a2fb0948a684e7092cd5332947658b63f8b9264a8d106721a2
1024 64 64 0 1 0 0 fe24e0a624a3c122ef1d32db88427e2d0bd22113ddc4445e08faa288858b8140
1024 64 64 0 1 0 1 2c07cba4d7fd89206ef0dd6640359968bc07fd9b7ab34a29335e26a37de95a36
1024 64 64 0 2 0 0 f3b4fd2da9be6c2bc075d029e91641be81930d463a7843805a3b55adfbad1dee
1024 64 64 0 2 0 1 75d4b1983ae1cab9740a53c9a7e4b24d6b57cd0df65994e08fe3deb2827ba08c
1024 64 64 0 2 1 0 afeb947ba367696dcbbc880b5b4735b2a21d586e8b3b2f2726a46cdf4de00707
1024 64 64 0 2 1 1 c81b65b0b5c036d3152f8b6b7061ceb68859498dc83d42ef6c31f1924e5fe6f9
1024 64 64 0 4 0 0 5274d5ea46a730bbce1bd6e56130e6da2e65c2b9336f41821a01f1af5fbce4c9
1024 64 64 0 4 0 1 cbb71a1ef0ca6f40090f3a5157542b732f0b448918b80bd2a0a4409be52a58dc
1024 64 64 0 4 6 0 3f5f9cf7c358edae19395d585d0ff837286c16cb46039fd3ebab7cca4d91ead5
1024 64 64 0 4 6 1 8d2fdd74b51efe5718ee846028ad47c7d0f0a794ea4b148d4db0721b67a80c0b
1024 64 64 0 6 0 0 86b09592c1fa27a9ac6525108fab415c6e1f3b3969ec91bc3e5563195289f029
1024 64 64 0 6 0 1 e6b7341603a6f77363f8a7cb262a505635d5ee1f178bfa975764312fce3b6b86
1024 256 64 0 1 0 0 db6cf436b387330aa5460c9cfcf96b5abf33399b4a76ece0966e245669664686
1024 256 64 0 1 0 1 e3972a7f16108d8ed95f47ae6db5bf8f6ffd2c29b04238148578ec87bb618cb4
1024 256 64 0 2 0 0 f102448117fd7135d5d044b5bc8621bc49244e554c984eed4530300980cf8fa7
1024 256 64 0 2 0 1 5353bb1f71b733f7c2f3a6112bcdcf7244c51c9a976f8912b6c07b6f03f8ab5d
1024 256 64 0 2 1 0 a1053925fcc4244e31fc0dd7a02abc36703c6e3c2c5e85be9ae26aab20a7ed0e
1024 256 64 0 2 1 1 f395458f6f3fd8219b07b038c679f6b546a06ff4f4104d6477500305bf0b3e33
1024 256 64 0 4 0 0 ce2bbb89c36fbdecef6541f579136f681110904995dd6f2455646f3bc75ef9ad
1024 256 64 0 4 0 1 ccfb5f4ef29bd69b58655778a30b6e08631a448ef80d2907d5f0eafc71d0f5ae
1024 256 64 0 4 6 0 b60bd65f5558e192d3527a5f4e9c0e108f4be5998c7ac771f37abc1c6c01f9c5
1024 256 64 0 4 6 1 21c3ea82ff3dca74c5affd410a5cfb8a47634d3df3d6de04a1c5a1b3f4dde58b
1024 256 64 0 6 0 0 86db5baece9f87d53bacc62f7358670ffeaeb497661e985940730418c1870167
1024 256 64 0 6 0 1 6654f9645b9de01c67948b05b8b6a0c3dd67ff2be4e1fdda78c76094b3d39f5d
1024 64 128 0 1 0 0 33f4a2937434a5bdcbbde8ecafc31cc0ed6c115cf925043ad8c6aa04fd4dbe0e
1024 64 128 0 1 0 1 e6536296d405c73b65bcf86bb59ac5329ed30e813ce90b6e2943895b6608fdb6
1024 64 128 0 2 0 0 958141067e8ddfbd9e99e1c105410d3a6efcda9c1147831db9925b2bc64ba3fe
1024 64 128 0 2 0 1 79e8a5d0cfd171050fe6dc36f625fc0cdf439442fe136ef877dbf1ac42073a41
1024 64 128 0 2 1 0 ed9c82bf2d8f90c2cb9153fbb7ff45ce523ecbb910ea8d155e37db18ab2d9722
1024 64 128 0 2 1 1 a9e53beb595236512c6536a73a52a0ea50a872f1049f466106ff2ec305607b49
1024 64 128 0 4 0 0 f1d754e7ea182b8639e468c5b7904cad4232f81b01863ccb659468859b895b34
1024 64 128 0 4 0 1 edf66fd1a60176450d6326e7dd673806502d21ba8f364a5625d0d8715cce41b9
1024 64 128 0 4 6 0 584af8bddf0a11d6161facfe304ae9d916450864a6f6fa6b722955d75915e274
1024 64 128 0 4 6 1 cf045dde50d535ddf79004b754ca8fabdaf34ae29514a457eb0b991346943540
1024 64 128 0 6 0 0 a2bc28714ef30dccab84304769cd1d9c3d5f3a937653589eed87fc7582438add
1024 64 128 0 6 0 1 cc9cb9985595e8ce335e74becc17c92179b5ddac84c9f710d6b3d33b4a33c6d6
1024 256 128 0 1 0 0 f8f94d124c064d70234220ab10e6e207bfee40761d03b4a2a1fde93297ae20cc
1024 256 128 0 1 0 1 154382e6e86f9dbdb38896d85c3df3bc7780458ca0617f1f8dba15b352462471
1024 256 128 0 2 0 0 52e7fb188e474aeded76ef12eaec06de31d4fd3534bf8a1a22de36c909814f00
1024 256 128 0 2 0 1 b88086fb743f78d175c3a3b538c4aefccdb439b66cf9d63f38f5c3cdb1e16e1a
1024 256 128 0 2 1 0 2b0ab6470f03c06ea7421ae7cbeb3cf33f182c8054c215bde5bfd8719d841e82
1024 256 128 0 2 1 1 7c891cbdf3193fdb2c822db97060efad15946d000206e8212005bcfd775443e2
1024 256 128 0 4 0 0 119d30e5b77b8a37f9474685056f79df67891a4067462d58dd6d019e5b830185
1024 256 128 0 4 0 1 3acaaca56b5a32a1fcf0d11fec78068dc9a7c34b7d68adf7722995da70893a6a
1024 256 128 0 4 6 0 f220e07721049757b561a6225ec49b7c94a73c46c632546438d4114e1aa9acf7
1024 256 128 0 4 6 1 d2759e457af0cf2831ec0782fc152f541368d714dd08eba3286ee690954dae13
1024 256 128 0 6 0 0 8a1e229cc62f37d0c05264bf4e9ad36f64a42b52787c690dd4951f6d2f27b426
1024 256 128 0 6 0 1 75dce0e538634cff679070511f400e8bd2adba7cffdefd1a35c76960096f3fda
1024 256 32 0 1 0 0 749ee290567fac68f4bb9189ce42f3c6a7859cf839e0bc25317da1ea514aa228
1024 256 32 0 1 0 1 f4b0dd3867ef973e25ac6b175b6504e046b4d777dedf5fbb22c5a3cd79a5d13f
1024 256 32 0 2 0 0 369d93e25d9494f58653871531f94e2b09bff3747b664ab43db291fa977cdb21
1024 256 32 0 2 0 1 be48ecb6f632091fb0d82afb316bbf1ee349430d7ba76e0b98c6ff785eb4cf18
1024 256 32 0 2 1 0 b160c1037df786c57eadbe33baaa0ca1e47b17ad94ae6f9f1a5b2ff6bfc2e2ff
1024 256 32 0 2 1 1 924530869044a8aa59ce3b891d45d50db6afb4c59423b15aa4898e387466753b
1024 256 32 0 4 0 0 5917f43c08ab79fecff28f1ef8d4ca637e64a3ee845dffc63c077c7bae3c2d46
1024 256 32 0 4 0 1 ec8b7b10d97cdc307fbc73f1ce74a6ededb86a4fa4eb4075b8eab36bb94dde25
1024 256 32 0 4 6 0 dfd55a32908ef89ef759093ac6c9aa0e1dd9cf33c2fec049cea1c277badfd96a
1024 256 32 0 4 6 1 04ba43bc38817ec686a15965a8007b7a6fd1a2fc0e9189778a3fadf37ec78334
1024 256 32 0 6 0 0 44b5e78fc62451278a988f581e85f0a16fa3464e70b0f536aec77084d39afd61
1024 256 32 0 6 0 1 1f14443096e7d9465663795e56b6278453f5efd0c8ff011d3bd364044cc362de
1024 256 16 0 1 0 0 568512b6986e54d995878ca2095ada1332cf49d5e01168bb5371d1b62bc0279a
1024 256 16 0 1 0 1 0d1352fc754a140a029b7f668733125ccd079f3de65ef437bcbb94d02e53936f
1024 256 16 0 2 0 0 f1643e1a82a8db503cd82b5bb0a6c23ca877d1cbbd9125e388954fa1f9ab4462
1024 256 16 0 2 0 1 4c951d0af6bd5b01024190f4458e31e9347649546b5d91fd15a447d1079c9aae
1024 256 16 0 2 1 0 48bdefc7efebd77087f01fd320ce4f01b2760a730d2cb1330d0b9c7e8250ce31
1024 256 16 0 2 1 1 25fb17e1c72a9f5dd575d5c4526edd42fdce82e43f09cd6f458092e51ac71a12
1024 256 16 0 4 0 0 3a3121d30dbae8fb8dd0e049765d0723bc81dd839c4f1cb78a240e05e973db0c
1024 256 16 0 4 0 1 7bcb9752743dee6998208b6b07fcc5d7bd3cdcac651618ba5fa81ea69ed3225a
1024 256 16 0 4 6 0 9c93f910d4d2c97d45578e6494c30aedf8611e3f6b08adc45b9a378a62cef952
1024 256 16 0 4 6 1 f644eb06881fe6e5b505fef7799dde8f4ba91419178feb36a2d672032d89374e
1024 256 16 0 6 0 0 e9cb2e05d97f7a26fe4a276e2a948d7ce716bccb3d6b1cc5292ffeed71139c5e
1024 256 16 0 6 0 1 cf8b967cdcc2ec2cc07215d306e12ff16a6cf2fb4a785d366102d18db4384d43
1024 256 64 1 1 0 0 a67da6171f587aa697fd3c8e4945fa19409bb25cadc8b2693e5f7217df7e369e
1024 256 64 1 1 0 1 852d43322e51b59a719bba351c2fb9c88f39ae0dbcde4fca4a606a92acdd7281
1024 256 64 1 2 0 0 a1287ac64bdd9e65ab33fbe67d95c2a3830c272e196109386090bb5fd253bcf9
1024 256 64 1 2 0 1 87c9561e749bcb40715bd05992a0e3b61571cc263c2813b518c73f8856f70219
1024 256 64 1 2 1 0 73dd6bb42d6ad2c991166aa809375f8ec559e5fa0e9f8cd98f951148278e8575
1024 256 64 1 2 1 1 a1eae3b28d20f1b271c81b5b865a655d52794501f748d3cfaf338b4d944f8535
1024 256 64 1 4 0 0 501f3450f6fd84c82b401483c07fcbaee8f479be525806893df13857297ffd54
1024 256 64 1 4 0 1 7fac9eeeb6a138d8c41df9841600f960aad6b87f1da1d690eb830b9758560392
1024 256 64 1 4 6 0 ac5e54d043360481aaf382de0d1aa574c6a15dafcb543d0d71e8fbb668eb6145
1024 256 64 1 4 6 1 1c6456196d2b6938c1c9d2b7178fc46415621a6e0fade700e3459e8c78a283a8
1024 256 64 1 6 0 0 98e730c95e42dca59095f5dfe5e5830cc0bdce3fbed0d7f63b58802f00b68740
1024 256 64 1 6 0 1 f11e3380697a9f8e2d43c03f84bb41f6d9123e106e745c945af794d136ad7c12
1024 256 128 1 1 0 0 2b5de62990c22326f84dd3d42c4b7005cd4cca4730ebfd8dcc555582e69adae0
1024 256 128 1 1 0 1 1c235537ffa84b8cc648975fa569103241be025d4cc168cef3a8f54dd9ccc812
1024 256 128 1 2 0 0 29b962ff4eb592573683f3c54563df3917297430d760f66a9557221e018d3d33
1024 256 128 1 2 0 1 e91dd2b6ed18c64d3df7aefbc292a2c60b284f8569ec218d44e203c9ea69b632
1024 256 128 1 2 1 0 7708a5dec4385f4180cd6324410319d383aca3e02dc9c835020208fbb8482e8a
1024 256 128 1 2 1 1 45977598521ab809caf63be7f41890c050dbc62091d1a8ea4257a62ddbf4a3ce
1024 256 128 1 4 0 0 d6c2575d02f8cfa350e0a69c63361abc527c6750428d89cc29724247fea0a042
1024 256 128 1 4 0 1 831d0ca79fc29d57829efb37ec0459bb52723376908b6124de3ba18e8025632c
1024 256 128 1 4 6 0 ecc55071a6b0f96c4219657f6be0525e8c38c4d4455ec984d5ff6f32cca68c02
1024 256 128 1 4 6 1 fa80d94fe0c35b98d7427fc909a7d2a3fb0b9a69f4679d5838b920ef3c7a2cf9
1024 256 128 1 6 0 0 39930013bf8dba3c40b1b74c2c5804691ed84362b3a30ca74e6346b4e280fe6f
1024 256 128 1 6 0 1 cb3ea857b7225091a285811677a043e378a547b5a2d339ca10085bf4bb4351e7
1024 256 256 1 1 0 0 72adb6973f204bb00769ccaa8044eda40af875a93975ec4c23b9543cabaa2df3
1024 256 256 1 1 0 1 72adb6973f204bb00769ccaa8044eda40af875a93975ec4c23b9543cabaa2df3
1024 256 256 1 2 0 0 269ae00f8f1c2d9d322f182f5ba86060a7b08f1195ac5be820eb571f95dad9f1
1024 256 256 1 2 0 1 921a248c9507999cc85786cd3e52312af3832edba705a4a212e0634164ae54a4
1024 256 256 1 2 1 0 66ce0b6298b668db183fea6b410fe3b1899f548e786c25f89198c3b14d6fd15d
1024 256 256 1 2 1 1 f44a9d274703fa5e4a24cc24bfc3165b1346aee2d763cc8ae1837b401faabbae
1024 256 256 1 4 0 0 20de13a658617bb602213dddce07ca9355e061c09de441d9ba532a9ea393aa60
1024 256 256 1 4 0 1 1176820ea0b0e2a1c808d539d48e8eb568610f2a9d1b80a6c1ab7d68a205efa1
1024 256 256 1 4 6 0 561c7ddfd2c35331912bf4aa155fc5f42801f12011c85d8e4086125025796b3c
1024 256 256 1 4 6 1 4667a7e4aaed571e40f17d0055c8ad70272391b2b9c081e1fec5dc972234449f
1024 256 256 1 6 0 0 1ccb6f3012b78a690b8db3ee7c1a86f1f107ac630ee24dfa0e8bab9c7f308793
1024 256 256 1 6 0 1 b76b619dba8a64ee1d19480f4c2f0f6ecd0552cd94fd7baa029ecc0ee9fe8665
2048 256 256 0 1 0 0 29e8ed696a097a1c627c577b593326dac20594fcadb701085afb2b23dfff3d17
2048 256 256 0 1 0 1 b07961d60031cdf319f9a52d2933150879e8a0c39823dd45063f273a88aa5c10
2048 256 256 0 2 0 0 da485b5cec8ff65a6c31467d2246eeca1f7ace82001f3218f2b9f78097652cac
2048 256 256 0 2 0 1 9c70a0589069655d792bd10426cce18e52cb784cb0a2996934b5449a288331d8
2048 256 256 0 2 1 0 f6ec1169907d0479c638b17a299aabf45bb3f80bbf216f6c935e69bc828933f7
2048 256 256 0 2 1 1 96f00c0cb1a3d56c97ab7af704e72decc7a8ff9c1c8e145232d7996bcd767caf
2048 256 256 0 4 0 0 99b08f84c3dd6438d6fa2a7f9884693d4057ef3ac7ee0c442d5bcc11df500086
2048 256 256 0 4 0 1 8d250fdbf411f0b33b4eba5c549df46be1a5238bf8b7a1b8149c3336416c606e
2048 256 256 0 4 6 0 7df1e5776a72c5fc786e78fba6b793c278445cfe329765c0fabf3ac368228212
2048 256 256 0 4 6 1 17d0189ccdb5d4ff482bae14f65f398c6bace350070baa7b9c94c4f3962079eb
2048 256 256 0 6 0 0 fd49230409e547c353243996f61b6ad0d7398c4be467da7d6367af9f262b558a
2048 256 256 0 6 0 1 7e6ac09300292df6cfa8bb0dda60ae9a62796f27c5d290a8edae7b46071f1cb6
2048 64 64 0 1 0 0 21d5209863a5068c79991eebdd7b0d93b8df054bc7798a80993a98c59fd22a96
2048 64 64 0 1 0 1 912308ef88a70c824135c29e7dba9baa04686c06d2d7d58fbd6cc8bc2b88d322
2048 64 64 0 2 0 0 59d8d88d202bd5d4b2e5a6da0a46daba58185ed372bc2ab7436dc85a0d5058b5
2048 64 64 0 2 0 1 efe1ca7992a3c183bd131268672f61772d6e33b9f439398a3dfce9eda575e90d
2048 64 64 0 2 1 0 b79faeaabce05d6e11b354fc8dba8c7d316da55db486f7f9020a6fca6094e3db
2048 64 64 0 2 1 1 5ec252625aaf21c9f21f8c4a507ae653612acd1925826f8f530d8ca8ec4b550a
2048 64 64 0 4 0 0 e4f7e24629fae0267c9e7dcd64f5811b4baf21af26f760981e763bb0ef5a2058
2048 64 64 0 4 0 1 5898f24406fbce783e0cfe7a6a54ee204b0bf9bc375f65f5422ff1bf949a0a6b
2048 64 64 0 4 6 0 c204ac8caf67c9b8bcb7d0660a99837a4fc66d650c3766288facc5122c580d34
2048 64 64 0 4 6 1 5ecca56deffac0a0faeb35a82c0756e77c93afdfa7f3f0912033cd4e0243fbc7
2048 64 64 0 6 0 0 f080016a3f855a8afef2f63cfc5e9405e51ec9d015dc2c7f809ef946cf9287c4
2048 64 64 0 6 0 1 7a685d4d4f77e27264d8d40e93449cee73d15bca8beb38521f4b03ceaad61bde
2048 256 64 0 1 0 0 2d03f49eb2fb8912ae93d6e845ed0254ca01e188539abd078a4e69070f97292e
2048 256 64 0 1 0 1 748140db8fb9d08cbd81a8abf771a1cf936ccb54a866e9a537a55060bfb6e91c
2048 256 64 0 2 0 0 aac1f49f4133ddbd4d0dd06acea6ed179263c021286b05cc7698948d6fda5460
2048 256 64 0 2 0 1 f2018a89a6cba37478eee4717deaa8c7c56db302bbf6577b4eac833aa806d857
2048 256 64 0 2 1 0 eb02843617bc42e69d5661a682857a171c7f291bf485210e915ba0cb5c9d695b
2048 256 64 0 2 1 1 4fbf2bd2d107510dcad57ad81459b7f5022be7cb964f41789a851df99fbee39b
2048 256 64 0 4 0 0 5e145baaa4892e7ab750845bcec676f4c19b416632bb04885f5d74f70509e74c
2048 256 64 0 4 0 1 87916cef25757a1b406764293e11e1815bccde009144f4ba3f79e899e9901801
2048 256 64 0 4 6 0 e31c24dd625436c36c5141550a388f9114d0d4e428f23e01a1371d6fe48ef55f
2048 256 64 0 4 6 1 08154f8e9fbb5a7516fba5d160bf16b503dcb860474c65c6683302532e7eee8c
2048 256 64 0 6 0 0 2d022b41c9de01dfb9840efbea3f90b65e5287517bcb847114d4e6d8f763f32f
2048 256 64 0 6 0 1 1f6fe72e64a34acf403dff860f992b36bb48eb517e9a91c50bf5e6d0b3fc1361
2048 64 128 0 1 0 0 3c9c9f3148286d176c0d9d3d8088a401b3348fe0b6e4f2eae5ca91c47c0633fa
2048 64 128 0 1 0 1 ff784b5dc4f0aea6a8409797e93bc45bcee4c29b2da6d3e0c9fb3180ac8cce13
2048 64 128 0 2 0 0 162c82589457fe87cf501850a1c399a7a97c5e4aab7c0e9fa4eec1961fc1799a
2048 64 128 0 2 0 1 6e41bafc68e9270c1dfa2929c3e74adfd217247ab628e626ad9a95927e5e310f
2048 64 128 0 2 1 0 bb1ac9336d06ebb4c4e72f22bfe5690b34474089f03cc9cd2be0299b53d5ada5
2048 64 128 0 2 1 1 fa24e756bf86c074446053f20c8ff1d3f25644ed914f4a26869b2dfa46f514a0
2048 64 128 0 4 0 0 fc0384b3ce0ce0162c78b27f8036044e20a0a911389debd884b239eb1faa55a4
2048 64 128 0 4 0 1 ac52888f790f458c5f7cee95ed0f5a75aa0fde1ef2115a3c4c8da2d54e410cfc
2048 64 128 0 4 6 0 207244bf275f2dc68b17c01a40f3f0bc9bb9f3d3af669bb0d54ee6ea91a12b8d
2048 64 128 0 4 6 1 a188e464389fdff6b47813f7e5d982b3677b9d53e536b723b847e11431493ddc
2048 64 128 0 6 0 0 f4cba7ce5412f380a87510cfb0eb3de364fd167ee4c8d224e080e8be08f2cbb5
2048 64 128 0 6 0 1 45761d972ab6a3614e3283ea9142c0f6b251314fe698be940d098e47a2900a57
2048 256 128 0 1 0 0 58d7070e3b2222bc42570b2f6f1d2688691c3000e118a15aeb2762d4a271cb3a
2048 256 128 0 1 0 1 5eee329aea845f724d8b7f018ac4e3d8abb46438d6ee10821629409a88234f49
2048 256 128 0 2 0 0 af26128b8393df06959ab0a5b1b3bf8f8ae8921ebf7846c8c2d34eea9932d96c
2048 256 128 0 2 0 1 5132702bed1e4cff86c560fec4adb5456843e2ea29c9a3aa8c2512527ebe3e80
2048 256 128 0 2 1 0 3bb123c9ddcc08026d777ce1fc4b7044852f3d4af3ff55a6cb06292b2c80080c
2048 256 128 0 2 1 1 856a7ddd25f0a9791775ea408450a133b9ba74aa63aa2b96e7c0b8736be16ddc
2048 256 128 0 4 0 0 3d2e9739c459288effa639888e4130c667225e0ca41c0b572e3ae8b5fecaae11
2048 256 128 0 4 0 1 9c0ad11f27801b58e058f30d73651ba1d6ebd8f80efe332e6260653c002f1946
2048 256 128 0 4 6 0 bb03d89eab052d90a14e7aac0b3e487a671ba3e1fc3e34197f9bfe3e6e017172
2048 256 128 0 4 6 1 10ce2dd4e062eaba3756517101816037ae910752d61b7b71c5f84e18f667e1f2
2048 256 128 0 6 0 0 700a54bc2c8528588528940006dd4811c758b0f49d4e8c309a63df08c725cbf1
2048 256 128 0 6 0 1 4df18da6ee52bb57fa31c1ded6f9f3cd8bddb815b6eb0e4f641223e355f12f00
2048 256 32 0 1 0 0 7f5ad9d9df87cdceae366e02142c2f37a047b2f96e4821ad4dea2dfef4e5ae63
2048 256 32 0 1 0 1 ecfde4cb4ddaee614b3ab12da49afa76b2dcd681e25ddd48ba855080612740fc
2048 256 32 0 2 0 0 dfba7794d88988164048931cb6f3db02660ecfada7dc5f27379612f39be61bce
2048 256 32 0 2 0 1 199e44768011d56a59e00bf5878c284d93093089f6b2a950a584865f7ca16a7d
2048 256 32 0 2 1 0 52e04e7dfc5260eed1291a0a63deaca2d31263f285c538ea76fc285c15d8a05e
2048 256 32 0 2 1 1 aa2b07049d41fff812c62a99ed80de307510c93d2f6347487e304028fc661212
2048 256 32 0 4 0 0 150f563139dcf8fe67f01bc7ffe800187154a50deb139d4bb91eef6e4bb656db
2048 256 32 0 4 0 1 9d3448278681696ff936fe1010ef9bbea32cd5c187167aa7e1a395cdcb5fec61
2048 256 32 0 4 6 0 441173eeb7f66dc4df4dc1c7407f809ebf42807057ce637ce5c78ef85933fc07
2048 256 32 0 4 6 1 f4444ad9e71e5daeaa1b403144d970d05243c624e591ae6786d8b3661c8ccc27
2048 256 32 0 6 0 0 ccfd183f08d6aded8929beb3226cc02854f33471cd5c8b264ef1a2339cd75420
2048 256 32 0 6 0 1 2c55222d9fa5a28594367a090c81ff3828c8e1d1a618d3a3f1b5a16a86da31c1
2048 256 16 0 1 0 0 8c5d515336b81f8dae74eaac6906486552cbbe74692bd295ad62307b8a57da1e
2048 256 16 0 1 0 1 5c684b0f176d9574755e295a8dcf1bc5068fa5673c12d8f02f70c8f1eba4a70d
2048 256 16 0 2 0 0 9407c7cd9d0376623db5ecb0476ba6897d0b1c10bdeb4d5941acb06fa8ca96cd
2048 256 16 0 2 0 1 6385e221836fe32470130300ebef3e6b7eae8b185e70d61c8003cac542e87532
2048 256 16 0 2 1 0 ee89ebd6bdca389afdf0af4476830d2f051ae5783e044bab8e61c50e128b464f
2048 256 16 0 2 1 1 4d3a5a22caabb226b2bff6a8467f24eba09a38b01026ad72791372f789f6f7eb
2048 256 16 0 4 0 0 1bed9271db6d32787add17a6ee53a2c6d94d524c1285fba1a9a8cfed53d5224c
2048 256 16 0 4 0 1 68cd7f2cbc0e6c7c67c36f2ff6dd8c25ffcc178520f5338956ba0d352429da6b
2048 256 16 0 4 6 0 baa5dfac595aa135239a0d5f710ddb0649fa6c84e560f7f06f20e8ed6af29c71
2048 256 16 0 4 6 1 ea39af120d78ee2f28a7c69e3e553499b57fa6769dff81812bb0d9a70ef6a748
2048 256 16 0 6 0 0 2ce291ddf2405457653053df7a99c05010abeabe2cc30420003378e0ddd717c0
2048 256 16 0 6 0 1 2e154de1e125f4e6d986d409e22ed0ce767af914a83da6a82c035f9b43540e8f
2048 256 64 1 1 0 0 233fdaec630a486e0d4bcb0619a263fef2bd026db78d43e5b8b3d2fa90bdc60d
2048 256 64 1 1 0 1 5cb6ba55e6a115c79150dc2f34a5d5ce4f70dacb93c6c3392ea88e079e9b0c4a
2048 256 64 1 2 0 0 9f5c36ef89d1d17b8acdfda9cad9498da458585c32cae080c1025bf048072418
2048 256 64 1 2 0 1 45f333265fb7ce5d1e54cbe3b31a1c0631fc37eeaab3e54bf5c185a3cc50a0a7
2048 256 64 1 2 1 0 5f01ce2c93d1dd6cfa02dc41487eadf717aed47645bbee06cb5a5022e2da48c4
2048 256 64 1 2 1 1 5ab2c1a1345953ee6a0e1a1d7d7cc32073777bd867deee64d949ec74219e3ab3
2048 256 64 1 4 0 0 8988bea78d8471b286e6773340a85540498f3bd82b006268bdca77beda28bda0
2048 256 64 1 4 0 1 02a7387f396f4593c346daafd4fdf198c8933fee03576f5568e1b6fafaa0e426
2048 256 64 1 4 6 0 4b92cb3b090a3e5f71b77e59545b4c728ccefa3abefc0fe19ad1d41f65084c45
2048 256 64 1 4 6 1 f04566c804ade61960d403e8d8ab749a7877d5d4b6b0457af77327ec372b2c1a
2048 256 64 1 6 0 0 0f33da124a8bc71d266058c03acfb28c21093c3573eb4344da61937ed7c7d846
2048 256 64 1 6 0 1 e85c25e045a10983d01668f50c7e8f03e871c216f95700d781471f61d15ca2fe
2048 256 128 1 1 0 0 6ba883393625971cbb5b50df042d834615fa18431efae0027a5b6bb46b76ff70
2048 256 128 1 1 0 1 b02b661a2a762fa5dcafe3b5a5e132af2e1ab5b63b37439d5f30cefa468649be
2048 256 128 1 2 0 0 73558d9c0130692135cab3606122a4f6f88f9c792ec01039426f3e39c45f0a25
2048 256 128 1 2 0 1 c5bc993b036eabcfa2d9477240dbcab4419c330276d9ea6922a2e1dc1d0b341f
2048 256 128 1 2 1 0 b288abda6c4dcef511bbdab20f6d66932d6ffe760f93f27d22957bdf163a5d82
2048 256 128 1 2 1 1 c5885b365968fbcae291ef35999f0c6fc6c51e8906f87e837f7b676aef102e4f
2048 256 128 1 4 0 0 7f9cd4431c3ea664af753121e08076e5f89fea02934b8a4082c7fa4cec773ef8
2048 256 128 1 4 0 1 a433d98b2bd94630a3a7146c3ecd7e5a8addf5ef91bd8c441f91cc5cdbe7468c
2048 256 128 1 4 6 0 548e9c14a7dc17784983b47c360d79472a0c4c57862f1d6d632124f710bcde9f
2048 256 128 1 4 6 1 8ce3498ae073691b013cb9ccbaec58f36d9c255f700316d1c692c31f07cfa141
2048 256 128 1 6 0 0 8c54cca8b322d5ce5a2db56606b1c872af98721e473b2b91b1e7539c4375b1c7
2048 256 128 1 6 0 1 eb85e37a56815c0c676a23822e1b3e0bc4bfa97fe6ee95c7ec443202e17edf17
2048 256 256 1 1 0 0 96d04251fe51e7c9dd65144d11e587421eb9d4cdab37fb19fee32120ea83db02
2048 256 256 1 1 0 1 c858f92198a9228152626646338290e8fa421e9e07231ef38f37c3ea67f61274
2048 256 256 1 2 0 0 154a17321e6e23665fae27be8fe94c00d787cc8226b0cdfa2e1bd3d54d7dc51b
2048 256 256 1 2 0 1 a451b6477c54c061a7f99f7e3a7bf3a3a8889425e69807337ef6c5eb0fbadd69
2048 256 256 1 2 1 0 6972b5595adea19a1701dcac63e2392d83f2fcb8f7b1fdf8d95a515631fc5053
2048 256 256 1 2 1 1 16876d2a403c3de39f4f6f6d2ff1cd5534b35cb72fadf10c56163d7ce055a5ba
2048 256 256 1 4 0 0 d6fc396391bee90eeec429a5cf580e5a4ed0ec6957cef809a813c0fdfc8e4190
2048 256 256 1 4 0 1 015b760513f4e21424ecff4e7ab7f0fa9c7162c97a7a3366cac82fce324bd84d
2048 256 256 1 4 6 0 67c6d60f50ad786207f97b958d455220a35504acbd897c9b030e5fccdaab385e
2048 256 256 1 4 6 1 6bd868879580cfe97b7b78feecddbbc941a385cc51fbad0278793407a74abe9d
2048 256 256 1 6 0 0 8735252f32424aca059e49d338385c3c237ab489fd1156e89cb1a1a45e365e84
2048 256 256 1 6 0 1 07bb76bfa97fa34b38ef1be81f15b350e727b9a0dbf706846ea9e2155f48770d
fcs 64 2 256 87b200635fd08e0c87ad65adba7b238f36968ae781b5292e85ed3c6eb1676588
fcs 64 2 64 87b200635fd08e0c87ad65adba7b238f36968ae781b5292e85ed3c6eb1676588
fcs 64 2 128 87b200635fd08e0c87ad65adba7b238f36968ae781b5292e85ed3c6eb1676588
fcs 64 3 256 4c5946d224fd0e42b1ece1a1fb400c3d4d1e4f33565ff33a4b7e4da2f6844de4
fcs 64 3 64 4c5946d224fd0e42b1ece1a1fb400c3d4d1e4f33565ff33a4b7e4da2f6844de4
fcs 64 3 128 4c5946d224fd0e42b1ece1a1fb400c3d4d1e4f33565ff33a4b7e4da2f6844de4
fcs 64 4 256 a3244141f64ec60d5e3fd1726399dc33b033425f2f27c4f20a9289c65069f2a2
fcs 64 4 64 a3244141f64ec60d5e3fd1726399dc33b033425f2f27c4f20a9289c65069f2a2
fcs 64 4 128 a3244141f64ec60d5e3fd1726399dc33b033425f2f27c4f20a9289c65069f2a2
fcs 128 2 256 623748a2fffa1347aecf70d5f05cfde1dfda79f3144bf954f0cac97843c0e50e
fcs 128 2 64 d06daf36fd193cb0af7d428ac16f54afaf2642fc54e2bad586391d8305edccd5
fcs 128 2 128 623748a2fffa1347aecf70d5f05cfde1dfda79f3144bf954f0cac97843c0e50e
fcs 128 3 256 38cf32515e402784a37d4155e1530b47669032b10984270c7cc99fc7cb78b740
fcs 128 3 64 b831eeedafdd01c1404db750e20d7ffae214dd3aaf9b8d3fadab9e7fc77ed278
fcs 128 3 128 38cf32515e402784a37d4155e1530b47669032b10984270c7cc99fc7cb78b740
fcs 128 4 256 5777198ec6bef15901683808f4b26ddb2ef741a0488dd5cec76d5bbb1e355974
fcs 128 4 64 26a7f4c8a781219462604cdf22a8d4d1332ff50a610f682adca4153479861a74
fcs 128 4 128 5777198ec6bef15901683808f4b26ddb2ef741a0488dd5cec76d5bbb1e355974
fcs 192 2 256 42a15f26534977077346af4bccc7afff106890f5b7d2943bf64c996ff6b21cf4
fcs 192 2 64 c74f77f6f6df06b7cd03c31afddb7867a8d5a3a28499ddcb7cf892be933f2a3e
fcs 192 2 128 d99391f435df9e56a69885ffce54ffe33c39f863133ea3cf194a858164ddc268
fcs 192 3 256 de1fa48319e0421d739b90f9c6888e5fe5ce54e1fd5f1ac8807cf7ca27535425
fcs 192 3 64 3abf3e84108508a9af516d853a4527f716a5550d3321c742d16a362d4d2ec0e7
fcs 192 3 128 5790053944f0cd2b0584241a186cdfaa1f96bbdf3ada6f54e980411b0e9cce0c
fcs 192 4 256 12706188b8f5aaf468ccacea75cf8c87fa61fe78497bb4312a7c43aed1a6f4c8
fcs 192 4 64 c18c80d0ee5d5c2e64fe1f62b48de5f0d05929f2036e742ceb3b93472a19fd27
fcs 192 4 128 677228cf3c4dc1d00b25dfaa149813866dafb47d76a01e2846f2e90e07de7687
fcs 320 2 256 09708a3a36b9660826170b78c88420f59b71acda28229663ddabf11c41a69558
fcs 320 2 64 707ac4fb1165e34579fb4cff016bcb1058b923369d1cf519767a7d5cf7aef30e
fcs 320 2 128 5946fe58f43217319b3dfe0a9ac41a1f69c07e151ff82c49692837a9c5f89fad
fcs 320 3 256 36910fd4d849d104e9840d0eee1e2b0af0811f91abe96af2bf8c5a4b39d99841
fcs 320 3 64 8337d04b01468ac844a1dbbf20a88ccf5fa88e9c72c0636b42b3000e70ccfc1a
fcs 320 3 128 145a991ddbe5c6f6a64b0706014f06a88237df7c8cb1946e00d1e92132435e6b
fcs 320 4 256 27e7f63d431c361128cfb3ca068153bc02e9835dcc8ed967d83b31ab0bc1ef39
fcs 320 4 64 fecba981fc55d612cbc0ede66b56001b8581997742d604ab8fb3f607d981b345
fcs 320 4 128 ae0b9f6ec72d68b662532e45b5d4719d7549c295ae443e92389ac1b71578d590
fcs 1024 2 256 3ea1ffea142f904e899e52619dc0f31ed38eb64c52068d7490f512642cf388b8
fcs 1024 2 64 f60af23b39154bced9a975a12d3f319c31a45331403a3833b0fa0ff500908d20
fcs 1024 2 128 8534f3cdc9269b593f92809a2276eb205382c369de5cd6c15b491992b9a84c33
fcs 1024 3 256 7aba8e25b2b95e992df09ebd0ec0d0e1b897dd9a31157db3724c0579c786f02c
fcs 1024 3 64 c54351a3ef0a7997624f34d7e0a1db237c2da71519bbb8e5b8ca57d4c0ac0cbe
fcs 1024 3 128 be653836febfe2e16c9c2bb95ee7383b3ad3093bf9743126e797006307130e2c
fcs 1024 4 256 749a6954a47634c6ddc055246607ec76388be10178988ee08c6b3ae04fb3b219
fcs 1024 4 64 3a5dd3bff9f93a4731fb6df061755030208423df06047e21b7b186cb5bff38dc
fcs 1024 4 128 d83fafc0146872391d1bbb9f7a20ce2cc76f45c2f2640347ecaae40e78a4f598
fcs 2048 2 256 05ac87dcee861a4bf9b8cec82eda1fa0c25c26c01418d87e501706e05b7abcd3
fcs 2048 2 64 48a4985a735c99140686f89d25f50d91eb3181d78959b805265d76bb0cb8208b
fcs 2048 2 128 31f03f219a1b7e5d1427098c36c0d22d00e0cc31fc67f2708cfa6cf70d0db333
fcs 2048 3 256 8509df8d1bb36902f7247cfa4f09d5d697c075a7bb584d18f33eabafb85062cc
fcs 2048 3 64 a16c7e6b427a7824299a091781068d3f147385a8c74bff5fdaa3d489e444ea80
fcs 2048 3 128 a3e570b09697248facd25a710e351c01fc6516f8705f4f797cf73e1b7deddd8e
fcs 2048 4 256 326651441afdcceaac1d7ec433ec30a315aecdce9d6b8886b1bbffbd393dd6c0
fcs 2048 4 64 31667e5b23533d6e905f9cf9b6eb70dcfa4a16aea5756193d2ef7ce010dd194d
fcs 2048 4 128 685258b12d51e0e44cbf94d6a9b71520753d5d5049e35d10780430ee4e84a5ef
runs 4096 6 1012 8ae3ac3cf029c10e39f386a57b01fa7609a7569f956f1510e61f45b4fa329603
runs 2560 6 1012 830efda584df229319c5dde72608275338fbb8b51d5c13428111f5e4b8795003
runs 3072 5 1014 9abb8393816c5415a9108c58caefc7f0545207b9a3cb5db4fe541ec19037a503
runs 2752 5 1014 bae5ba0d5fa9c44e289e655386cf899cc3ef2e1535248f05fbc0b5a5007efdcc
runs 4096 7 1010 7d8c7f0d486e7c5fe2dfbe7c0691e9061b983dc5be902280a88eb57e1747d984
runs 4032 6 1012 9cdf24f5da1368d0ed7385adb4cdd941914b937e44a09d39766336a001652859
"""
