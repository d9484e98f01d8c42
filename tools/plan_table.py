#!/usr/bin/env python3
"""The rollout's plan selection as a table: one line per (pack, call shape) with what gpmpc_plan_describe says the call launches --
kernel form, tiling, workgroups, split, head row chunks and the workspace size, which covers the buffer layout.  Two builds of the
library that print the same table make the same decisions: the instrument a change of a threshold (or of the code that holds the
thresholds, csrc/plan.hip) is reviewed with.

    python tools/plan_table.py > table.txt                     # the whole grid and the override passes
    python tools/plan_table.py --quick                         # a corner of it
    python tools/plan_table.py --coverage < table.txt          # does a table reach every form / tiling / split the library can print?
    python tools/plan_table.py --autotune 300:2:1:10:64:0:1 .. # N:ds:da:H:B:shared:graph -- gpmpc_pack_autotune's candidate list, times stripped

The packs are synthetic (random inputs, zero weights: a plan depends on the sizes, on whether the GPs share one lambda, on the nominal
model and on the GPMPC_* overrides, never on the data).  A GPU is needed only because a pack lives in device memory: nothing is launched
except under --autotune.  Only the public C ABI is used, so the tool runs against any build (GPMPC_LIB_PATH)."""
import argparse, ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (100, 200, 300, 400, 512, 640, 1024, 2048, 4096)
DIMS = ((2, 1), (3, 2), (4, 1), (6, 1))
BS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 288, 384, 512, 768, 1024, 2048)
HS = (10, 20)
# one pass per override: (label, environment).  The first pass is the selection as shipped.
PASSES = [("-", {})] + [(f"{k}={v}", {k: str(v)}) for k, vals in (
    ("GPMPC_TILING", (0, 1, 2, 3, 4, 5, 6)), ("GPMPC_FUSED_SB", (0, 1)), ("GPMPC_PERSIST", (0, 8, 16)), ("GPMPC_PAIR_SB", (0,)),
    ("GPMPC_SPLIT", (1, 2, 4)), ("GPMPC_HEAD_CHUNKS", (1, 4))) for v in vals]
FORMS = ("persist", "fused_sb", "fused_sb_shared", "fused_staged", "lowprec", "head+pair_sbs", "head+pair_sb", "head+pair_staged")
TILINGS = ("256x256", "64x64", "256x64", "64x128", "256x128", "256x32", "256x16")


def coverage(lines):
    """What a table must contain to exercise every branch of the describe function; returns the missing items."""
    seen = {"form": set(), "tiling": set(), "split": set()}
    hch = nominal = False
    for ln in lines:
        if "|" not in ln:
            continue
        kv = dict(f.split("=", 1) for f in ln.split("|", 1)[1].split())
        for k in seen:
            seen[k].add(kv.get(k))
        hch = hch or int(kv.get("hchunks", 0)) > 0
        nominal = nominal or kv.get("nominal") == "1"
    missing = [f"form={f}" for f in FORMS if f not in seen["form"]] + [f"tiling={t}" for t in TILINGS if t not in seen["tiling"]]
    missing += [f"split={s}" for s in ("1", "2", "4") if s not in seen["split"]]
    return missing + ([] if hch else ["hchunks>0"]) + ([] if nominal else ["nominal=1"])


def make_pack(N, ds, da, shared, nominal):
    import torch
    from gaussian_process_mpc_amd.rollout import GPPack
    rng = np.random.default_rng(N * 131 + ds * 17 + da)
    D = ds + da
    lam = rng.uniform(0.5, 2.0, (1 if shared else ds, D)).repeat(ds if shared else 1, axis=0)
    nom = (rng.normal(size=(ds, D)), rng.normal(size=ds)) if nominal else None
    return GPPack(torch.as_tensor(rng.uniform(-1, 1, (N, D))), torch.as_tensor(rng.normal(size=(N, ds))), None, lam, np.ones(ds),
                  y_is_beta=True, nominal=nom)


def describe(pack, B, H, flags):
    from gaussian_process_mpc_amd._lib import check, lib
    buf = ctypes.create_string_buffer(512)
    check(lib().gpmpc_plan_describe(pack._h, B, H, flags, buf, 512), "gpmpc_plan_describe")
    return buf.value.decode()


def table(a):
    from gaussian_process_mpc_amd import _lib
    quick = a.quick
    for N in (NS[2::4] if quick else NS):
        for ds, da in (DIMS[::2] if quick else DIMS):
            for shared in (0, 1):
                for nominal in (0, 1):
                    pack = make_pack(N, ds, da, shared, nominal)
                    for label, env in (PASSES[:3] if quick else PASSES):
                        os.environ.update(env)
                        pack.reload_tuning()
                        # the override passes: objective + gradient under graph replay; the shipped selection: every flag
                        calls = [(H, g, gr, 0) for H in HS for g in (1, 0) for gr in (1, 0)] if not env else [(10, 1, 1, 0)]
                        if not env:
                            calls += [(H, 0, gr, pf) for H in HS for gr in (1, 0) for pf in (_lib.FP32_ACCUM, _lib.FP32_ALL)]
                        for H, grad, graph, pf in calls:
                            for B in (BS[::3] if quick else BS):
                                flags = (_lib.WANT_GRAD if grad else 0) | (_lib.USE_GRAPH if graph else 0) | pf
                                prec = {0: "fp64", _lib.FP32_ACCUM: "fp32acc", _lib.FP32_ALL: "fp32"}[pf]
                                print(f"N={N} ds={ds} da={da} lam={'shared' if shared else 'distinct'} nominal={nominal} env={label} B={B} H={H} "
                                      f"grad={grad} graph={graph} prec={prec} | {describe(pack, B, H, flags)}")
                        for k in env:
                            del os.environ[k]
                    pack.reload_tuning()
                    del pack


def autotune(a):
    """Candidate names, shape fields and split of gpmpc_pack_autotune in the library's order (no times: they differ from run to run), then
    what the shape plans to AFTER tuning -- the tuned-table path.  The winner and its margin go on a `#` line: they are measurements."""
    from gaussian_process_mpc_amd import _lib
    for shape in a.autotune:
        N, ds, da, H, B, shared, graph = (int(v) for v in shape.split(":"))
        pack = make_pack(N, ds, da, shared, 0)
        flags = _lib.WANT_GRAD | (_lib.USE_GRAPH if graph else 0)
        print(f"shape {shape} default | {describe(pack, B, H, flags)}")
        res = pack.autotune(B, H, graph=bool(graph))
        for r in res:
            print(f"shape {shape} candidate {r['name']} " + " ".join(f"{k}={v}" for k, v in r.items() if k not in ("name", "ms", "winner")))
        win = next(r for r in res if r["winner"])
        print(f"# shape {shape} winner {win['name']} {win['ms']:.4f} ms, default {res[0]['ms']:.4f} ms")
        print(f"shape {shape} tuned | {describe(pack, B, H, flags)}")
        print(f"shape {shape} tuned, other launch mode | {describe(pack, B, H, flags ^ _lib.USE_GRAPH)}", flush=True)
        del pack


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="a corner of the grid")
    ap.add_argument("--coverage", action="store_true", help="read a table from stdin, list what it does not reach (exit status 1 if anything)")
    ap.add_argument("--autotune", nargs="+", metavar="N:ds:da:H:B:shared:graph", help="candidate lists of these shapes instead of the table")
    a = ap.parse_args()
    if a.coverage:
        missing = coverage(sys.stdin)
        print("missing: " + (", ".join(missing) if missing else "nothing"))
        sys.exit(1 if missing else 0)
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    for k in [k for k in os.environ if k.startswith("GPMPC_") and k not in ("GPMPC_LIB_PATH", "GPMPC_LIB_ALLOW_MISSING")]:
        del os.environ[k]                                   # the table sets its own overrides
    (autotune if a.autotune else table)(a)
