#!/usr/bin/env python3
"""What the noise model of the rollout costs: the kernels now LOAD init_cov / action_var / process_var from a buffer
of the pack where they used to carry two compile-time constants.  Protocol of tools/nominal_ab.py (every call followed by a
synchronisation -- the latency a solver loop sees --, best of --blocks blocks of calls), one child process per library:

    parent library (--parent-lib, built from the parent commit)       run TWICE: its own run-to-run spread is the yardstick
    this build, (d) defaults and (m) a model set, interleaved within a block
    this build, (s) the callback with a set_noise in front of every call: what a per-solve initial covariance adds

Shapes (N:ds:da:H:B[:cb|:fc]): the C2 solver callback (captured graph), C3 at B = 256, N = 300 / ds = 4 at B = 256 (whole-horizon kernel),
C5 (full covariance) at B = 1.  Then bench.py --dump-outputs under both libraries: the arrays must be bit-equal.
The result goes to --out (profiles/noise/ab.txt); where (d) falls outside the parent's spread the file says by how much.
Run on the GPU box:
    python tools/noise_ab.py --parent-lib PATH/libgpmpc_hip.so [--out profiles/noise/ab.txt] [shape ...]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["512:3:1:20:1:cb", "2048:4:1:20:256", "300:4:1:10:256", "2048:4:1:20:1:fc"]


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_process_mpc_amd as g
    from gaussian_process_mpc_amd.rollout import CostParams, GPPack, rollout, rollout_fullcov
    from gaussian_process_mpc_amd.synth import synth_problem
    dev = g.require_gpu()
    this = args.child == "this"
    last, pack, pb = None, None, None
    for shape in args.shapes:
        f = shape.split(":")
        N, ds, da, H, B = (int(v) for v in f[:5])
        kind = f[5] if len(f) > 5 else "graph"
        if (N, ds, da) != last:
            pack = None
            torch.cuda.empty_cache()
            pb = synth_problem(3, N, ds, da, H, max(B, 2))
            kinv = []
            for a in range(ds):
                gp = g.GaussianProcessRegression(ds + da)
                gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_f(np.array(1.0)); gp.set_sigma_n(np.array(pb["sigma_n"][a]))
                gp.append_train_data(pb["X"], pb["Y"][:, a]); kinv.append(gp.Ky_inv)
            pack = GPPack(pb["X"], pb["Y"], torch.stack(kinv), pb["lambdas"], pb["sigma_f"])
            del kinv
            last = (N, ds, da)
        cost = CostParams(-1.0, pb["Q"], pb["R"])
        x0, U = torch.as_tensor(pb["x0"][:B], device=dev), torch.as_tensor(pb["U"][:B, :H], device=dev)
        x0h, Uh = pb["x0"][0].copy(), pb["U"][0, :H].copy()
        rng = np.random.default_rng(5 + ds)
        A = rng.uniform(-1.0, 1.0, (ds, ds))
        P = 0.02 * A @ A.T / ds + np.diag(rng.uniform(1e-4, 3e-2, ds))
        model = dict(init_cov=0.5 * (P + P.T), action_var=rng.uniform(1e-4, 1e-2, da), process_var=rng.uniform(1e-5, 2e-3, ds))

        def run(mode):
            if mode == "s":
                pack.set_noise(**model)
            if kind == "cb":
                return pack.objective_gradient(x0h, Uh, cost)
            r = rollout_fullcov(pack, x0, U, cost) if kind == "fc" else rollout(pack, x0, U, cost, want_traj=False, graph=True)
            torch.cuda.synchronize()
            return r

        modes = ["d"] + (["m"] + (["s"] if kind == "cb" else []) if this else [])
        for _ in range(3):
            run("d")
        t0 = time.perf_counter()
        run("d")
        reps = int(min(30, max(3, round(0.25 / max(time.perf_counter() - t0, 1e-5)))))
        best = {m: 1e9 for m in modes}
        for _ in range(args.blocks):
            for m in modes:
                if this:
                    pack.set_noise(**(model if m != "d" else {}))
                    run(m)
                t0 = time.perf_counter()
                for _ in range(reps):
                    run(m)
                best[m] = min(best[m], (time.perf_counter() - t0) / reps)
        form = pack.plan_fullcov(B, H)["form"] if kind == "fc" else pack.plan(B, H, graph=True)["form"]
        if this:
            pack.set_noise()
        print("AB " + json.dumps({"shape": shape, "form": form, "reps": reps, "ms": {m: best[m] * 1e3 for m in modes}}), flush=True)


def run_child(variant, lib_path, shapes, blocks):
    env = dict(os.environ)
    if lib_path:
        env["GPMPC_LIB_PATH"], env["GPMPC_LIB_ALLOW_MISSING"] = lib_path, "1"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--blocks", str(blocks)] + shapes, env=env,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit("noise_ab: the %s child failed (%d):\n%s" % (variant, out.returncode, out.stderr[-2000:]))
    return {r["shape"]: r for r in (json.loads(ln[3:]) for ln in out.stdout.splitlines() if ln.startswith("AB "))}


def dump(lib_path, outdir, config):
    env = dict(os.environ)
    if lib_path:
        env["GPMPC_LIB_PATH"], env["GPMPC_LIB_ALLOW_MISSING"] = lib_path, "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", config,
                          "--no-cpu-baseline", "--no-legs", "--no-extras", "--dump-outputs", outdir], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit("noise_ab: bench.py --dump-outputs failed (%d):\n%s" % (out.returncode, out.stderr[-2000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("parent", "this"), default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise", "ab.txt"))
    ap.add_argument("--dump-configs", default="C2,C3")
    ap.add_argument("shapes", nargs="*")
    args = ap.parse_args()
    args.shapes = args.shapes or SHAPES
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("noise_ab: --parent-lib must name the library built from the parent commit")
    import numpy as np
    p1 = run_child("parent", args.parent_lib, args.shapes, args.blocks)
    th = run_child("this", "", args.shapes, args.blocks)
    p2 = run_child("parent", args.parent_lib, args.shapes, args.blocks)
    lines = ["# tools/noise_ab.py, %s; ms per call incl. synchronisation, best of %d blocks; ONE run of this tool" % (time.strftime("%Y-%m-%d"), args.blocks),
             "# parent 1 | parent 2: the parent commit's library, run twice (spread = yardstick); (d) this build, defaults; (m) a model set;",
             "# (s) callback with a set_noise before every call"]
    for s in args.shapes:
        a, b, t = p1[s]["ms"]["d"], p2[s]["ms"]["d"], th[s]["ms"]
        lo, hi = min(a, b), max(a, b)
        spread = (hi - lo) / lo
        d, m = t["d"], t["m"]
        where = "inside the parent's spread" if lo <= d <= hi else ("%.2f %% %s the parent's range" % (abs(d - (lo if d < lo else hi)) / (lo if d < lo else hi) * 100, "below" if d < lo else "above"))
        line = "%-20s %-16s parent %9.4f | %9.4f (spread %.2f %%)   (d) %9.4f: %s   (m) %9.4f = (d) x %.4f" % (
            s, th[s]["form"], a, b, spread * 100, d, where, m, m / d)
        if "s" in t:
            line += "   (s) %9.4f: set_noise per solve adds %.1f us" % (t["s"], (t["s"] - m) * 1e3)
        lines.append(line)
    for cfg in [c for c in args.dump_configs.split(",") if c]:
        with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
            dump(args.parent_lib, da, cfg)
            dump("", db, cfg)
            names = sorted(os.listdir(da))
            same = names == sorted(os.listdir(db)) and all(
                np.array_equal(np.load(os.path.join(da, n)).view(np.uint64), np.load(os.path.join(db, n)).view(np.uint64)) for n in names)
            lines.append("bench.py --config %s --dump-outputs: %s under both libraries: %s" % (cfg, ", ".join(names), "bit-equal" if same else "DIFFERENT"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
