#!/usr/bin/env python3
"""Timings around the commanded input under feedback (include/gpmpc.h, "the commanded input") on one MI355X.

    python tools/feedback_inputs_ab.py --out profiles/linprop/inputs_ab.txt [--parent-lib PATH/libgpmpc_hip.so] [--quick]

Sizes: N = 2048 and N = 300 (ds = 4, da = 1, H = 20, a Kinv per GP) at B = 1 / 16 / 256, under the TILE and the STREAM form of the step.
  (a) the untouched gpmpc_linearised_fc_rollout (with gradient, one gain) of this build against the library given by --parent-lib (the
      parent commit's build): a library is chosen when the process starts (GPMPC_LIB_PATH), so each block is a fresh child process;
      ``--blocks`` blocks per library, alternating; reported are the SHA-256 of (cost, grad, means, covs) of both and the median block
      with its spread.  Without --parent-lib the part is left out and said so.
  (b) gpmpc_linearised_fc_rollout_inputs with the input cost and two input rows against the same rollout without them, with gradient:
      alternating blocks in one process (tools/linprop_fc_ab.py's method).
  (c) particle_rollout (P = 1024, H = 20) with and without a gain, the same way.
No ratio is fixed in advance."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, DS, DA = 20, 4, 1
SHAPES = [(2048, (1, 16, 256)), (300, (1, 16, 256))]


def problem(B, rng, torch):
    x0 = torch.as_tensor(rng.uniform(-1, 1, (B, DS)), device="cuda")
    U = torch.as_tensor(rng.uniform(-1, 1, (B, H, DA)), device="cuda")
    return x0, U


def child(a):
    """One block of part (a) with the library this process loaded: {key: [ms per call, digest]}."""
    import time
    import torch
    import gaussian_process_mpc_amd as G
    from linprop_ab import models
    G.require_gpu()
    cost = G.CostParams(-1.0, np.eye(DS), 0.1 * np.eye(DA))
    rng = np.random.default_rng(1)
    K = torch.as_tensor(rng.uniform(-0.5, 0.5, (DA, DS)), device="cuda")
    out = {}
    for n, batches in ([(300, (16,))] if a.quick else SHAPES):
        gm, pack = models(n, DS, DA, False)
        for B in batches:
            x0, U = problem(B, rng, torch)
            for form in ("tile", "stream"):
                f = lambda: G.linearised_rollout(gm, x0, U, cost, form=form, full_covariance=True, feedback=K)  # noqa: E731
                r = f()
                torch.cuda.synchronize()
                h = hashlib.sha256()
                for k in ("cost", "grad", "means", "covs"):
                    h.update(r[k].cpu().numpy().tobytes())
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    f()
                torch.cuda.synchronize()
                out["N=%d B=%d %s" % (n, B, form)] = [1e3 * (time.perf_counter() - t0) / a.reps, h.hexdigest()[:16]]
        del gm, pack
    print("CHILD " + json.dumps(out))


def run_child(a, libpath):
    env = dict(os.environ)
    if libpath:
        env["GPMPC_LIB_PATH"], env["GPMPC_LIB_ALLOW_MISSING"] = libpath, "1"      # (the older build lacks the entries added since)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(txt):
        lines.append(txt)
        print(txt, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    fmt = lambda t: "%.3f (%.3f ... %.3f)" % (float(np.median(t)), min(t), max(t))  # noqa: E731
    say("# tools/feedback_inputs_ab.py: ms per call, median block (min ... max) of %d alternating blocks of %d calls; H = %d, ds = %d, da = %d, "
        "a Kinv per GP" % (a.blocks, a.reps, H, DS, DA))
    # (a) before this process opens the GPU: one child per block and library
    if a.parent_lib:
        say("# (a) gpmpc_linearised_fc_rollout with gradient, this build | the parent commit's library (%s): one fresh process per block"
            % os.path.basename(a.parent_lib))
        new, old = [], []
        for _ in range(a.blocks):
            new.append(run_child(a, None))
            old.append(run_child(a, os.path.abspath(a.parent_lib)))
        for key in new[0]:
            tn, to = [b[key][0] for b in new], [b[key][0] for b in old]
            same = len({b[key][1] for b in new + old}) == 1
            say("(a) %-22s this %s parent %s this/parent %.3f inside the parent's spread: %s bits: %s" % (
                key, fmt(tn), fmt(to), np.median(tn) / np.median(to), "yes" if min(to) <= np.median(tn) <= max(to) else "no",
                "same (%s)" % new[0][key][1] if same else "DIFFERENT"))
    else:
        say("# (a) not measured: no --parent-lib given")
    import torch
    import gaussian_process_mpc_amd as G
    from linprop_ab import models
    from linprop_fc_ab import ab_blocks
    G.require_gpu()
    say("# device: %s" % torch.cuda.get_device_name(0))
    cost = G.CostParams(-1.0, np.eye(DS), 0.1 * np.eye(DA))
    ic = G.InputConstraints.box([-1.0], [1.0], DA, prob=0.95)
    rng = np.random.default_rng(1)
    K = torch.as_tensor(rng.uniform(-0.5, 0.5, (DA, DS)), device="cuda")
    tup = lambda t: "%.3f (%.3f ... %.3f)" % t  # noqa: E731
    for n, batches in ([(300, (16,))] if a.quick else SHAPES):
        gm, pack = models(n, DS, DA, False)
        for B in batches:
            x0, U = problem(B, rng, torch)
            for form in ("tile", "stream"):
                kw = dict(form=form, feedback=K, want_traj=False)
                t_in, t_pl = ab_blocks(lambda: G.linearised_rollout(gm, x0, U, cost, input_cost=True, input_constraints=ic, **kw),
                                       lambda: G.linearised_rollout(gm, x0, U, cost, **kw), a.reps, a.blocks)
                say("(b) N=%d B=%d %-6s with gradient: cost + 2 input rows %s plain %s with/plain %.3f (+%.3f ms)" % (
                    n, B, form, tup(t_in), tup(t_pl), t_in[0] / t_pl[0], t_in[0] - t_pl[0]))
            if B <= 16:
                mu = G.linearised_rollout(gm, x0, U, None, want_grad=False, feedback=K)["means"]
                t_fb, t_ol = ab_blocks(lambda: G.particle_rollout(gm, x0, U, particles=1024, feedback=K, mean_ref=mu, input_constraints=ic),
                                       lambda: G.particle_rollout(gm, x0, U, particles=1024), a.reps, a.blocks)
                say("(c) N=%d B=%d P=1024 particle_rollout: under the gain, with input statistics %s open loop %s with/open %.3f" % (
                    n, B, tup(t_fb), tup(t_ol), t_fb[0] / t_ol[0]))
        del gm, pack
        torch.cuda.empty_cache()
    say("# not measured: objective-only calls, per-step gains, more rows, other ds / da / H, a shared Kinv, sparse models, B above 256, "
        "particle_rollout at B = 256, per-kernel times and hardware counters of the new kernels, multi-GPU")


if __name__ == "__main__":
    main()
