#!/usr/bin/env python3
"""Is the HIP path less accurate than the reference's op order where fp64 runs out (sigma_n <= 1e-4 on dense synthetic
training sets), or are both the same noise?  tools/accuracy_stress.py draws ONE problem per noise level (round 2: HIP 8.5e-2
vs 4.1e-2 at sigma_n = 1e-5).  Here: SEEDS problems per noise level (N = 400, ds = 3, da = 1, H = 3, 2 trajectories), max
relative deviation of the propagated variances from the x87 extended-precision yardstick (oracle/cport/gpmpc_cpu_ld.c) for
the HIP path and for the reference's op order evaluated in fp64 (oracle faithful mode: N^3 trace); reported per noise level:
median and range of both, and of their ratio.  Also the same for the README experiment's own data (tests/golden/g10).
Run on the GPU box:  python tools/accuracy_seeds.py [SEEDS]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gaussian_process_mpc_amd as G
from oracle import cport, golden, gpmpc_oracle as O
from gaussian_process_mpc_amd.synth import synth_problem
torch.set_num_threads(16)
seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = lambda a, e: float(np.abs(a[:, 1:] / e[:, 1:] - 1).max())      # noqa: E731
N, ds, da, H = 400, 3, 1, 3
print(f"# N = {N}, ds = {ds}, da = {da}, H = {H}, 2 trajectories, {seeds} seeded problems per noise level; deviation = max |var / var_extended - 1|")
for sn in (1e-2, 1e-3, 1e-4, 1e-5):
    hip, ref = [], []
    for s in range(seeds):
        pb = synth_problem(500 + s, N, ds, da, H, 2, sigma_n=sn)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        kinv = gp.Ky_inv.numpy()
        pack = G.GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"])
        r = G.rollout(pack, pb["x0"], pb["U"], G.CostParams(1e-5, pb["Q"], pb["R"]), want_grad=False)
        e = cport.rollout_extended(pb, kinv, nthreads=16)
        fa = np.stack([O.objective_and_gradient(gp, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], 1e-5,
                                                mode="faithful", want_grad=False)["vars"] for b in range(2)])
        hip.append(dev(r["vars"].cpu().numpy(), e["vars"])); ref.append(dev(fa, e["vars"]))
    hip, ref = np.array(hip), np.array(ref)
    ratio = hip / ref
    print(f"sigma_n={sn:<6g} HIP median {np.median(hip):.1e} [{hip.min():.1e} .. {hip.max():.1e}] | reference op order median {np.median(ref):.1e} "
          f"[{ref.min():.1e} .. {ref.max():.1e}] | HIP / reference: median {np.median(ratio):.2f} [{ratio.min():.2f} .. {ratio.max():.2f}], "
          f"HIP closer in {int((ratio < 1).sum())} of {seeds}")
z = golden.load("g10_readme_regime.npz")          # (two files, triangle-stored inverses: merged by oracle/golden.py)
Ng, dsg, dag, Hg = (int(v) for v in z["dims"])
for si, sn in enumerate(z["sigma_ns"]):
    kinv = np.stack([z[f"s{si}_Ky_inv"]] * dsg)
    pb = {"X": z["X"], "Y": z["Y"], "lambdas": z["lambdas"], "sigma_f": z["sigma_f"], "ds": dsg, "da": dag,
          "x0": np.tile(z["x0"], (z["U"].shape[0], 1)), "U": z["U"]}
    pack = G.GPPack(z["X"], z["Y"], kinv, z["lambdas"], z["sigma_f"])
    r = G.rollout(pack, pb["x0"], pb["U"], G.CostParams(1e-5, z["Q"], z["R"]), want_grad=False)
    e = cport.rollout_extended(pb, kinv, nthreads=16)
    print(f"README experiment data (N = {Ng}, lambda = 0.5 for every GP), sigma_n={sn:g}: HIP {dev(r['vars'].cpu().numpy(), e['vars']):.1e} | "
          f"the REFERENCE's own values (g10 fixture) {dev(z[f's{si}_vars'], e['vars']):.1e}")
