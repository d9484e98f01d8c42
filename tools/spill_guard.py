#!/usr/bin/env python3
"""Build-time spill guard (round 5): the register / spill / scratch table of EVERY kernel the library ships, and a budget check.

Round 4 found two compiler miscompiles in spill paths (a D = 8 whole-horizon instance that lost low mantissa words, an inline-asm zero
that broke ds = 7): only the runtime parity tests stood between a compiler update and a silent 1e-6 error.  The build now records
`-Rpass-analysis=kernel-resource-usage` of every translation unit (csrc/Makefile: <object>.res beside each object) and this tool
fails the build (`make check`, __graft_entry__.build(), tests/test_host_cpu.py) when a kernel exceeds its budget:

  * default budget: 0 VGPR spills, 0 bytes of scratch;
  * exemptions are listed BY NAME below with the ceiling they are allowed (instances the planner never takes, or kernels that keep
    runtime-indexed per-thread arrays in scratch by design); anything above its ceiling, or any unlisted kernel that starts to
    spill, is an error.

    python tools/spill_guard.py <build dir> [--table profiles/r05/kernel_resources.txt] [--all]
"""
import glob
import os
import re
import subprocess
import sys

# name pattern (regex on the demangled kernel name) -> (max VGPR spills, max scratch bytes per lane), first match wins.
# Why each is allowed is said on its line; the numbers are ceilings, not targets.
EXEMPT = [
    # bug-compatible direct cross-covariance (moment.hip), D >= 7: D x D arrays per thread, never on the rollout path
    (r"^k_cross_cov<[78], true>", (16, 1200)),
    # D >= 7 whole-horizon instances: gpmpc_choose_shape never takes the whole-horizon form for D >= 7 (plan.hip); forced
    # only by tests/test_gpu_instances.py, which holds every one of them to the C port
    (r"^k_traj_persist<[78], ", (32, 128)),
    # one-launch-per-step kernel for D >= 7 (no BASELINE config beyond C4's D = 7, ds = 6, which runs the <7, 6, true, 0, 1> instance
    # without spills): small spills in the prologue of the multi-GP / D = 8 instances; held by test_gpu_instances.py
    (r"^k_step_fused<[78], ", (32, 128)),
]
# kernels that keep per-thread arrays in scratch BY DESIGN (no register spill: runtime-indexed small matrices outside hot loops)
SCRATCH_OK = [
    (r"^k_cross_cov<", 1200),      # D x D matrices per thread (direct form of src/tools/uncertainty_prop.py:402-465)
    (r"^k_cost_full$", 1400),       # ds x ds LU of the full-covariance cost term per thread (gpmpc_cost / gpmpc_cost_grad: per call, not per pair)
]


def parse_res(path):
    rows, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: +(?:Function Name|Name): (\S+)", line)
        if m:
            cur = {"name": m.group(1), "tu": os.path.basename(path)}
            rows.append(cur)
            continue
        m = re.search(r"remark: +([A-Za-z ]+(?:\[[a-zA-Z/]+\])?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [n.replace("void ", "").split("(")[0] for n in out]


def budget(name):
    for pat, b in EXEMPT:
        if re.search(pat, name):
            return b, pat
    return (0, 0), None


def scratch_allowed(name):
    for pat, b in SCRATCH_OK:
        if re.search(pat, name):
            return b
    return 0


def main(argv):
    if not argv or argv[0].startswith("-"):
        print(__doc__)
        return 2
    build = argv[0]
    table = argv[argv.index("--table") + 1] if "--table" in argv else None
    files = sorted(glob.glob(os.path.join(build, "*.res")))
    if not files:
        print(f"spill_guard: no *.res files under {build} (build with the repository's Makefile)", file=sys.stderr)
        return 2
    rows = []
    for f in files:
        rows += parse_res(f)
    seen, uniq = set(), []
    for r in rows:                                          # a kernel instantiated in two TUs appears once
        if r["name"] not in seen:
            seen.add(r["name"])
            uniq.append(r)
    names = demangle([r["name"] for r in uniq])
    lines, bad = [], []
    for r, n in sorted(zip(uniq, names), key=lambda x: x[1]):
        vs, ss, sc = r.get("VGPRs Spill", 0), r.get("SGPRs Spill", 0), r.get("ScratchSize [bytes/lane]", 0)
        (bv, bs), pat = budget(n)
        if vs == 0:
            bs = max(bs, scratch_allowed(n))
        status = "ok"
        if vs > bv or sc > bs:
            status = "OVER BUDGET"
            bad.append((n, vs, sc, bv, bs))
        elif vs or sc:
            status = f"exempt (<= {bv} spills, {bs} B)" if pat else f"scratch by design (<= {bs} B)"
        lines.append(f"{n:64s} vgpr {r.get('VGPRs', -1):4d} agpr {r.get('AGPRs', 0):3d} sgpr {r.get('TotalSGPRs', r.get('SGPRs', -1)):4d} "
                     f"spill v{vs:3d} s{ss:3d} scratch {sc:5d} occ {r.get('Occupancy [waves/SIMD]', -1)} lds {r.get('LDS Size [bytes/block]', -1):6d}  {status}")
    text = "\n".join(lines)
    if table:
        os.makedirs(os.path.dirname(table) or ".", exist_ok=True)
        with open(table, "w") as f:
            f.write(f"# kernel resources of libgpmpc_hip.so (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), {len(lines)} kernels; "
                    f"written by tools/spill_guard.py\n# budget: 0 VGPR spills / 0 scratch unless exempt by name (tools/spill_guard.py EXEMPT, SCRATCH_OK)\n")
            f.write(text + "\n")
    if "--all" in argv:
        print(text)
    else:
        for ln in lines:
            if not ln.endswith(" ok"):
                print(ln)
    print(f"spill_guard: {len(lines)} kernels, {sum(1 for ln in lines if not ln.endswith(' ok'))} with spills or scratch, {len(bad)} over budget")
    for n, vs, sc, bv, bs in bad:
        print(f"  OVER BUDGET: {n}: {vs} VGPR spills (allowed {bv}), {sc} B scratch (allowed {bs})", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
