"""Timing of the Metropolis sampler (Ensemble.metropolis; include/rbl.h section 5): trials per second and milliseconds per sweep at
R = 1 and R = 256 for cfg 1 (10 x shell_N_12 above the wall, the built-in model), the same with a pair table of n = 1025, and 19 x
shell_N_12 (the most an ensemble holds); beside each the time of one ensemble_interaction_forces evaluation at the same R, the
least a host-loop sampler would pay per trial.  5 windows a figure; one JSON line per system into profiles/ensemble_mc.jsonl.
Both are host wall-clock times of whole calls: a metropolis call includes its own energy_start evaluation, its uploads and its
read-back, so the time per trial is an upper bound on the kernel's and the ratio a lower bound on what the kernel alone would show.
With --parent-tree DIR (a built checkout of the parent commit): the Brownian Ensemble.run step at R = 256 x cfg 1 and the cfg 3 force
evaluation, in fresh processes of the parent's tree and of this one, alternated (tools/bench_blob_types.py's comparison: no kernel of
theirs changes, so the ratio of the medians has to lie inside the parent's own window spread).  With --resources: VGPRs, SGPRs, LDS
bytes and scratch of k_ens_mc, from the compiler's resource remarks for the source as the build compiles it (needs hipcc).

    python tools/bench_ensemble_mc.py [--sweeps 64] [--windows 5] [--parent-tree DIR] [--resources] [--out profiles/ensemble_mc.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lattice(nb, spacing, R, seed=0):
    side = int(np.ceil(nb ** (1.0 / 3.0) - 1e-9))
    i = np.arange(nb)
    X = np.stack([i % side, (i // side) % side, i // (side * side)], axis=1) * spacing + [0.0, 0.0, spacing]
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((R, nb, 4))
    return np.tile(X, (R, 1, 1)) + rng.uniform(-0.1, 0.1, (R, nb, 3)), Q / np.linalg.norm(Q, axis=-1, keepdims=True)


def windows(fn, n):
    import torch
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def resources():
    """k_ens_mc's registers, LDS and scratch: the remarks of a device-only compile with the build's flags"""
    import re
    import subprocess
    import tempfile
    spec_path = os.path.join(ROOT, "rigid_body_light_amd", "build.py")
    import importlib.util
    spec = importlib.util.spec_from_file_location("rbl_build", spec_path)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + b.ARCH, "-x", "hip", "--offload-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(b.CSRC, "rbl_ens_mc.hip"), "-o",
                            os.path.join(tmp, "mc.o")], capture_output=True, text=True, check=True)
    out = dict(what="k_ens_mc_resources", arch=b.ARCH)
    for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
        out[key] = int(re.search(pat, p.stderr).group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--sweeps", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_mc.jsonl"))
    args = ap.parse_args()
    from rigid_body_light_amd import Ensemble, load_structure
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max())
    r = np.linspace(0.0, 4.0 * a, 1025)
    table = (-0.5 * np.exp(-(r - 2 * a) ** 2), (r - 2 * a) * np.exp(-(r - 2 * a) ** 2), 0.0, 4.0 * a)
    lines = []
    for name, nb, tab in (("cfg1", 10, None), ("cfg1_pair_table_1025", 10, table), ("shells_19", 19, None)):
        for R in (1, 256):
            X, Q = lattice(nb, 2.0 * (Rb + a) + 0.5, R)
            ens = Ensemble(cfg, X, Q, a=a, eta=1.0, dt=0.01, kBT=1.0, wall=True)
            ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1, eps_blob=4.0, b_blob=0.1, r_cut=3.0 * a)
            if tab is not None:
                ens.set_pair_table(*tab)
            ens.metropolis(args.sweeps, 0.1, 0.1, seed=1)                                   # burn-in, warm-up
            w = windows(lambda: ens.metropolis(args.sweeps, 0.1, 0.1, seed=2), args.windows)
            e = windows(lambda: ens.interaction_energy(), args.windows)
            t, te = float(np.median(w)), float(np.median(e))
            trials = args.sweeps * nb
            lines.append(dict(system=name, R=R, n_bodies=nb, sweeps=args.sweeps, call_ms=1e3 * t, call_ms_windows=[1e3 * x for x in w],
                              ms_per_sweep=1e3 * t / args.sweeps, us_per_trial_per_replica=1e6 * t / trials,
                              trials_per_s=trials * R / t, forces_eval_ms=1e3 * te, forces_eval_ms_windows=[1e3 * x for x in e],
                              eval_over_trial=te / (t / trials)))
            print(json.dumps(lines[-1]))
            ens.close()
    if args.parent_tree:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import bench_blob_types as bt
        line = bt.never_set_vs_parent(argparse.Namespace(parent_tree=args.parent_tree, windows=args.windows, reps=100, steps=200, replicas=256))
        line["what"] = "unchanged_kernels_vs_parent"
        lines.append(line)
        print(json.dumps(line))
    if args.resources:
        lines.append(resources())
        print(json.dumps(lines[-1]))
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
