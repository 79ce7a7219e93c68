"""What a run of ensemble steps (rbl_ensemble_run, Ensemble.run) costs per step against the Python loop of one-step calls.

Workload: cfg 1, 10 x shell_N_12 above the wall, with the force model of tools/bench_ensemble.py (weight and wall repulsion), R in
{1, 32, 256} replicas, the Brownian step -- all bodies free, and masked with 9 of the 10 bodies held.  Four variants, ms per step:

    a   the Python loop of step_brownian (step_brownian_mixed when masked)
    b   the same loop with a get_config() after every step (what a trajectory costs today)
    c   run(n_steps, stride=0)
    d   run(n_steps, stride=1)            (a frame per step, downloaded once)

Windows and spread: every variant is timed in `rounds` windows of `steps` steps, the variants alternating inside a round, every
window starting from the same configuration and the same seed and ending in a device synchronise.  Reported per variant: the
windows, their median and the spread (max - min) / median, which is the margin any ratio of two medians is to be read against.
The claims are c against a and d against b, on one build and one box.  --variants a,b measures the loops alone (to compare the
one-step calls of two builds: run the same command on each).

One JSON line per (R, masked); --out appends them to a file as well.

    python tools/bench_ensemble_run.py [--steps 400] [--rounds 5] [--reps 1,32,256] [--variants a,b,c,d] [--out profiles/ensemble_run.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
IT, RTOL = 50, 1e-8


def main():
    import torch
    from rigid_body_light_amd import Ensemble, make_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", default="1,32,256")
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ensemble_run: no GPU (timings are taken on the device or not at all)")
    variants = args.variants.split(",")
    c = make_config(10, 12, True)
    nb, a = 10, c["a"]
    model = dict(w=0.5, eps_wall=4.0, b_wall=0.1, eps_blob=0.0, b_blob=0.05, r_cut=2 * a + 1.0)
    mask = np.zeros(nb, dtype=bool)
    mask[:9] = True
    load = np.zeros(6 * nb)
    S = args.steps
    for R in [int(r) for r in args.reps.split(",")]:
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        for masked in (False, True):
            ens = Ensemble(c["cfg"], X, Q, a=a, eta=1.0, dt=c["dt"], kBT=1.0, wall=True)
            ens.set_interactions(**model)

            def step(seed):
                if masked:
                    return ens.step_brownian_mixed(mask, load, seed=seed, max_iter=IT, rtol=RTOL)
                return ens.step_brownian(load, seed=seed, max_iter=IT, rtol=RTOL)

            def run(n, stride, seed):
                if masked:
                    return ens.run(n, prescribed=mask, body_in=load, seed=seed, stride=stride, max_iter=IT, rtol=RTOL)
                return ens.run(n, F=load, seed=seed, stride=stride, max_iter=IT, rtol=RTOL)

            def variant(v, n, seed):
                if v == "a":
                    for k in range(n):
                        step(seed + k)
                elif v == "b":
                    for k in range(n):
                        step(seed + k)
                        ens.get_config()
                else:
                    run(n, 0 if v == "c" else 1, seed)

            for v in variants:                           # every shape the windows use
                ens.set_config(X, Q)
                variant(v, args.warmup, 0)
            ms = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v in variants:
                    ens.set_config(X, Q)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    variant(v, S, 100)
                    torch.cuda.synchronize()
                    ms[v].append(1e3 * (time.perf_counter() - t0) / S)
            ens.close()
            line = {"workload": "cfg1_10x12_wall", "R": R, "masked_9_of_10": masked, "steps_per_window": S, "rounds": args.rounds}
            for v in variants:
                med = float(np.median(ms[v]))
                line[v + "_ms"] = [round(t, 4) for t in ms[v]]
                line[v + "_median_ms"] = round(med, 4)
                line[v + "_spread"] = round((max(ms[v]) - min(ms[v])) / med, 4)
            for num, den in (("c", "a"), ("d", "b")):
                if num in ms and den in ms:
                    line[num + "_over_" + den] = round(line[num + "_median_ms"] / line[den + "_median_ms"], 4)
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
