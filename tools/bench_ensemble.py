"""Replica ensembles against the sequential single-context loop (include/rbl.h section 5).

Workloads: (a) one shell_N_12 above the wall with the force model of examples/ensemble_gibbs.py; (b) cfg 1, 10 x shell_N_12 with
the wall.  For each, ensemble Brownian steps (dense Cholesky root, seeded noise) at R in {1, 64, 256, 1024} and the loop of
rbl_step_brownian(method 0) on one context, in the same process, each timed after warm-up and ending in a device synchronise.
Prints replica-steps/s and the ratio to the sequential loop, one JSON line per measurement.

    python tools/bench_ensemble.py [--steps 20] [--reps 1,64,256,1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload(name):
    from rigid_body_light_amd import load_structure, make_config
    if name == "gibbs_1x12":
        p, cfg = load_structure(12)
        a = p["sep"] / 2.0
        Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
        return dict(cfg=cfg, a=a, X=np.array([[0.1, -0.2, Rb + a + 0.2]]), Q=np.array([[0.9, 0.1, 0.3, -0.2]]), dt=0.02,
                    model=dict(w=0.5, eps_wall=4.0, b_wall=0.1, eps_blob=0.0, b_blob=0.05, r_cut=2 * a + 1.0))
    c = make_config(10, 12, True)
    return dict(cfg=c["cfg"], a=c["a"], X=c["X"], Q=c["Q"], dt=c["dt"], model=None)


def main():
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", default="1,64,256,1024")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    for name in ("gibbs_1x12", "cfg1_10x12_wall"):
        w = workload(name)
        nb = w["X"].shape[0]
        F = np.zeros(6 * nb)

        def ctx():
            c = DeviceContext(w["a"], 1.0, True, cfg=w["cfg"], dt=w["dt"], kBT=1.0, stream_ptr=stream)
            if w["model"]:
                c.set_interactions(**w["model"])
            return c
        s = ctx()
        s.set_config(w["X"], w["Q"])
        for n in range(args.warmup):
            s.step_brownian(F, max_iter=50, rtol=1e-8, seed=n, method=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(args.steps):
            s.step_brownian(F, max_iter=50, rtol=1e-8, seed=100 + n, method=0)
        torch.cuda.synchronize()
        seq = args.steps / (time.perf_counter() - t0)
        s.close()
        print(json.dumps({"workload": name, "mode": "sequential", "R": 1, "replica_steps_per_s": round(seq, 1),
                          "ms_per_step": round(1e3 / seq, 3)}), flush=True)
        for R in [int(r) for r in args.reps.split(",")]:
            e = ctx()
            e.ensemble_set_config(np.repeat(w["X"][None], R, axis=0), np.repeat(w["Q"][None], R, axis=0))
            for n in range(args.warmup):
                e.ensemble_step_brownian(F, seed=n, max_iter=50, rtol=1e-8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(args.steps):
                it, _ = e.ensemble_step_brownian(F, seed=100 + n, max_iter=50, rtol=1e-8)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            e.close()
            print(json.dumps({"workload": name, "mode": "ensemble", "R": R, "replica_steps_per_s": round(R / dt, 1),
                              "ms_per_step": round(dt * 1e3, 3), "ratio_vs_sequential": round(R / dt / seq, 2),
                              "mean_iters": float(np.mean(it))}), flush=True)


if __name__ == "__main__":
    main()
