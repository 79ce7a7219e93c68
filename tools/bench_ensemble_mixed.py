"""Replica ensembles with held or driven bodies against the sequential single-context loop (include/rbl.h sections 5 and 7).

Workload: cfg 1, 10 x shell_N_12 above the wall, with 0, 1 and 9 of the 10 bodies prescribed (held).  For each, Brownian steps of
the masked ensemble (dense Cholesky root, seeded noise) at R in {1, 64, 256, 1024} and the loop of
rbl_step_brownian_mixed(method 0) on one context, in the same process, each timed after warm-up and ending in a device
synchronise -> replica-steps/s and the ratio to the sequential loop.

The cost of the mask: at every R the masked step with NOBODY prescribed and the plain rbl_ensemble_step_brownian alternate, several
rounds each on their own context, every window starting from the same configuration and ending in a device synchronise -> the
ratio of the medians next to the spread the plain step shows between its own rounds (the margin against which the ratio is to
be read).

One JSON line per measurement.

    python tools/bench_ensemble_mixed.py [--steps 20] [--rounds 5] [--reps 1,64,256,1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
IT, RTOL = 100, 1e-8


def main():
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", default="1,64,256,1024")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    c = make_config(10, 12, True)
    nb = 10
    name = "cfg1_10x12_wall"
    bi = np.zeros(6 * nb)

    def ctx():
        return DeviceContext(c["a"], 1.0, True, cfg=c["cfg"], dt=c["dt"], kBT=1.0, stream_ptr=stream)

    def window(step, first_seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(args.steps):
            out = step(first_seed + n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    reps = [int(r) for r in args.reps.split(",")]
    for npres in (0, 1, 9):
        mask = np.zeros(nb, dtype=np.uint8)
        mask[:npres] = 1
        s = ctx()
        s.set_config(c["X"], c["Q"])
        step = lambda seed: s.step_brownian_mixed(mask, bi, max_iter=IT, rtol=RTOL, seed=seed, method=0)
        for n in range(args.warmup):
            step(n)
        dt, out = window(step, 100)
        s.close()
        seq = 1.0 / dt
        print(json.dumps({"workload": name, "prescribed": npres, "mode": "sequential", "R": 1, "replica_steps_per_s": round(seq, 1),
                          "ms_per_step": round(1e3 * dt, 3), "iters": int(out[1])}), flush=True)
        for R in reps:
            e = ctx()
            e.ensemble_set_config(np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0))
            step = lambda seed: e.ensemble_step_brownian_mixed(mask, bi, seed=seed, max_iter=IT, rtol=RTOL)
            for n in range(args.warmup):
                step(n)
            dt, out = window(step, 100)
            e.close()
            print(json.dumps({"workload": name, "prescribed": npres, "mode": "ensemble_mixed", "R": R,
                              "replica_steps_per_s": round(R / dt, 1), "ms_per_step": round(dt * 1e3, 3),
                              "ratio_vs_sequential": round(R / dt / seq, 2), "mean_iters": float(np.mean(out[1]))}), flush=True)
    # the cost of the mask: masked with nobody prescribed against the plain step, alternated
    mask = np.zeros(nb, dtype=np.uint8)
    for R in reps:
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        a, b = ctx(), ctx()
        a.ensemble_set_config(X, Q)
        b.ensemble_set_config(X, Q)
        masked = lambda seed: a.ensemble_step_brownian_mixed(mask, bi, seed=seed, max_iter=IT, rtol=RTOL)
        plain = lambda seed: b.ensemble_step_brownian(bi, seed=seed, max_iter=IT, rtol=RTOL)
        for n in range(args.warmup):
            masked(n)
            plain(n)
        tm, tp = [], []
        for k in range(args.rounds):                     # every window from the start: no steric model here, so a long free walk
            b.ensemble_set_config(X, Q)                  # of a thousand replicas ends with blobs inside each other or the wall
            tp.append(window(plain, 100 + k * args.steps)[0])
            a.ensemble_set_config(X, Q)
            tm.append(window(masked, 100 + k * args.steps)[0])
        a.close()
        b.close()
        mp, mm = float(np.median(tp)), float(np.median(tm))
        print(json.dumps({"workload": name, "mode": "mask_cost", "R": R, "rounds": args.rounds, "steps_per_round": args.steps,
                          "plain_ms": [round(1e3 * t, 4) for t in tp], "masked_none_ms": [round(1e3 * t, 4) for t in tm],
                          "plain_median_ms": round(1e3 * mp, 4), "masked_none_median_ms": round(1e3 * mm, 4),
                          "masked_over_plain": round(mm / mp, 4),
                          "plain_spread": round((max(tp) - min(tp)) / mp, 4)}), flush=True)


if __name__ == "__main__":
    main()
