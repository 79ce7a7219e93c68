"""What the flow model (include/rbl.h section 8) costs inside a step.

Two workloads: the deterministic step at cfg 3 (200 x shell_N_642 above the wall, block preconditioner) and the deterministic
ensemble step at cfg 1 (10 x shell_N_12 above the wall) with R = 256 replicas, every body under a constant load.  Each in four
states -- off (no model, no slip: the step every commit has), host_slip (no model; the caller passes the term of the window's first
configuration as `slip`, the upload the model removes: the same right-hand side up to the drift of the configuration, so the same
solve), on (shear over the wall and a body-frame slip pattern, evaluated on the device every step), on_record (on, with
RBL_OPT_RECORD_MOMENTS) -- every state on its own context, the states ALTERNATED window by window, every window starting from the
same configuration and ending in a device synchronise; `rounds` windows of `steps` steps each, medians.  What the model costs is
on against host_slip (off solves another right-hand side and takes another number of iterations).  The margin against which "off
costs nothing" and the ratios are to be read is the off state's own (max - min) / median over its windows, printed next to them:
run the same tool on the parent commit (where only the off state exists: --off-only) and compare the off medians within that margin.

One JSON line per workload, appended to profiles/flow.jsonl.

    python tools/bench_flow.py [--steps 20] [--rounds 5] [--off-only] [--skip-cfg3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IT, RTOL = 100, 1e-8


def main():
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--off-only", action="store_true", help="only the state every commit has (the parent's figure)")
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow.jsonl"))
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    states = ["off"] if args.off_only else ["off", "host_slip", "on", "on_record"]
    G = np.zeros((3, 3))
    G[0, 2] = 0.5

    def arm(ctx, state, nb, nblb):
        if state in ("off", "host_slip"):
            return
        ctx.set_background_flow(G=G)
        ctx.set_body_slip(0.1 * np.random.default_rng(1).standard_normal((nblb, 3)), np.linspace(0.0, 1.0, nb))
        if state == "on_record":
            ctx.record_moments()

    def window(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(args.steps):
            out = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    def measure(name, make, reset, step, extra):
        ctxs = {s: make(s) for s in states}
        for s in states:
            reset(ctxs[s])
            for n in range(args.warmup):
                step(ctxs[s], s)
        times = {s: [] for s in states}
        iters = {}
        for k in range(args.rounds):
            for s in states:                                 # alternated: a drift of the machine hits every state alike
                reset(ctxs[s])
                dt, out = window(lambda: step(ctxs[s], s))
                times[s].append(dt)
                iters[s] = float(np.mean(out[0]))
        for c in ctxs.values():
            c.close()
        med = {s: float(np.median(times[s])) for s in states}
        row = dict(extra, workload=name, rounds=args.rounds, steps_per_round=args.steps,
                   ms={s: [round(1e3 * t, 4) for t in times[s]] for s in states},
                   median_ms={s: round(1e3 * med[s], 4) for s in states}, mean_iters=iters,
                   off_spread=round((max(times["off"]) - min(times["off"])) / med["off"], 4))
        for s in states[2:]:
            row[s + "_over_host_slip"] = round(med[s] / med["host_slip"], 4)
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    if not args.skip_cfg3:
        nb, nblb = 200, 642
        c = make_config(nb, nblb, True)
        F = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], nb)
        term3 = {}

        def make3(state):
            ctx = DeviceContext(c["a"], 1.0, True, cfg=c["cfg"], dt=c["dt"], kBT=1.0, stream_ptr=stream)
            ctx._chk(ctx.L.rbl_set_blk_pc(ctx.h, 1))
            arm(ctx, state, nb, nblb)
            if state == "on":
                ctx.set_config(c["X"], c["Q"])
                term3["t"] = ctx.flow_slip()
            return ctx

        measure("cfg3_200x642_wall_step_deterministic", make3, lambda ctx: ctx.set_config(c["X"], c["Q"]),
                lambda ctx, s: ctx.step_deterministic(F, max_iter=IT, rtol=RTOL, slip=term3["t"] if s == "host_slip" else None), {"R": 1})
    nb, nblb, R = 10, 12, args.reps
    c1 = make_config(nb, nblb, True)
    X, Q = np.repeat(c1["X"][None], R, axis=0), np.repeat(c1["Q"][None], R, axis=0)
    F1 = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], nb)
    term1 = {}

    def make1(state):
        ctx = DeviceContext(c1["a"], 1.0, True, cfg=c1["cfg"], dt=c1["dt"], kBT=1.0, stream_ptr=stream)
        ctx.ensemble_set_config(X, Q)
        arm(ctx, state, nb, nblb)
        if state == "on":
            term1["t"] = ctx.ensemble_flow_slip()
        return ctx

    measure("cfg1_10x12_wall_ensemble_step_deterministic", make1, lambda ctx: ctx.ensemble_set_config(X, Q),
            lambda ctx, s: ctx.ensemble_step_deterministic(F1, max_iter=IT, rtol=RTOL, slip=term1["t"] if s == "host_slip" else None),
            {"R": R})


if __name__ == "__main__":
    main()
