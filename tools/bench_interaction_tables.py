"""Cost of the tabulated pair term beside the built-in force model (include/rbl.h section 4).  One JSON line per measurement:
  eval_cfg3       rbl_interaction_forces_dev at cfg 3 (200 x shell_N_642, wall): built-in model alone, built-in + pair table, pair
                  table alone (device time between two events, median of --reps)
  eval_ens        rbl_ensemble_interaction_forces of R = 256 x cfg 1 (10 x shell_N_12, wall): the same three (wall clock of the
                  call, read-back included, median)
  run_ens         per-step wall clock of a Brownian Ensemble.run of R = 256 x cfg 1: built-in model alone and with the table
The model is tools/bench_interactions.py's (w = 0.3, eps_wall = 1, b_wall = 0.1, eps_blob = 1, b_blob = 0.05, r_cut = 2a + 20 b_blob);
the table holds the same steric law on [2a, r_cut] with n = 1025 points, so both terms walk the same pairs.
    python tools/bench_interaction_tables.py [--reps 50] [--steps 200] [--jsonl out.jsonl]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from rigid_body_light_amd import Ensemble, make_config, tabulate
from rigid_body_light_amd._lib import DeviceContext

MODEL = dict(w=0.3, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
VARIANTS = ("builtin", "builtin+table", "table")


def steric_table(a, n=1025, eps=1.0, b=0.05):
    r_cut = 2 * a + 20 * b
    U = lambda r: eps * (2 * a / r) * np.exp(-(r - 2 * a) / b)
    return tabulate(U, lambda r: -U(r) * (1.0 / r + 1.0 / b), 2 * a, r_cut, n) + (2 * a, r_cut)


def set_variant(obj, a, variant):
    obj.set_interactions(**dict(MODEL, on=variant != "table"))
    obj.set_pair_table(*steric_table(a), on=variant != "builtin")


def eval_cfg3(reps):
    c = make_config(200, 642, True)
    nb = c["X"].shape[0]
    st = torch.cuda.current_stream()
    out = {}
    for variant in VARIANTS:
        ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=st.cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        set_variant(ctx, c["a"], variant)
        FT = torch.empty(6 * nb, dtype=torch.float64, device="cuda:0")
        for _ in range(3):
            ctx.interaction_forces_dev(None, FT.data_ptr())
        ctx.sync_check()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.interaction_forces_dev(None, FT.data_ptr())
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ctx.sync_check()
        out[variant] = dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), blob_pairs=ctx.interaction_stats()[1])
        ctx.close()
    return out


def ensemble(R, variant):
    c = make_config(10, 12, True)
    X = np.tile(c["X"], (R, 1, 1)) + np.random.default_rng(1).uniform(-0.05, 0.05, (R, 10, 3))
    Q = np.tile(c["Q"], (R, 1, 1))
    ens = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=1e-3, kBT=1.0, wall=True)
    set_variant(ens, c["a"], variant)
    return ens


def eval_ens(R, reps):
    out = {}
    for variant in VARIANTS:
        ens = ensemble(R, variant)
        for _ in range(3):
            ens.interaction_forces()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ens.interaction_forces()
            ts.append(1e3 * (time.perf_counter() - t0))
        out[variant] = dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)))
        ens.close()
    return out


def run_ens(R, steps):
    out = {}
    for variant in ("none", "builtin", "builtin+table"):
        ens = ensemble(R, "builtin" if variant == "none" else variant)
        if variant == "none":
            ens.set_interactions(**dict(MODEL, on=False))
        ens.run(20, F=np.zeros(60), seed=1)
        ts = []
        for k in range(3):
            t0 = time.perf_counter()
            ens.run(steps, F=np.zeros(60), seed=100 + 1000 * k)
            ts.append(1e3 * (time.perf_counter() - t0) / steps)
        out[variant] = dict(ms_per_step=float(np.median(ts)), ms_per_step_min=float(np.min(ts)))
        ens.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--jsonl", default="")
    args = ap.parse_args()
    lines = [dict(what="eval_cfg3", n_table=1025, **eval_cfg3(args.reps)),
             dict(what="eval_ens", replicas=args.replicas, n_table=1025, **eval_ens(args.replicas, args.reps)),
             dict(what="run_ens", replicas=args.replicas, steps=args.steps, n_table=1025, **run_ens(args.replicas, args.steps))]
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.jsonl:
        with open(args.jsonl, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
