"""The Brownian midpoint step with prescribed velocity components: that the existing steps did not move, and what the new ones cost
(include/rbl.h sections 5 and 7).

Two workloads: cfg 3 (200 x shell_N_642 above the wall, block preconditioner, lanczos_pc roots to 1e-3, GMRES to 1e-8) on one
context, and R = 256 replicas of cfg 1 (10 x shell_N_12 above the wall, GMRES to 1e-8) as an ensemble.

  parent check  step_brownian_mixed at cfg 3 with nobody prescribed, and Ensemble.step_brownian_mixed at R = 256 x cfg 1 with bodies
                0, 1, 2 held -- on THIS build and, with --parent-root, on a build of the parent commit (a checkout of it, built,
                anywhere on this machine).  The two alternate, visit by visit, each visit a fresh process that imports the package
                from its own root; the windows of all visits of a build are pooled.  The verdict line compares this build's median
                with the parent's against the PARENT's own window spread: the parent is the yardstick.
  new steps     on this build: step_brownian_mixed_dof at cfg 3 with z of all bodies held and with the rotations of all bodies
                driven (a spin about y); Ensemble.step_brownian_mixed_dof at R = 256 x cfg 1 with the same two masks, beside the
                sequential loop of rbl_step_brownian_mixed_dof (dense root) on one context.  Reported, not gated.

Every window starts from the same configuration with the same seeds, is timed by the host clock around `steps` steps after untimed
warm-up steps and ends in a device synchronise (each step reads its results back anyway).  Every line carries the windows, their
spread (max - min) / median and the iteration count.  One JSON line per measurement, appended to --out.

    python tools/bench_brownian_dof.py [--parent-root DIR] [--rounds 5] [--visits 2] [--out profiles/brownian_dof.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IT, RTOL = 200, 1e-8
R_ENS, NB1 = 256, 10


def _mask6(which, nb):
    """mask (nb, 6) and body_in (nb, 6): small loads on the free components, the velocities of the prescribed ones"""
    load = 0.1 * np.random.default_rng(7).standard_normal((nb, 6))
    P, vel = np.zeros((nb, 6), dtype=bool), np.zeros((nb, 6))
    if which == "z":
        P[:, 2] = True                                      # a quasi-2D layer: U_z = 0
    elif which == "rotations":
        P[:, 3:] = True
        vel[:, 4] = 1.0                                     # a spin about the lab's y axis
    else:
        raise KeyError(which)
    return P, np.where(P, vel, load)


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import RigidBody, make_config
    from rigid_body_light_amd._lib import DeviceContext
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream

    def windows(reset, step, steps):
        reset()
        for n in range(args.warmup):
            out = step(n)
        ts = []
        for _ in range(args.rounds):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(steps):
                out = step(n)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / steps)
        return ts, out

    def line(workload, mode, mask, R, steps, ts, iters, **more):
        med = float(np.median(ts))
        d = {"workload": workload, "build": args.label, "mode": mode, "mask": mask, "R": R, "steps_per_window": steps,
             "windows_ms": [round(1e3 * t, 4) for t in ts], "ms_per_step": round(1e3 * med, 4),
             "window_spread": round((max(ts) - min(ts)) / med, 4), "mean_iters": round(float(np.mean(iters)), 2)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    kinds = args.kinds.split(",")
    if any(k.startswith("cfg3") for k in kinds):
        nb = 200
        c = make_config(nb, 642, True)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
        rb.cb.set_lanczos(200, 1e-3)
        F = np.random.default_rng(1).standard_normal((nb, 6))
        reset = lambda: rb.set_config(c["X"], c["Q"])
        for k in kinds:
            if k == "cfg3_none":
                p = np.zeros(nb, dtype=bool)
                step = lambda n: rb.step_brownian_mixed(p, F, seed=1 + n, method="lanczos_pc", max_iter=IT, rtol=RTOL)[1]
                ts, its = windows(reset, step, args.steps3)
                line("cfg3_200x642_wall", "step_brownian_mixed", "none", 1, args.steps3, ts, its)
            elif k.startswith("cfg3_"):
                P, bi = _mask6(k[5:], nb)
                step = lambda n: rb.step_brownian_mixed_dof(P, bi, seed=1 + n, method="lanczos_pc", max_iter=IT, rtol=RTOL)[1]
                ts, its = windows(reset, step, args.steps3)
                line("cfg3_200x642_wall", "step_brownian_mixed_dof", k[5:], 1, args.steps3, ts, its)
    c = make_config(NB1, 12, True)
    ctx = lambda: DeviceContext(c["a"], 1.0, True, cfg=c["cfg"], dt=c["dt"], kBT=1.0, stream_ptr=stream)
    X, Q = np.repeat(c["X"][None], R_ENS, axis=0), np.repeat(c["Q"][None], R_ENS, axis=0)
    for k in kinds:
        if not k.startswith("ens_"):
            continue
        e = ctx()
        e.ensemble_set_config(X, Q)
        reset = lambda: e.ensemble_set_config(X, Q)
        if k == "ens_whole":
            mask = np.arange(NB1) < 3
            bi = np.where(mask[:, None], 0.0, 0.1 * np.random.default_rng(7).standard_normal((NB1, 6))).reshape(-1)
            step = lambda n: e.ensemble_step_brownian_mixed(mask, bi, seed=1 + n, max_iter=IT, rtol=RTOL)[1]
            ts, its = windows(reset, step, args.steps1)
            line("cfg1_10x12_wall", "ensemble_step_brownian_mixed", "whole_body", R_ENS, args.steps1, ts, its)
        else:
            P, bi = _mask6(k[4:], NB1)
            s = ctx()                                          # the sequential loop on one context, dense root as the ensemble's
            seq_reset = lambda: s.set_config(c["X"], c["Q"])
            seq_step = lambda n: s.step_brownian_mixed_dof(P, bi, max_iter=IT, rtol=RTOL, seed=1 + n, method=0)[1]
            ts, its = windows(seq_reset, seq_step, args.steps1)
            s.close()
            seq = line("cfg1_10x12_wall", "sequential_step_brownian_mixed_dof", k[4:], 1, args.steps1, ts, its)
            step = lambda n: e.ensemble_step_brownian_mixed_dof(P, bi.reshape(-1), seed=1 + n, max_iter=IT, rtol=RTOL)[1]
            ts, its = windows(reset, step, args.steps1)
            line("cfg1_10x12_wall", "ensemble_step_brownian_mixed_dof", k[4:], R_ENS, args.steps1, ts, its,
                 replica_steps_over_sequential=round(R_ENS * seq / float(np.median(ts)), 2))
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps3", type=int, default=2, help="steps per window at cfg 3")
    ap.add_argument("--steps1", type=int, default=50, help="steps per window at cfg 1")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "brownian_dof.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="cfg3_none,ens_whole", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--steps3", str(args.steps3),
               "--steps1", str(args.steps1), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        print("visit: %s build, %s" % (label, kinds), file=sys.stderr, flush=True)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        return [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("JSON ")]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(d):                                              # as it is measured: a later failure loses nothing
        print(json.dumps(d), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(d) + "\n")

    pooled = {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "cfg3_none,ens_whole"):
                d["visit"] = v
                emit(d)
                pooled.setdefault((label, d["mode"]), []).extend(d["windows_ms"])
    for mode in sorted({k[1] for k in pooled}):
        t = pooled[("this", mode)]
        d = {"mode": "parent_check", "of": mode, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if ("parent", mode) in pooled:
            p = pooled[("parent", mode)]
            mp = float(np.median(p))
            d.update({"parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        emit(d)
    for d in visit(HERE, "this", "cfg3_z,cfg3_rotations,ens_z,ens_rotations"):
        emit(d)


if __name__ == "__main__":
    main()
