"""Ensembles in a periodic cell: what a step of R replicas costs with the image sum inside the one-kernel solver (include/rbl.h
section 5, rbl_ensemble_set_periodic).

  periodic     ms per Ensemble.step_deterministic and per Ensemble.step_brownian of the layer of tests/periodic_cases.py: layer10()
               (10 x shell_N_12, 120 blobs, in a cell of three lattice spacings by three plus 0.7) with the built-in force model,
               GMRES to 1e-8, at R in {1, 256}: with the cell off, with (1, 1) and with (2, 2) images.  Mean iteration counts, and
               the cost per image relative to the cell-off step: (t_cell / t_off) / ((2 nx + 1)(2 ny + 1)).
  sequential   the same steps from the single context in its own cell (RigidBody.set_periodic, diagonal preconditioner, the same
               tolerance, lanczos_pc roots for the Brownian step), one replica after the other, and the ensemble's replica-steps
               per second over it.  These figures are reported, not conditioned.
  plain        the cell-off Ensemble.step_deterministic and step_brownian of the same layer on THIS build and, with --parent-root,
               on a build of the parent commit (a built checkout of it anywhere on this machine).  The two alternate, visit by
               visit, each visit a fresh process that imports the package from its own root; the windows of all visits of a build
               are pooled.  The verdict compares this build's median with the parent's against the PARENT's own window spread.

Every window starts from the same configuration, is timed by the host clock around `steps` steps and ends in a device synchronise.
ONE JSON line with every measurement is appended to --out.

    python tools/bench_ensemble_periodic.py [--parent-root DIR] [--steps 50] [--rounds 5] [--visits 2] [--reps 1,256]
                                            [--out profiles/ensemble_periodic.jsonl]
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
MODEL = dict(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)     # 2 R_body + r_cut = 3.6 <= L / 2


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import Ensemble, RigidBody, make_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    reps = [int(r) for r in args.reps.split(",")]

    def windows(reset, step, steps):
        for _ in range(args.warmup):
            out = step()
        ts = []
        for _ in range(args.rounds):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / steps)
        return ts, out

    def line(mode, R, images, ts, iters, steps, **more):
        med = float(np.median(ts))
        d = {"build": args.label, "mode": mode, "R": R, "images": images, "steps_per_window": steps,
             "windows_ms": [round(1e3 * t, 4) for t in ts], "ms_per_step": round(1e3 * med, 4),
             "window_spread": round((max(ts) - min(ts)) / med, 4), "mean_iters": round(float(np.mean(iters)), 2)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    c = make_config(10, 12, True)                              # tests/periodic_cases.py: layer10()
    s = 2.0 * (1.0 + c["a"]) + 0.5
    L = (3.0 * s, 3.0 * s + 0.7)
    dt = 1e-3
    F = 0.1 * np.random.default_rng(7).standard_normal(60)
    kinds = ("det", "bd")

    def ens_step(e, kind, n):
        if kind == "det":
            return e.step_deterministic(F, max_iter=IT, rtol=RTOL)[0]
        n[0] += 1                                              # fresh noise every step: a random walk, not a drift
        return e.step_brownian(F, seed=n[0], max_iter=IT, rtol=RTOL)[0]

    cells = [None] if args.kinds == "plain" else [None, (1, 1), (2, 2)]
    seq = {}
    if args.kinds == "periodic":                               # the sequential single-context loop in its own cell
        for images in ((1, 1), (2, 2)):
            rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt, wall_PC=True, block_PC=False)
            rb.set_interactions(**MODEL)
            rb.set_periodic(L[0], L[1], images=images)
            for kind in kinds:
                n = [0]

                def step():
                    if kind == "det":
                        return rb.step_deterministic(F, max_iter=IT, rtol=RTOL)[0]
                    n[0] += 1
                    return rb.step_brownian(F, seed=n[0], method="lanczos_pc", max_iter=IT, rtol=RTOL)[0]
                ts, out = windows(lambda: rb.set_config(c["X"], c["Q"]), step, args.seq_steps)
                seq[(kind, images)] = line("sequential_single_context_" + kind, 1, list(images), ts, out, args.seq_steps)
    for R in reps:
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        off = {}
        for images in cells:
            e = Ensemble(c["cfg"], X, Q, c["a"], c["eta"], dt, kBT=1.0, wall=True)
            e.set_interactions(**MODEL)
            if images:
                e.set_cell(L[0], L[1], images=images)
            for kind in kinds:
                n = [0]
                ts, out = windows(lambda: e.set_config(X, Q), lambda: ens_step(e, kind, n), args.steps)
                more = {}
                if images:
                    ni = (2 * images[0] + 1) * (2 * images[1] + 1)
                    more["cost_per_image_over_cell_off"] = round(float(np.median(ts)) / off[kind] / ni, 4)
                    more["replica_steps_over_sequential"] = round(R * seq[(kind, images)] / float(np.median(ts)), 2)
                med = line("ensemble_step_" + kind, R, list(images) if images else None, ts, out, args.steps, **more)
                if not images:
                    off[kind] = med
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seq-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_periodic.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="plain", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--steps", str(args.steps),
               "--seq-steps", str(args.seq_steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--reps", args.reps]
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        print("visit: %s build, %s" % (label, kinds), file=sys.stderr, flush=True)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        out = [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("JSON ")]
        for d in out:
            print(json.dumps(d), flush=True)
        return out

    result = {"workload": "layer10_10x12_wall_builtin_model", "rtol": RTOL, "periodic": visit(HERE, "this", "periodic"), "plain": [], "check": []}
    pooled = {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "plain"):
                d["visit"] = v
                result["plain"].append(d)
                pooled.setdefault((label, d["mode"], d["R"]), []).extend(d["windows_ms"])
    for mode, R in sorted({k[1:] for k in pooled}):
        t = pooled[("this", mode, R)]
        d = {"mode": mode, "R": R, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if ("parent", mode, R) in pooled:
            p = pooled[("parent", mode, R)]
            mp = float(np.median(p))
            d.update({"parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        print(json.dumps(d), flush=True)
        result["check"].append(d)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
