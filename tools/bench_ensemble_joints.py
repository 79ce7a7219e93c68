"""Replica ensembles with hard joints: what one jointed step of R replicas costs (include/rbl.h section 5, rbl_ensemble_step_jointed).

  jointed      ms per Ensemble.step_jointed at R in {1, 256}, GMRES to 1e-8, for two systems above the wall:
                 chain    cfg 1 (10 x shell_N_12) with the 9-joint ball chain of tools/bench_joints.py through the bodies in index
                          order, small random loads, gamma = 0 (the anchors are drawn at random: the joints are open and stay so)
                 swimmer  the 3-link swimmer of examples/three_link_swimmer.py: two driven hinges (a ball and a lock joint each),
                          the motors running, gamma = 1
  sequential   the same step from the single-context RigidBody.step_jointed with the diagonal preconditioner, one replica after
               the other, and the ensemble's replica-steps per second over it.
  plain        Ensemble.step_deterministic of cfg 1 (no joints) on THIS build and, with --parent-root, on a build of the parent
               commit (a built checkout of it anywhere on this machine).  The two alternate, visit by visit, each visit a fresh
               process that imports the package from its own root; the windows of all visits of a build are pooled.  The verdict
               line compares this build's median with the parent's against the PARENT's own window spread.

Every window starts from the same configuration (and motor angles), is timed by the host clock around `steps` steps and ends in a
device synchronise.  One JSON line per measurement, appended to --out.

    python tools/bench_ensemble_joints.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--reps 1,256]
                                          [--out profiles/ensemble_joints.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IT, RTOL = 100, 1e-8


def chain(X, seed=3):
    """joints through the bodies in index order, anchors off the centres (tools/bench_joints.py's)"""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    return np.array([[i, i + 1] for i in range(n - 1)]), 0.3 * rng.standard_normal((n - 1, 6))


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import Ensemble, RigidBody, load_structure, make_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    reps = [int(r) for r in args.reps.split(",")]

    def windows(reset, step):
        for _ in range(args.warmup):
            out = step()
        ts = []
        for _ in range(args.rounds):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / args.steps)
        return ts, out

    def line(mode, workload, R, ts, iters, **more):
        med = float(np.median(ts))
        d = {"workload": workload, "build": args.label, "mode": mode, "R": R, "steps_per_window": args.steps,
             "windows_ms": [round(1e3 * t, 4) for t in ts], "ms_per_step": round(1e3 * med, 4),
             "window_spread": round((max(ts) - min(ts)) / med, 4), "mean_iters": round(float(np.mean(iters)), 2)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    c = make_config(10, 12, True)
    if "plain" in args.kinds:
        F = 0.1 * np.random.default_rng(7).standard_normal(60)
        for R in reps:
            X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
            e = Ensemble(c["cfg"], X, Q, c["a"], c["eta"], c["dt"], kBT=0.0, wall=True)
            ts, out = windows(lambda: e.set_config(X, Q), lambda: e.step_deterministic(F, max_iter=IT, rtol=RTOL)[0])
            e.close()
            line("ensemble_step_deterministic", "cfg1_10x12_wall", R, ts, out)
    if "jointed" not in args.kinds:
        return
    from rigid_body_light_amd._lib import JOINT_BALL, joint_rows
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    pitch = 2.0 * Rb + 4.0 * a
    Xs = np.array([[(i - 1) * pitch, 0.0, 3.0] for i in range(3)])
    Qs = np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    body, anchor = chain(c["X"])
    cases = {
        "chain": dict(cfg=c["cfg"], X=c["X"], Q=c["Q"], a=c["a"], dt=c["dt"], gamma=0.0, F=0.1 * np.random.default_rng(7).standard_normal(60),
                      rows=dict(body=body, kind=np.zeros(body.shape[0], dtype=np.int32), anchor_a=anchor[:, :3], anchor_b=anchor[:, 3:]),
                      rates=None, workload="cfg1_10x12_wall_chain9"),
        "swimmer": dict(cfg=cfg, X=Xs, Q=Qs, a=a, dt=0.02, gamma=1.0, F=np.zeros(18), rows=None, rates=[0.0, 0.3, 0.0, -0.3],
                        workload="swimmer_3x12_wall_two_motors"),
    }
    for name, k in cases.items():
        s = RigidBody(k["cfg"], k["X"], k["Q"], k["a"], 1.0, k["dt"], wall_PC=True, block_PC=False)
        if k["rows"] is None:
            z = [0.0, 0.0, 1.0]
            k["rows"] = joint_rows(s.motor(1, 0, 0.5 * (k["X"][0] + k["X"][1]), z), s.motor(1, 2, 0.5 * (k["X"][1] + k["X"][2]), z))
        s.set_joint_kinds(**k["rows"])
        if k["rates"] is not None:
            s.set_joint_rates(k["rates"])

        def reset_single():
            s.set_config(k["X"], k["Q"])
            s.set_joint_kinds(**k["rows"])                     # (the motor angles start again at zero)
            if k["rates"] is not None:
                s.set_joint_rates(k["rates"])
        ts, out = windows(reset_single, lambda: s.step_jointed(k["F"], gamma=k["gamma"], max_iter=IT, rtol=RTOL)[1])
        seq = line("sequential_step_jointed_diagonal_pc", k["workload"], 1, ts, out, joints=int(k["rows"]["body"].shape[0]))
        for R in reps:
            X, Q = np.repeat(k["X"][None], R, axis=0), np.repeat(k["Q"][None], R, axis=0)
            e = Ensemble(k["cfg"], X, Q, k["a"], 1.0, k["dt"], kBT=0.0, wall=True)
            e.set_joint_kinds(**k["rows"])
            if k["rates"] is not None:
                e.set_joint_rates(k["rates"])

            def reset():
                e.set_config(X, Q)
                e.set_joint_angles(np.zeros(k["rows"]["body"].shape[0]))
            ts, out = windows(reset, lambda: e.step_jointed(k["F"], gamma=k["gamma"], max_iter=IT, rtol=RTOL)[1])
            e.close()
            line("ensemble_step_jointed", k["workload"], R, ts, out, joints=int(k["rows"]["body"].shape[0]),
                 replica_steps_over_sequential=round(R * seq / float(np.median(ts)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_joints.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="plain", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--reps", args.reps]
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

    for d in visit(HERE, "this", "jointed"):
        emit(d)
    pooled = {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "plain"):
                d["visit"] = v
                emit(d)
                pooled.setdefault((label, d["R"]), []).extend(d["windows_ms"])
    for R in sorted({k[1] for k in pooled}):
        t = pooled[("this", R)]
        d = {"workload": "cfg1_10x12_wall", "mode": "unjointed_step_check", "R": R, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if ("parent", R) in pooled:
            p = pooled[("parent", R)]
            mp = float(np.median(p))
            d.update({"parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        emit(d)


if __name__ == "__main__":
    main()
