"""Ensemble runs with hard joints: what a jointed step costs inside Ensemble.run_jointed against the loop it replaces (include/rbl.h
section 5, rbl_ensemble_run_jointed), in the manner of tools/bench_ensemble_joints.py.

  systems      chain    cfg 1 (10 x shell_N_12) above the wall with the 9-joint ball chain of tools/bench_joints.py, small random
                        loads, gamma = 0, no motors (the stored rates: zero)
               swimmer  the 3-link swimmer of examples/ensemble_swimmers.py with its four-stroke schedule, 25 steps per stroke,
                        gamma = 1
               each at R in {1, 256}, GMRES to 1e-8.
  variants     loop         set_joint_rates at the stroke boundaries + step_jointed
               loop_state   the same with joint_state() every step, as examples/ensemble_swimmers.py does
               run          run_jointed, one call per window
               run_frames   run_jointed with a frame per step (stride = 1)
               The verdict line of a case: run below loop by more than the spread of the loop's own windows.
  no regression  Ensemble.step_jointed (the swimmer, R = 256) and a plain Brownian Ensemble.run (cfg 1, R = 256) on THIS build and, with
               --parent-root, on a build of the parent commit; the two alternate, visit by visit, each visit a fresh process that
               imports the package from its own root, and the windows of all visits of a build are pooled.  The verdict line
               compares this build's median with the parent's against the PARENT's own window spread.

Every window starts from the same configuration and motor angles, is timed by the host clock around `steps` steps and ends in a
device synchronise.  One JSON line per measurement, appended to --out.

    python tools/bench_ensemble_run_joints.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--reps 1,256]
                                              [--out profiles/ensemble_run_joints.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IT, RTOL, STROKE = 100, 1e-8, 25


def chain(X, seed=3):
    """joints through the bodies in index order, anchors off the centres (tools/bench_joints.py's)"""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    return np.array([[i, i + 1] for i in range(n - 1)]), 0.3 * rng.standard_normal((n - 1, 6))


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import Ensemble, load_structure, make_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    reps = [int(r) for r in args.reps.split(",")]

    def windows(reset, window):
        """window(): `steps` steps, however it makes them -> something of the last one"""
        reset()
        out = window(max(args.warmup, 1))
        ts = []
        for _ in range(args.rounds):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = window(args.steps)
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
        return d

    from rigid_body_light_amd._lib import joint_rows
    c = make_config(10, 12, True)
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    pitch = 2.0 * Rb + 4.0 * a
    Xs = np.array([[(i - 1) * pitch, 0.0, 3.0] for i in range(3)])
    Qs = np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    omega = 0.6 / (STROKE * 0.02)
    strokes = np.zeros((4, 4))
    for k, (s1, s2) in enumerate([(+1, 0), (0, +1), (-1, 0), (0, -1)]):
        strokes[k, [1, 3]] = [s1 * omega, -s2 * omega]

    def swimmer(R):
        X, Q = np.repeat(Xs[None], R, axis=0), np.repeat(Qs[None], R, axis=0)
        e = Ensemble(cfg, X, Q, a, 1.0, 0.02, kBT=0.0, wall=True)
        z = [0.0, 0.0, 1.0]
        e.set_joint_kinds(**joint_rows(e.motor(1, 0, 0.5 * (Xs[0] + Xs[1]), z), e.motor(1, 2, 0.5 * (Xs[1] + Xs[2]), z)))
        return e, X, Q

    if "plain" in args.kinds:                                  # what the parent has too: the one-step jointed call and a plain Brownian run
        R = max(reps)
        e, X, Q = swimmer(R)
        e.set_joint_rates(strokes[0])

        def reset():
            e.set_config(X, Q)
            e.set_joint_angles(np.zeros(4))

        def loop(n):
            for _ in range(n):
                out = e.step_jointed(np.zeros(18), gamma=1.0, max_iter=IT, rtol=RTOL)[1]
            return out
        ts, out = windows(reset, loop)
        e.close()
        line("ensemble_step_jointed", "swimmer_3x12_wall_two_motors", R, ts, out)
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        e = Ensemble(c["cfg"], X, Q, c["a"], 1.0, c["dt"], kBT=1.0, wall=True)       # tools/bench_ensemble_run.py's free Brownian run
        e.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1, eps_blob=0.0, b_blob=0.05, r_cut=2 * c["a"] + 1.0)
        F = np.zeros(60)
        ts, out = windows(lambda: e.set_config(X, Q), lambda n: e.run(n, F=F, brownian=True, seed=5, max_iter=IT, rtol=RTOL).iters_sum / n)
        e.close()
        line("ensemble_run_brownian", "cfg1_10x12_wall", R, ts, out)
    if "jointed" not in args.kinds:
        return
    body, anchor = chain(c["X"])
    for R in reps:
        for name in ("chain", "swimmer"):
            if name == "chain":
                X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
                e = Ensemble(c["cfg"], X, Q, c["a"], 1.0, c["dt"], kBT=0.0, wall=True)
                e.set_joint_kinds(body, None, anchor[:, :3], anchor[:, 3:])
                F, gamma, nj, sched, workload = 0.1 * np.random.default_rng(7).standard_normal(60), 0.0, 9, None, "cfg1_10x12_wall_chain9"
            else:
                e, X, Q = swimmer(R)
                F, gamma, nj, sched, workload = np.zeros(18), 1.0, 4, ([STROKE] * 4, strokes), "swimmer_3x12_wall_four_strokes"

            def reset():
                e.set_config(X, Q)
                e.set_joint_angles(np.zeros(nj))

            def loop(n, state=False):
                for k in range(n):
                    if sched is not None and k % STROKE == 0:
                        e.set_joint_rates(strokes[(k // STROKE) % 4])
                    out = e.step_jointed(F, gamma=gamma, max_iter=IT, rtol=RTOL)[1]
                    if state:
                        e.joint_state()
                return out

            def run(n, stride=0):
                return e.run_jointed(n, F, gamma=gamma, schedule=sched, stride=stride, max_iter=IT, rtol=RTOL).iters_sum / n
            got = {}
            for mode, fn in (("loop", loop), ("loop_state", lambda n: loop(n, True)), ("run", run), ("run_frames", lambda n: run(n, 1))):
                ts, out = windows(reset, fn)
                got[mode] = line(mode, workload, R, ts, out, joints=nj)
            e.close()
            lo, ru = got["loop"], got["run"]
            d = {"workload": workload, "build": args.label, "mode": "run_against_loop", "R": R,
                 "loop_ms_per_step": lo["ms_per_step"], "loop_state_ms_per_step": got["loop_state"]["ms_per_step"],
                 "run_ms_per_step": ru["ms_per_step"], "run_frames_ms_per_step": got["run_frames"]["ms_per_step"],
                 "loop_window_spread": lo["window_spread"], "loop_over_run": round(lo["ms_per_step"] / ru["ms_per_step"], 3),
                 "run_below_loop_by_more_than_its_spread": bool(ru["ms_per_step"] < lo["ms_per_step"] * (1.0 - lo["window_spread"]))}
            print("JSON " + json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_run_joints.jsonl"))
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
                pooled.setdefault((label, d["mode"], d["workload"], d["R"]), []).extend(d["windows_ms"])
    for (label, mode, workload, R) in sorted(k for k in pooled if k[0] == "this"):
        t = pooled[(label, mode, workload, R)]
        d = {"workload": workload, "mode": mode + "_check", "R": R, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if ("parent", mode, workload, R) in pooled:
            p = pooled[("parent", mode, workload, R)]
            mp = float(np.median(p))
            d.update({"parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        emit(d)


if __name__ == "__main__":
    main()
