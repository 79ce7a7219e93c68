"""Replica ensembles with prescribed velocity components: what the component mask costs (include/rbl.h sections 5 and 7).

Workload: cfg 1, 10 x shell_N_12 above the wall, deterministic steps (rtol 1e-8), R in {1, 256} replicas, ms per ensemble step.

  whole_body   rbl_ensemble_step_mixed with bodies 0, 1, 2 held -- on THIS build and, with --parent-root, on a build of the parent
               commit (a checkout of it, built, anywhere on this machine).  The two alternate, visit by visit, each visit a fresh
               process that imports the package from its own root; the windows of all visits of a build are pooled.  The verdict
               line compares this build's median with the parent's, against the PARENT's own window spread: the parent is the
               yardstick.
  dof          rbl_ensemble_step_mixed_dof on this build with the rotations of all bodies prescribed (a spin about y), z of all
               bodies held, and a random half of the components.
  sequential   the loop of rbl_step_mixed_dof on one context with the same three masks, and the ensemble's replica-steps/s over it.

Every window starts from the same configuration, is timed by the host clock around `steps` steps and ends in a device synchronise
(each step reads its results back anyway).  Every line carries the windows, their spread (max - min) / median and the iteration
count.  One JSON line per measurement, appended to --out.

    python tools/bench_ensemble_dof.py [--parent-root DIR] [--steps 400] [--rounds 5] [--visits 2] [--reps 1,256]
                                       [--out profiles/ensemble_dof.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IT, RTOL = 100, 1e-8
NB = 10
NAME = "cfg1_10x12_wall"


def _inputs(which):
    """mask (NB, 6) and body_in (6 NB): small loads on the free components, the velocities of the prescribed ones"""
    rng = np.random.default_rng(7)
    load = 0.1 * rng.standard_normal((NB, 6))
    vel = 0.1 * rng.uniform(-1.0, 1.0, (NB, 6))
    P = np.zeros((NB, 6), dtype=bool)
    if which == "whole_body":
        P[:3] = True
        vel[:] = 0.0                                        # held
    elif which == "rotations":
        P[:, 3:] = True
        vel[:] = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]             # a spin about the lab's y axis
    elif which == "z":
        P[:, 2] = True
        vel[:] = 0.0
    elif which == "random":
        P = rng.random((NB, 6)) < 0.5
    else:
        raise KeyError(which)
    return P, np.where(P, vel, load).reshape(-1)


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    import rigid_body_light_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    c = make_config(NB, 12, True)

    def ctx():
        return DeviceContext(c["a"], 1.0, True, cfg=c["cfg"], dt=c["dt"], kBT=1.0, stream_ptr=stream)

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

    def line(mode, mask, R, ts, iters, **more):
        med = float(np.median(ts))
        d = {"workload": NAME, "build": args.label, "mode": mode, "mask": mask, "R": R, "steps_per_window": args.steps,
             "windows_ms": [round(1e3 * t, 4) for t in ts], "ms_per_step": round(1e3 * med, 4),
             "window_spread": round((max(ts) - min(ts)) / med, 4), "mean_iters": round(float(np.mean(iters)), 2)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    reps = [int(r) for r in args.reps.split(",")]
    for which in args.kinds.split(","):
        P, bi = _inputs(which)
        seq = None
        if which != "whole_body":                             # the sequential loop on one context
            s = ctx()
            s.set_config(c["X"], c["Q"])
            m = np.ascontiguousarray(P, dtype=np.uint8).reshape(-1)
            F = np.zeros(6 * NB)
            it, res = C.c_int(0), C.c_double(0.0)

            def one():
                s._chk(s.L.rbl_step_mixed_dof(s.h, m.ctypes.data, bi.ctypes.data, None, IT, RTOL, F.ctypes.data, C.byref(it), C.byref(res)))
                return it.value
            ts, out = windows(lambda: s.set_config(c["X"], c["Q"]), one)
            s.close()
            seq = line("sequential_step_mixed_dof", which, 1, ts, out)
        for R in reps:
            X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
            e = ctx()
            e.ensemble_set_config(X, Q)
            if which == "whole_body":
                mask = np.ascontiguousarray(P[:, 0])
                step = lambda: e.ensemble_step_mixed(mask, bi, max_iter=IT, rtol=RTOL)[1]
                mode = "ensemble_step_mixed"
            else:
                step = lambda: e.ensemble_step_mixed_dof(P, bi, max_iter=IT, rtol=RTOL)[1]
                mode = "ensemble_step_mixed_dof"
            ts, out = windows(lambda: e.ensemble_set_config(X, Q), step)
            e.close()
            more = {}
            if seq is not None:
                more["replica_steps_over_sequential"] = round(R * seq / float(np.median(ts)), 2)
            line(mode, which, R, ts, out, **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_dof.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="whole_body", help=argparse.SUPPRESS)
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

    pooled = {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "whole_body"):
                d["visit"] = v
                emit(d)
                pooled.setdefault((label, d["R"]), []).extend(d["windows_ms"])
    for R in sorted({k[1] for k in pooled}):
        t = pooled[("this", R)]
        d = {"workload": NAME, "mode": "whole_body_check", "mask": "whole_body", "R": R, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if ("parent", R) in pooled:
            p = pooled[("parent", R)]
            mp = float(np.median(p))
            d.update({"parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        emit(d)
    for d in visit(HERE, "this", "rotations,z,random"):
        emit(d)


if __name__ == "__main__":
    main()
