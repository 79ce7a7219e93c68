"""Driven ensemble runs (include/rbl.h section 5, rbl_ensemble_run_driven; Ensemble.run_driven): what the drive and the lock-in sums
cost inside a run, what the run saves over the loop it replaces, and that the paths it does not touch cost what they did.

Workload: cfg 1 -- 10 x shell_N_12 above the wall with the built-in force model (tools/bench_ensemble_observed.py's), GMRES to
1e-8, Brownian steps -- at R in {1, 256}; the protocol of tools/bench_ensemble_run.py: 5 windows of 200 steps, every window from
the same configuration and seed, timed by the host clock and ended by a device synchronise, the variants alternating inside a round.

  driven       ms per step of Ensemble.run (F constant), of Ensemble.run_driven with a harmonic part (cos and sin amplitudes per
               replica, one frequency per replica) and lockin=True, and of the loop that run replaces: Ensemble.drive_eval (one
               launch and a read-back) followed by step_brownian(seed + n).  Recorded: run_driven over run (the added cost is two
               launches over R 6 N_bod entries; no target), run_driven over the loop with the loop's own window spread, and
               whether the run lies below the loop by more than that spread.
  plain        Ensemble.run (Brownian) and the one-step step_brownian on THIS build and, with --parent-root, on a build of the
               parent commit (a built checkout of it anywhere on this machine), alternated visit by visit, each visit a fresh
               process that imports the package from its own root; the windows of all visits of a build are pooled.  The verdict
               compares this build's median with the parent's against the PARENT's own window spread.

ONE JSON line with every measurement is appended to --out.

    python tools/bench_ensemble_driven.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--reps 1,256]
                                          [--parts driven,plain] [--out profiles/ensemble_driven.jsonl]
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
MODEL = dict(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import Ensemble, make_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    reps = [int(r) for r in args.reps.split(",")]
    c = make_config(10, 12, True)
    nb, dt = 10, 1e-3
    F = 0.1 * np.random.default_rng(7).standard_normal(6 * nb)

    def timed(reset, variants, steps, rounds):
        for w in variants.values():
            reset()
            w(max(args.warmup, 1))
        ms = {v: [] for v in variants}
        for _ in range(rounds):
            for v, w in variants.items():
                reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w(steps)
                torch.cuda.synchronize()
                ms[v].append(1e3 * (time.perf_counter() - t0) / steps)
        return ms

    def stats(ts):
        med = float(np.median(ts))
        return {"windows_ms": [round(t, 4) for t in ts], "ms_per_step": round(med, 4), "window_spread": round((max(ts) - min(ts)) / med, 4)}

    def emit(d):
        d["build"] = args.label
        print("JSON " + json.dumps(d), flush=True)

    for R in reps:
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        e = Ensemble(c["cfg"], X, Q, c["a"], c["eta"], dt, kBT=1.0, wall=True)
        e.set_interactions(**MODEL)
        n = [0]

        def steps_bd(k):
            for _ in range(k):
                n[0] += 1
                e.step_brownian(F, seed=n[0], max_iter=IT, rtol=RTOL)
        variants = {"run": lambda k: e.run(k, F=F, seed=100, max_iter=IT, rtol=RTOL), "step_brownian": steps_bd}
        if args.kinds == "driven":
            rng = np.random.default_rng(11)
            Cc, Ss = 0.05 * rng.standard_normal((R, 6 * nb)), 0.05 * rng.standard_normal((R, 6 * nb))
            om = np.geomspace(1.0, 1.0e3, R) if R > 1 else np.array([30.0])
            drive = dict(cos=Cc, sin=Ss, omega=om)

            def loop(k):
                acc = np.zeros(R, dtype=np.int32)
                for m in range(k):
                    acc[:] = m
                    inp, _ = e.drive_eval(F, accepted=acc, **drive)
                    e.step_brownian(inp, seed=100 + m, max_iter=IT, rtol=RTOL)
            variants = {"run": variants["run"], "run_driven": lambda k: e.run_driven(k, F=F, seed=100, lockin=True, max_iter=IT, rtol=RTOL, **drive),
                        "loop": loop}
        ms = timed(lambda: e.set_config(X, Q), variants, args.steps, args.rounds)
        e.close()
        if args.kinds == "driven":
            st = {v: stats(ts) for v, ts in ms.items()}
            emit(dict(mode="driven_run_vs_run_and_loop", R=R, steps_per_window=args.steps, run=st["run"], run_driven=st["run_driven"], loop=st["loop"],
                      driven_over_run=round(st["run_driven"]["ms_per_step"] / st["run"]["ms_per_step"], 4),
                      added_ms_per_step=round(st["run_driven"]["ms_per_step"] - st["run"]["ms_per_step"], 4),
                      driven_over_loop=round(st["run_driven"]["ms_per_step"] / st["loop"]["ms_per_step"], 4),
                      run_beats_loop_by_more_than_its_spread=bool(st["run_driven"]["ms_per_step"] <
                                                                  st["loop"]["ms_per_step"] * (1.0 - st["loop"]["window_spread"]))))
        else:
            for mode, ts in ms.items():
                emit(dict(mode=mode, R=R, steps_per_window=args.steps, **stats(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parts", default="driven,plain")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_driven.jsonl"))
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
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        out = [json.loads(ln[5:]) for ln in p.stdout.splitlines() if ln.startswith("JSON ")]
        for d in out:
            print(json.dumps(d), flush=True)
        return out

    parts = args.parts.split(",")
    result = {"workload": "cfg1_10x12_wall_builtin_model_brownian", "rtol": RTOL, "visits": args.visits,
              "driven": visit(HERE, "this", "driven") if "driven" in parts else [], "plain": [], "check": []}
    pooled, medians = {}, {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits if "plain" in parts else 0):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "plain"):
                d["visit"] = v
                result["plain"].append(d)
                pooled.setdefault((label, d["mode"], d["R"]), []).extend(d["windows_ms"])
                medians.setdefault((label, d["mode"], d["R"]), []).append(d["ms_per_step"])
    for mode, R in sorted({k[1:] for k in pooled}):
        t = pooled[("this", mode, R)]
        d = {"mode": mode, "R": R, "this_ms_per_step": round(float(np.median(t)), 4),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t),
             "this_visit_medians": medians[("this", mode, R)]}
        if ("parent", mode, R) in pooled:
            p = pooled[("parent", mode, R)]
            mp = float(np.median(p))
            d.update({"parent_visit_medians": medians[("parent", mode, R)], "parent_ms_per_step": round(mp, 4),
                      "parent_window_spread": round((max(p) - min(p)) / mp, 4), "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        print(json.dumps(d), flush=True)
        result["check"].append(d)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
