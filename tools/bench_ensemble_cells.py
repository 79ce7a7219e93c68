"""Ensembles with a periodic cell per replica (include/rbl.h section 5, rbl_ensemble_set_cells): what the table costs, what it buys.

The workload is the project's: 10 x shell_N_12 above the wall (tests/periodic_cases.py: layer10(), a cell of three lattice spacings
by three plus 0.7) with the built-in force model, GMRES to 1e-8, windows of `--steps` steps timed by the host clock and ended by a
device synchronise, every window from the same configuration.

  shared      Ensemble.step_deterministic and step_brownian with the SHARED cell (set_cell, (1, 1) images) and with the cell off, at
              R in {1, 256}, on THIS build and, with --parent-root, on a build of the parent commit: the two alternate, visit by
              visit, each visit a fresh process that imports the package from its own root; the windows of all visits of a build
              are pooled.  The verdict compares this build's median with the parent's against the PARENT's own window spread.
  table       the same steps after set_cells with R equal rows, in this build: the table against the by-value cell, judged against
              this build's window spread with set_cell.
  sweep       one Brownian run of R = 256 as 8 cells x 32 replicas (the lattice and the cell stretched together by 1 ... 2) against
              the eight runs of R = 32 with a shared cell each that are needed without a cell per replica; ms per replica-step.
  imbalance   one replica at (4, 4) images among 255 at (1, 1), against all at (1, 1) and all at (4, 4): a launch lasts as long as
              its slowest replica.  Reported, not conditioned.

ONE JSON line with every measurement is appended to --out.

    python tools/bench_ensemble_cells.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--imbalance-steps 50]
                                         [--out profiles/ensemble_cells.jsonl]
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
    from rigid_body_light_amd import Ensemble, make_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"

    def windows(reset, step, steps, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
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

    def line(mode, R, cell, ts, steps, **more):
        med = float(np.median(ts))
        d = {"build": args.label, "mode": mode, "R": R, "cell": cell, "steps_per_window": steps,
             "windows_ms": [round(1e3 * t, 4) for t in ts], "ms_per_step": round(1e3 * med, 4),
             "window_spread": round((max(ts) - min(ts)) / med, 4)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    c = make_config(10, 12, True)                              # tests/periodic_cases.py: layer10()
    s = 2.0 * (1.0 + c["a"]) + 0.5
    L = (3.0 * s, 3.0 * s + 0.7)
    dt = 1e-3
    F = 0.1 * np.random.default_rng(7).standard_normal(60)

    def ensemble(X, Q):
        e = Ensemble(c["cfg"], X, Q, c["a"], c["eta"], dt, kBT=1.0, wall=True)
        e.set_interactions(**MODEL)
        return e

    def steps_of(e, X, Q, mode, R, cell, steps, kinds=("det", "bd"), **more):
        for kind in kinds:
            n = [0]

            def step():
                if kind == "det":
                    return e.step_deterministic(F, max_iter=IT, rtol=RTOL)[0]
                n[0] += 1                                      # fresh noise every step: a random walk, not a drift
                return e.step_brownian(F, seed=n[0], max_iter=IT, rtol=RTOL)[0]
            ts, out = windows(lambda: e.set_config(X, Q), step, steps)
            line(mode + "_" + kind, R, cell, ts, steps, mean_iters=round(float(np.mean(out)), 2), **more)

    def copies(R):
        return np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)

    if args.kinds in ("shared", "table"):
        for R in (1, 256):
            X, Q = copies(R)
            for cell in (("off", "set_cell") if args.kinds == "shared" else ("set_cells",)):
                e = ensemble(X, Q)
                if cell == "set_cell":
                    e.set_cell(L[0], L[1], images=(1, 1))
                elif cell == "set_cells":
                    e.set_cells(np.full(R, L[0]), np.full(R, L[1]), images=(1, 1))
                steps_of(e, X, Q, "step", R, cell, args.steps)
                e.close()
    if args.kinds == "sweep":
        stretch = np.linspace(1.0, 2.0, 8)

        def run(e, X, Q, mode, R, cell):
            def go():
                return e.run(args.steps, F=F, brownian=True, seed=11, on_error="reject", max_iter=IT, rtol=RTOL)
            ts, out = windows(lambda: e.set_config(X, Q), go, 1, warmup=1)    # (a window is one run of --steps steps)
            return [t / args.steps for t in ts], float(out.iters_sum.sum()) / float(out.accepted.sum()), int(out.rejected.sum())

        def stretched(R, scale):
            X, Q = copies(R)
            X[:, :, :2] *= np.asarray(scale).reshape(-1, 1, 1)
            return X, Q
        scale = np.repeat(stretch, 32)
        X, Q = stretched(256, scale)
        e = ensemble(X, Q)
        e.set_cells(L[0] * scale, L[1] * scale, images=(1, 1))
        ts, iters, rej = run(e, X, Q, "run", 256, "8 cells x 32")
        e.close()
        one = line("sweep_one_run_8x32", 256, "set_cells", ts, args.steps, mean_iters=round(iters, 2), rejected=rej,
                   ms_per_replica_step=round(1e3 * float(np.median(ts)) / 256, 6))
        total = np.zeros(args.rounds)
        for k, f in enumerate(stretch):
            X, Q = stretched(32, f)
            e = ensemble(X, Q)
            e.set_cell(L[0] * f, L[1] * f, images=(1, 1))
            ts, iters, rej = run(e, X, Q, "run", 32, "shared")
            e.close()
            total += np.array(ts)
            line("sweep_run_R32_cell_%d" % k, 32, "set_cell", ts, args.steps, mean_iters=round(iters, 2), rejected=rej,
                 stretch=round(float(f), 4))
        eight = line("sweep_eight_runs_R32", 256, "set_cell", list(total), args.steps,
                     ms_per_replica_step=round(1e3 * float(np.median(total)) / 256, 6))
        print("JSON " + json.dumps({"build": args.label, "mode": "sweep_verdict", "eight_runs_over_one_run": round(eight / one, 3)}), flush=True)
    if args.kinds == "imbalance":
        R = 256
        X, Q = copies(R)
        for name, n in (("all_1_1", np.tile([1, 1], (R, 1))), ("one_4_4", np.array([[4, 4]] + [[1, 1]] * (R - 1))),
                        ("all_4_4", np.tile([4, 4], (R, 1)))):
            e = ensemble(X, Q)
            e.set_cells(L[0], L[1], images=n)
            steps_of(e, X, Q, "imbalance_" + name, R, "set_cells", args.imbalance_steps)
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--imbalance-steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_cells.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="shared", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--steps", str(args.steps),
               "--imbalance-steps", str(args.imbalance_steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        print("visit: %s build, %s" % (label, kinds), file=sys.stderr, flush=True)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        out = [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("JSON ")]
        for d in out:
            print(json.dumps(d), flush=True)
        return out

    result = {"workload": "layer10_10x12_wall_builtin_model", "rtol": RTOL, "shared": [], "check": []}
    pooled = {}
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):                              # parent, this, parent, this, ...
        for label, root in builds:
            for d in visit(root, label, "shared"):
                d["visit"] = v
                result["shared"].append(d)
                pooled.setdefault((label, d["mode"], d["R"], d["cell"]), []).extend(d["windows_ms"])
    result["table"] = visit(HERE, "this", "table")
    for d in result["table"]:
        pooled.setdefault(("this", d["mode"], d["R"], d["cell"]), []).extend(d["windows_ms"])

    def stats(w):
        m = float(np.median(w))
        return m, (max(w) - min(w)) / m
    for mode, R, cell in sorted({k[1:] for k in pooled if k[3] != "set_cells"}):
        t, ts = stats(pooled[("this", mode, R, cell)])
        d = {"check": "shared cell against the parent build", "mode": mode, "R": R, "cell": cell, "this_ms_per_step": round(t, 4),
             "this_window_spread": round(ts, 4), "windows": len(pooled[("this", mode, R, cell)])}
        if ("parent", mode, R, cell) in pooled:
            p, ps = stats(pooled[("parent", mode, R, cell)])
            d.update({"parent_ms_per_step": round(p, 4), "parent_window_spread": round(ps, 4), "this_over_parent": round(t / p, 4),
                      "within_parent_spread": bool(t <= p * (1.0 + ps))})
        print(json.dumps(d), flush=True)
        result["check"].append(d)
    for mode, R in sorted({k[1:3] for k in pooled if k[3] == "set_cells"}):
        t, _ = stats(pooled[("this", mode, R, "set_cells")])
        p, ps = stats(pooled[("this", mode, R, "set_cell")])
        d = {"check": "table of equal rows against the by-value cell", "mode": mode, "R": R, "set_cells_ms_per_step": round(t, 4),
             "set_cell_ms_per_step": round(p, 4), "set_cell_window_spread": round(ps, 4), "set_cells_over_set_cell": round(t / p, 4),
             "within_spread": bool(t <= p * (1.0 + ps))}
        print(json.dumps(d), flush=True)
        result["check"].append(d)
    result["sweep"] = visit(HERE, "this", "sweep")
    result["imbalance"] = visit(HERE, "this", "imbalance")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
