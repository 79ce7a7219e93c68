"""Observers of ensemble runs (include/rbl.h section 5, rbl_ensemble_run_observed; Ensemble.run with probes / moments): what the
flow at probe points and the stresslets cost inside a run, and that a run without them costs what it did.

Workload: cfg 1 -- 10 x shell_N_12 above the wall (tests/periodic_cases.py: layer10()'s layer), the built-in force model of
tools/bench_ensemble_periodic.py, GMRES to 1e-8 -- at R in {1, 256}, with the ensemble's cell off and on at (1, 1) images.

  observed     ms per step of a Brownian Ensemble.run (stride 0): without observers, with P = 256 and P = 4096 lab probe points,
               with moments, the variants alternating inside a round; the overhead of each over the plain run.
  kernel       the probe kernel alone (device events around rbl_ensemble_velocity_field_dev: the kernel, the clearing of R error
               words and their read-back), its pairs per second (R P N images per call), and the host form of
               Ensemble.velocity_field at P = 4096 (recorded only).
  loop         what the parent commit can do for the flow of a deterministic run: solve_jointed -> lambda to the host, then per
               replica a single-context velocity_field with explicit positions, then step_deterministic -- against
               run(brownian=False, probes, stride=1).  The verdict: the run below the loop by more than the spread of the loop's
               windows; the ratio is recorded.  (Cell off: the single context has no field in a cell.)
  plain        Ensemble.run, Ensemble.run_jointed (the 9-joint ball chain of tools/bench_ensemble_run_joints.py) without
               observers and the one-step step_brownian on THIS build and, with --parent-root, on a build of the parent commit
               (a built checkout of it anywhere on this machine).  The two alternate, visit by visit, each visit a fresh process
               that imports the package from its own root; the windows of all visits of a build are pooled.  The verdict compares
               this build's median with the parent's against the PARENT's own window spread.

Every window starts from the same configuration and seed, is timed by the host clock around `steps` steps and ends in a device
synchronise.  ONE JSON line with every measurement is appended to --out.

--parts plain repeats the comparison with the parent alone (more visits show how far two processes of ONE build lie apart, which
the windows inside a process do not).

    python tools/bench_ensemble_observed.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--reps 1,256]
                                            [--parts observed,plain] [--out profiles/ensemble_observed.jsonl]
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


def chain(X, seed=3):
    """joints through the bodies in index order, anchors off the centres (tools/bench_joints.py's)"""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    return np.array([[i, i + 1] for i in range(n - 1)]), 0.3 * rng.standard_normal((n - 1, 6))


def probes(P, L, seed=5):
    """P lab points over the layer and a cell's width beyond it, from the damped layer up to z = 8"""
    rng = np.random.default_rng(seed)
    return rng.uniform([-0.5 * L[0], -0.5 * L[1], 0.1], [1.5 * L[0], 1.5 * L[1], 8.0], (P, 3))


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import Ensemble, make_config
    from rigid_body_light_amd._lib import DeviceContext
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    reps = [int(r) for r in args.reps.split(",")]
    c = make_config(10, 12, True)
    a, nb, N = c["a"], 10, 120
    s = 2.0 * (1.0 + a) + 0.5
    L = (3.0 * s, 3.0 * s + 0.7)
    dt = 1e-3
    F = 0.1 * np.random.default_rng(7).standard_normal(6 * nb)

    def timed(reset, variants, steps, rounds):
        """variants: {name: window(n)}; every shape warmed up, then `rounds` rounds with the variants alternating"""
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

    def ensemble(R, cell=None, kBT=1.0, model=True):
        X, Q = np.repeat(c["X"][None], R, axis=0), np.repeat(c["Q"][None], R, axis=0)
        e = Ensemble(c["cfg"], X, Q, a, c["eta"], dt, kBT=kBT, wall=True)
        if model:
            e.set_interactions(**MODEL)
        if cell:
            e.set_cell(L[0], L[1], images=cell)
        return e, X, Q

    if args.kinds == "plain":
        for R in reps:
            e, X, Q = ensemble(R)
            n = [0]

            def steps_bd(k):
                for _ in range(k):
                    n[0] += 1
                    e.step_brownian(F, seed=n[0], max_iter=IT, rtol=RTOL)
            ms = timed(lambda: e.set_config(X, Q), {"run": lambda k: e.run(k, F=F, seed=100, max_iter=IT, rtol=RTOL), "step_brownian": steps_bd},
                       args.steps, args.rounds)
            e.close()
            e, X, Q = ensemble(R, kBT=0.0)
            body, anchor = chain(c["X"])
            e.set_joint_kinds(body, None, anchor[:, :3], anchor[:, 3:])
            ms.update(timed(lambda: e.set_config(X, Q), {"run_jointed": lambda k: e.run_jointed(k, F, gamma=0.0, max_iter=IT, rtol=RTOL)},
                            args.steps, args.rounds))
            e.close()
            for mode, ts in ms.items():
                emit(dict(mode=mode, R=R, steps_per_window=args.steps, **stats(ts)))
        return

    # ---- observed: the observers' cost inside a Brownian run
    for cell in (None, (1, 1)):
        n_img = 9 if cell else 1
        for R in reps:
            e, X, Q = ensemble(R, cell)
            p256, p4096 = probes(256, L), probes(4096, L)
            kw = dict(F=F, seed=100, max_iter=IT, rtol=RTOL)
            ms = timed(lambda: e.set_config(X, Q),
                       {"P0": lambda k: e.run(k, **kw), "P256": lambda k: e.run(k, probes=p256, **kw),
                        "P4096": lambda k: e.run(k, probes=p4096, **kw), "moments": lambda k: e.run(k, moments=True, **kw)},
                       args.steps, args.rounds)
            base = float(np.median(ms["P0"]))
            for v, ts in ms.items():
                emit(dict(mode="brownian_run_" + v, R=R, images=list(cell) if cell else None, steps_per_window=args.steps,
                          over_plain=round(float(np.median(ts)) / base, 4), added_ms=round(float(np.median(ts)) - base, 4), **stats(ts)))
            # the probe kernel alone, device events; then the host form
            for P in (256, 4096):
                pts = torch.tensor(probes(P, L), device="cuda")
                lam = torch.randn(R, 3 * N, dtype=torch.float64, device="cuda")
                u = torch.empty(R, P, 3, dtype=torch.float64, device="cuda")
                call = lambda: e.ctx.ensemble_velocity_field_dev(pts.data_ptr(), P, 1, lam.data_ptr(), u.data_ptr())   # noqa: E731
                for _ in range(3):
                    call()
                ts = []
                for _ in range(10):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(); call(); t1.record()
                    torch.cuda.synchronize()
                    ts.append(t0.elapsed_time(t1))
                med = float(np.median(ts))
                emit(dict(mode="probe_kernel_alone", R=R, P=P, images=list(cell) if cell else None, geometry=list(e.probe_info(P)),
                          ms=round(med, 4), spread=round((max(ts) - min(ts)) / med, 4),
                          pairs_per_s=float("%.4g" % (R * P * N * n_img / (1e-3 * med)))))
            lam = np.random.default_rng(3).standard_normal((R, 3 * N))
            e.velocity_field(p4096, lam)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                e.velocity_field(p4096, lam)
                ts.append(1e3 * (time.perf_counter() - t0))
            emit(dict(mode="velocity_field_host_form", R=R, P=4096, images=list(cell) if cell else None, ms=round(float(np.median(ts)), 3)))
            e.close()

    # ---- loop: the flow of a deterministic run, as the parent commit can obtain it
    from oracle import oracle as O
    cfg0 = O.remove_mean(c["cfg"])
    for R in reps:
        e, X, Q = ensemble(R, kBT=0.0)
        ctx = DeviceContext(a, c["eta"], True, stream_ptr=torch.cuda.current_stream().cuda_stream)
        pts = probes(256, L)

        def loop(k):
            for _ in range(k):
                lam = e.solve_jointed(F, max_iter=IT, rtol=RTOL)[0]
                Xn, Qn = e.get_config()
                for r in range(R):
                    pos = np.concatenate([cfg0 @ O.rot_matrix(Qn[r, b]).T + Xn[r, b] for b in range(nb)])
                    ctx.velocity_field(pts, lam[r], pos)
                e.step_deterministic(F, max_iter=IT, rtol=RTOL)
        steps = max(args.steps // (1 if R == 1 else 10), 5)
        ms = timed(lambda: e.set_config(X, Q),
                   {"loop": loop, "observed_run": lambda k: e.run(k, F=F, brownian=False, probes=pts, stride=1, max_iter=IT, rtol=RTOL)}, steps, args.rounds)
        lo, ob = stats(ms["loop"]), stats(ms["observed_run"])
        emit(dict(mode="deterministic_flow_loop_vs_observed_run", R=R, P=256, steps_per_window=steps, loop=lo, observed_run=ob,
                  run_over_loop=round(ob["ms_per_step"] / lo["ms_per_step"], 4),
                  run_beats_loop_by_more_than_its_spread=bool(ob["ms_per_step"] < lo["ms_per_step"] * (1.0 - lo["window_spread"]))))
        ctx.close(); e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--reps", default="1,256")
    ap.add_argument("--parts", default="observed,plain")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ensemble_observed.jsonl"))
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
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        out = [json.loads(ln[5:]) for ln in p.stdout.splitlines() if ln.startswith("JSON ")]
        for d in out:
            print(json.dumps(d), flush=True)
        return out

    parts = args.parts.split(",")
    result = {"workload": "cfg1_layer10_10x12_wall_builtin_model", "rtol": RTOL, "visits": args.visits,
              "observed": visit(HERE, "this", "observed") if "observed" in parts else [], "plain": [], "check": []}
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
            d.update({"parent_visit_medians": medians[("parent", mode, R)], "parent_ms_per_step": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        print(json.dumps(d), flush=True)
        result["check"].append(d)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
