"""What the bonds of the force model cost (include/rbl.h section 4: bonds and tethers between anchor points fixed in the bodies),
and the figures of the equipartition test.

  (a) eval        rbl_interaction_forces_dev at cfg 3 (200 x shell_N_642 above the wall): the built-in model alone and with a
                  chain of 199 bonds (body i to body i + 1, every other one tabulated) and 200 tethers added; ms per evaluation.
  (b) run         per-step time of a Brownian Ensemble.run at R = 256 replicas of 10 x shell_N_12 above the wall (dt = 1e-3), with the built-in
                  model alone and with a chain of 9 bonds added.
  (d) equipartition  k <|p_A - P|^2> / (3 kBT) and its standard error of tests/test_bonds_gpu.py's tethered bead at k mu dt = 0.02
                  (dt_factor 1) and at half of it, the step the test runs at (the discretisation bias of the scheme).
  (c) run_parent  the step of (b) with the new term off, on THIS build and, with --parent-root, on a build of the parent commit
                  (a checkout of it, built, anywhere on this machine).  The two alternate, visit by visit, each visit a fresh
                  process that imports the package from its own root; the windows of all visits of a build are pooled.  The verdict
                  line compares this build's median with the parent's against the PARENT's own window spread.

Every window is timed by the host clock around its work and ends in a device synchronise; every line carries its windows and
their spread (max - min) / median.  One JSON line per measurement, appended to --out.

    python tools/bench_bonds.py [--parent-root DIR] [--steps 200] [--rounds 5] [--visits 2] [--out profiles/bonds.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_RUN, NB, DT_RUN = 256, 10, 1e-3                            # dt as tools/bench_magnetic.py: no overlaps within a window
BUILTIN = dict(w=0.3, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    import rigid_body_light_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream

    def line(mode, terms, ts, per, **more):
        med = float(np.median(ts))
        d = {"build": args.label, "mode": mode, "terms": terms, "windows_ms": [round(1e3 * t, 5) for t in ts],
             "ms_per_" + per: round(1e3 * med, 5), "window_spread": round((max(ts) - min(ts)) / med, 4)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)

    def bonded(ctx, X, tethers):
        """a chain through the bodies in index order, rest lengths the present distances (every other bond tabulated: a quadratic
        well about the bond's own length would need a table per bond, so the table is a stiffening spring T(d) = d^4 / 4 over the
        lengths present), and with `tethers` every body tethered to the point it is at"""
        n = X.shape[0]
        rng = np.random.default_rng(3)
        d = np.linalg.norm(X[1:] - X[:-1], axis=1)
        body = [[i, i + 1] for i in range(n - 1)]
        anchor_a, anchor_b = 0.2 * rng.standard_normal((n - 1, 3)), 0.2 * rng.standard_normal((n - 1, 3))
        kind, k, l0 = np.arange(n - 1) % 2, np.where(np.arange(n - 1) % 2, 1e-3, 1.0), d.copy()
        if tethers:
            body += [[i, -1] for i in range(n)]
            anchor_a, anchor_b = np.concatenate([anchor_a, np.zeros((n, 3))]), np.concatenate([anchor_b, X])
            kind, k, l0 = np.concatenate([kind, np.zeros(n, dtype=int)]), np.concatenate([k, np.ones(n)]), np.concatenate([l0, np.zeros(n)])
        x = np.linspace(0.5 * d.min(), 1.5 * d.max(), 257)
        ctx.set_bond_table(0.25 * x ** 4, x ** 3, x[0], x[-1])
        ctx.set_bonds(np.array(body), anchor_a, anchor_b, k, l0, kind=kind)
        return len(body)

    for kind in args.kinds.split(","):
        if kind == "eval":
            c = make_config(200, 642, True)
            nb = c["X"].shape[0]
            ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=stream)
            ctx.set_config(c["X"], c["Q"])
            ctx.set_interactions(**BUILTIN)
            FT = torch.empty(6 * nb, dtype=torch.float64, device="cuda:0")
            n_bonds = 0
            for terms in ("builtin", "builtin+bonds"):
                if terms != "builtin":
                    n_bonds = bonded(ctx, np.reshape(c["X"], (nb, 3)), True)
                for _ in range(args.warmup):
                    ctx.interaction_forces_dev(None, FT.data_ptr())
                ts = []
                for _ in range(args.rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.evals):
                        ctx.interaction_forces_dev(None, FT.data_ptr())
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) / args.evals)
                ctx.sync_check()
                line("eval", terms, ts, "eval", workload="cfg3_200x642_wall", evals_per_window=args.evals,
                     active=ctx.interactions_active(), bonds=n_bonds)
            ctx.close()
        elif kind == "equipartition":
            sys.path.insert(0, os.path.join(args.worker, "tests"))
            import test_bonds_gpu
            for factor in (1.0, 0.5):
                ratio, se, dt = test_bonds_gpu.tethered_bead_ratio(dt_factor=factor)
                print("JSON " + json.dumps({"build": args.label, "mode": "tethered_bead_equipartition", "dt_factor": factor, "dt": round(dt, 6),
                                            "k_r2_over_3kT": round(ratio, 5), "standard_error": round(se, 5), "R": 256}), flush=True)
        else:                                                   # "run": both variants; "run_off": the new term off only
            c = make_config(NB, 12, True)
            X, Q = np.repeat(c["X"][None], R_RUN, axis=0), np.repeat(c["Q"][None], R_RUN, axis=0)
            for terms in (("builtin",) if kind == "run_off" else ("builtin", "builtin+bonds")):
                e = DeviceContext(c["a"], 1.0, True, cfg=c["cfg"], dt=DT_RUN, kBT=1.0, stream_ptr=stream)
                e.ensemble_set_config(X, Q)
                e.set_interactions(**BUILTIN)
                if terms != "builtin":
                    bonded(e, np.reshape(c["X"], (NB, 3)), False)
                F = np.zeros((R_RUN, 6 * NB))

                def run(n, seed):
                    res, rc = e.ensemble_run(n, F_body=F, brownian=True, seed=seed, max_iter=50, rtol=1e-8)
                    assert rc == 0, res.error
                    return res
                run(args.warmup, 1)
                ts, acc = [], 0
                for w in range(args.rounds):
                    e.ensemble_set_config(X, Q)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = run(args.steps, 100 + 1000 * w)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) / args.steps)
                    acc += int(res.accepted.sum())
                active = e.interactions_active()
                e.close()
                line("run_brownian", terms, ts, "step", workload="cfg1_10x12_wall", R=R_RUN, steps_per_window=args.steps,
                     accepted=acc, active=active)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--evals", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bonds.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="eval,run", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--steps", str(args.steps),
               "--evals", str(args.evals), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
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

    for d in visit(HERE, "this", "eval,run,equipartition"):   # (a), (b) and (d)
        emit(d)
    pooled = {}                                               # (c): parent, this, parent, this, ...
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):
        for label, root in builds:
            for d in visit(root, label, "run_off"):
                d["visit"] = v
                emit(d)
                pooled.setdefault(label, []).extend(d["windows_ms"])
    t = pooled["this"]
    d = {"workload": "cfg1_10x12_wall", "mode": "terms_off_check", "R": R_RUN, "this_ms_per_step": round(float(np.median(t)), 5),
         "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
    if "parent" in pooled:
        p = pooled["parent"]
        mp = float(np.median(p))
        d.update({"parent_ms_per_step": round(mp, 5), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                  "this_over_parent": round(float(np.median(t)) / mp, 4)})
        d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
    emit(d)


if __name__ == "__main__":
    main()
