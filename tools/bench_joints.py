"""What the hard joints cost (include/rbl.h section 9), what they cost while they are off, and what they buy over the stiff spring.

  (a) solve       cfg 1 (10 x shell_N_12), cfg 2 (50 x shell_N_162), cfg 3 (200 x shell_N_642, wall), block preconditioner, 1e-8:
                  the plain saddle solve against the jointed one with a chain through the bodies in index order (cfg 3: the
                  199-joint chain, and a pivot on each of the 200 bodies, one set after the other: see joint_sets).  Per case: iterations, ms per solve; from fixed-work
                  solves (rtol = 0) of two lengths the ms per iteration (slope) and the ms per solve outside the iterations
                  (intercept: the preconditioner build of this configuration and, jointed, the Schur complement's assembly,
                  factorisation and inverse); one preconditioner application timed alone.  Derived: the share of a jointed
                  iteration the second preconditioner application takes, and the share left for the joint kernels
                  (slope_jointed - slope_plain - one application).
  (b) off         the existing step_deterministic and solve_mixed (nobody prescribed) at cfg 1 and cfg 3 on THIS build with joints
                  set, against a build of the parent commit (--parent-root: a checkout of it, built, anywhere on this machine),
                  alternated visit by visit, each visit a fresh process; the verdict compares the medians against the PARENT's own
                  window spread.
  (c) spring      the chain of examples/jointed_chain.py (no field: a transverse load on the last bead) stepped --spring-steps times
                  at a ladder of dt: with hard joints (gamma = 1) and with the bonds of set_bonds whose stiffness makes the
                  bonded gap under the same tension equal the jointed gap at the reference dt = 0.02.  Per dt: the largest gap
                  over the first and over the second half of the steps, or the error that ended the run.  The largest dt at
                  which the gap does not grow (no error, second half at most twice the first) is reported for both.

  (d) hinges      the solve of (a) at cfg 3 (or --configs) with a chain of hinges through the bodies in index order, the same axes and
                  points both times: as two ball joints half a unit either side of the point on the axis (one redundant row a
                  hinge, given an eigenvalue in the preconditioner) and as a ball joint and an axis joint (five rows, set_joint_kinds).
                  Iterations, ms per solve and per iteration, and the shares of (a).
  (e) ball        the ball-only cases of (a) on THIS build against the parent's (--parent-root), alternated visit by visit as in
                  (b); the verdict per case compares the medians against the PARENT's own window spread.

Every window is timed by the host clock around its work and ends in a device synchronise; every line carries its windows and
their spread (max - min) / median.  One JSON line per measurement, appended to --out.

    python tools/bench_joints.py [--parent-root DIR] [--kinds solve,off,spring,hinges,ball] [--rounds 5] [--visits 2] [--out profiles/joints.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"cfg1": (10, 12, False), "cfg2": (50, 162, False), "cfg3": (200, 642, True)}


def chain(X, seed=3):
    """joints through the bodies in index order, anchors off the centres"""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    return np.array([[i, i + 1] for i in range(n - 1)]), 0.3 * rng.standard_normal((n - 1, 6))


def pivots(X, seed=4):
    """every body on a pivot of its own, anchor and lab point off the centre"""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    return (np.array([[i, -1] for i in range(n)]),
            np.concatenate([0.3 * rng.standard_normal((n, 3)), X + 0.3 * rng.standard_normal((n, 3))], axis=1))


def hinge_chain(X, Q, five, seed=6):
    """a hinge between the bodies i and i + 1 for every i, at a point near the middle of the two centres about a random axis ->
    the keyword arguments of set_joint_kinds: five rows a hinge (ball + axis joint) or two ball joints half a unit either side
    of the point on the axis"""
    from rigid_body_light_amd import _lib as lib
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(X.shape[0] - 1):
        p = 0.5 * (X[i] + X[i + 1]) + 0.2 * rng.standard_normal(3)
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        if five:
            rows.append(lib.hinge(X, Q, i, i + 1, p, ax))
        else:
            for s in (0.5, -0.5):
                r = lib.hinge(X, Q, i, i + 1, p + s * ax, ax)
                rows.append({k: v[:1] for k, v in r.items()})             # its ball joint alone
    return lib.joint_rows(*rows)


def joint_sets(name, X):
    """cfg 1, cfg 2: the chain; cfg 3: the 199-joint chain, and the 200 pivots.  (Chain AND pivots in one set pin every body and
    then ask 597 more rows of the 600 rotations left: with anchors drawn at random J has singular values down to 4e-12 of its
    largest -- forces are levered from body to body along the whole chain -- and the solve refuses the set as redundant.)"""
    sets = [("chain",) + chain(X)]
    if name == "cfg3":
        sets.append(("pivots",) + pivots(X))
    return sets


def windows(fn, rounds, sync):
    ts = []
    for _ in range(rounds):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    import rigid_body_light_amd
    from rigid_body_light_amd import RigidBody, load_structure, make_config
    from rigid_body_light_amd._lib import DeviceContext
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    sync = torch.cuda.synchronize

    def line(mode, workload, ts, per, **more):
        med = float(np.median(ts))
        d = {"build": args.label, "mode": mode, "workload": workload, "windows_ms": [round(1e3 * t, 4) for t in ts],
             "ms_per_" + per: round(1e3 * med, 4), "window_spread": round((max(ts) - min(ts)) / med, 4)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)

    for kind in args.kinds.split(","):
        if kind in ("solve", "hinges"):
            for name in args.configs.split(","):
                nb, nblb, wall = CONFIGS[name]
                c = make_config(nb, nblb, wall)
                rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=True)
                rng = np.random.default_rng(5)
                F = rng.standard_normal(6 * nb)
                rhs = np.concatenate([np.zeros(3 * nb * nblb), -F])
                its = {}

                def plain(m=200, rt=args.rtol):
                    its["last"] = rb.solve_saddle(rhs, max_iter=m, rtol=rt)[1]

                def jointed(m=200, rt=args.rtol):
                    its["last"] = rb.solve_jointed(F, max_iter=m, rtol=rt)[3]
                out = {}
                if kind == "hinges":
                    Qn = c["Q"] / np.linalg.norm(c["Q"], axis=1, keepdims=True)
                    sets = [(n_, hinge_chain(c["X"], Qn, five)) for n_, five in (("hinges_two_ball", False), ("hinges_five_row", True))]
                    sets = [(n_, r["body"], r) for n_, r in sets]
                else:
                    sets = [(n_, b_, a_) for n_, b_, a_ in joint_sets(name, c["X"])]
                for case, fn, body, anchor in [("plain", plain, None, None)] + [(n_, jointed, b_, a_) for n_, b_, a_ in sets]:
                    if isinstance(anchor, dict):
                        rb.set_joint_kinds(**anchor)
                    elif body is not None:
                        rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
                    fn()                                     # warm-up: code loading, factors, workspaces
                    ts = windows(fn, args.rounds, sync)
                    used = its["last"]
                    lo, hi = args.fixed
                    t_lo = float(np.median(windows(lambda: fn(lo, 0.0), args.rounds, sync)))
                    t_hi = float(np.median(windows(lambda: fn(hi, 0.0), args.rounds, sync)))
                    slope = (t_hi - t_lo) / (hi - lo)
                    out[case] = dict(its=used, slope=slope, joints=0 if body is None else int(body.shape[0]))
                    line(kind, name, ts, "solve", case=case, joints=out[case]["joints"], rtol=args.rtol, iterations=used,
                         ms_per_iteration=round(1e3 * slope, 4), ms_outside_iterations=round(1e3 * (t_lo - lo * slope), 4))
                # one application of the same preconditioner alone, on device vectors (a context of its own)
                ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
                ctx._chk(ctx.L.rbl_set_blk_pc(ctx.h, 1))
                ctx.set_config(c["X"], c["Q"])
                ctx.prepare()
                nsys = 3 * nb * nblb + 6 * nb
                v = torch.randn(nsys, dtype=torch.float64, device="cuda:0")
                w = torch.empty_like(v)
                reps = 20 if name == "cfg3" else 200

                def pcs():
                    for _ in range(reps):
                        ctx.apply_PC(v.data_ptr(), w.data_ptr())
                pcs()
                t_pc = float(np.median(windows(pcs, args.rounds, sync))) / reps
                ctx.close()
                sp = out["plain"]["slope"]
                for case, o in out.items():
                    if case == "plain":
                        continue
                    sj = o["slope"]
                    print("JSON " + json.dumps({"build": args.label, "mode": "iteration_shares", "workload": name, "case": case, "joints": o["joints"],
                                                "ms_per_iteration_plain": round(1e3 * sp, 4), "ms_per_iteration_jointed": round(1e3 * sj, 4),
                                                "iterations_plain": out["plain"]["its"], "iterations_jointed": o["its"],
                                                "ms_per_pc_application": round(1e3 * t_pc, 4), "second_pc_share_of_iteration": round(t_pc / sj, 4),
                                                "joint_kernels_share_of_iteration": round((sj - sp - t_pc) / sj, 4)}), flush=True)
        elif kind == "off":
            for name in args.configs.split(","):
                if name == "cfg2":
                    continue
                nb, nblb, wall = CONFIGS[name]
                c = make_config(nb, nblb, wall)
                rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 1e-3, wall_PC=wall, block_PC=True)
                if hasattr(rb, "set_joints"):                 # this build: joints SET (and on) while the old entry points run
                    body, anchor = chain(c["X"])
                    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
                F = np.random.default_rng(5).standard_normal(6 * nb)
                nobody = np.zeros(nb, dtype=bool)
                n = 2 if name == "cfg3" else 50

                def steps():
                    rb.set_config(c["X"], c["Q"])
                    for _ in range(n):
                        rb.step_deterministic(F, max_iter=200, rtol=args.rtol)

                def mixed():
                    for _ in range(n):
                        rb.solve_mixed(nobody, F, max_iter=200, rtol=args.rtol)
                for mode, fn in (("step_deterministic", steps), ("solve_mixed", mixed)):
                    fn()
                    ts = [t / n for t in windows(fn, args.rounds, sync)]
                    line("off_" + mode, name, ts, "call", calls_per_window=n, joints_set=bool(hasattr(rb, "set_joints")))
        elif kind == "spring":
            p, cfg = load_structure(12)
            a = p["sep"] / 2.0
            Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
            nbead, gap = 6, 2.0 * a
            pitch = 2.0 * Rb + gap
            pivot = np.array([0.0, 0.0, a])
            X0 = np.array([[0.0, 0.0, pivot[2] + 0.5 * gap + Rb + i * pitch] for i in range(nbead)])
            Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (nbead, 1))
            top, bottom = np.array([0.0, 0.0, Rb + 0.5 * gap]), np.array([0.0, 0.0, -Rb - 0.5 * gap])
            body = np.array([[0, -1]] + [[i, i + 1] for i in range(nbead - 1)])
            anchor_a = np.array([bottom] + [top] * (nbead - 1))
            anchor_b = np.array([pivot] + [bottom] * (nbead - 1))
            F = np.zeros((nbead, 6))
            F[-1, :3] = [3.0, 0.0, 2.0]                         # the last bead pulled sideways and up
            nsteps = args.spring_steps

            def run(dt, k):
                """nsteps steps -> (largest gap of the first half, of the second half, largest |phi| or tension, error or None);
                k None: hard joints"""
                rb = RigidBody(cfg, X0, Q0, a, 1.0, dt, wall_PC=True, block_PC=True)
                rb.set_interactions(w=0.05, eps_wall=10.0, b_wall=0.25 * a, eps_blob=10.0, b_blob=0.25 * a)
                if k is None:
                    rb.set_joints(body, anchor_a, anchor_b)
                else:
                    rb.set_bonds(body, anchor_a, anchor_b, k, 0.0)
                half, load = [0.0, 0.0], 0.0
                try:
                    for step in range(nsteps):
                        if k is None:
                            phi, _, _ = rb.step_jointed(F, gamma=1.0, max_iter=200, rtol=args.rtol)
                            g = np.linalg.norm(rb.joint_state()[0], axis=1)
                            load = max(load, float(np.linalg.norm(phi.reshape(-1, 3), axis=1).max()))
                        else:
                            rb.step_deterministic(F, max_iter=200, rtol=args.rtol)
                            length, tension, _ = rb.bond_state()
                            g, load = np.asarray(length), max(load, float(np.abs(tension).max()))
                        h = 2 * step // nsteps
                        half[h] = max(half[h], float(g.max()))
                        if not np.isfinite(half[h]) or half[h] > pitch:
                            return half[0], half[1], load, "a gap exceeded the bead spacing at step %d" % step
                except RuntimeError as e:
                    return half[0], half[1], load, str(e)[:80]
                return half[0], half[1], load, None
            ref = run(0.02, None)
            k = ref[2] / max(ref[0], ref[1], 1e-300)          # tension / k = the jointed gap at the reference dt
            ladders = {"joints": [0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4],
                       "bonds": [q * 10.0 ** e for e in range(-10, -1) for q in (1.0, 3.0)]}
            for label, kk in (("joints", None), ("bonds", k)):
                rows = []
                for dt in ladders[label]:
                    first, second, load, err = run(dt, kk)
                    rows.append(dict(dt=dt, gap_max_first_half=first, gap_max_second_half=second, load_max=load, error=err))
                ok = [r["dt"] for r in rows if r["error"] is None and r["gap_max_second_half"] <= 2.0 * max(r["gap_max_first_half"], 1e-300)]
                print("JSON " + json.dumps({"build": args.label, "mode": "spring_vs_joint", "chain": label, "beads": nbead, "steps": nsteps,
                                            "k": None if kk is None else float("%.4g" % kk), "reference_dt": 0.02,
                                            "jointed_gap_at_reference_dt": float("%.4g" % max(ref[0], ref[1])),
                                            "largest_dt_gap_not_growing": max(ok) if ok else None,
                                            "criterion": "no error, and the largest gap of the second half of the steps at most twice that of the first",
                                            "ladder": [{q: (float("%.4g" % v) if isinstance(v, float) else v) for q, v in r.items()} for r in rows]}),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--fixed", type=int, nargs=2, default=[4, 12], help="the two lengths of the fixed-work solves")
    ap.add_argument("--spring-steps", type=int, default=200)
    ap.add_argument("--configs", default="cfg1,cfg2,cfg3")
    ap.add_argument("--kinds", default="solve,off,spring")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "joints.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--rounds", str(args.rounds),
               "--rtol", str(args.rtol), "--configs", args.configs, "--fixed", str(args.fixed[0]), str(args.fixed[1]),
               "--spring-steps", str(args.spring_steps)]
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        print("visit: %s build, %s" % (label, kinds), file=sys.stderr, flush=True)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            sys.exit("the %s build's worker failed (exit %d):\n%s" % (label, p.returncode, (p.stdout + p.stderr)[-3000:]))
        return [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("JSON ")]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(d):                                              # as it is measured: a later failure loses nothing
        print(json.dumps(d), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(d) + "\n")

    kinds = args.kinds.split(",")
    for kind in ("solve", "spring", "hinges"):
        if kind in kinds:
            for d in visit(HERE, "this", kind):
                emit(d)
    for against in ("off", "ball"):
        if against not in kinds:
            continue
        pooled = {}                                           # parent, this, parent, this, ...
        builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
        for v in range(args.visits):
            for label, root in builds:
                for d in visit(root, label, "off" if against == "off" else "solve"):
                    if "windows_ms" not in d:
                        continue                              # (the shares of a solve visit: not timed windows)
                    d["visit"] = v
                    if against == "ball":
                        d["mode"] = "ball_solve_" + d["case"]
                    emit(d)
                    pooled.setdefault((d["mode"], d["workload"]), {}).setdefault(label, []).extend(d["windows_ms"])
        for (mode, workload), w in pooled.items():
            t = w["this"]
            d = {"mode": mode + "_check", "workload": workload, "this_ms_per_call": round(float(np.median(t)), 4),
                 "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
            if "parent" in w:
                p = w["parent"]
                mp = float(np.median(p))
                d.update({"parent_ms_per_call": round(mp, 4), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                          "this_over_parent": round(float(np.median(t)) / mp, 4)})
                d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
            emit(d)


if __name__ == "__main__":
    main()
