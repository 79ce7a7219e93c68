#!/usr/bin/env python3
"""python tools/bench_prescribed_multi.py [--rounds 5] [--cfgs cfg2,cfg3] [--columns 16] [--sequential-only] -- what many
right-hand sides under one mask cost in lock step (include/rbl.h section 7, rbl_solve_mixed_multi / rbl_solve_mixed_dof_multi)
next to the sequential loop over solve_mixed / solve_mixed_dof that body_resistance_matrix runs by default: 16 unit-velocity
columns at cfg 2 (50 x shell_N_162) and cfg 3 (200 x shell_N_642), wall, block preconditioner, rtol 1e-8, one process, one box.
Two cases: `all` -- every body prescribed, the first 16 columns of the body resistance matrix; `rotations_all` -- the rotations
of all bodies prescribed (a component mask), unit angular velocities.

Timing as tools/bench_multi_rhs.py and tools/bench_prescribed.py: host wall clock around the host-array entry points (each ends
in a stream synchronise), after one untimed warm-up of each form; then `rounds` rounds (windows) that alternate the sequential
loop and the lock-step solve.  Per case: the columns' iteration counts, median ms of each form, (min, max) over the rounds, the
relative spread (max - min) / median of the sequential windows, `ratio` = lock-step / sequential and `faster_beyond_spread`:
whether the lock-step median is below the sequential median by more than that spread.  --sequential-only times the loop alone
(it calls nothing this tool's lock-step half needs, so it also runs against an older build of the library: the baseline that is
not the code under test).  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np

CFGS = {"cfg2": (50, 162), "cfg3": (200, 642)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfgs", default="cfg2,cfg3")
    ap.add_argument("--cases", default="all,rotations_all")
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--sequential-only", action="store_true")
    args = ap.parse_args()
    from rigid_body_light_amd import RigidBody, make_config
    k = args.columns
    out = {"bench": "prescribed_multi", "wall": True, "block_PC": True, "rtol": args.rtol, "rounds": args.rounds, "columns": k,
           "sequential_only": bool(args.sequential_only)}
    for name in args.cfgs.split(","):
        nb, nblb = CFGS[name]
        c = make_config(nb, nblb, True)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
        everyone = np.ones(nb, dtype=bool)
        rot = np.zeros((nb, 6), dtype=bool)
        rot[:, 3:] = True
        U_all = np.zeros((k, 6 * nb))
        U_all[np.arange(k), np.arange(k)] = 1.0                                  # the first k unit velocities
        U_rot = np.zeros((k, nb, 6))
        U_rot[np.arange(k), np.arange(k) // 3 % nb, 3 + np.arange(k) % 3] = 1.0   # unit angular velocities, no loads on the translations
        U_rot = U_rot.reshape(k, 6 * nb)
        cases = {"all": (lambda u: rb.solve_mixed(everyone, u, max_iter=200, rtol=args.rtol),
                         lambda u: rb.solve_mixed_multi(everyone, u, max_iter=200, rtol=args.rtol), U_all),
                 "rotations_all": (lambda u: rb.solve_mixed_dof(rot, u, max_iter=200, rtol=args.rtol),
                                   lambda u: rb.solve_mixed_dof_multi(rot, u, max_iter=200, rtol=args.rtol), U_rot)}
        res = {}
        for case in args.cases.split(","):
            one, multi, U = cases[case]

            def sequential():
                t0 = time.perf_counter()
                its = [int(one(U[j])[3]) for j in range(k)]
                return its, (time.perf_counter() - t0) * 1e3

            def lock_step():
                t0 = time.perf_counter()
                its = multi(U)[3]
                return [int(i) for i in its], (time.perf_counter() - t0) * 1e3
            forms = {"sequential": sequential} if args.sequential_only else {"sequential": sequential, "lock_step": lock_step}
            for f in forms.values():                           # warm-up: code loading, factors, workspaces
                f()
            ms, its = {f: [] for f in forms}, {}
            for _ in range(args.rounds):
                for f, fn in forms.items():
                    its[f], t = fn()
                    ms[f].append(t)
            r = {}
            for f in forms:
                med = float(np.median(ms[f]))
                r[f] = {"iterations": its[f], "ms": round(med, 2), "ms_min_max": [round(min(ms[f]), 2), round(max(ms[f]), 2)],
                        "rel_spread": round((max(ms[f]) - min(ms[f])) / med, 4),
                        "ms_per_column_iteration": round(med / sum(its[f]), 4)}
            if not args.sequential_only:
                ratio = r["lock_step"]["ms"] / r["sequential"]["ms"]
                r["ratio"] = round(ratio, 4)
                r["faster_beyond_spread"] = bool(1.0 - ratio > r["sequential"]["rel_spread"])
            res[case] = r
        out[name] = {"bodies": nb, "blobs_per_body": nblb, **res}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
