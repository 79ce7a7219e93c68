#!/usr/bin/env python3
"""python tools/bench_prescribed.py [--rounds 5] [--cfgs cfg2,cfg3] -- what a solve with prescribed bodies costs next to the
unconstrained one (include/rbl.h section 7): solve_saddle and solve_mixed with none / a quarter / all of the bodies prescribed, at
cfg 2 (50 x shell_N_162) and cfg 3 (200 x shell_N_642), or with --cfgs cfg1 at cfg 1 (10 x shell_N_12: launch-bound, where added
host-side work would show); wall, block preconditioner, rtol 1e-8, one process, one box.

Timing: host wall clock around each solve of the host-array entry points (each ends in a stream synchronise), after one untimed
warm-up solve per case (code loading, the factor build); then `rounds` rounds that alternate the cases.  Per case: iterations,
median ms per solve, median ms per iteration, the spread (min, max) over the rounds.  The yardstick is solve_saddle in the same
run; `ms_per_iter_ratio` = mixed / solve_saddle.  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np

CFGS = {"cfg1": (10, 12), "cfg2": (50, 162), "cfg3": (200, 642)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfgs", default="cfg2,cfg3")
    ap.add_argument("--rtol", type=float, default=1e-8)
    args = ap.parse_args()
    from rigid_body_light_amd import RigidBody, make_config
    out = {"bench": "prescribed_kinematics", "wall": True, "block_PC": True, "rtol": args.rtol, "rounds": args.rounds}
    for name in args.cfgs.split(","):
        nb, nblb = CFGS[name]
        c = make_config(nb, nblb, True)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
        n3 = 3 * nb * nblb
        rng = np.random.default_rng(1)
        F, Up = rng.standard_normal((nb, 6)), rng.standard_normal((nb, 6))
        rhs = np.concatenate([np.zeros(n3), -F.reshape(-1)])
        quarter = np.zeros(nb, dtype=bool)
        quarter[rng.permutation(nb)[:nb // 4]] = True
        masks = {"mixed_none": np.zeros(nb, dtype=bool), "mixed_quarter": quarter, "mixed_all": np.ones(nb, dtype=bool)}

        def run(case):
            t0 = time.perf_counter()
            if case == "solve_saddle":
                _, its, _ = rb.solve_saddle(rhs, max_iter=200, rtol=args.rtol)
            else:
                p = masks[case]
                _, _, _, its, _ = rb.solve_mixed(p, np.where(p[:, None], Up, F).reshape(-1), max_iter=200, rtol=args.rtol)
            return int(its), (time.perf_counter() - t0) * 1e3
        cases = ["solve_saddle"] + list(masks)
        for case in cases:                                   # warm-up: code loading, factors, workspaces
            run(case)
        ms = {case: [] for case in cases}
        its = {}
        for _ in range(args.rounds):
            for case in cases:
                its[case], t = run(case)
                ms[case].append(t)
        res = {}
        for case in cases:
            per_it = [t / its[case] for t in ms[case]]
            res[case] = {"iterations": its[case], "ms": round(float(np.median(ms[case])), 3),
                         "ms_per_iter": round(float(np.median(per_it)), 4),
                         "ms_per_iter_min_max": [round(min(per_it), 4), round(max(per_it), 4)]}
        for case in masks:
            res[case]["ms_per_iter_ratio"] = round(res[case]["ms_per_iter"] / res["solve_saddle"]["ms_per_iter"], 4)
        out[name] = {"bodies": nb, "blobs_per_body": nblb, "prescribed_quarter": int(quarter.sum()), **res}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
