#!/usr/bin/env python3
"""python tools/bench_prescribed_dof.py [--rounds 5] [--cfgs cfg2,cfg3] [--free-space] -- what a solve with a mask per velocity
component costs (include/rbl.h section 7, rbl_solve_mixed_dof) next to the whole-body solve of tools/bench_prescribed.py:
solve_saddle, solve_mixed with every body prescribed (`mixed_all`, the yardstick for the per-iteration cost) and solve_mixed_dof
with nothing prescribed / the rotations of all bodies / the translations of a quarter of the bodies, at cfg 2 (50 x shell_N_162)
and cfg 3 (200 x shell_N_642), wall, block preconditioner, rtol 1e-8, one process, one box.  --free-space: no wall (cfg 2 then
takes the body-frame tables, whose masked bodies cost a second factor application per iteration).

Timing as tools/bench_prescribed.py: host wall clock around each solve of the host-array entry points (each ends in a stream
synchronise), after one untimed warm-up solve per case; then `rounds` rounds (windows) that alternate the cases.  Per case:
iterations, median ms per solve, median ms per iteration, its (min, max) over the rounds and the relative spread (max - min) /
median; `ms_per_iter_vs_mixed_all` = the case's median ms per iteration / mixed_all's.  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np

CFGS = {"cfg2": (50, 162), "cfg3": (200, 642)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfgs", default="cfg2,cfg3")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--free-space", action="store_true")
    args = ap.parse_args()
    wall = not args.free_space
    from rigid_body_light_amd import RigidBody, make_config
    out = {"bench": "prescribed_dof", "wall": wall, "block_PC": True, "rtol": args.rtol, "rounds": args.rounds}
    for name in args.cfgs.split(","):
        nb, nblb = CFGS[name]
        c = make_config(nb, nblb, wall)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=True)
        n3 = 3 * nb * nblb
        rng = np.random.default_rng(1)
        F, Up = rng.standard_normal((nb, 6)), rng.standard_normal((nb, 6))
        rhs = np.concatenate([np.zeros(n3), -F.reshape(-1)])
        quarter = np.zeros(nb, dtype=bool)
        quarter[rng.permutation(nb)[:nb // 4]] = True
        rot, trq = np.zeros((nb, 6), dtype=bool), np.zeros((nb, 6), dtype=bool)
        rot[:, 3:] = True
        trq[quarter, :3] = True
        everyone = np.ones(nb, dtype=bool)
        masks = {"dof_none": np.zeros((nb, 6), dtype=bool), "dof_rotations_all": rot, "dof_translations_quarter": trq}

        def run(case):
            t0 = time.perf_counter()
            if case == "solve_saddle":
                _, its, _ = rb.solve_saddle(rhs, max_iter=200, rtol=args.rtol)
            elif case == "mixed_all":
                _, _, _, its, _ = rb.solve_mixed(everyone, Up.reshape(-1), max_iter=200, rtol=args.rtol)
            else:
                P = masks[case]
                _, _, _, its, _ = rb.solve_mixed_dof(P, np.where(P, Up, F).reshape(-1), max_iter=200, rtol=args.rtol)
            return int(its), (time.perf_counter() - t0) * 1e3
        cases = ["solve_saddle", "mixed_all"] + list(masks)
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
            med = float(np.median(per_it))
            res[case] = {"iterations": its[case], "ms": round(float(np.median(ms[case])), 3), "ms_per_iter": round(med, 4),
                         "ms_per_iter_min_max": [round(min(per_it), 4), round(max(per_it), 4)],
                         "rel_spread": round((max(per_it) - min(per_it)) / med, 4)}
        for case in cases:
            res[case]["ms_per_iter_vs_mixed_all"] = round(res[case]["ms_per_iter"] / res["mixed_all"]["ms_per_iter"], 4)
        out[name] = {"bodies": nb, "blobs_per_body": nblb, "prescribed_quarter": int(quarter.sum()), **res}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
