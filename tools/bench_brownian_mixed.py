#!/usr/bin/env python3
"""python tools/bench_brownian_mixed.py [--rounds 5] [--cfgs cfg2,cfg3] [--out profiles/brownian_mixed.jsonl] -- what a Brownian
midpoint step with prescribed bodies costs next to the all-free one (include/rbl.h section 7): step_brownian and
step_brownian_mixed with none / a quarter / all but one of the bodies prescribed (held), at cfg 2 (50 x shell_N_162) and cfg 3
(200 x shell_N_642), wall, block preconditioner, lanczos_pc roots to 1e-3, GMRES to 1e-8, one process, one box.

Timing (the protocol of tools/bench_prescribed.py): host wall clock around each step of the host-array entry points, closed by a
device synchronise, after one untimed warm-up step per case (code loading, workspaces); then `rounds` rounds that alternate the
cases.  Every step starts from the same configuration (set_config outside the timed region, so each step builds the factors of q^n
and of q^{n+1/2} itself) and the cases of a round share the seed, hence the noise.  Per case: GMRES iterations, median ms per
step with (min, max) over the rounds, ms per iteration.  The yardstick is step_brownian in the same run; `ms_ratio` =
mixed / step_brownian.  One JSON line, appended to --out when given."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rigid_body_light_amd import RigidBody, make_config
    out = {"bench": "brownian_mixed", "wall": True, "block_PC": True, "roots": "lanczos_pc 1e-3", "rtol": args.rtol, "rounds": args.rounds}
    for name in args.cfgs.split(","):
        nb, nblb = CFGS[name]
        c = make_config(nb, nblb, True)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
        rb.cb.set_lanczos(200, 1e-3)
        rng = np.random.default_rng(1)
        F = rng.standard_normal((nb, 6))
        quarter = np.zeros(nb, dtype=bool)
        quarter[rng.permutation(nb)[:nb // 4]] = True
        all_but_one = np.ones(nb, dtype=bool)
        all_but_one[0] = False
        masks = {"mixed_none": np.zeros(nb, dtype=bool), "mixed_quarter": quarter, "mixed_all_but_one": all_but_one}

        def run(case, seed):
            rb.set_config(c["X"], c["Q"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if case == "step_brownian":
                its, _ = rb.step_brownian(F.reshape(-1), seed=seed, method="lanczos_pc", max_iter=200, rtol=args.rtol)
            else:
                p = masks[case]
                _, its, _ = rb.step_brownian_mixed(p, np.where(p[:, None], 0.0, F), seed=seed, method="lanczos_pc", max_iter=200,
                                                   rtol=args.rtol)
            torch.cuda.synchronize()
            return int(its), (time.perf_counter() - t0) * 1e3
        cases = ["step_brownian"] + list(masks)
        for case in cases:                                   # warm-up: code loading, workspaces
            run(case, 0)
        ms = {case: [] for case in cases}
        its = {case: [] for case in cases}
        for rnd in range(args.rounds):
            for case in cases:
                i, t = run(case, 1 + rnd)
                its[case].append(i)
                ms[case].append(t)
        res = {}
        for case in cases:
            res[case] = {"iterations": int(np.median(its[case])), "ms": round(float(np.median(ms[case])), 3),
                         "ms_min_max": [round(min(ms[case]), 3), round(max(ms[case]), 3)],
                         "ms_per_iter": round(float(np.median([t / i for t, i in zip(ms[case], its[case])])), 4)}
        for case in masks:
            res[case]["ms_ratio"] = round(res[case]["ms"] / res["step_brownian"]["ms"], 4)
        out[name] = {"bodies": nb, "blobs_per_body": nblb, "prescribed_quarter": int(quarter.sum()), **res}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
