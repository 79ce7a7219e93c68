"""What the periodic cell (include/rbl.h section 10) costs, and that it costs nothing while it is off.

  (a) product     the periodic product (k_apply_M_per) at cfg 2 (50 x shell_N_162 above the wall) and cfg 3 (200 x shell_N_642) for
                  images (1, 1) and (2, 2), against the ordered non-periodic kernel of the same build (matvec_kernel = 1): ms per
                  product and the ratio PER IMAGE, ratio / ((2 nx + 1)(2 ny + 1)).  The cell is the lattice of make_config: as
                  many lattice spacings as the lattice has columns, plus 0.7 in y.
  (b) step        one converged step_deterministic at cfg 2 with the cell on (block preconditioner, rtol 1e-8): ms, iterations.
  (c) off         with the cell NEVER set: the cfg 3 product (the default symmetric kernel), a cfg 3 step_deterministic and the
                  cfg 3 force evaluation, on THIS build and, with --parent-root, on a build of the parent commit (a checkout of
                  it, built, anywhere on this machine).  The two alternate, visit by visit, each visit a fresh process that
                  imports the package from its own root; the windows of all visits of a build are pooled.  The verdict line
                  compares this build's median with the parent's against the PARENT's own window spread.

Every window is timed by the host clock around its work and ends in a device synchronise; every line carries its windows and
their spread (max - min) / median.  One JSON line per measurement, appended to --out.

    python tools/bench_periodic.py [--parent-root DIR] [--rounds 5] [--visits 2] [--out profiles/periodic.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILTIN = dict(w=0.3, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
CFG = {"cfg2_50x162_wall": (50, 162), "cfg3_200x642_wall": (200, 642)}


def worker(args):
    sys.path.insert(0, args.worker)
    import torch
    from rigid_body_light_amd import RigidBody, make_config
    from rigid_body_light_amd._lib import DeviceContext
    import rigid_body_light_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(rigid_body_light_amd.__file__))) == os.path.abspath(args.worker)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda:0")

    def line(mode, workload, ts, per, **more):
        med = float(np.median(ts))
        d = {"build": args.label, "mode": mode, "workload": workload, "windows_ms": [round(1e3 * t, 5) for t in ts],
             "ms_per_" + per: round(1e3 * med, 5), "window_spread": round((max(ts) - min(ts)) / med, 4)}
        d.update(more)
        print("JSON " + json.dumps(d), flush=True)
        return med

    def windows(fn, calls):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / calls)
        return ts

    def cell(c, nb):
        side = int(np.ceil(nb ** (1.0 / 3.0) - 1e-9))
        s = 2.0 * (1.0 + c["a"]) + 0.5                           # make_config's lattice spacing
        return side * s, side * s + 0.7

    def context(workload):
        nb, nblb = CFG[workload]
        c = make_config(nb, nblb, True)
        ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=stream)
        ctx.set_config(c["X"], c["Q"])
        N = nb * nblb
        r = torch.empty(3 * N, dtype=torch.float64, device=dev)
        ctx.blob_positions(0, nb, r.data_ptr())
        F = torch.from_numpy(np.random.default_rng(5).standard_normal(3 * N)).to(dev)
        return c, ctx, N, r, F, torch.empty_like(F)

    for kind in args.kinds.split(","):
        if kind == "product":
            for workload in CFG:
                c, ctx, N, r, F, U = context(workload)
                L = cell(c, CFG[workload][0])
                calls = 20 if N < 20000 else 2

                def product():
                    ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr())
                ctx.set_option("matvec_kernel", 1)
                t_ord = line("product_ordered_open", workload, windows(product, calls * 5), "product", blobs=N, calls_per_window=calls * 5)
                ctx.set_option("matvec_kernel", 0)
                for n in ((1, 1), (2, 2)):
                    ctx.set_periodic(L[0], L[1], images=n)
                    t = line("product_periodic", workload, windows(product, calls), "product", blobs=N, calls_per_window=calls,
                             cell=[round(L[0], 4), round(L[1], 4)], images=list(n))
                    ctx.sync_check()
                    ni = (2 * n[0] + 1) * (2 * n[1] + 1)
                    print("JSON " + json.dumps({"build": args.label, "mode": "product_ratio", "workload": workload, "images": list(n),
                                                "pair_images": ni, "periodic_over_ordered": round(t / t_ord, 3),
                                                "ratio_per_image": round(t / t_ord / ni, 4)}), flush=True)
                ctx.close()
        elif kind == "step":
            workload = "cfg2_50x162_wall"
            nb, nblb = CFG[workload]
            c = make_config(nb, nblb, True)
            L = cell(c, nb)
            Fb = np.random.default_rng(6).standard_normal(6 * nb)
            ts, its = [], []
            for w in range(args.warmup + args.rounds):            # a step moves the bodies: every window starts from q^0
                rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
                rb.set_periodic(L[0], L[1], images=(1, 1))
                rb.step_deterministic(Fb, max_iter=100, rtol=1e-8)    # (workspaces, factors)
                rb.set_config(c["X"], c["Q"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it, res = rb.step_deterministic(Fb, max_iter=100, rtol=1e-8)
                torch.cuda.synchronize()
                if w >= args.warmup:
                    ts.append(time.perf_counter() - t0); its.append(it)
                assert 0 < it < 100 and res < 1e-8
            line("step_deterministic_periodic", workload, ts, "step", images=[1, 1], iterations=its, rtol=1e-8, preconditioner="block")
        else:                                                   # "off": the cell never set
            workload = "cfg3_200x642_wall"
            c, ctx, N, r, F, U = context(workload)
            nb = CFG[workload][0]
            line("off_apply_M", workload, windows(lambda: ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr()), 10), "product",
                 blobs=N, calls_per_window=10)
            ctx.set_interactions(**BUILTIN)
            FT = torch.empty(6 * nb, dtype=torch.float64, device=dev)
            line("off_forces", workload, windows(lambda: ctx.interaction_forces_dev(None, FT.data_ptr()), 100), "eval", calls_per_window=100)
            ctx.sync_check()
            ctx.close()
            Fb = np.random.default_rng(6).standard_normal(6 * nb)
            rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 1e-6, wall_PC=True, block_PC=True)   # dt: the bodies barely move
            its = []

            def step():
                its.append(rb.step_deterministic(Fb, max_iter=100, rtol=1e-8)[0])
            line("off_step_deterministic", workload, windows(step, 1), "step", iterations=its[-1], rtol=1e-8, preconditioner="block")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "periodic.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="product,step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def visit(root, label, kinds):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--label", label, "--kinds", kinds, "--warmup", str(args.warmup),
               "--rounds", str(args.rounds)]
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

    for d in visit(HERE, "this", "product,step"):             # (a) and (b)
        emit(d)
    pooled = {}                                               # (c): parent, this, parent, this, ...
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    for v in range(args.visits):
        for label, root in builds:
            for d in visit(root, label, "off"):
                d["visit"] = v
                emit(d)
                pooled.setdefault((d["mode"], label), []).extend(d["windows_ms"])
    for mode in ("off_apply_M", "off_forces", "off_step_deterministic"):
        t = pooled[(mode, "this")]
        d = {"workload": "cfg3_200x642_wall", "mode": mode + "_check", "this_ms": round(float(np.median(t)), 5),
             "this_window_spread": round((max(t) - min(t)) / float(np.median(t)), 4), "windows": len(t)}
        if (mode, "parent") in pooled:
            p = pooled[(mode, "parent")]
            mp = float(np.median(p))
            d.update({"parent_ms": round(mp, 5), "parent_window_spread": round((max(p) - min(p)) / mp, 4),
                      "this_over_parent": round(float(np.median(t)) / mp, 4)})
            d["within_parent_spread"] = bool(float(np.median(t)) <= mp * (1.0 + d["parent_window_spread"]))
        emit(d)


if __name__ == "__main__":
    main()
