"""Blob types and typed pair tables (include/rbl.h section 4): what they cost, and that they cost nothing while never set.
One JSON line per measurement:
  never_set_vs_parent   with --parent-tree DIR (a built checkout of the parent commit): the cfg 3 force evaluation (200 x shell_N_642,
                        built-in model, device time between two events, median of --reps) and the per-step wall clock of a Brownian
                        Ensemble.run at R = 256 x cfg 1 with the built-in model, in fresh processes of the parent's tree and of
                        this one, alternated (parent first in every pair), --windows each.  The same kernels run in both, so the
                        ratio of the medians has to lie inside the parent's own window spread; the line carries both spreads
  eval_cfg3             cfg 3 with hemisphere types (patch_types) and the tables T_00, T_01, T_11 of n = 1025 points at the built-in
                        cutoff, each the steric law of tools/bench_interaction_tables.py, beside the untyped pair table holding
                        that law and beside the built-in model alone (the same pairs are walked by all)
  run_ens               per-step wall clock of the Brownian run at R = 256 x cfg 1 with the built-in model, without and with the term
    python tools/bench_blob_types.py [--parent-tree DIR] [--windows 3] [--reps 100] [--steps 200] [--jsonl profiles/blob_types.jsonl]"""
import argparse, json, os, subprocess, sys, time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("RBL_BENCH_TREE") or os.path.join(HERE, ".."))      # a worker measures the tree it is given
import numpy as np

MODEL = dict(w=0.3, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)


def steric_table(a, n=1025, eps=1.0, b=0.05):
    from rigid_body_light_amd import tabulate
    r_cut = 2 * a + 20 * b
    U = lambda r: eps * (2 * a / r) * np.exp(-(r - 2 * a) / b)
    return tabulate(U, lambda r: -U(r) * (1.0 / r + 1.0 / b), 2 * a, r_cut, n) + (2 * a, r_cut)


def set_variant(obj, a, cfg, variant):
    """builtin | builtin+table | builtin+typed: the built-in model alone, with the untyped table, with the three type tables"""
    obj.set_interactions(**MODEL)
    if variant == "builtin+table":
        obj.set_pair_table(*steric_table(a))
    if variant == "builtin+typed":
        from rigid_body_light_amd import patch_types
        obj.set_blob_types(patch_types(cfg, [0.0, 0.0, 1.0]), n_types=2)
        for ta, tb in ((0, 0), (0, 1), (1, 1)):
            obj.set_type_table(ta, tb, *steric_table(a))


def eval_cfg3(reps, variants):
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    c = make_config(200, 642, True)
    nb = c["X"].shape[0]
    st = torch.cuda.current_stream()
    out = {}
    for variant in variants:
        ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=st.cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        set_variant(ctx, c["a"], c["cfg"], variant)
        FT = torch.empty(6 * nb, dtype=torch.float64, device="cuda:0")
        for _ in range(5):
            ctx.interaction_forces_dev(None, FT.data_ptr())
        ctx.sync_check()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.interaction_forces_dev(None, FT.data_ptr())
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ctx.sync_check()
        out[variant] = dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), blob_pairs=int(ctx.interaction_stats()[1]),
                            active=ctx.interactions_active())
        ctx.close()
    return out


def run_ens(R, steps, variants):
    from rigid_body_light_amd import Ensemble, make_config
    c = make_config(10, 12, True)
    X = np.tile(c["X"], (R, 1, 1)) + np.random.default_rng(1).uniform(-0.05, 0.05, (R, 10, 3))
    Q = np.tile(c["Q"], (R, 1, 1))
    out = {}
    for variant in variants:
        ens = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=1e-3, kBT=1.0, wall=True)
        set_variant(ens, c["a"], c["cfg"], variant)
        ens.run(20, F=np.zeros(60), seed=1)
        ts = []
        for k in range(3):
            t0 = time.perf_counter()
            ens.run(steps, F=np.zeros(60), seed=100 + 1000 * k)
            ts.append(1e3 * (time.perf_counter() - t0) / steps)
        out[variant] = dict(ms_per_step=float(np.median(ts)), ms_per_step_min=float(np.min(ts)))
        ens.close()
    return out


def worker(args):
    """one window of the never-set comparison: only what the parent commit offers is called"""
    print(json.dumps(dict(cfg3=eval_cfg3(args.reps, ("builtin",))["builtin"], run=run_ens(args.replicas, args.steps, ("builtin",))["builtin"])))


def never_set_vs_parent(args):
    trees = (("parent", os.path.abspath(args.parent_tree)), ("this", os.path.abspath(os.path.join(HERE, ".."))))
    got = {name: [] for name, _ in trees}
    for _ in range(args.windows):
        for name, tree in trees:                                    # parent first in every pair
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(args.reps), "--steps", str(args.steps),
                   "--replicas", str(args.replicas)]
            env = dict(os.environ, RBL_BENCH_TREE=tree)
            env.pop("RBL_LIBRARY", None)
            p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode:
                raise RuntimeError("worker of the %s tree failed:\n%s" % (name, p.stderr[-2000:]))
            got[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = dict(what="never_set_vs_parent", windows=args.windows, reps=args.reps, steps=args.steps, replicas=args.replicas)
    for key, pick in (("cfg3_eval_ms", lambda w: w["cfg3"]["ms"]), ("run_ms_per_step", lambda w: w["run"]["ms_per_step"])):
        par, this = [pick(w) for w in got["parent"]], [pick(w) for w in got["this"]]
        ratio, spread_p, spread_t = float(np.median(this) / np.median(par)), max(par) / min(par), max(this) / min(this)
        line[key] = dict(parent=par, this=this, ratio_of_medians=ratio, parent_spread_max_over_min=spread_p, this_spread_max_over_min=spread_t,
                         inside_parent_spread=bool(1.0 / spread_p <= ratio <= spread_p))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--jsonl", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    if args.parent_tree:
        lines.append(never_set_vs_parent(args))
    ev = eval_cfg3(args.reps, ("builtin", "builtin+table", "builtin+typed"))
    lines.append(dict(what="eval_cfg3", n_table=1025, tables=3, typed_over_untyped_table=ev["builtin+typed"]["ms"] / ev["builtin+table"]["ms"],
                      typed_over_builtin=ev["builtin+typed"]["ms"] / ev["builtin"]["ms"], **ev))
    rn = run_ens(args.replicas, args.steps, ("builtin", "builtin+typed"))
    lines.append(dict(what="run_ens", replicas=args.replicas, steps=args.steps, n_table=1025, tables=3,
                      typed_over_builtin=rn["builtin+typed"]["ms_per_step"] / rn["builtin"]["ms_per_step"], **rn))
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.jsonl:
        with open(args.jsonl, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
