"""Time rbl_interaction_forces_dev (neighbour lists + pair kernel + K^T f) at three sizes and print, per size, the median
milliseconds, the candidate (ordered) body pairs and the ordered blob pairs inside r_cut:
  cfg3          200 x shell_N_642 with the wall (synth.make_config, surface gap ~0.55)
  cfg2          50 x shell_N_162, free space
  cfg3_packed   the cfg 3 lattice compressed to a surface gap of ~2 b_blob
Model: w = 0.3, eps_wall = 1, b_wall = 0.1, eps_blob = 1, b_blob = 0.05, r_cut = 2a + 20 b_blob.
    python tools/bench_interactions.py [--reps 50] [--json out.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from rigid_body_light_amd import make_config
from rigid_body_light_amd._lib import DeviceContext


def case(name):
    if name == "cfg2":
        return make_config(50, 162, False), False
    c = make_config(200, 642, True)
    if name == "cfg3_packed":           # lattice spacing 2 (R_body + a) + gap with gap = 2 b_blob, as make_config lays it out
        R = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
        old = 2.0 * (1.0 + c["a"]) + 0.5
        new = 2.0 * (R + c["a"]) + 2 * 0.05
        z0 = c["X"][:, 2].min()
        c["X"] = c["X"] * (new / old)
        c["X"][:, 2] += z0 - c["X"][:, 2].min()
    return c, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    out = {}
    for name in ("cfg3", "cfg2", "cfg3_packed"):
        c, wall = case(name)
        nb, nblb = c["X"].shape[0], c["cfg"].shape[0]
        st = torch.cuda.current_stream()
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=st.cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        ctx.set_interactions(w=0.3, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
        FT = torch.empty(6 * nb, dtype=torch.float64, device="cuda:0")
        for _ in range(3):
            ctx.interaction_forces_dev(None, FT.data_ptr())
        ctx.sync_check()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.interaction_forces_dev(None, FT.data_ptr())
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ctx.sync_check()
        bp, pp = ctx.interaction_stats()
        ms = float(np.median(ts))
        out[name] = dict(ms=ms, ms_min=float(np.min(ts)), body_pairs=bp, blob_pairs=pp, n_blobs=nb * nblb,
                         pairs_per_ns=pp / (ms * 1e6))
        print("%-12s %6d blobs  %8.4f ms (min %.4f)  candidate body pairs %6d  ordered blob pairs %11d  %.2f pairs/ns"
              % (name, nb * nblb, ms, np.min(ts), bp, pp, pp / (ms * 1e6)), flush=True)
        ctx.close()
    if args.json:
        json.dump(out, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
