"""One-vector symmetric product (four rows per lane, four-wave workgroups, work queue) against its unit schedule: chunk length C
(RBL_OPT_SYM_CHUNK) x short chunk length C_f (RBL_OPT_SYM_TAIL_CHUNK) x share of the column tiles at the short length
(RBL_OPT_SYM_TAIL_SHARE), interleaved with the one-length schedules of the same C -- "rect": the old draw over the whole (row group
x chunk) rectangle, "live": live units only, shortest last -- what sym_geometry's SYM_TAIL_RULE is set from
(profiles/sym_unit_schedule.md).  Prints one line per schedule and size: minimum and median over ROUNDS alternations of the mean
of REPS products, and the ratio of the minimum to rect at the heuristic's C.
usage: bench_unit_schedule.py [bodies:blobs[:wall] ...]   (default: shell_N_642 suspensions of 2 007, 1 004 and 642 tiles, wall)
env: ROUNDS (5), REPS (5), CHUNKS ("8,12,15"), TAILS ("3,4,5"), SHARES per cent ("10,20,30")"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from rigid_body_light_amd import make_config
from rigid_body_light_amd._lib import DeviceContext

ROUNDS = int(os.environ.get("ROUNDS", "5")); REPS = int(os.environ.get("REPS", "5"))
CHUNKS = [int(x) for x in os.environ.get("CHUNKS", "8,12,15").split(",")]
TAILS = [int(x) for x in os.environ.get("TAILS", "3,4,5").split(",")]
SHARES = [int(x) for x in os.environ.get("SHARES", "10,20,30").split(",")]
sizes = [tuple(int(x) for x in a.split(":")) for a in sys.argv[1:]] or [(200, 642, 1), (100, 642, 1), (64, 642, 1)]
dev = torch.device("cuda:0"); st = torch.cuda.current_stream()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for sz in sizes:
    nb, nblb = sz[0], sz[1]
    wall = bool(sz[2]) if len(sz) > 2 else True
    c = make_config(nb, nblb, wall); N = nb * nblb
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], stream_ptr=st.cuda_stream); ctx.set_config(c["X"], c["Q"])
    r = torch.empty(3 * N, dtype=torch.float64, device=dev); ctx.blob_positions(0, nb, r.data_ptr())
    F = torch.from_numpy(np.random.default_rng(2).standard_normal(3 * N)).to(dev)
    U = torch.empty_like(F)
    ctx.set_option("sym_waves", 4); ctx.set_option("sym_rows_per_lane", 4)
    c_auto = ctx.apply_M_sym_info(N, 1, 1)[1]
    # schedule = (label, sym_chunk, sym_tail_chunk, sym_tail_share)
    scheds = [("default", 0, 0, 0)]
    for C in sorted(set(CHUNKS + [c_auto])):
        scheds += [("C%d rect" % C, C, C, 1000), ("C%d live" % C, C, C, 0)]
        scheds += [("C%d Cf%d %d%%" % (C, cf, sh), C, cf, 10 * sh) for cf in TAILS for sh in SHARES if cf < C]
    times = {s[0]: [] for s in scheds}
    for _ in range(ROUNDS):
        for label, C, cf, share in scheds:
            ctx.set_option("sym_chunk", C); ctx.set_option("sym_tail_chunk", cf); ctx.set_option("sym_tail_share", share)
            ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr()); ctx.sync_check()
            e0.record(st)
            for _ in range(REPS):
                ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr())
            e1.record(st); ctx.sync_check()
            times[label].append(e0.elapsed_time(e1) / REPS)
    ref = min(times["C%d rect" % c_auto])
    print("%d x shell_N_%d %s N=%d tiles=%d heuristic C=%d" % (nb, nblb, "wall" if wall else "free", N, (N + 63) // 64, c_auto), flush=True)
    for label, *_ in scheds:
        v = sorted(times[label])
        print("  %-16s min %.4f med %.4f max %.4f ms   min / (C%d rect) = %.4f" % (label, v[0], v[len(v) // 2], v[-1], c_auto, v[0] / ref), flush=True)
    print(json.dumps({"tool": "bench_unit_schedule", "n_blobs": N, "tiles": (N + 63) // 64, "wall": wall, "rounds": ROUNDS, "reps": REPS,
                      "ms": {k: [round(x, 4) for x in v] for k, v in times.items()}}), flush=True)
    ctx.close()
