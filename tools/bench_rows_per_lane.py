"""One-vector symmetric product with two against four rows per lane (RBL_OPT_SYM_ROWS_PER_LANE = 2 / 4, four-wave workgroups) at
several sizes, interleaved: what sym_geometry's RBL_SYM_NI4_TILES threshold is set from.  Prints one line per size: the minimum
and median over ROUNDS alternations of the mean of 10 products each.
usage: bench_rows_per_lane.py [bodies:blobs[:wall] ...]   (default: a size sweep of shell_N_642 suspensions, wall-corrected)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from rigid_body_light_amd import make_config
from rigid_body_light_amd._lib import DeviceContext

ROUNDS = int(os.environ.get("ROUNDS", "5"))
sizes = [tuple(int(x) for x in a.split(":")) for a in sys.argv[1:]] or [(25, 642, 1), (41, 642, 1), (64, 642, 1), (100, 642, 1), (200, 642, 1)]
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
    ctx.set_option("sym_waves", 4)
    times = {2: [], 4: []}
    for _ in range(ROUNDS):
        for rows in (2, 4):
            ctx.set_option("sym_rows_per_lane", rows)
            ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr()); ctx.sync_check()
            e0.record(st)
            for _ in range(10):
                ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr())
            e1.record(st); ctx.sync_check()
            times[rows].append(e0.elapsed_time(e1) / 10)
    ctx.set_option("sym_rows_per_lane", 0); ctx.set_option("sym_waves", 0)
    dflt = ctx.apply_M_sym_kernel(N, wall, 1, 1)
    s = {k: (min(v), sorted(v)[len(v) // 2]) for k, v in times.items()}
    print("%4d x shell_N_%d %s N=%7d tiles=%5d  2 rows: min %.4f med %.4f ms   4 rows: min %.4f med %.4f ms   4/2 = %.3f   default: %s"
          % (nb, nblb, "wall" if wall else "free", N, (N + 63) // 64, s[2][0], s[2][1], s[4][0], s[4][1], s[4][0] / s[2][0], dflt), flush=True)
    ctx.close()
