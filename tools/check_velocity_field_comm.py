"""Velocity field on a context with a communicator, against the single-rank result, bitwise: launch with
    python -m torch.distributed.run --nproc-per-node 3 --master-addr 127.0.0.1 tools/check_velocity_field_comm.py
(gloo process group, every rank on cuda:0, the callbacks of rbl_set_comm_ops), or with RBL_VF_NCCL=1 as a plain process: a
communicator of ONE rank over RCCL inside librbl (the code path N ranks run).  Every rank evaluates its share of the points
and one all-gather completes u; the point count is not a multiple of the rank count nor of the point tiles."""
import os, socket, sys
import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rigid_body_light_amd import make_config                      # noqa: E402
from rigid_body_light_amd._lib import DeviceContext               # noqa: E402
from rigid_body_light_amd.dist import ShardedMobility             # noqa: E402
from oracle import Oracle                                         # noqa: E402


def main():
    native = os.environ.get("RBL_VF_NCCL", "0") == "1"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if native:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    ok = True
    for wall in (True, False):
        nb, nblb = 20, 42
        c = make_config(nb, nblb, wall)
        rng = np.random.default_rng(3)
        lam = rng.standard_normal(3 * nb * nblb)
        lo, hi = c["X"].min(axis=0) - 3.0, c["X"].max(axis=0) + 3.0
        P = 1000 + 3 * 128 + 7                                         # ragged against ranks and point tiles
        pts = rng.uniform(lo, hi, (P, 3))
        r = Oracle().multi_body_pos(c["X"], c["Q"], c["cfg"] - c["cfg"].mean(axis=0))   # explicit positions; None: the context's own
        out = []
        for sharded in (False, True):
            ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
            ctx.set_config(c["X"], c["Q"])
            if sharded:
                ctx.set_comm(ShardedMobility(nb, nblb, device=dev, ctx=ctx, force_collectives=native), native=native)
            out.append((ctx.velocity_field(pts, lam, positions=r), ctx.velocity_field(pts, lam)))
            ctx.close()
        same = bool(np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]))
        diff = float(np.abs(out[0][0] - out[1][0]).max())
        t = torch.tensor([0.0 if same else 1.0, diff], device=dev if native else "cpu"); dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if rank == 0:
            print("world %d (%s), wall %s: bitwise equal %s, max |u_sharded - u_single| = %.3e"
                  % (world, "RCCL in librbl" if native else "gloo callbacks", wall, t[0].item() == 0.0, t[1].item()), flush=True)
        ok = ok and t[0].item() == 0.0
    dist.destroy_process_group()
    if rank == 0:
        print("ALL OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
