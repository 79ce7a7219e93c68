"""Rehearsal of the multi-rank Brownian step WITH the force model on ONE GPU: launch with
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 tools/check_sharded_interactions.py
(gloo process group, every rank on cuda:0).  Each rank evaluates the whole (replicated) force model at q^n inside
ShardedBrownianStepper's step and compares the new configuration with the single-process BrownianStepper."""
import os, sys
import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rigid_body_light_amd import make_config                      # noqa: E402
from rigid_body_light_amd._lib import DeviceContext, lib          # noqa: E402
from rigid_body_light_amd.dist import ShardedMobility             # noqa: E402
from rigid_body_light_amd.krylov import BrownianStepper, ShardedBrownianStepper   # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda:0")
    nb, nblb, wall, kBT, ltol, gtol = 6, 162, True, 0.05, 1e-11, 1e-10
    c = make_config(nb, nblb, wall)
    W = np.random.default_rng(11).standard_normal(9 * nb * nblb)
    Fb = np.zeros(6 * nb)
    model = dict(w=0.2, eps_wall=1.0, b_wall=0.05, eps_blob=1.0, b_blob=0.05, r_cut=2 * c["a"] + 1.0)
    out, FTmax = [], 0.0
    for sharded in (True, False):
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], kBT=kBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        lib().rbl_set_blk_pc(ctx.h, 1)
        ctx.set_interactions(**model)
        FTmax = float(np.abs(ctx.interaction_forces()[1]).max())
        if sharded:
            st = ShardedBrownianStepper(ctx, ShardedMobility(nb, nblb, device=dev, ctx=ctx), nb, nblb, dev, c["a"], wall, kBT,
                                        c["dt"], lanczos_tol=ltol, lanczos_max_iter=255)
            m, resid = st.step(Fb, W=W, iters=150, rtol=gtol)
        else:
            ctx.set_lanczos(255, ltol)
            m, resid = BrownianStepper(ctx, nb, nblb, dev).step(Fb, W=W, method=2, iters=150, rtol=gtol)
        out.append(ctx.get_config(nb))
        ctx.close()
    dX = float(np.abs(out[0][0] - out[1][0]).max()); dQ = float(np.abs(out[0][1] - out[1][1]).max())
    moved = float(np.abs(out[0][0] - c["X"]).max())
    t = torch.tensor([dX, dQ]); dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print("world %d: max |X_sharded - X_single| = %.3e, max |Q diff| = %.3e (bodies moved by %.3e, |K^T f| max %.3e)"
              % (world, t[0], t[1], moved, FTmax))
    ok = t[0] < 1e-8 and t[1] < 1e-8 and moved > 1e-4 and resid < gtol and FTmax > 0.1
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
