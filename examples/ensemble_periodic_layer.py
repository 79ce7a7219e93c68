#!/usr/bin/env python3
"""The sedimented Brownian layer of examples/periodic_layer.py -- 9 shells of 12 blobs above the wall in a periodic cell of three
lattice spacings by three -- as R independent replicas stepped together in ONE call (include/rbl.h section 5:
rbl_ensemble_set_periodic, rbl_ensemble_run; Ensemble.set_cell, Ensemble.run).  A layer at a fixed area fraction needs thousands of
decorrelated steps before it measures anything; the replicas take them side by side, each in its own workgroup of the one-kernel
solver, whose pair sweep sums the wall-corrected mobility over (1, 1) periodic images on either side of every pair's nearest one.
The steric repulsion acts through the boundaries by minimum image; replicas never interact.  Coordinates stay unwrapped.
Prints, per recorded frame, the mean height over all replicas and the closest centres by minimum image in any replica."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=64)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--stride", type=int, default=20, help="steps between recorded frames")
args = ap.parse_args()

nb, nblb = 9, 12
c = make_config(nb, nblb, wall=True)           # one 3 x 3 layer of bodies above the wall
spacing = 2.0 * (1.0 + c["a"]) + 0.5
Lx = Ly = 3.0 * spacing
R_body = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
print("%d replicas, cell %.3f x %.3f, area fraction of the bodies' discs %.3f"
      % (args.replicas, Lx, Ly, nb * np.pi * (R_body + c["a"]) ** 2 / (Lx * Ly)))
X0 = np.repeat(c["X"][None], args.replicas, axis=0)          # every replica starts from the lattice; the noise decorrelates them
Q0 = np.repeat(c["Q"][None], args.replicas, axis=0)
ens = Ensemble(c["cfg"], X0, Q0, c["a"], c["eta"], dt=0.01, kBT=1.0, wall=True)
ens.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)   # r_cut = 2a + 1: 2 R_body + r_cut <= L / 2
ens.set_cell(Lx, Ly, images=(1, 1))
out = ens.run(args.steps, F=np.zeros(6 * nb), brownian=True, seed=7, stride=args.stride, on_error="reject", max_iter=100, rtol=1e-8)
for k in range(out.X.shape[0]):
    X = out.X[k]                                             # (R, N_bod, 3), unwrapped
    d = X[:, :, None, :] - X[:, None, :, :]
    d[..., 0] -= Lx * np.rint(d[..., 0] / Lx)
    d[..., 1] -= Ly * np.rint(d[..., 1] / Ly)
    dist = np.linalg.norm(d, axis=3) + 1e9 * np.eye(nb)
    print("step %4d: mean height %.4f, closest centres (minimum image) %.3f" % ((k + 1) * args.stride, X[:, :, 2].mean(), dist.min()))
print("accepted steps per replica %d .. %d, rejected %d in all; %.1f GMRES iterations per step"
      % (out.accepted.min(), out.accepted.max(), out.rejected.sum(), out.iters_sum.sum() / max(1, out.accepted.sum())))
ens.close()
