#!/usr/bin/env python3
"""An area-fraction sweep in ONE call: the sedimented Brownian layer of examples/ensemble_periodic_layer.py -- 9 shells of 12 blobs
above the wall, periodic in x and y -- at eight area fractions, `--replicas` replicas each, every replica in a periodic cell of its
own (include/rbl.h section 5: rbl_ensemble_set_cells, rbl_ensemble_run; Ensemble.set_cells, Ensemble.run).  The cell is the one
physical parameter of a layer that sets its area fraction; with a cell per replica the whole sweep is one ensemble and one run,
and costs barely more than one of its points, because the steps are latency-bound.  Replica r starts from the 3 x 3 lattice
stretched to its cell.  Prints the short-time self-diffusion coefficient in the plane, <|dX_xy|^2> / (4 t) over the accepted
steps, against the area fraction of the bodies' discs (Ensemble.area_fraction)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=32, help="replicas per area fraction")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--images", type=int, default=1, help="periodic images on either side of the nearest one, per axis")
args = ap.parse_args()

nb, nblb, dt = 9, 12, 0.01
c = make_config(nb, nblb, wall=True)           # one 3 x 3 layer of bodies above the wall
spacing = 2.0 * (1.0 + c["a"]) + 0.5
stretch = np.linspace(1.0, 2.0, 8)             # the lattice and the cell stretched together: eight area fractions
scale = np.repeat(stretch, args.replicas)      # (R,), the fractions' replicas side by side
R = scale.size
X0 = np.repeat(c["X"][None], R, axis=0)
X0[:, :, :2] *= scale[:, None, None]
Q0 = np.repeat(c["Q"][None], R, axis=0)
ens = Ensemble(c["cfg"], X0, Q0, c["a"], c["eta"], dt=dt, kBT=1.0, wall=True)
ens.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)   # r_cut = 2a + 1: 2 R_body + r_cut <= L / 2
ens.set_cells(3.0 * spacing * scale, 3.0 * spacing * scale, images=(args.images, args.images))
R_body = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
phi = ens.area_fraction(np.pi * (R_body + c["a"]) ** 2)
out = ens.run(args.steps, F=np.zeros(6 * nb), brownian=True, seed=7, on_error="reject", max_iter=100, rtol=1e-8)
X1, _ = ens.get_config()
t = dt * np.maximum(out.accepted, 1)                           # a rejected step does not advance its replica
D = ((X1[:, :, :2] - X0[:, :, :2]) ** 2).sum(axis=2).mean(axis=1) / (4.0 * t)
print("%d replicas: 8 area fractions x %d, %d steps; accepted %d .. %d per replica, rejected %d in all, %.1f GMRES iterations per step"
      % (R, args.replicas, args.steps, out.accepted.min(), out.accepted.max(), out.rejected.sum(),
         out.iters_sum.sum() / max(1, out.accepted.sum())))
print("area fraction   cell      D_s (plane)   +- (standard error over the replicas)")
for k in range(stretch.size):
    sel = slice(k * args.replicas, (k + 1) * args.replicas)
    print("   %.4f    %7.3f    %.5f       %.5f" % (phi[sel][0], ens.cells()["Lx"][sel][0], D[sel].mean(),
                                                   D[sel].std(ddof=1) / np.sqrt(args.replicas) if args.replicas > 1 else 0.0))
ens.close()
