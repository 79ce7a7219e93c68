#!/usr/bin/env python3
"""A sedimented Brownian layer at a fixed area fraction: 9 shells of 12 blobs above the wall in a periodic cell of three lattice
spacings by three (include/rbl.h section 10; RigidBody.set_periodic).  Every mobility product of the step -- the Lanczos roots,
the drift term, the saddle solve -- sums the wall-corrected pair mobility over (1, 1) periodic images on either side of every
pair's nearest one, and the steric repulsion acts through the boundaries by minimum image, so the layer neither spreads nor has
an edge.  Coordinates stay unwrapped: the area fraction is that of the cell, whatever the bodies' excursions.  The sum is
truncated -- its remainder falls like 1 / n with the image count -- and its positivity is observed, not proven
(tests/test_periodic_cpu.py).  Prints the mean height and the smallest centre distance by minimum image per step."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, make_config

nb, nblb, steps = 9, 12, 20
c = make_config(nb, nblb, wall=True)           # one 3 x 3 layer of bodies above the wall
spacing = 2.0 * (1.0 + c["a"]) + 0.5
Lx = Ly = 3.0 * spacing
R_body = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
print("cell %.3f x %.3f, area fraction of the bodies' discs %.3f" % (Lx, Ly, nb * np.pi * (R_body + c["a"]) ** 2 / (Lx * Ly)))
rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt=0.01, wall_PC=True, block_PC=True)
rb.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)   # r_cut = 2a + 1: 2 R_body + r_cut <= L / 2
rb.set_periodic(Lx, Ly, images=(1, 1))
F = np.zeros(6 * nb)                            # no external force beyond the model
for n in range(steps):
    iters, resid = rb.step_brownian(F, seed=n, method="lanczos_pc", max_iter=60, rtol=1e-8)
    X = rb.get_config()[0].reshape(-1, 3)
    d = X[:, None, :] - X[None, :, :]
    d[..., 0] -= Lx * np.rint(d[..., 0] / Lx)
    d[..., 1] -= Ly * np.rint(d[..., 1] / Ly)
    dist = np.linalg.norm(d, axis=2) + 1e9 * np.eye(nb)
    print("step %2d: mean height %.4f, closest centres (minimum image) %.3f  (%d GMRES iterations)" % (n, X[:, 2].mean(), dist.min(), iters))
