#!/usr/bin/env python3
"""A quasi-two-dimensional Brownian layer (include/rbl.h sections 5 and 7, the Brownian midpoint step with a mask per velocity
component): R replicas of a few shells of 12 blobs above the wall, every body with U_z = 0 -- the z component of every body is
prescribed (held), the in-plane translations and the whole rotation stay free and Brownian.  `Ensemble.step_brownian_mixed_dof`
advances all replicas in one launch sequence per step.  The heights keep their bits; in the plane the bodies diffuse with the
constrained mobility Ntilde = ((K D_f)^T M^-1 K D_f)^-1, which the example estimates without an oracle from the library's own
constrained solve (`Ensemble.solve_mixed_dof`: a unit force along x or y on one body, z of all bodies held, gives a column of
Ntilde) at the first configuration.  It prints the in-plane mean-squared displacement next to 2 kBT (Ntilde_xx + Ntilde_yy) t.
The comparison is loose -- Ntilde changes as the bodies move, and the sample is R x N_bod bodies -- and is printed, not asserted.

python examples/ensemble_quasi2d.py [--replicas 64] [--bodies 4] [--steps 40]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, load_structure

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=64)
ap.add_argument("--bodies", type=int, default=4)
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()

p, cfg = load_structure(12)
a, dt, kBT, R, nb = p["sep"] / 2.0, 1e-2, 1.0, args.replicas, args.bodies
radius = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()) + a       # outermost blob centre plus a blob radius
X = np.zeros((R, nb, 3))
X[:, :, 0] = 4.0 * radius * (np.arange(nb) % 2)                                 # a small lattice, two shell diameters apart
X[:, :, 1] = 4.0 * radius * (np.arange(nb) // 2)
X[:, :, 2] = 1.5 * radius                                                      # the layer's height: half a radius of gap
Q = np.random.default_rng(1).standard_normal((R, nb, 4))
Q /= np.linalg.norm(Q, axis=2, keepdims=True)
ens = Ensemble(cfg, X, Q, a, 1.0, dt, kBT=kBT, wall=True)

prescribed = np.zeros((nb, 6), dtype=bool)
prescribed[:, 2] = True                         # U_z of every body; x, y and the rotation are free
body_in = np.zeros((nb, 6))                     # no loads, U_z = 0

# Ntilde_xx + Ntilde_yy per body from the constrained solve: U = -Ntilde F on the free components (rhs [slip; -F])
N_plane = np.zeros((R, nb))
for b in range(nb):
    for k in (0, 1):
        load = np.zeros((nb, 6))
        load[b, k] = -1.0
        U = ens.solve_mixed_dof(prescribed, load, max_iter=100, rtol=1e-10)[1].reshape(R, nb, 6)
        N_plane[:, b] += U[:, b, k]
N_mean = float(N_plane.mean())

X0 = ens.get_config()[0]
print("#  step      t   MSD_xy(sample)   2 kBT (Nxx + Nyy) t   ratio   mean iterations")
for n in range(args.steps):
    F, iters, resid = ens.step_brownian_mixed_dof(prescribed, body_in, seed=100 + n, max_iter=100, rtol=1e-8)
    Xn = ens.get_config()[0]
    msd = float(((Xn - X0)[:, :, :2] ** 2).sum(axis=2).mean())
    t = (n + 1) * dt
    print("step %3d %6.3f %14.6e %14.6e %8.3f %8.1f" % (n + 1, t, msd, 2.0 * kBT * N_mean * t, msd / (2.0 * kBT * N_mean * t), iters.mean()))
held = bool(np.array_equal(Xn[:, :, 2], X0[:, :, 2]))
se = np.sqrt(2.0 / (2 * R * nb))                # the relative standard error of a variance from 2 R N_bod Gaussian samples
print("heights unchanged bit for bit: %s; %d bodies in %d replicas, %d steps of dt = %g; Ntilde_xx + Ntilde_yy = %.5f (first configuration);"
      " one-step sampling error of the ratio about %.0f %%" % (held, nb, R, args.steps, dt, N_mean, 100 * se))
ens.close()
