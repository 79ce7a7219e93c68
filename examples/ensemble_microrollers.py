#!/usr/bin/env python3
"""A height sweep of a microroller in ONE call per step (include/rbl.h section 5, ensembles with a mask per velocity component):
R replicas of one shell of 12 blobs above the wall, replica r at its own height.  In every replica the ANGULAR velocity is
prescribed in the lab frame -- Omega about y, none about x and z -- while the three translations stay free and carry no load.
`Ensemble.step_mixed_dof` solves and steps all R systems in one launch of the one-kernel solver: the free translations come back
as the displacement of the step, the rotational slots of F hold the torque it takes to keep the shell spinning.  The nearer the
wall, the faster the shell rolls and the larger the torque; it rolls towards +x for Omega_y > 0 (examples/microroller.py) and the
other way when Omega changes sign.  Prints rolling velocity and driving torque against height.

python examples/ensemble_microrollers.py [--replicas 16] [--steps 3] [--omega 10.0]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, load_structure

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=16)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--omega", type=float, default=10.0)
args = ap.parse_args()

p, cfg = load_structure(12)
a, dt, R = p["sep"] / 2.0, 1e-3, args.replicas
radius = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()) + a       # outermost blob centre plus a blob radius
heights = radius * np.geomspace(1.1, 6.0, R)                                    # centre heights: a tenth of a radius of gap, upwards
X = np.zeros((R, 1, 3))
X[:, 0, 2] = heights
Q = np.zeros((R, 1, 4))
Q[:, 0, 0] = 1.0
ens = Ensemble(cfg, X, Q, a, 1.0, dt, wall=True)

prescribed = np.zeros((1, 6), dtype=bool)
prescribed[0, 3:] = True                        # the three rotational components; the translations are free
body_in = np.zeros((1, 6))                      # free slots: no load
body_in[0, 4] = args.omega                      # rotation about the lab's y axis

X0 = ens.get_config()[0]
for n in range(args.steps):
    F, iters, resid = ens.step_mixed_dof(prescribed, body_in, max_iter=100, rtol=1e-10)
Xn = ens.get_config()[0]
# the library's load convention is the reference's (rhs = [slip; -F]): the PHYSICAL torque on a body is -F
torque_y = -F.reshape(R, 6)[:, 4]
Ux = (Xn - X0)[:, 0, 0] / (args.steps * dt)    # the free translation the steps solved for, averaged over the run
print("#  replica   height/radius   rolling U_x   U_x/(Omega radius)   torque_y   iterations")
for r in range(R):
    print("roller %3d %12.4f %14.6e %14.6e %14.6e %4d" % (r, heights[r] / radius, Ux[r], Ux[r] / (args.omega * radius), torque_y[r], iters[r]))
print("Omega_y = %g, shell radius %.3f, %d steps of dt = %g: %d systems per launch" % (args.omega, radius, args.steps, dt, R))
ens.close()
