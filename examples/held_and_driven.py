#!/usr/bin/env python3
"""Held and driven bodies (include/rbl.h section 7): nine shells of 42 blobs above a wall.  The shell in the middle of the layer
is HELD (an obstacle: U = 0), one shell is DRAGGED parallel to the wall at a fixed speed one layer above the others -- it starts
half a lattice spacing before the middle row and, with the default 160 steps, has passed over the whole row, the held shell
included, by the end -- and the remaining seven are free and sediment under the library's force model (weight, wall and steric repulsion;
RigidBody.set_interactions).  Every step is one `step_mixed`: a single GMRES solve on the GPU returns the velocities of the free
shells and the loads on the two prescribed ones.  Prints, per step, the physical force it takes to drag the driven shell and the
one that holds the obstacle in place -- the total that the outside world supplies together with the model, whose own share on
those two shells (`interaction_forces`) is printed once at the start.  At the end: the 54 x 54 body resistance matrix of the final
configuration, its unit velocities solved in lock step (`body_resistance_matrix(lock_step=True)`, 16 columns advancing together).

python examples/held_and_driven.py [--steps 160] [--speed 1.0]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=160)
ap.add_argument("--speed", type=float, default=1.0)
args = ap.parse_args()

nb, nblb, dt = 9, 42, 0.05
c = make_config(nb, nblb, wall=True)            # one 3 x 3 layer of shells above the wall
X = c["X"].copy()
held, driven = 4, 0
spacing = X[1, 0] - X[0, 0]
X[driven] = [X[3, 0] - 0.5 * spacing, X[4, 1], X[4, 2] + spacing]       # one layer up, in line with the held shell
rb = RigidBody(c["cfg"], X, c["Q"], c["a"], c["eta"], dt=dt, wall_PC=True, block_PC=True)
rb.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)

body_in = np.zeros((nb, 6))                     # free shells: no load beyond the model's; held shell: U = 0
body_in[driven, 0] = args.speed                 # dragged along x, no rotation
# the library's load convention is the reference's (rhs = [slip; -F], U = -N F): the PHYSICAL force on a body is -F
share = -rb.interaction_forces().reshape(nb, 6)
print("the model's own share of the physical forces: driven %s, held %s"
      % (np.array2string(share[driven, :3], precision=4), np.array2string(share[held, :3], precision=4)))
print("#  step    time   drag_x   drag_y   drag_z   hold_x   hold_y   hold_z  iterations")
for n in range(args.steps):
    F, iters, resid = rb.step_mixed([held, driven], body_in, max_iter=100, rtol=1e-8)
    F = -F.reshape(nb, 6)                       # physical force everything other than the fluid exerts on each body
    print("step %3d %7.3f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %4d"
          % (n, (n + 1) * dt, F[driven, 0], F[driven, 1], F[driven, 2], F[held, 0], F[held, 1], F[held, 2], iters))
Xn, _ = rb.get_config()
Xn = Xn.reshape(-1, 3)
print("driven shell moved %.4f along x (speed x time = %.4f); held shell moved %.1e; mean height of the free shells %.4f"
      % (Xn[driven, 0] - X[driven, 0], args.speed * args.steps * dt, np.abs(Xn[held] - X[held]).max(),
         np.delete(Xn[:, 2], [held, driven]).mean()))
# the resistance matrix of where they ended up: R U = the physical loads that move all nine shells with velocities U
R, its = rb.body_resistance_matrix(rtol=1e-8, lock_step=True)
print("resistance matrix in lock step: %d columns, iterations %d..%d, asymmetry %.1e; drag coefficient of the held shell along x, y, z: %s"
      % (R.shape[1], its.min(), its.max(), np.linalg.norm(R - R.T) / np.linalg.norm(R),
         np.array2string(np.diag(R)[6 * held:6 * held + 3], precision=4)))
