#!/usr/bin/env python3
"""Active microrheology (include/rbl.h section 7): nine shells of 42 blobs above a wall with the library's force model on (weight,
wall and steric repulsion; RigidBody.set_interactions).  One shell, the PROBE, is dragged parallel to the wall at a constant
velocity one layer above the others, the shell in the middle of the layer is HELD (an obstacle), and the remaining seven are
BROWNIAN (kBT = 1, the wrapper's value).  Every step is one `step_brownian_mixed`: the midpoint scheme with the random
displacements kept inside the free shells, one GMRES solve on the GPU, and the instantaneous loads on the probe and the obstacle,
thermal part included.  What a microrheology measurement reads is the TIME AVERAGE of the probe's load; it is printed next to the
load of the same run without temperature (`step_mixed` on a twin object).

python examples/probe_microrheology.py [--steps 200] [--speed 1.0] [--seed 1]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--speed", type=float, default=1.0)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

nb, nblb, dt = 9, 42, 0.01
c = make_config(nb, nblb, wall=True)            # one 3 x 3 layer of shells above the wall
X = c["X"].copy()
held, probe = 4, 0
spacing = X[1, 0] - X[0, 0]
X[probe] = [X[3, 0] - 0.5 * spacing, X[4, 1], X[4, 2] + spacing]        # one layer up, in line with the held shell


def new():
    rb = RigidBody(c["cfg"], X, c["Q"], c["a"], c["eta"], dt=dt, wall_PC=True, block_PC=True)
    rb.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
    return rb


hot, cold = new(), new()                        # the Brownian suspension and its twin without temperature
body_in = np.zeros((nb, 6))                     # free shells: no load beyond the model's; held shell: U = 0
body_in[probe, 0] = args.speed                  # dragged along x, no rotation
# the library's load convention is the reference's (rhs = [slip; -F], U = -N F): the PHYSICAL force on a body is -F
drag, drag0 = np.zeros((args.steps, 3)), np.zeros((args.steps, 3))
print("#  step    time   drag_x   drag_y   drag_z   hold_x   hold_y   hold_z  drag_x(T=0)  iterations")
for n in range(args.steps):
    F, iters, resid = hot.step_brownian_mixed([held, probe], body_in, seed=args.seed + n, max_iter=100, rtol=1e-8)
    F0, _, _ = cold.step_mixed([held, probe], body_in, max_iter=100, rtol=1e-8)
    F, F0 = -F.reshape(nb, 6), -F0.reshape(nb, 6)
    drag[n], drag0[n] = F[probe, :3], F0[probe, :3]
    print("step %3d %7.3f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %4d"
          % (n, (n + 1) * dt, F[probe, 0], F[probe, 1], F[probe, 2], F[held, 0], F[held, 1], F[held, 2], F0[probe, 0], iters))
sem = drag.std(axis=0) / np.sqrt(max(args.steps, 1))
print("mean drag on the probe over %d steps: %s +- %s (standard error of uncorrelated samples); without temperature: %s"
      % (args.steps, np.array2string(drag.mean(axis=0), precision=4), np.array2string(sem, precision=4),
         np.array2string(drag0.mean(axis=0), precision=4)))
Xn = hot.get_config()[0].reshape(-1, 3)
print("probe moved %.4f along x (speed x time = %.4f); held shell moved %.1e; the free shells moved %.4f on average"
      % (Xn[probe, 0] - X[probe, 0], args.speed * args.steps * dt, np.abs(Xn[held] - X[held]).max(),
         np.linalg.norm(np.delete(Xn - X, [held, probe], axis=0), axis=1).mean()))
