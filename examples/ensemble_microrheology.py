#!/usr/bin/env python3
"""Active microrheology as an ENSEMBLE average (include/rbl.h sections 5 and 7): the scene of probe_microrheology.py with shells
of 12 blobs -- nine shells above a wall with the force model on, one dragged parallel to the wall one layer above the others
(the PROBE), the one in the middle of the layer HELD, seven BROWNIAN -- run as R replicas that start from the same configuration
and see independent noise.  Every step is ONE `Ensemble.step_brownian_mixed`: a fixed number of launches whatever R is, and the
instantaneous load on the probe in every replica.  A measurement wants the average over noise realisations: printed per step is
the ensemble mean of the probe's drag with its standard error over the replicas, next to the drag of the same step without
temperature (`step_mixed` on a one-replica twin).

python examples/ensemble_microrheology.py [--replicas 256] [--steps 100] [--speed 1.0] [--seed 1]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", type=int, default=256)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--speed", type=float, default=1.0)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

nb, nblb, dt, R = 9, 12, 0.01, args.replicas     # 9 x 12 = 108 blobs: up to 21 such shells fit the one-kernel solver
c = make_config(nb, nblb, wall=True)            # one 3 x 3 layer of shells above the wall
X = c["X"].copy()
held, probe = 4, 0
spacing = X[1, 0] - X[0, 0]
X[probe] = [X[3, 0] - 0.5 * spacing, X[4, 1], X[4, 2] + spacing]        # one layer up, in line with the held shell


def new(replicas):
    ens = Ensemble(c["cfg"], np.repeat(X[None], replicas, axis=0), np.repeat(c["Q"][None], replicas, axis=0), a=c["a"], eta=c["eta"],
                   dt=dt, kBT=1.0, wall=True)
    ens.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
    return ens


hot, cold = new(R), new(1)                      # the Brownian replicas and one twin without temperature
body_in = np.zeros((nb, 6))                     # free shells: no load beyond the model's; held shell: U = 0
body_in[probe, 0] = args.speed                  # dragged along x, no rotation
# the library's load convention is the reference's (rhs = [slip; -F], U = -N F): the PHYSICAL force on a body is -F
mean, mean0 = np.zeros((args.steps, 3)), np.zeros((args.steps, 3))
print("#  step    time   <drag_x>      +-   <drag_y>      +-   <drag_z>      +-  drag_x(T=0)  iterations(max)")
for n in range(args.steps):
    F, iters, resid = hot.step_brownian_mixed([held, probe], body_in, seed=args.seed + n, max_iter=100, rtol=1e-8)
    F0, _, _ = cold.step_mixed([held, probe], body_in, max_iter=100, rtol=1e-8)
    drag = -F.reshape(R, nb, 6)[:, probe, :3]
    m, se = drag.mean(axis=0), drag.std(axis=0, ddof=1 if R > 1 else 0) / np.sqrt(R)
    mean[n], mean0[n] = m, -F0.reshape(nb, 6)[probe, :3]
    print("step %3d %7.3f %9.4f %7.4f %9.4f %7.4f %9.4f %7.4f %9.4f %4d"
          % (n, (n + 1) * dt, m[0], se[0], m[1], se[1], m[2], se[2], mean0[n, 0], iters.max()))
sem = mean.std(axis=0) / np.sqrt(max(args.steps, 1))
print("mean drag on the probe over %d replicas and %d steps: %s +- %s (standard error of the step means); without temperature: %s"
      % (R, args.steps, np.array2string(mean.mean(axis=0), precision=4), np.array2string(sem, precision=4),
         np.array2string(mean0.mean(axis=0), precision=4)))
Xn = hot.get_config()[0]
print("every probe moved %.4f along x (speed x time = %.4f); the held shells moved %.1e; the free shells moved %.4f on average"
      % (Xn[0, probe, 0] - X[probe, 0], args.speed * args.steps * dt, np.abs(Xn[:, held] - X[held]).max(),
         np.linalg.norm(np.delete(Xn - X[None], [held, probe], axis=1), axis=2).mean()))
