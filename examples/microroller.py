#!/usr/bin/env python3
"""Microrollers (include/rbl.h section 7, masks per velocity component): four shells of 42 blobs just above a wall, spun by a
rotating field.  The ANGULAR velocity of every shell is prescribed in the lab frame -- Omega about y, none about x and z -- while
its three translations stay free and carry only what the library's force model supplies (weight, wall and steric repulsion;
RigidBody.set_interactions).  Every step is one `step_mixed_dof`: a single GMRES solve on the GPU returns the translation the
spinning shells pick up from the wall -- they roll along x, and the other way when Omega changes sign -- and, in the rotational
slots of F, the torque it takes to keep them spinning.  Prints both per step.

python examples/microroller.py [--steps 40] [--omega 10.0]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--omega", type=float, default=10.0)
args = ap.parse_args()

nb, nblb, dt = 4, 42, 0.01
c = make_config(nb, nblb, wall=True)            # a 2 x 2 layer of shells above the wall
rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt=dt, wall_PC=True, block_PC=True)
rb.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)

prescribed = np.zeros((nb, 6), dtype=bool)
prescribed[:, 3:] = True                        # the three rotational components; the translations are free
body_in = np.zeros((nb, 6))                     # free slots: no load beyond the model's
body_in[:, 4] = args.omega                      # rotation about the lab's y axis
X0 = np.array(rb.get_config()[0]).reshape(nb, 3)
Xp = X0
print("#  step    time   mean_U_x   mean_U_z   mean_height   mean_torque_y  iterations")
for n in range(args.steps):
    F, iters, resid = rb.step_mixed_dof(prescribed, body_in, max_iter=100, rtol=1e-8)
    Xn = np.array(rb.get_config()[0]).reshape(nb, 3)
    U = (Xn - Xp) / dt                          # the free translations the step solved for
    Xp = Xn
    # the library's load convention is the reference's (rhs = [slip; -F]): the PHYSICAL torque on a body is -F
    torque_y = -F.reshape(nb, 6)[:, 4]
    print("step %3d %7.3f %10.5f %10.5f %10.5f %12.5f %4d" % (n, (n + 1) * dt, U[:, 0].mean(), U[:, 2].mean(), Xn[:, 2].mean(), torque_y.mean(), iters))
T = args.steps * dt
radius = float(np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()) + c["a"]      # outermost blob centre plus a blob radius
print("rolling velocity along x %.5f (Omega_y = %g, shell radius %.3f: rolling on the wall without slipping would be %g); "
      "mean torque about y at the last step %.5f" % ((Xp[:, 0] - X0[:, 0]).mean() / T, args.omega, radius, args.omega * radius, torque_y.mean()))
