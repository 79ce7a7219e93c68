#!/usr/bin/env python3
"""Sedimentation of 9 shells of 42 blobs onto a wall under the library's force model (include/rbl.h section 4): buoyant
weight, a screened wall repulsion and a steric repulsion between blobs of different bodies, evaluated on the GPU at the start
of every stochastic midpoint step (RigidBody.set_interactions; the drop-in class fixes kBT = 1).  The shells start 3 units
above their resting height, fall, and settle into a layer above the wall.  Prints the mean height per step and the GPU time
spent in the force model (RBL_T_FORCES)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, make_config
from rigid_body_light_amd._lib import DeviceContext, lib

nb, nblb, steps = 9, 42, 300
c = make_config(nb, nblb, wall=True)           # one 3 x 3 layer of bodies above the wall
X = c["X"].copy()
X[:, 2] += 3.0
rb = RigidBody(c["cfg"], X, c["Q"], c["a"], c["eta"], dt=0.05, wall_PC=True)
rb.set_interactions(w=0.5, eps_wall=5.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)   # r_cut = 2a + 20 b_blob
h = ctypes.c_void_p(rb.cb.handle())
L = lib()
L.rbl_set_timing(h, 1)
F = np.zeros(6 * nb)                            # no external force beyond the model
for n in range(steps):
    iters, resid = rb.step_brownian(F, seed=n, max_iter=60, rtol=1e-8)
    Xn, _ = rb.get_config()
    print("step %3d: mean height %.4f  (%d GMRES iterations)" % (n, Xn.reshape(-1, 3)[:, 2].mean(), iters))
ms, calls = (ctypes.c_double * len(DeviceContext.TIMING_PHASES))(), (ctypes.c_int64 * len(DeviceContext.TIMING_PHASES))()
L.rbl_get_timings(h, ms, calls)
k = DeviceContext.TIMING_PHASES.index("forces")
print("forces: %.3f ms in %d evaluations (%.1f us each)" % (ms[k], calls[k], 1e3 * ms[k] / max(calls[k], 1)))
