#!/usr/bin/env python3
"""A suspension in a flow (include/rbl.h section 8): background flow, stresslets, and the same inside an ensemble.

(a) One shell of 162 blobs, force- and torque-free, in a free-space straining flow u = E r: it moves with the fluid and its
    stresslet is S = c E.  Prints c next to the sphere's (20/3) pi eta r_h^3, r_h the shell's hydrodynamic radius.
(b) Shells of 42 blobs in the shear u = (gamma z, 0, 0) over the wall, sedimented by the force model (weight, wall and steric
    repulsion).  Every step is one `step_deterministic`: the flow enters the right-hand side on the device, the first moments of
    the step's blob forces are recorded.  Prints the drift velocity against the height and the mean stresslet S_xz.
(c) The same suspension of 12-blob shells as an `Ensemble` of replicas with Brownian motion: one launch adds the flow to every
    replica, one launch records the moments of all of them.

python examples/shear_flow.py [--steps 40] [--bodies 16] [--replicas 64] [--quick]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import Ensemble, RigidBody, load_structure, make_config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--bodies", type=int, default=16)
ap.add_argument("--replicas", type=int, default=64)
ap.add_argument("--shear", type=float, default=1.0)
ap.add_argument("--quick", action="store_true", help="a few seconds: 12-blob shell, 4 bodies, 3 steps, 4 replicas")
args = ap.parse_args()
if args.quick:
    args.steps, args.bodies, args.replicas = 3, 4, 4

# ---- (a) one shell in strain ------------------------------------------------------------------------------------------------------
nblb = 12 if args.quick else 162
params, cfg = load_structure(nblb)
a, eta = params["sep"] / 2.0, 1.0
E = np.array([[1.0, 0.3, 0.0], [0.3, -0.4, 0.2], [0.0, 0.2, -0.6]])         # symmetric, traceless
X = np.array([[0.5, -1.0, 2.0]])
rb = RigidBody(cfg, X, np.array([[0.8, 0.2, -0.4, 0.4]]), a, eta, dt=0.01, block_PC=True)
rb.set_background_flow(G=E)
lam, U, F, its, res = rb.solve_mixed([], np.zeros(6), slip=rb.flow_slip(), rtol=1e-10)     # the bare solve takes the term as slip
S = rb.stresslets(lam)[0]
m = np.abs(E) > 0.1
c = (S[m] / E[m]).mean()
print("(a) shell_N_%d in strain: U - E X = %s, Omega = %s (%d iterations)" % (nblb, U[:3] - E @ X[0], U[3:], its))
print("    S / E = %.6f for every component (spread %.1e); (20/3) pi eta r_h^3 = %.6f; ratio %.4f"
      % (c, np.ptp(S[m] / E[m]) / abs(c), 20.0 / 3.0 * np.pi * eta * params["Rh"] ** 3, abs(c) / (20.0 / 3.0 * np.pi * eta * params["Rh"] ** 3)))

# ---- (b) shells in shear over the wall ---------------------------------------------------------------------------------------------
nb, nblb = args.bodies, 12 if args.quick else 42
cw = make_config(nb, nblb, wall=True)
G = np.zeros((3, 3))
G[0, 2] = args.shear
model = dict(w=0.3, eps_wall=4.0, b_wall=0.1, eps_blob=1.0, b_blob=0.05)
rb = RigidBody(cw["cfg"], cw["X"], cw["Q"], cw["a"], cw["eta"], dt=0.02, wall_PC=True, block_PC=True)
rb.set_interactions(**model)
rb.set_background_flow(G=G)
rb.record_moments()
Sxz = []
for n in range(args.steps):
    X0 = rb.get_config()[0].copy()
    its, res = rb.step_deterministic(np.zeros(6 * nb), max_iter=100, rtol=1e-8)
    Sxz.append(0.5 * (rb.step_moments()[:, 0, 2] + rb.step_moments()[:, 2, 0]).mean())
X1 = rb.get_config()[0]
Ux = (X1[:, 0] - X0[:, 0]) / 0.02
print("(b) %d x shell_N_%d in shear %.2f over the wall, %d steps (last: %d iterations)" % (nb, nblb, args.shear, args.steps, its))
print("    height   drift U_x   U_x / (shear z)")
for k in np.argsort(X1[:, 2])[:: max(1, nb // 8)]:
    print("    %6.3f   %9.5f   %7.4f" % (X1[k, 2], Ux[k], Ux[k] / (args.shear * X1[k, 2])))
print("    mean stresslet S_xz per body: first step %.5f, last step %.5f" % (Sxz[0], Sxz[-1]))

# ---- (c) the same as an ensemble ----------------------------------------------------------------------------------------------------
R, nb = args.replicas, min(args.bodies, 10)
ce = make_config(nb, 12, wall=True)
ens = Ensemble(ce["cfg"], np.repeat(ce["X"][None], R, axis=0), np.repeat(ce["Q"][None], R, axis=0), ce["a"], ce["eta"], dt=0.005,
               kBT=0.05, wall=True)
ens.set_interactions(**model)
ens.set_background_flow(G=G)
ens.record_moments()
for n in range(args.steps):
    X0 = ens.get_config()[0]
    its, res = ens.step_brownian(np.zeros(6 * nb), seed=n, max_iter=100, rtol=1e-8)
D = ens.step_moments()
X1 = ens.get_config()[0]
Sxz = 0.5 * (D[..., 0, 2] + D[..., 2, 0])
print("(c) ensemble of %d replicas x %d shell_N_12, Brownian, %d steps: mean height %.3f, mean drift U_x %.4f, S_xz %.5f +- %.5f (over replicas)"
      % (R, nb, args.steps, X1[..., 2].mean(), ((X1 - X0)[..., 0] / 0.005).mean(), Sxz.mean(), Sxz.mean(axis=1).std() / np.sqrt(R)))
ens.close()
