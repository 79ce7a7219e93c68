"""The chain of examples/tethered_chain.py with hard joints in place of the springs: magnetic beads linked surface to surface by
ball joints, the first bead on a pivot just above the wall, driven by a precessing field.

Every bead is a shell_N_12 with a permanent moment along its own z axis.  The point (0, 0, +R_b + gap / 2) fixed in bead i and the
point (0, 0, -R_b - gap / 2) fixed in bead i + 1 are ONE point: a ball joint in the middle of the gap between the two surfaces,
and the lowest bead's lower point sits on a lab point above the wall (a pivot).  The joints are constraints of the saddle solve
(RigidBody.set_joints / step_jointed, include/rbl.h section 9): their forces are unknowns of the linear system, so the chain
holds together to the solver's tolerance at a step set by the hydrodynamics, where the stiff springs of the tethered chain set
it.  Weight, wall repulsion and steric repulsion keep the beads apart and above the wall; the steps are deterministic.

The example prints the largest gap |p_A - p_B| over the run -- the O(dt^2) the explicit rotation update leaves in a step, which
the relaxation gamma = 1 takes out in the next -- beside the end-to-end distance of the chain and the largest joint force.
Reports; asserts nothing.

    python examples/jointed_chain.py [--steps 400] [--beads 6] [--dt 0.02] [--gamma 1.0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import RigidBody, load_structure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--beads", type=int, default=6)
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--gamma", type=float, default=1.0)
    args = ap.parse_args()
    kT, eta = 1.0, 1.0                                          # kT only sets the scale of the field and the repulsions
    p, cfg = load_structure(12)
    a, Rh = p["sep"] / 2.0, p["Rh"]
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    nb = args.beads
    gap = 2.0 * a                                               # surface to surface: the blobs of two beads just clear
    pitch = 2.0 * Rb + gap
    pivot = np.array([0.0, 0.0, a])                             # the point above the wall the chain hangs on
    X = np.array([[0.0, 0.0, pivot[2] + 0.5 * gap + Rb + i * pitch] for i in range(nb)])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    top, bottom = np.array([0.0, 0.0, Rb + 0.5 * gap]), np.array([0.0, 0.0, -Rb - 0.5 * gap])
    body = [[0, -1]] + [[i, i + 1] for i in range(nb - 1)]      # the pivot, then the chain
    anchor_a = [bottom] + [top] * (nb - 1)
    anchor_b = [pivot] + [bottom] * (nb - 1)
    B = 30.0 * kT
    mu_rr = 1.0 / (8 * np.pi * eta * Rh ** 3)
    omega = 0.25 * B * mu_rr
    tilt = np.deg2rad(30.0)
    rb = RigidBody(cfg, X, Q, a, eta, args.dt, wall_PC=True, block_PC=True)
    rb.set_interactions(w=0.05, eps_wall=10.0, b_wall=0.25 * a, eps_blob=10.0, b_blob=0.25 * a)
    rb.set_dipoles([0.0, 0.0, 1.0], c_dd=1.0, r_core=2.0 * Rb, r_cut=4.0 * pitch)
    rb.set_magnetic_field(B0=[0.0, 0.0, B * np.cos(tilt)], B1=[B * np.sin(tilt), 0.0, 0.0], B2=[0.0, B * np.sin(tilt), 0.0], omega=omega)
    rb.set_joints(body, np.array(anchor_a), np.array(anchor_b))
    print("%d beads on %d ball joints and a pivot, field tilted %.0f deg, omega = %.3f, dt = %.3g, gamma = %.2f"
          % (nb, nb - 1, np.rad2deg(tilt), omega, args.dt, args.gamma))
    F = np.zeros(6 * nb)
    worst, its_sum, phi_max = 0.0, 0, 0.0
    t0 = time.time()
    for step in range(args.steps):
        rb.set_field_time(step * args.dt)
        phi, its, res = rb.step_jointed(F, gamma=args.gamma, max_iter=100, rtol=1e-8)
        gaps = np.linalg.norm(rb.joint_state()[0], axis=1)
        worst, its_sum, phi_max = max(worst, gaps.max()), its_sum + its, max(phi_max, np.abs(phi).max())
    elapsed = time.time() - t0
    Xe = rb.get_config()[0]
    ee = np.linalg.norm(Xe[-1] - pivot)
    contour = 0.5 * gap + Rb + (nb - 1) * pitch
    lean = np.degrees(np.arccos(np.clip((Xe[-1, 2] - pivot[2]) / ee, -1.0, 1.0)))
    print("%.1f s, %.1f ms per step, %.1f GMRES iterations per step" % (elapsed, 1e3 * elapsed / args.steps, its_sum / args.steps))
    print("end-to-end distance: %.4f (contour length %.4f), leaning %.1f deg from the normal after %.2f turns of the field"
          % (ee, contour, lean, omega * args.dt * args.steps / (2 * np.pi)))
    print("largest gap over the run: %.3e (bead radius %.3f); largest joint force component %.2f" % (worst, Rb + a, phi_max))


if __name__ == "__main__":
    main()
