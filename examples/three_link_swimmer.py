"""Purcell's three-link swimmer near the wall: three shells in a row, the outer two on driven hinges of the middle one.

Each hinge is a ball joint in the gap between two shells and a lock joint whose rate is a motor (RigidBody.motor /
set_joint_kinds / set_joint_rates, include/rbl.h section 9): the joint forces and torques are unknowns of the saddle solve, so the
links hold together and turn at exactly the prescribed rate whatever the hydrodynamic load, and the swimmer as a whole stays
force- and torque-free -- J^T phi is an internal load.  The hinge axes are the wall's normal; the arms move in Purcell's
four-stroke order (arm 1 up, arm 2 up, arm 1 down, arm 2 down), which is not time-reversible, so every cycle leaves a net
displacement.  No external force acts: the wall enters through the mobility alone.

The example prints the displacement of the middle link per cycle, along and across the swimmer's initial axis, beside the largest
translational gap |p_A - p_B| and angular gap |e| over the run -- the O(dt^2) the explicit rotation update leaves in a step, taken
out by the next (gamma = 1).  Reports; asserts nothing.

    python examples/three_link_swimmer.py [--cycles 2] [--steps-per-stroke 25] [--amplitude 0.6] [--dt 0.02] [--height 3.0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import RigidBody, load_structure
from rigid_body_light_amd._lib import JOINT_BALL, joint_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--steps-per-stroke", type=int, default=25)
    ap.add_argument("--amplitude", type=float, default=0.6, help="the angle an arm sweeps in one stroke, radians")
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--height", type=float, default=3.0)
    args = ap.parse_args()
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    pitch = 2.0 * Rb + 4.0 * a                                  # room for the arms to turn without touching
    X = np.array([[(i - 1) * pitch, 0.0, args.height] for i in range(3)])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    rb = RigidBody(cfg, X, Q, a, 1.0, args.dt, wall_PC=True, block_PC=True)
    z = [0.0, 0.0, 1.0]
    rows = joint_rows(rb.motor(1, 0, 0.5 * (X[0] + X[1]), z), rb.motor(1, 2, 0.5 * (X[1] + X[2]), z))
    rb.set_joint_kinds(**rows)
    lock = rows["kind"] != JOINT_BALL                           # joints 1 and 3: the two motors
    omega = args.amplitude / (args.steps_per_stroke * args.dt)
    strokes = [(+1, 0), (0, +1), (-1, 0), (0, -1)]
    print("three shell_N_12 links, pitch %.2f, %.2f above the wall; arms sweep %.2f rad in %d steps of dt = %g (rate %.3f)"
          % (pitch, args.height, args.amplitude, args.steps_per_stroke, args.dt, omega))
    F = np.zeros(18)
    gap_max, ang_max, its_sum, steps = 0.0, 0.0, 0, 0
    t0 = time.time()
    start = rb.get_config()[0][1].copy()
    for cycle in range(args.cycles):
        for s1, s2 in strokes:
            rates = np.zeros(4)
            rates[np.flatnonzero(lock)] = [s1 * omega, -s2 * omega]     # the arms are mirror images: opposite signs lift both
            rb.set_joint_rates(rates)
            for _ in range(args.steps_per_stroke):
                _, its, _ = rb.step_jointed(F, gamma=1.0, max_iter=100, rtol=1e-8)
                gap, _, theta = rb.joint_state()
                gap_max = max(gap_max, np.linalg.norm(gap[~lock], axis=1).max())
                ang_max = max(ang_max, np.linalg.norm(gap[lock], axis=1).max())
                its_sum, steps = its_sum + its, steps + 1
        here = rb.get_config()[0][1]
        print("cycle %d: middle link moved %+.5f along and %+.5f across the axis, %+.5f in height; motor angles %+.3e %+.3e"
              % (cycle + 1, here[0] - start[0], here[1] - start[1], here[2] - start[2], theta[1], theta[3]))
        start = here.copy()
    elapsed = time.time() - t0
    print("%.1f s, %.1f ms per step, %.1f GMRES iterations per step" % (elapsed, 1e3 * elapsed / steps, its_sum / steps))
    print("largest gap over the run: %.3e, largest angular gap: %.3e rad (link radius %.3f)" % (gap_max, ang_max, Rb + a))


if __name__ == "__main__":
    main()
