"""Purcell's three-link swimmer at R heights above the wall, all of them stepped in one call (Ensemble.step_jointed).

The swimmer of examples/three_link_swimmer.py -- three shells in a row, the outer two on driven hinges of the middle one, each
hinge a ball joint and a lock joint whose rate is a motor -- as an ensemble: replica r is the same swimmer at its own height, the
joint set is shared, and every step of the four-stroke cycle (arm 1 up, arm 2 up, arm 1 down, arm 2 down) is one launch of the
jointed one-kernel solver for all heights.  The stroke is switched with set_joint_rates between the segments.  No external force
acts: the wall enters through the mobility alone, so the displacement per cycle depends on the height and tends to the free
swimmer's far from the wall.

Prints the displacement of the middle link per cycle against the height, and the largest translational gap over the run per
replica (the O(dt^2) the explicit rotation update leaves in a step, taken out by the next: gamma = 1).  Reports; asserts nothing.

    python examples/ensemble_swimmers.py [--cycles 1] [--steps-per-stroke 25] [--amplitude 0.6] [--dt 0.02] [--heights 2 2.5 3 4 6 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure
from rigid_body_light_amd._lib import JOINT_BALL, joint_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=1)
    ap.add_argument("--steps-per-stroke", type=int, default=25)
    ap.add_argument("--amplitude", type=float, default=0.6, help="the angle an arm sweeps in one stroke, radians")
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--heights", type=float, nargs="+", default=[2.0, 2.5, 3.0, 4.0, 6.0, 10.0])
    args = ap.parse_args()
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    pitch = 2.0 * Rb + 4.0 * a                                  # room for the arms to turn without touching
    heights = np.asarray(args.heights, dtype=np.float64)
    R = heights.size
    X = np.array([[[(i - 1) * pitch, 0.0, h] for i in range(3)] for h in heights])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (R, 3, 1))
    ens = Ensemble(cfg, X, Q, a, 1.0, args.dt, kBT=0.0, wall=True)
    z = [0.0, 0.0, 1.0]
    # the anchors, axes and q_rel are body-frame quantities: those of replica 0 serve every height
    rows = joint_rows(ens.motor(1, 0, 0.5 * (X[0, 0] + X[0, 1]), z), ens.motor(1, 2, 0.5 * (X[0, 1] + X[0, 2]), z))
    ens.set_joint_kinds(**rows)
    lock = rows["kind"] != JOINT_BALL                           # joints 1 and 3: the two motors
    omega = args.amplitude / (args.steps_per_stroke * args.dt)
    strokes = [(+1, 0), (0, +1), (-1, 0), (0, -1)]
    print("%d swimmers of three shell_N_12 links, pitch %.2f; arms sweep %.2f rad in %d steps of dt = %g (rate %.3f)"
          % (R, pitch, args.amplitude, args.steps_per_stroke, args.dt, omega))
    F = np.zeros(18)
    gap_max, its_sum, steps = np.zeros(R), 0, 0
    t0 = time.time()
    start = ens.get_config()[0][:, 1].copy()
    for cycle in range(args.cycles):
        for s1, s2 in strokes:
            rates = np.zeros(4)
            rates[np.flatnonzero(lock)] = [s1 * omega, -s2 * omega]     # the arms are mirror images: opposite signs lift both
            ens.set_joint_rates(rates)
            for _ in range(args.steps_per_stroke):
                _, its, _ = ens.step_jointed(F, gamma=1.0, max_iter=100, rtol=1e-8)
                gap = ens.joint_state()[0]
                gap_max = np.maximum(gap_max, np.linalg.norm(gap[:, ~lock], axis=2).max(axis=1))
                its_sum, steps = its_sum + its.mean(), steps + 1
        here = ens.get_config()[0][:, 1]
        for r in range(R):
            print("cycle %d height %5.2f: displacement %+.5f along and %+.5f across the axis, %+.5f in height"
                  % (cycle + 1, heights[r], here[r, 0] - start[r, 0], here[r, 1] - start[r, 1], here[r, 2] - start[r, 2]))
        start = here.copy()
    elapsed = time.time() - t0
    print("%.1f s, %.2f ms per step of all %d swimmers, %.1f GMRES iterations per step and swimmer" % (elapsed, 1e3 * elapsed / steps, R, its_sum / steps))
    for r in range(R):
        print("height %5.2f: largest gap over the run %.3e" % (heights[r], gap_max[r]))


if __name__ == "__main__":
    main()
