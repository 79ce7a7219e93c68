"""Purcell's three-link swimmer at R heights above the wall, whole stroke cycles in ONE call (Ensemble.run_jointed).

The swimmer of examples/ensemble_swimmers.py -- three shells in a row, the outer two on driven hinges of the middle one, each
hinge a ball joint and a lock joint whose rate is a motor; replica r is the same swimmer at its own height -- without the loop:
the four strokes (arm 1 up, arm 2 up, arm 1 down, arm 2 down) are the four phases of a motor schedule, which the run evaluates
on the device, so set_joint_rates at the stroke boundaries, step_jointed and joint_state every step become one run_jointed per
requested number of cycles.  A frame per step brings back the gaps; phi_mean of a motor's lock rows is its mean torque.

Prints the displacement of the middle link per cycle against the height, the largest translational gap over the run per replica
and each motor's mean torque about its axis.  Reports; asserts nothing.

    python examples/ensemble_swimmers_run.py [--cycles 1] [--steps-per-stroke 25] [--amplitude 0.6] [--dt 0.02] [--heights 2 2.5 3 4 6 10]
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
    # the four strokes as a schedule: one phase per stroke, the arms mirror images (opposite signs lift both)
    n = args.steps_per_stroke
    rates = np.zeros((4, 4))
    for k, (s1, s2) in enumerate([(+1, 0), (0, +1), (-1, 0), (0, -1)]):
        rates[k, np.flatnonzero(lock)] = [s1 * omega, -s2 * omega]
    print("%d swimmers of three shell_N_12 links, pitch %.2f; arms sweep %.2f rad in %d steps of dt = %g (rate %.3f)"
          % (R, pitch, args.amplitude, n, args.dt, omega))
    t0 = time.time()
    start = ens.get_config()[0][:, 1].copy()
    res = ens.run_jointed(4 * n * args.cycles, np.zeros(18), gamma=1.0, schedule=([n] * 4, rates), stride=1, max_iter=100, rtol=1e-8)
    elapsed = time.time() - t0
    steps = 4 * n * args.cycles
    for cycle in range(args.cycles):
        here = res.X[4 * n * (cycle + 1) - 1][:, 1]              # the frame after the cycle's last step
        for r in range(R):
            print("cycle %d height %5.2f: displacement %+.5f along and %+.5f across the axis, %+.5f in height"
                  % (cycle + 1, heights[r], here[r, 0] - start[r, 0], here[r, 1] - start[r, 1], here[r, 2] - start[r, 2]))
        start = here.copy()
    print("%.1f s, %.2f ms per step of all %d swimmers, %.1f GMRES iterations per step and swimmer"
          % (elapsed, 1e3 * elapsed / steps, R, res.iters_sum.sum() / (steps * R)))
    gap_max = np.linalg.norm(res.frame_gap[:, :, ~lock], axis=3).max(axis=(0, 2))
    axis = rows["axis"][lock]                                   # a lock's phi is a torque in body A's frame; about the hinge's axis:
    for r in range(R):
        torque = (res.phi_mean[r, lock] * axis).sum(axis=1)
        print("height %5.2f: largest gap over the run %.3e, mean motor torques about the axes %+.4f %+.4f, final angles %+.4f %+.4f"
              % (heights[r], gap_max[r], torque[0], torque[1], res.theta[r, 1], res.theta[r, 3]))


if __name__ == "__main__":
    main()
