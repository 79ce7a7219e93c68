"""The stroke-averaged flow around Purcell's three-link swimmer, from ONE run_jointed per cycle count.

The swimmer of examples/ensemble_swimmers_run.py -- three shells in a row, the outer two on driven hinges of the middle one, the
four strokes as a motor schedule evaluated on the device; replica r is the same swimmer at its own height above the wall -- with
a plane of probe points FIXED IN THE MIDDLE LINK (probe_body=1): a square grid in the plane of the stroke, through the link's
centre, that translates and turns with it.  Every step evaluates the fluid velocity at the grid from that step's blob forces while
they lie in the solver's workspace (Ensemble.run_jointed(probes=..., probe_body=...)); the run returns the sum over the steps,
so u_mean is the flow averaged over whole strokes in the swimmer's frame of reference (lab-frame components: the link barely turns
over a cycle).  Nothing is solved twice and no lambda leaves the device.

Prints the mean flow's magnitude against the distance from the link for the highest replica, and the exponent n of the far-field
decay |u| ~ r^-n fitted over the outer half of the grid (a force-free swimmer's flow decays at least like r^-2; near the wall
faster).  Reports; asserts nothing.  The last line is a JSON summary.

    python examples/ensemble_swimmer_flow.py [--cycles 1] [--steps-per-stroke 25] [--grid 17] [--extent 12] [--replicas 4]
"""
import argparse
import json
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
    ap.add_argument("--replicas", type=int, default=4, help="swimmers, at heights 6, 8, ... above the wall")
    ap.add_argument("--grid", type=int, default=17, help="probe points per side of the square grid")
    ap.add_argument("--extent", type=float, default=12.0, help="half the side of the grid, in link radii")
    args = ap.parse_args()
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    pitch = 2.0 * Rb + 4.0 * a
    R = args.replicas
    heights = 6.0 + 2.0 * np.arange(R)
    X = np.array([[[(i - 1) * pitch, 0.0, h] for i in range(3)] for h in heights])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (R, 3, 1))
    ens = Ensemble(cfg, X, Q, a, 1.0, args.dt, kBT=0.0, wall=True)
    z = [0.0, 0.0, 1.0]
    rows = joint_rows(ens.motor(1, 0, 0.5 * (X[0, 0] + X[0, 1]), z), ens.motor(1, 2, 0.5 * (X[0, 1] + X[0, 2]), z))
    ens.set_joint_kinds(**rows)
    lock = rows["kind"] != JOINT_BALL
    n = args.steps_per_stroke
    omega = args.amplitude / (n * args.dt)
    rates = np.zeros((4, 4))
    for k, (s1, s2) in enumerate([(+1, 0), (0, +1), (-1, 0), (0, -1)]):
        rates[k, np.flatnonzero(lock)] = [s1 * omega, -s2 * omega]
    # the probes: offsets in the middle link's frame, a grid in its x-y plane (the plane of the stroke: the hinges' axes are z)
    g = np.linspace(-args.extent * Rb, args.extent * Rb, args.grid)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    probes = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    steps = 4 * n * args.cycles
    t0 = time.time()
    res = ens.run_jointed(steps, np.zeros(18), gamma=1.0, schedule=([n] * 4, rates), probes=probes, probe_body=1, max_iter=100, rtol=1e-8)
    elapsed = time.time() - t0
    ens.close()
    u = res.u_mean                                              # (R, P, 3): the mean over the accepted steps, whole cycles
    dist = np.linalg.norm(probes, axis=1)
    speed = np.linalg.norm(u, axis=2)
    top = R - 1                                                 # the swimmer farthest from the wall
    print("%d swimmers, %d steps (%d cycles) with %d probes fixed in the middle link: %.2f s, %.2f ms per step"
          % (R, steps, args.cycles, probes.shape[0], elapsed, 1e3 * elapsed / steps))
    edges = np.linspace(2.0 * Rb, dist.max(), 7)
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (dist >= lo) & (dist < hi)
        if sel.any():
            print("height %4.1f  r in [%5.2f, %5.2f): mean |<u>| = %.3e over %d probes" % (heights[top], lo, hi, speed[top, sel].mean(), sel.sum()))
    far = (dist >= 0.5 * dist.max()) & (speed[top] > 0.0)
    slope = np.polyfit(np.log(dist[far]), np.log(speed[top, far]), 1)[0] if far.sum() >= 2 else float("nan")
    print("far-field decay of the stroke-averaged flow at height %.1f: |<u>| ~ r^%.2f" % (heights[top], slope))
    print(json.dumps({"example": "ensemble_swimmer_flow", "replicas": R, "steps": steps, "probes": int(probes.shape[0]),
                      "accepted": res.accepted.tolist(), "ms_per_step": 1e3 * elapsed / steps, "decay_exponent": float(-slope),
                      "max_mean_speed": float(speed.max())}))


if __name__ == "__main__":
    main()
