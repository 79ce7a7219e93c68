"""A layer of shells in a periodic cell, equilibrated by Metropolis sampling from a lattice (Ensemble.metropolis), then a Brownian run
from that configuration and one from the lattice: the height distribution of the body centres of all three, side by side.  The
Metropolis chain samples exp(-E / kBT) of the force model directly; a Brownian run started on the lattice spends its first steps
getting there.  It reports and asserts nothing.

    python examples/ensemble_equilibrate.py [--replicas 64] [--sweeps 400] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--sweeps", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max())
    R, nb, side = args.replicas, 9, 3
    spacing = 2.0 * (Rb + a) + 1.0
    L = max(side * spacing, 2.0 * (2.0 * Rb + 3.0 * a) + 0.1)
    i = np.arange(nb)
    X = np.stack([i % side, i // side, np.zeros(nb)], axis=1) * (L / side) + [0.0, 0.0, Rb + 3.0 * a]
    X = np.tile(X, (R, 1, 1))
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (R, nb, 1))

    def make():
        e = Ensemble(cfg, X, Q, a=a, eta=1.0, dt=0.01, kBT=1.0, wall=True)
        e.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1, eps_blob=4.0, b_blob=0.1, r_cut=3.0 * a)
        e.set_cell(L, L)
        return e

    bins = np.linspace(0.0, 6.0, 13)
    ens = make()
    sx, st = ens.metropolis_tune(target=0.4, n_sweeps=20, rounds=8, step_x=0.2, step_theta=0.2)      # tune first ...
    res = ens.metropolis(args.sweeps, sx, st, seed=1, sweep_start=160, stride=4)                     # ... then sample, steps fixed
    h_mc = np.histogram(res.X[len(res.X) // 2:, :, :, 2], bins=bins, density=True)[0]
    run_eq = ens.run(args.steps, F=np.zeros(6 * nb), seed=3, stride=4)
    h_eq = np.histogram(run_eq.X[:, :, :, 2], bins=bins, density=True)[0]
    ens.close()
    lat = make()
    run_lat = lat.run(args.steps, F=np.zeros(6 * nb), seed=3, stride=4)
    h_lat = np.histogram(run_lat.X[:, :, :, 2], bins=bins, density=True)[0]
    lat.close()
    print("steps %.3f %.3f, acceptance %.2f" % (sx, st, res.acceptance.mean()))
    print("  height   Metropolis   Brownian from MC   Brownian from lattice")
    for k in range(len(bins) - 1):
        print("  %5.2f    %8.4f     %8.4f           %8.4f" % (0.5 * (bins[k] + bins[k + 1]), h_mc[k], h_eq[k], h_lat[k]))


if __name__ == "__main__":
    main()
