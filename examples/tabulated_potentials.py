"""Three shell_N_12 colloids per replica with a Lennard-Jones-like attraction between their blobs, held together by optical traps of
finite stiffness: an ensemble run with a tabulated pair potential and harmonic traps evaluated on the GPU inside every step.

The pair law U(r) = 4 eps ((sigma / r)^12 - (sigma / r)^6), shifted so that U(r_cut) = 0, is tabulated with its derivative on a
uniform grid (`tabulate`); below r_min the library continues it along its tangent, so overlapping blobs feel a finite push.  Each
body sits in a trap whose centre is its starting position, slightly softer along z.  R replicas x `steps` stochastic midpoint
steps are ONE Ensemble.run: neither the table nor the traps cost a host round trip.  The example prints the mean pair energy per
replica, the mean squared excursion from the trap centres beside the free-trap value kT / k, and the throughput.  Reports;
asserts nothing.

    python examples/tabulated_potentials.py [--replicas 128] [--steps 400] [--burn 100]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure, tabulate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=128)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    kT, dt, eps, k = 1.0, 0.01, 0.15, np.array([20.0, 20.0, 10.0])
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    sigma, r_min, r_cut = 2.0 * a, 1.7 * a, 5.0 * a

    def lj(r):
        s6 = (sigma / r) ** 6
        return 4 * eps * (s6 * s6 - s6)

    U, dU = tabulate(lambda r: lj(r) - lj(r_cut), lambda r: -24 * eps * (2 * (sigma / r) ** 12 - (sigma / r) ** 6) / r, r_min, r_cut, 1025)
    R = args.replicas
    d = 2.0 * Rb + 2.0 * a                                        # surfaces one blob diameter apart: inside the attractive well
    centres = np.array([[0.0, 0.0, 0.0], [d, 0.0, 0.0], [0.5 * d, 0.87 * d, 0.0]]) + [0.0, 0.0, Rb + 4.0 * a]
    X = np.tile(centres, (R, 1, 1))
    Q = np.random.default_rng(args.seed).standard_normal((R, 3, 4))
    ens = Ensemble(cfg, X, Q, a=a, eta=1.0, dt=dt, kBT=kT, wall=True)
    ens.set_pair_table(U, dU, r_min, r_cut)
    ens.set_traps(np.tile(k, (3, 1)), centres)
    E0 = ens.interaction_energy()
    t0 = time.time()
    out = ens.run(args.steps, F=np.zeros(18), seed=args.seed, stride=1, on_error="reject", max_iter=50, rtol=1e-8)
    elapsed = time.time() - t0
    E1 = ens.interaction_energy()
    Xe = ens.get_config()[0]
    ens.close()
    burn = min(args.burn, args.steps // 2)
    dev2 = ((out.X[burn:] - centres) ** 2).mean(axis=(0, 1, 2))   # per axis, over frames, replicas and bodies
    trap_E = 0.5 * (k * (Xe - centres) ** 2).sum(axis=(1, 2))
    print("%d replicas x %d steps in one run: %.1f s, %.0f replica-steps/s; rejected %d" % (
        R, args.steps, elapsed, R * args.steps / elapsed, out.rejected.sum()))
    print("pair energy per replica: %.4f at the start, %.4f +- %.4f at the end (trap energy %.4f)" % (
        (E0 - 0.0).mean(), (E1 - trap_E).mean(), (E1 - trap_E).std(ddof=1) / np.sqrt(R), trap_E.mean()))
    print("trap: <(X - X0)^2> per axis %s, kT / k %s (the attraction pulls the bodies off their centres)" % (
        np.array2string(dev2, precision=4), np.array2string(kT / k, precision=4)))


if __name__ == "__main__":
    main()
