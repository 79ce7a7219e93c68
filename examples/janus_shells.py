"""Pairs of Janus shells above the wall: an orientation-dependent attraction from blob types alone.

Every shell_N_42 carries two blob types (`patch_types`): type 1 on the hemisphere about its body-frame z axis, type 0 elsewhere.  The
only attraction in the system is the type table T_11, a smooth well between type-1 blobs of different bodies; T_00 and T_01 are not
set, so bare faces only repel through the built-in steric term.  Whether two shells stick therefore depends on how they are turned
towards each other -- with no angular term anywhere: the pair kernel sees blob positions and types.  Each replica holds one pair,
started cap to cap; gravity and the wall repulsion keep the shells near the wall.  R replicas x `steps` stochastic midpoint steps
are ONE Ensemble.run.  The example prints the fraction of (replica, frame) samples in which the pair is bound (at least one type-1
blob pair could be inside the well: centres closer than 2 R_body + r_cut), beside the same run with the types switched off, and the
throughput.  Reports; asserts nothing.

    python examples/janus_shells.py [--replicas 64] [--steps 2000] [--depth 15]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure, patch_types, tabulate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--depth", type=float, default=15.0, help="depth of the well between two type-1 blobs, in kT")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    kT, dt = 1.0, 4e-3
    p, cfg = load_structure(42)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    r_cut = 4.0 * a
    # U = -depth (1 - r / r_cut)^2: zero with zero slope at the cutoff, so nothing jumps there
    U, dU = tabulate(lambda r: -args.depth * (1.0 - r / r_cut) ** 2, lambda r: 2.0 * args.depth * (1.0 - r / r_cut) / r_cut, 0.0, r_cut, 257)
    R = args.replicas
    s = np.sqrt(0.5)
    Q1 = np.array([[s, 0.0, s, 0.0], [s, 0.0, -s, 0.0]])           # body z^ -> +x^ and -x^: the caps face each other
    X1 = np.array([[0.0, 0.0, Rb + 3.0 * a], [2.0 * Rb + 2.2 * a, 0.0, Rb + 3.0 * a]])
    X, Q = np.tile(X1, (R, 1, 1)), np.tile(Q1, (R, 1, 1))
    bound_at = 2.0 * Rb + r_cut
    result = {}
    for label, typed in (("Janus caps", True), ("types off", False)):
        ens = Ensemble(cfg, X, Q, a=a, eta=1.0, dt=dt, kBT=kT, wall=True)
        ens.set_interactions(w=0.05, eps_wall=4.0, b_wall=0.5 * a, eps_blob=4.0, b_blob=0.25 * a, r_cut=2.0 * a + 2.0 * a)
        ens.set_blob_types(patch_types(cfg, [0.0, 0.0, 1.0]), n_types=2, on=typed)
        ens.set_type_table(1, 1, U, dU, 0.0, r_cut)
        active = ens.ctx.interactions_active()
        t0 = time.time()
        out = ens.run(args.steps, F=np.zeros(12), seed=args.seed, stride=max(1, args.steps // 50), on_error="reject", max_iter=50, rtol=1e-8)
        elapsed = time.time() - t0
        ens.close()
        dist = np.linalg.norm(out.X[:, :, 0] - out.X[:, :, 1], axis=2)         # (frames, R)
        late = dist[dist.shape[0] // 2:]
        result[label] = (late <= bound_at).mean()
        print("%-10s (interactions_active %3d): %d replicas x %d steps in one run, %.1f s, %.0f replica-steps/s, rejected %d; "
              "bound fraction over the second half %.3f, mean centre distance %.3f (contact %.3f, bound below %.3f)" % (
                  label, active, R, args.steps, elapsed, R * args.steps / elapsed, out.rejected.sum(), result[label], late.mean(),
                  2.0 * Rb + 2.0 * a, bound_at))
    print("bound fraction: %.3f with the caps, %.3f without" % (result["Janus caps"], result["types off"]))


if __name__ == "__main__":
    main()
