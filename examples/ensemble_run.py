"""Gibbs-Boltzmann height distribution of one shell_N_12 above a wall: examples/ensemble_gibbs.py done with ONE call.

The same system (weight w = 0.5 per blob, wall repulsion eps_wall = 4, b_wall = 0.1, kT = 1, dt = 0.02) and the same seeds, but the
R replicas x `steps` stochastic midpoint steps are one Ensemble.run(steps, stride=1, on_error="reject"): the inputs go to the
device once, every step's verdict and commit are taken per replica on the device, and the trajectory comes back as frames in one
read-back.  A replica whose move would put a blob below the wall keeps its configuration and draws again at the next step (the
customary treatment, not an unbiased one), so the rejected share is printed beside the mean and the variance of the centre height:
it says how much that treatment can matter.  Reports; asserts nothing.

    python examples/ensemble_run.py [--replicas 512] [--steps 400] [--burn 150]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure
from ensemble_gibbs import reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=512)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    w, eps_w, b_w, kT, dt = 0.5, 4.0, 0.1, 1.0, 0.02
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    R = args.replicas
    X = np.tile([0.1, -0.2, Rb + a + 0.2], (R, 1, 1))
    Q = np.random.default_rng(args.seed).standard_normal((R, 1, 4))
    ens = Ensemble(cfg, X, Q, a=a, eta=1.0, dt=dt, kBT=kT, wall=True)
    ens.set_interactions(w=w, eps_wall=eps_w, b_wall=b_w, eps_blob=0.0, b_blob=0.05)
    t0 = time.time()
    out = ens.run(args.steps, F=np.zeros(6), seed=args.seed, stride=1, on_error="reject", max_iter=50, rtol=1e-10)
    elapsed = time.time() - t0
    ens.close()
    h = out.X[:, :, 0, 2]                                       # (steps, R): a rejected step repeats the replica's height
    hs = h[args.burn:]
    per_rep = hs.mean(axis=0)                                   # one sample per replica
    m, se_m = per_rep.mean(), per_rep.std(ddof=1) / np.sqrt(R)
    per_rep_v = ((hs - m) ** 2).mean(axis=0)
    v, se_v = per_rep_v.mean(), per_rep_v.std(ddof=1) / np.sqrt(R)
    mref, vref = reference(cfg, a, w, eps_w, b_w, kT)
    share = out.rejected.sum() / float(R * args.steps)
    print("%d replicas x %d steps (burn-in %d) in one run: %.1f s, %.0f replica-steps/s" % (R, args.steps, args.burn, elapsed,
                                                                                            R * args.steps / elapsed))
    print("rejected %d of %d replica-steps (share %.2e; most in one replica: %d)" % (out.rejected.sum(), R * args.steps, share,
                                                                                     out.rejected.max()))
    print("h mean %.5f +- %.5f  (reference %.5f, %+.1f standard errors)" % (m, se_m, mref, (m - mref) / se_m))
    print("h var  %.6f +- %.6f  (reference %.6f, %+.1f standard errors)" % (v, se_v, vref, (v - vref) / se_v))


if __name__ == "__main__":
    main()
