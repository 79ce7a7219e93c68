"""Gibbs-Boltzmann height distribution of one shell_N_12 above a wall, sampled by an ENSEMBLE of independent replicas.

The system of tests/test_interactions_gpu.py's Gibbs-Boltzmann check (weight w = 0.5 per blob, wall repulsion eps_wall = 4,
b_wall = 0.1, kT = 1, dt = 0.02), run as R replicas x `steps` stochastic midpoint steps in one process: every step advances all
replicas with a fixed number of launches (rigid_body_light_amd.Ensemble).  Prints the mean and the variance of the centre height
with standard errors (each replica's time average after the burn-in is one sample) next to the numpy reference
p(h) ~ int dOmega exp(-U(h, Omega) / kT).  Reports; asserts nothing.

    python examples/ensemble_gibbs.py [--replicas 512] [--steps 400] [--burn 150]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure


def wall_energy(h, a, eps_w, b_w):
    return np.where(h >= a, eps_w * np.exp(-(h - a) / b_w), eps_w + eps_w / b_w * (a - h))


def reference(cfg, a, w, eps_w, b_w, kT):
    cfg = cfg - cfg.mean(axis=0)
    q = np.random.default_rng(7).standard_normal((4000, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w0, x, y, z = q.T
    Rz = np.stack([2 * (x * z - w0 * y), 2 * (y * z + w0 * x), 1 - 2 * (x * x + y * y)], axis=1)   # third row of R(q)
    lz = Rz @ cfg.T
    H = np.linspace(0.0, 4.0, 4001)
    lw = np.empty(H.size)
    for i, Z in enumerate(H):
        hb = Z + lz
        U = np.sum(w * hb + wall_energy(hb, a, eps_w, b_w), axis=1) / kT
        lw[i] = -U.min() + np.log(np.mean(np.exp(-(U - U.min()))))
    p = np.exp(lw - lw.max())
    p /= p.sum()
    m = float(np.sum(p * H))
    return m, float(np.sum(p * (H - m) ** 2))


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
    h = np.empty((args.steps, R))
    t0 = time.time()
    for n in range(args.steps):
        ens.step_brownian(np.zeros(6), seed=args.seed + n, max_iter=50, rtol=1e-10)
        h[n] = ens.get_config()[0][:, 0, 2]
    elapsed = time.time() - t0
    ens.close()
    hs = h[args.burn:]
    per_rep = hs.mean(axis=0)                                   # one sample per replica
    m, se_m = per_rep.mean(), per_rep.std(ddof=1) / np.sqrt(R)
    per_rep_v = ((hs - m) ** 2).mean(axis=0)
    v, se_v = per_rep_v.mean(), per_rep_v.std(ddof=1) / np.sqrt(R)
    mref, vref = reference(cfg, a, w, eps_w, b_w, kT)
    print("%d replicas x %d steps (burn-in %d): %.1f s, %.0f replica-steps/s" % (R, args.steps, args.burn, elapsed,
                                                                                  R * args.steps / elapsed))
    print("h mean %.5f +- %.5f  (reference %.5f, %+.1f standard errors)" % (m, se_m, mref, (m - mref) / se_m))
    print("h var  %.6f +- %.6f  (reference %.6f, %+.1f standard errors)" % (v, se_v, vref, (v - vref) / se_v))


if __name__ == "__main__":
    main()
