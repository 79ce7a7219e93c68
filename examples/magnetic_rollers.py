"""Brownian microrollers driven the way they are in the laboratory: every shell_N_12 carries a permanent magnetic moment fixed in
its body, and a uniform field rotating about a lab axis parallel to the wall exerts the torque m x B(t) on it.

Two rollers per replica sediment against the wall (weight, wall repulsion, steric repulsion) and interact through their dipoles.
Below the critical frequency omega_c = |m| |B| mu_rr a roller turns with the field, lagging it by a constant angle, and rolls
along the wall; above it the roller steps out: it falls behind, slips back once per beat and rolls far more slowly.  The field
B(t) = B (cos(omega t) x^ - sin(omega t) z^) turns about +y^, so a synchronous roller moves along +x^.

Each frequency is ONE Ensemble.run of R replicas x `steps` stochastic midpoint steps: the force model evaluates the field at
every step's own time on the GPU (t = t0 + dt * accepted steps, per replica), so the rotating field costs no host round trip.
The example prints, for omega = 0.5 omega_c and 2 omega_c, the mean rolling velocity along x and the turns of the moments about
y beside the turns of the field.  omega_c uses the free-space estimate mu_rr = 1 / (8 pi eta R_h^3); near the wall the true
value is somewhat lower.  Reports; asserts nothing.

    python examples/magnetic_rollers.py [--replicas 64] [--steps 2000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure


def lab_moments(Q, m_body):
    """R(Q) m_body for quaternions of shape (..., 4), scalar first"""
    w, x, y, z = Q[..., 0], Q[..., 1], Q[..., 2], Q[..., 3]
    mx, my, mz = m_body
    return np.stack([(1 - 2 * (y * y + z * z)) * mx + 2 * (x * y - w * z) * my + 2 * (x * z + w * y) * mz,
                     2 * (x * y + w * z) * mx + (1 - 2 * (x * x + z * z)) * my + 2 * (y * z - w * x) * mz,
                     2 * (x * z - w * y) * mx + 2 * (y * z + w * x) * my + (1 - 2 * (x * x + y * y)) * mz], axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    kT, eta, dt = 1.0, 1.0, 0.04
    p, cfg = load_structure(12)
    a, Rh = p["sep"] / 2.0, p["Rh"]
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    m_body = np.array([1.0, 0.0, 0.0])                          # |m| = 1, fixed in the body
    B = 20.0 * kT                                               # |m| |B| = 20 kT: the thermal wobble about the field is small
    mu_rr = 1.0 / (8 * np.pi * eta * Rh ** 3)
    omega_c = B * mu_rr
    R, nb = args.replicas, 2
    centres = np.array([[0.0, 0.0, 0.0], [0.0, 4.0 * Rb, 0.0]]) + [0.0, 0.0, Rb + 2.0 * a]   # side by side across the rolling direction
    X = np.tile(centres, (R, 1, 1))
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (R, nb, 1))               # moments along x^, along B(0)
    stride = min(4, args.steps)
    print("omega_c = |m| |B| mu_rr = %.3f (free-space estimate), dt = %.3g, %d replicas x %d rollers" % (omega_c, dt, R, nb))
    for ratio in (0.5, 2.0):
        omega = ratio * omega_c
        ens = Ensemble(cfg, X, Q, a=a, eta=eta, dt=dt, kBT=kT, wall=True)
        ens.set_interactions(w=0.5, eps_wall=10.0, b_wall=0.25 * a, eps_blob=10.0, b_blob=0.25 * a)
        ens.set_dipoles(m_body, c_dd=1.0, r_core=2.0 * Rb, r_cut=8.0 * Rb)    # side-by-side parallel moments repel
        ens.set_magnetic_field(B1=[B, 0.0, 0.0], B2=[0.0, 0.0, -B], omega=omega)
        ens.set_field_time(0.0)
        t0 = time.time()
        out = ens.run(args.steps, F=np.zeros(6 * nb), seed=args.seed, stride=stride, on_error="reject", max_iter=50, rtol=1e-8)
        elapsed = time.time() - t0
        Xe = ens.get_config()[0]
        ens.close()
        T = dt * out.accepted                                   # every replica's own clock: what its field has run through
        ok = out.accepted > 0
        v = ((Xe[ok, :, 0] - X[ok, :, 0]) / T[ok, None]).mean(axis=1)
        # turns of the moments about +y^: the angle from x^ towards -z^, unwrapped over the frames
        m = lab_moments(out.Q, m_body)                          # (frames, R, nb, 3)
        ang = np.unwrap(np.concatenate([np.zeros((1, R, nb)), np.arctan2(-m[..., 2], m[..., 0])]), axis=0)
        turns = ang[-1] / (2 * np.pi)
        field_turns = omega * dt * out.accepted_at[-1] / (2 * np.pi)
        print("omega = %.1f omega_c: %.1f s, %.0f replica-steps/s, rejected %d" % (ratio, elapsed, R * args.steps / elapsed, out.rejected.sum()))
        print("  mean rolling velocity along x: %.4f +- %.4f (a synchronous roller of radius R_b turning at omega: up to ~ omega R_b / 4 = %.4f)" % (
            v.mean(), v.std(ddof=1) / np.sqrt(max(v.size, 2)) if v.size > 1 else 0.0, omega * Rb / 4))
        print("  turns of the moment about y: %.2f +- %.2f, of the field: %.2f -> %s" % (
            turns.mean(), turns.std(), field_turns.mean(),
            "synchronous" if abs(turns.mean() - field_turns.mean()) < 0.5 else "stepped out (slips %.2f turns)" % (field_turns.mean() - turns.mean())))


if __name__ == "__main__":
    main()
