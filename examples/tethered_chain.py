"""An artificial cilium: a chain of magnetic beads linked by short springs, its first bead tethered to a point on the wall, driven
by a precessing field.

Every bead is a shell_N_12 with a permanent moment along its own z axis.  Neighbouring beads are joined surface to surface: the
point (0, 0, +R_b) fixed in bead i is bonded to the point (0, 0, -R_b) fixed in bead i + 1 by a stiff harmonic spring of rest
length `gap`, and the lowest bead's point (0, 0, -R_b) is tethered to the lab point (0, 0, a) just above the wall.  Because the
anchors sit off the centres, the springs also resist bending: a bead that turns away from the chain's axis stretches its two
bonds.  The field B(t) = B_z z^ + B_xy (cos(omega t) x^ + sin(omega t) y^) precesses about the wall's normal; the moments follow
it, and the chain sweeps a cone.  Weight, wall repulsion and steric repulsion keep the beads apart and above the wall.

The whole trajectory is ONE Ensemble.run of R replicas x `steps` stochastic midpoint steps: bonds, dipoles and the field's clock
are part of the run's constant model and are evaluated on the GPU at every step.  The example prints the end-to-end distance of
the chain (tether point to the centre of the last bead) beside its contour length, and the largest bond extension d - l0 at the
end.  Reports; asserts nothing.

    python examples/tethered_chain.py [--replicas 64] [--steps 2000] [--beads 6]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--beads", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    kT, eta, dt = 1.0, 1.0, 0.005
    p, cfg = load_structure(12)
    a, Rh = p["sep"] / 2.0, p["Rh"]
    Rb = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    R, nb = args.replicas, args.beads
    gap = 2.0 * a                                               # surface-to-surface rest length: the blobs of two beads just clear
    pitch = 2.0 * Rb + gap
    tether = np.array([0.0, 0.0, a])                            # the point on the wall the chain hangs on
    centres = np.array([[0.0, 0.0, tether[2] + gap + Rb + i * pitch] for i in range(nb)])
    X = np.tile(centres, (R, 1, 1))
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (R, nb, 1))
    top, bottom = np.array([0.0, 0.0, Rb]), np.array([0.0, 0.0, -Rb])
    body = [[0, -1]] + [[i, i + 1] for i in range(nb - 1)]      # the tether, then the chain
    anchor_a = [bottom] + [top] * (nb - 1)
    anchor_b = [tether] + [bottom] * (nb - 1)
    k_bond = 50.0 * kT / a ** 2                                 # thermal stretch sqrt(kT / k) = 0.14 a; k mu_tt dt = 0.08
    B = 30.0 * kT
    mu_rr = 1.0 / (8 * np.pi * eta * Rh ** 3)
    omega = 0.25 * B * mu_rr                                    # well below a single bead's step-out frequency
    tilt = np.deg2rad(30.0)
    ens = Ensemble(cfg, X, Q, a=a, eta=eta, dt=dt, kBT=kT, wall=True)
    ens.set_interactions(w=0.05, eps_wall=10.0, b_wall=0.25 * a, eps_blob=10.0, b_blob=0.25 * a)
    ens.set_bonds(body, anchor_a, anchor_b, k_bond, gap)
    ens.set_dipoles([0.0, 0.0, 1.0], c_dd=1.0, r_core=2.0 * Rb, r_cut=4.0 * pitch)   # head-to-tail moments attract
    ens.set_magnetic_field(B0=[0.0, 0.0, B * np.cos(tilt)], B1=[B * np.sin(tilt), 0.0, 0.0], B2=[0.0, B * np.sin(tilt), 0.0], omega=omega)
    ens.set_field_time(0.0)
    print("%d replicas x %d beads, k = %.0f kT / a^2, rest length %.3f, field tilted %.0f deg, omega = %.3f, dt = %.3g"
          % (R, nb, k_bond * a ** 2 / kT, gap, np.rad2deg(tilt), omega, dt))
    t0 = time.time()
    out = ens.run(args.steps, F=np.zeros(6 * nb), seed=args.seed, on_error="reject", max_iter=60, rtol=1e-8)
    elapsed = time.time() - t0
    Xe = ens.get_config()[0]
    length, tension, energy = ens.bond_state()
    ens.close()
    ee = np.linalg.norm(Xe[:, -1, :] - tether, axis=1)
    contour = gap + Rb + (nb - 1) * pitch
    lean = np.degrees(np.arccos(np.clip((Xe[:, -1, 2] - tether[2]) / ee, -1.0, 1.0)))
    print("%.1f s, %.0f replica-steps/s, rejected %d" % (elapsed, R * args.steps / elapsed, out.rejected.sum()))
    print("end-to-end distance: %.3f +- %.3f (contour length %.3f), leaning %.1f deg from the normal after %.2f turns of the field"
          % (ee.mean(), ee.std(), contour, lean.mean(), omega * dt * out.accepted.mean() / (2 * np.pi)))
    print("largest bond extension: %.4f (rest length %.3f, thermal sqrt(kT / k) = %.4f); largest tension %.2f"
          % ((length - gap).max(), gap, np.sqrt(kT / k_bond), np.abs(tension).max()))


if __name__ == "__main__":
    main()
