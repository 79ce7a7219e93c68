"""Active microrheology with an oscillating force: one trapped shell_N_12 per replica, 64 driving frequencies across the replicas,
ONE driven run (Ensemble.run_driven, include/rbl.h section 5) -- a whole spectrum in one call.

Every replica holds one shell in free space in a harmonic trap of stiffness k and is pushed along x with F1 cos(omega_r t).  The
lock-in sums X_c = sum x cos, X_s = sum x sin and norm, kept on the GPU, give the in-phase and out-of-phase amplitudes by the 2 x 2
normal equations, exactly in discrete time.  A first run without lock-in lets the transient decay (20 relaxation times); the second
continues it from cycle_pos / t_end and measures.  The curve to compare with is the single relaxation of the explicit Euler step,
    x_n = Re[H e^{i omega t_n}],     H = dt mu F1 / (e^{i omega dt} - 1 + dt mu k)        (-> (F1 / k) / (1 + i omega tau), tau = 1 / (mu k)),
with the body mobility mu taken from the library's own solve.

    python examples/ensemble_oscillatory.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigid_body_light_amd import Ensemble, load_structure  # noqa: E402


def main():
    p, cfg = load_structure(12)
    a, eta, dt, k, F1, R = p["sep"] / 2.0, 1.0, 0.01, 50.0, 1.0, 64
    X, Q = np.zeros((R, 1, 3)), np.tile([1.0, 0.0, 0.0, 0.0], (R, 1, 1))
    ens = Ensemble(cfg, X, Q, a=a, eta=eta, dt=dt, kBT=0.0, wall=False)
    # the mobility: U = -N F_body (the library's sign convention), nobody prescribed, a unit load along x
    mu = -ens.solve_mixed(np.zeros((R, 1), dtype=bool), np.array([1.0, 0, 0, 0, 0, 0]), rtol=1e-12)[1][0, 0]
    tau = 1.0 / (mu * k)
    omega = np.geomspace(0.1, 30.0, R) / tau
    ens.set_traps(np.array([[k, 0.0, 0.0]]), np.zeros((1, 3)))
    amp = np.zeros(6)
    amp[0] = -F1                                         # F_body is minus the physical force
    kw = dict(F=np.zeros(6), cos=amp, omega=omega, brownian=False, rtol=1e-12, max_iter=100)
    burn, measure = int(20 * tau / dt), 1500
    t0 = time.perf_counter()
    first = ens.run_driven(burn, **kw)
    res = ens.run_driven(measure, t0=first.t_end, cycle_start=first.cycle_pos, lockin=True, **kw)
    wall = time.perf_counter() - t0
    ens.close()
    # amplitude of cos and sin from the lock-in sums: [sum cs^2, sum cs sn; sum cs sn, sum sn^2] (A, B) = (X_c, X_s)
    n = res.norm
    det = n[:, 2] * n[:, 3] - n[:, 4] ** 2
    xc, xs = res.X_c[:, 0, 0], res.X_s[:, 0, 0]
    A, B = (n[:, 3] * xc - n[:, 4] * xs) / det, (n[:, 2] * xs - n[:, 4] * xc) / det
    H = dt * mu * F1 / (np.exp(1j * omega * dt) - 1.0 + dt * mu * k)
    got = A - 1j * B                                     # x = Re[(A - i B) e^{i omega t}]
    print("mu = %.6f, tau = 1 / (mu k) = %.4f, %d + %d steps of %d replicas in %.2f s" % (mu, tau, burn, measure, R, wall))
    print(" omega tau   |x| k / F1    phase / pi    single relaxation (discrete)    continuous")
    for r in range(0, R, 7):
        cont = 1.0 / (1.0 + 1j * omega[r] * tau)
        print("%9.3f   %10.6f   %10.6f      %10.6f %10.6f      %10.6f %10.6f"
              % (omega[r] * tau, abs(got[r]) * k / F1, np.angle(got[r]) / np.pi, abs(H[r]) * k / F1, np.angle(H[r]) / np.pi, abs(cont),
                 np.angle(cont) / np.pi))
    err = np.abs(got - H).max() * k / F1
    print("largest deviation from the discrete single-relaxation curve over the %d frequencies: %.2e (in units of F1 / k)" % (R, err))
    assert err < 1e-6, err


if __name__ == "__main__":
    main()
