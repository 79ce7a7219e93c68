"""numpy restatement of the bonds and tethers of include/rbl.h section 4, written from the formulas there: bond b joins the point
p_A = X_i + R(Q_i) s_A of body i to p_B = X_j + R(Q_j) s_B of another body j, or to the lab point P (j = -1).  Kind 0 is harmonic,
U = k (d - l0)^2 / 2; kind 1 is k T(d) with T the bond table: the Hermite evaluation of tests/table_oracle.py inside the grid and
below it, and the tangent at the last grid point beyond it (a bond never breaks).  One bond at a time, one system (the replicas
of an ensemble are evaluated one by one by the caller).  A helper -- no test in it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magnetic_oracle as mo  # noqa: E402
import table_oracle  # noqa: E402


def bond_table_eval(tab, d):
    """tab = (U, dU, lo, hi) -> (T(d), dT/dd): table_oracle.table_eval up to hi, the tangent at hi above it"""
    U, dU, lo, hi = tab
    U, dU = np.asarray(U, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    if d > hi:
        return float(U[-1] + dU[-1] * (d - hi)), float(dU[-1])
    T, dT = table_oracle.table_eval(tab, np.float64(d))
    return float(T), float(dT)


def end_points(X, Q, body, anchor, b):
    """-> (l_A, l_B, p_A, p_B) of bond b: lever arms R(Q) s about the body centres (l_B = 0 for a lab point) and end points"""
    i, j = int(body[b][0]), int(body[b][1])
    lA = mo.rot(Q[i]) @ anchor[b][:3]
    pA = X[i] + lA
    if j >= 0:
        lB = mo.rot(Q[j]) @ anchor[b][3:]
        return lA, lB, pA, X[j] + lB
    return lA, np.zeros(3), pA, np.array(anchor[b][3:], dtype=np.float64)


def bonds(X, Q, body, anchor, k, l0, kind=None, table=None, with_scale=False):
    """X (N_bod, 3), Q (N_bod, 4), body (n, 2), anchor (n, 6) = s_A | s_B or P, k and l0 (n,), kind (n,) or None (all harmonic),
    table = (U, dU, r_min, r_cut) for the kind-1 bonds.
    -> FT (N_bod, 6) physical force and torque about the centre of every body, E total energy, state = (length, tension dU/dd,
    energy) per bond; with_scale: also the sum of the magnitudes of the energy's terms"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    body = np.asarray(body).reshape(-1, 2)
    anchor = np.asarray(anchor, dtype=np.float64).reshape(-1, 6)
    n = body.shape[0]
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (n,))
    l0 = np.broadcast_to(np.asarray(l0, dtype=np.float64), (n,))
    kind = np.zeros(n, dtype=int) if kind is None else np.asarray(kind)
    FT = np.zeros((X.shape[0], 6))
    length, tension, energy = np.zeros(n), np.zeros(n), np.zeros(n)
    for b in range(n):
        i, j = int(body[b, 0]), int(body[b, 1])
        assert i >= 0 and j >= -1 and i != j
        lA, lB, pA, pB = end_points(X, Q, body, anchor, b)
        r = pA - pB
        d = np.sqrt(r @ r)
        if kind[b] == 0:
            U, dU = 0.5 * k[b] * (d - l0[b]) ** 2, k[b] * (d - l0[b])
        else:
            T, dT = bond_table_eval(table, d)
            U, dU = k[b] * T, k[b] * dT
        f = -dU * r / d if d > 0.0 else np.zeros(3)             # on end A; coincident ends exert no force
        FT[i, :3] += f
        FT[i, 3:] += np.cross(lA, f)
        if j >= 0:
            FT[j, :3] -= f
            FT[j, 3:] += np.cross(lB, -f)
        length[b], tension[b], energy[b] = d, dU, U
    E = float(energy.sum())
    if with_scale:
        return FT, E, (length, tension, energy), float(np.abs(energy).sum())
    return FT, E, (length, tension, energy)
