"""numpy restatement of the dipole terms of include/rbl.h section 4, written from the formulas there: permanent moments fixed in
the bodies, the torque of a uniform field B(t) = B0 + B1 cos(omega t) + B2 sin(omega t) and the dipole pairs between the centres
of different bodies with a core radius and a cutoff.  All pairs, no lists; one system (the replicas of an ensemble are evaluated
one by one by the caller)."""
import numpy as np


def rot(q):
    """rotation matrix of a scalar-first quaternion (normalised here): lab = R body"""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(p, q):
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.array([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw])


def rotate(Q, delta):
    """dq(delta) Q: the orientation turned by the rotation vector delta (lab frame)"""
    delta = np.asarray(delta, dtype=np.float64)
    th = np.linalg.norm(delta)
    if th == 0.0:
        return np.array(Q, dtype=np.float64)
    dq = np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) * delta / th])
    return quat_mul(dq, Q)


def field(B0, B1, B2, omega, t):
    return np.asarray(B0, float) + np.asarray(B1, float) * np.cos(omega * t) + np.asarray(B2, float) * np.sin(omega * t)


def lab_moments(Q, m_body):
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    mb = np.broadcast_to(np.asarray(m_body, dtype=np.float64).reshape(-1, 3), (Q.shape[0], 3))
    return np.stack([rot(Q[i]) @ mb[i] for i in range(Q.shape[0])])


def pair_distances(X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    i, j = np.triu_indices(X.shape[0], 1)
    return np.linalg.norm(X[i] - X[j], axis=1)


def dipoles(X, Q, m_body, c_dd=0.0, r_core=1.0, r_cut=np.inf, B=None, with_scale=False):
    """-> (FT (N_bod, 6): physical force and torque about the centre of every body, E: total energy).  m_body: (3,) or (N_bod, 3);
    B: the field vector at the time of the evaluation or None (field off).  with_scale: also the sum of the magnitudes of the
    energy's terms -- what the rounding error of a sum of terms of both signs is relative to"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    m = lab_moments(Q, m_body)
    FT = np.zeros((n, 6))
    E = Eabs = 0.0
    if c_dd > 0.0 and n > 1:
        r = X[:, None, :] - X[None, :, :]                       # r[i, j] = X_i - X_j
        d = np.linalg.norm(r, axis=2)
        on = (d <= r_cut) & ~np.eye(n, dtype=bool)               # pairs with d > r_cut are skipped
        s = np.maximum(d, r_core)
        a = np.einsum("ic,ijc->ij", m, r)                        # m_i . r
        b = np.einsum("jc,ijc->ij", m, r)                        # m_j . r
        mm = m @ m.T
        U = c_dd * (mm / s ** 3 - 3 * a * b / s ** 5)
        E = 0.5 * U[on].sum()
        Eabs = 0.5 * c_dd * (np.abs(mm) / s ** 3 + 3 * np.abs(a * b) / s ** 5)[on].sum()
        outside = d >= r_core
        d2 = np.where(outside, d * d, 1.0)                       # no division by d below the core (d = 0 included)
        radial = np.where(outside, mm - 5 * a * b / d2, 0.0)
        F = 3 * c_dd * (a[..., None] * m[None, :, :] + b[..., None] * m[:, None, :] + radial[..., None] * r) / s[..., None] ** 5
        H = c_dd * (3 * b[..., None] * r / s[..., None] ** 5 - m[None, :, :] / s[..., None] ** 3)
        T = np.cross(np.broadcast_to(m[:, None, :], H.shape), H)
        FT[:, :3] = np.where(on[..., None], F, 0.0).sum(axis=1)
        FT[:, 3:] = np.where(on[..., None], T, 0.0).sum(axis=1)
    if B is not None:
        B = np.asarray(B, dtype=np.float64)
        FT[:, 3:] += np.cross(m, B)
        E -= (m @ B).sum()
        Eabs += np.abs(m * B).sum()
    return (FT, E, Eabs) if with_scale else (FT, E)
