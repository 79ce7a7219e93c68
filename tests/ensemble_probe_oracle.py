"""CPU restatement of the flow at probe points of one replica (include/rbl.h section 5, observers) on the CPU oracle.  It calls no
library code.  A helper -- no test in it.

    u(x_p) = nf d(z_p) sum_j sum_images M(x_p, r_j + image) d(z_j) lambda_j

Open system (field_open): the points are appended to the blobs as zero-force blobs and the oracle's apply_M_rows returns their
rows, as tests/test_velocity_field_gpu.py does.  Cell (field_cell): the points are appended after the blobs and
tests/periodic_oracle.py: rows gives their rows of B M_per B; at most 16 points per call, about 25 microseconds per pair and image.
A point that coincides with a blob (within 1e-12 a; in a cell: modulo the lattice) is NOT appended -- the oracle raises its overlap
error at distance 0 -- and takes that blob's own row instead: the self block, and every other pair from the blob's position.
With the wall a point at z <= 0 gets 0 and is not appended either.  Appended points must not coincide with each other.
Points fixed in a body are placed by place(): x = X_b + R(Q_b) s with the oracle's conventions (normalize_quats, rot_matrix),
which are multi_body_pos's."""
import numpy as np

import periodic_oracle as po

TINY = 1e-12                                               # the coincidence distance, in units of a


def place(points, X, Q, body=None):
    """lab positions of the probe points of one replica: the points themselves, or X_b + R(Q_b) s_p for offsets fixed in body b"""
    from oracle import oracle as O
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if body is None:
        return p.copy()
    Qn = O.normalize_quats(np.asarray(Q, dtype=np.float64).reshape(-1, 4))
    return p @ O.rot_matrix(Qn[body]).T + np.asarray(X, dtype=np.float64).reshape(-1, 3)[body]


def _coincident(r, x, a, L=None):
    """index of the blob the point x lies on, or -1"""
    d = x[None, :] - r
    if L is not None:
        d = po.nearest(d, L)
    k = int(np.argmin((d * d).sum(axis=1)))
    return k if np.linalg.norm(d[k]) < TINY * a else -1


def field_open(orc, r, lam, pts, a, eta, wall, nthreads=8):
    """u (P, 3) at the lab points pts of the blob forces lam on the blobs r (N, 3), open system or above the wall"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    N, P = r.shape[0], pts.shape[0]
    u = np.zeros((P, 3))
    free = []
    for p in range(P):
        if wall and not pts[p, 2] > 0.0:
            continue
        k = _coincident(r, pts[p], a)
        if k >= 0:
            u[p] = orc.apply_M_rows(lam, r.reshape(-1), k, k + 1, a, eta, wall)
        else:
            free.append(p)
    if free:
        F = np.concatenate([lam, np.zeros(3 * len(free))])
        rr = np.concatenate([r.reshape(-1), pts[free].reshape(-1)])
        u[free] = orc.apply_M_rows(F, rr, N, N + len(free), a, eta, wall, nthreads=nthreads).reshape(-1, 3)
    return u


def field_cell(orc, r, lam, pts, a, eta, L, n):
    """the same in the cell L = (Lx, Ly) with n = (nx, ny) images, wall on; at most 16 points"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    N, P = r.shape[0], pts.shape[0]
    assert P <= 16, "at most 16 sampled points per call"
    u = np.zeros((P, 3))
    free = []
    for p in range(P):
        if not pts[p, 2] > 0.0:
            continue
        k = _coincident(r, pts[p], a, L)
        if k >= 0:
            u[p] = po.rows(orc, r, [k], a, eta, L, n) @ lam
        else:
            free.append(p)
    if free:
        rr = np.concatenate([r, pts[free]])
        M = po.rows(orc, rr, [N + i for i in range(len(free))], a, eta, L, n)
        u[free] = (M[:, :3 * N] @ lam).reshape(-1, 3)
    return u


def stresslet(D):
    """symmetric traceless part of first moments D (..., 3, 3)"""
    D = np.asarray(D, dtype=np.float64)
    S = 0.5 * (D + np.swapaxes(D, -1, -2))
    return S - np.trace(S, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
