"""Plain-numpy restatement of include/rbl.h section 8 for the tests: the flow model's term and the first moments of blob forces,
each with the componentwise rounding bound its test uses.  Built on oracle.oracle's rot_matrix, normalize_quats, K_matrix and
Oracle.multi_body_pos, whose blob positions the device matches bit for bit."""
import numpy as np

from oracle import oracle as O

EPS = np.finfo(np.float64).eps


def geometry(orc, X, Q, cfg):
    """-> (Qn (nb, 4), R (nb, 3, 3), r (nb, nblb, 3), centred cfg (nblb, 3))"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    c = O.remove_mean(cfg)
    Qn = O.normalize_quats(Q)
    R = np.stack([O.rot_matrix(q) for q in Qn])
    r = orc.multi_body_pos(X, Qn, c).reshape(X.shape[0], c.shape[0], 3)
    return Qn, R, r, c


def flow_term(orc, X, Q, cfg, u0=None, G=None, slip_body=None, scale=None):
    """t_i = scale_b R(q_b) s_body,i - (u0 + G r_i) -> (t (3 N,), bound (3 N,)) with
    bound = 8 eps (|u0_i| + sum_j |G_ij| |r_j| + sum_j |R_ij| |s_j|): at most six roundings per component, FMA contraction either way"""
    _, R, r, _ = geometry(orc, X, Q, cfg)
    nb, nblb = r.shape[:2]
    t, mag = np.zeros((nb, nblb, 3)), np.zeros((nb, nblb, 3))
    if slip_body is not None:
        s = np.asarray(slip_body, dtype=np.float64).reshape(nblb, 3)
        sc = np.ones(nb) if scale is None else np.asarray(scale, dtype=np.float64)
        t += sc[:, None, None] * np.einsum("bij,kj->bki", R, s)
        mag += np.einsum("bij,kj->bki", np.abs(R), np.abs(s))
    if u0 is not None or G is not None:
        u0 = np.zeros(3) if u0 is None else np.asarray(u0, dtype=np.float64)
        G = np.zeros((3, 3)) if G is None else np.asarray(G, dtype=np.float64)
        t -= u0 + np.einsum("ij,bkj->bki", G, r)
        mag += np.abs(u0) + np.einsum("ij,bkj->bki", np.abs(G), np.abs(r))
    return t.reshape(-1), (8.0 * EPS * mag).reshape(-1)


def first_moments(orc, X, Q, cfg, lam):
    """D_b = sum_k (r_k - X_b) lambda_k^T -> (D (nb, 3, 3), bound (nb, 3, 3)) with
    bound_ij = 4 N_blb eps sum_k (|l_k,i| + |X_i|) |lambda_k,j|: any summation order; the lever arms carry one rounding of the position"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    _, _, r, _ = geometry(orc, X, Q, cfg)
    nb, nblb = r.shape[:2]
    lev = r - X[:, None, :]
    lam = np.asarray(lam, dtype=np.float64).reshape(nb, nblb, 3)
    D = np.einsum("bki,bkj->bij", lev, lam)
    bound = 4.0 * nblb * EPS * np.einsum("bki,bkj->bij", np.abs(lev) + np.abs(X)[:, None, :], np.abs(lam))
    return D, bound


def stresslet(D):
    """symmetric traceless part of (..., 3, 3)"""
    S = 0.5 * (D + np.swapaxes(D, -1, -2))
    return S - np.trace(S, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0


def torque(D):
    """the antisymmetric part as a vector: T = sum l x lambda"""
    return np.stack([D[..., 1, 2] - D[..., 2, 1], D[..., 2, 0] - D[..., 0, 2], D[..., 0, 1] - D[..., 1, 0]], axis=-1)
