"""numpy restatement of the hard joints of include/rbl.h section 9, for the tests: lever arms and gaps, the constraint matrix J,
the dense jointed solve and step on the oracle's M and K, the joint Schur complement of a block preconditioner, and the joint
sets the GPU tests share.  Nothing here calls the library."""
import numpy as np


def rot(q):
    """rotation matrix of a unit quaternion (w, x, y, z): lab = R body"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def unit(Q):
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


def geometry(X, Q, body, anchor):
    """-> (l_A (n, 3), l_B (n, 3) (zero for a pivot), gap p_A - p_B (n, 3))"""
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), unit(Q)
    body, anchor = np.asarray(body).reshape(-1, 2), np.asarray(anchor, dtype=np.float64).reshape(-1, 6)
    n = body.shape[0]
    lA, lB, gap = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for j, (a, b) in enumerate(body):
        lA[j] = rot(Q[a]) @ anchor[j, :3]
        if b >= 0:
            lB[j] = rot(Q[b]) @ anchor[j, 3:]
            pB = X[b] + lB[j]
        else:
            pB = anchor[j, 3:]
        gap[j] = X[a] + lA[j] - pB
    return lA, lB, gap


def cross_matrix(l):
    """[l]x: [l]x v = l x v"""
    return np.array([[0.0, -l[2], l[1]], [l[2], 0.0, -l[0]], [-l[1], l[0], 0.0]])


def J_matrix(X, Q, body, anchor):
    """(3 n, 6 N_bod): (J U)_j = (u_A + w_A x l_A) - (u_B + w_B x l_B), no B term for a pivot"""
    nb = np.asarray(X).reshape(-1, 3).shape[0]
    body = np.asarray(body).reshape(-1, 2)
    lA, lB, _ = geometry(X, Q, body, anchor)
    J = np.zeros((3 * body.shape[0], 6 * nb))
    for j, (a, b) in enumerate(body):
        J[3 * j:3 * j + 3, 6 * a:6 * a + 3] = np.eye(3)
        J[3 * j:3 * j + 3, 6 * a + 3:6 * a + 6] = -cross_matrix(lA[j])       # w x l = -l x w
        if b >= 0:
            J[3 * j:3 * j + 3, 6 * b:6 * b + 3] = -np.eye(3)
            J[3 * j:3 * j + 3, 6 * b + 3:6 * b + 6] = cross_matrix(lB[j])
    return J


def dense_matrices(orc, cfg, X, Q, a, eta, wall):
    """M (B M B with the wall, as apply_M applies it) and K of a configuration, as tests/test_prescribed_gpu.py builds them"""
    from oracle import oracle as O
    cfg = np.asarray(cfg) - np.asarray(cfg).mean(axis=0)
    Qn = O.normalize_quats(np.asarray(Q, dtype=np.float64).reshape(-1, 4))
    r = orc.multi_body_pos(X, Qn, cfg)
    K = O.K_matrix(X, Qn, cfg)
    M = orc.rotne_prager_tensor(r, a, eta, wall)
    if wall:
        B = orc.damp(r, a)
        M = B[:, None] * M * B[None, :]
    return M, K


def dense_jointed(M, K, J, F, slip, c):
    """numpy.linalg.solve on [M -K 0; K^T 0 J^T; 0 J 0] [lambda; U; phi] = [slip; -F; c] -> (lambda, U, phi)"""
    n3, nb6, nj3 = M.shape[0], K.shape[1], J.shape[0]
    A = np.zeros((n3 + nb6 + nj3,) * 2)
    A[:n3, :n3] = M
    A[:n3, n3:n3 + nb6] = -K
    A[n3:n3 + nb6, :n3] = K.T
    A[n3:n3 + nb6, n3 + nb6:] = J.T
    A[n3 + nb6:, n3:n3 + nb6] = J
    x = np.linalg.solve(A, np.concatenate([np.asarray(slip).reshape(-1), -np.asarray(F).reshape(-1), np.asarray(c).reshape(-1)]))
    return x[:n3], x[n3:n3 + nb6], x[n3 + nb6:]


def schur_block_pc(M, K, J, nblb):
    """S = J N^-1 J^T with N_b = K_b^T M_bb^-1 K_b of the per-body diagonal blocks of M: the joint Schur complement of the block
    preconditioner"""
    nb = K.shape[1] // 6
    Ninv = np.zeros((6 * nb, 6 * nb))
    for b in range(nb):
        s = slice(3 * nblb * b, 3 * nblb * (b + 1))
        Kb = K[s, 6 * b:6 * b + 6]
        Ninv[6 * b:6 * b + 6, 6 * b:6 * b + 6] = np.linalg.inv(Kb.T @ np.linalg.solve(M[s, s], Kb))
    return J @ Ninv @ J.T


# ---- the joint sets of the GPU tests ---------------------------------------------------------------------------------------
def blob(cfg, k):
    """body-frame position of blob k (the structure's mean removed)"""
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 3)
    return cfg[k] - cfg.mean(axis=0)


def probe_set(cfg, X):
    """4 bodies, 5 joints: the chain 0-1, 1-2, 2-3, a second joint 1-2 (with the first: a hinge), a pivot on body 3.  Anchors off
    the centres, two of them blobs, one a centre; the pivot's lab point half a unit from its anchor: no gap is zero"""
    body = np.array([[0, 1], [1, 2], [2, 3], [2, 1], [3, -1]])
    anchor = np.array([np.concatenate([blob(cfg, 3), [0.2, -0.3, 0.4]]),
                       np.concatenate([[0.5, 0.1, -0.2], blob(cfg, 7)]),
                       np.concatenate([[0.0, 0.0, 0.0], [-0.3, 0.4, 0.1]]),           # a centre anchor
                       np.concatenate([[0.1, -0.6, 0.3], [0.4, 0.3, 0.5]]),
                       np.concatenate([[0.3, 0.2, -0.4], np.asarray(X)[3] + [0.5, -0.2, 0.6]])])
    return body, anchor


def chain_set(nb, X, seed):
    """nb bodies in a chain (nb - 1 joints) and a pivot on each end body: nb + 1 joints, random anchors off the centres"""
    rng = np.random.default_rng(seed)
    body = np.array([[i, i + 1] for i in range(nb - 1)] + [[0, -1], [nb - 1, -1]])
    anchor = rng.uniform(-0.6, 0.6, (nb + 1, 6))
    anchor[nb - 1, 3:] = np.asarray(X)[0] + [0.3, 0.4, -0.2]
    anchor[nb, 3:] = np.asarray(X)[nb - 1] + [-0.4, 0.1, 0.5]
    return body, anchor


def hub_set(nb, seed):
    """nb - 1 joints, all to body 0, the later ones with body 0 in the second slot: more than 64 ends on one body for nb > 65"""
    rng = np.random.default_rng(seed)
    body = np.array([[0, i] if i % 3 else [i, 0] for i in range(1, nb)])
    return body, rng.uniform(-0.6, 0.6, (nb - 1, 6))


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def hinged_chain(seed, z0=3.0, open_by=0.02):
    """A 3-body chain that is nearly closed, for the step tests: a joint 0-1, a hinge (two joints) 1-2 whose anchors are one
    unit apart on both bodies -- so it CAN close -- and a pivot on body 0; anchors 1.5 from the centres, so joined shell_N_12
    bodies (radius 1.21) stay clear of each other; random orientations; every gap of the order open_by, none zero.
    -> (X, Q, body, anchor)"""
    rng = np.random.default_rng(seed)
    Q = unit(rng.standard_normal((3, 4)))
    R = [rot(q) for q in Q]
    d = _unit([1.0, 0.2, 0.1])                                  # body 0 -> body 1
    e = _unit(np.cross(d, [0.0, 0.0, 1.0]))                     # body 1 -> body 2, across
    h = _unit(np.cross(e, d))                                   # the hinge's axis
    X = np.array([[0.0, 0.0, z0], [0.0, 0.0, z0] + 3.0 * d, [0.0, 0.0, z0] + 3.0 * d + 3.0 * e])
    body = np.array([[0, 1], [1, 2], [1, 2], [0, -1]])
    anchor = np.zeros((4, 6))
    anchor[0, :3], anchor[0, 3:] = R[0].T @ (1.5 * d), R[1].T @ (-1.5 * d)
    for j, sgn in ((1, 1.0), (2, -1.0)):
        anchor[j, :3], anchor[j, 3:] = R[1].T @ (1.5 * e + 0.5 * sgn * h), R[2].T @ (-1.5 * e + 0.5 * sgn * h)
    anchor[3, :3] = [-0.2, 0.3, 0.5]
    anchor[3, 3:] = X[0] + R[0] @ anchor[3, :3] + open_by * np.array([0.5, -0.7, 0.4])
    # open every joint a little: the later bodies shifted, the last one also turned
    X[1] += open_by * np.array([0.6, -0.5, 0.3])
    X[2] += open_by * np.array([-0.4, 0.8, 0.5])
    w = 0.5 * open_by * np.array([0.3, -0.5, 0.8])
    dq = np.concatenate([[np.cos(np.linalg.norm(w) / 2)], np.sin(np.linalg.norm(w) / 2) * _unit(w)])
    q2 = Q[2]
    Q[2] = unit([[dq[0] * q2[0] - dq[1:] @ q2[1:], *(dq[0] * q2[1:] + q2[0] * dq[1:] + np.cross(dq[1:], q2[1:]))]])[0]
    return X, Q, body, anchor


def redundant_set():
    """Two bodies with identity orientations side by side, every anchor on the x axis through both centres and every number a
    short binary fraction: each body held by two pivots that sit exactly on their anchors, and a joint between the two bodies.
    Two pivots on a rigid body fix the distance between them twice, and along the common line the joint adds a third copy.
    -> (X, Q, body, anchor)"""
    X = np.array([[0.0, 0.0, 4.0], [4.0, 0.0, 4.0]])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    body = np.array([[0, -1], [0, -1], [1, -1], [1, -1], [0, 1]])
    sx = [-0.5, 0.5, -0.5, 0.5]
    anchor = np.zeros((5, 6))
    for j in range(4):
        anchor[j, 0] = sx[j]
        anchor[j, 3:] = X[body[j, 0]] + [sx[j], 0.0, 0.0]
    anchor[4, 0], anchor[4, 3] = 1.5, -1.5
    return X, Q, body, anchor
