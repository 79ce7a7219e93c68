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
    n3, nb6 = M.shape[0], K.shape[1]
    x = np.linalg.solve(jointed_matrix(M, K, J), rhs_jointed(F, slip, c))
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


# ---- the jointed matrix, its exact preconditioner and the library's GMRES, restated -----------------------------------------
def jointed_matrix(M, K, J):
    """[M -K 0; K^T 0 J^T; 0 J 0], dense: the matrix dense_jointed solves"""
    n3, nb6, nj3 = M.shape[0], K.shape[1], J.shape[0]
    A = np.zeros((n3 + nb6 + nj3,) * 2)
    A[:n3, :n3] = M
    A[:n3, n3:n3 + nb6] = -K
    A[n3:n3 + nb6, :n3] = K.T
    A[n3:n3 + nb6, n3 + nb6:] = J.T
    A[n3 + nb6:, n3:n3 + nb6] = J
    return A


def cond_jointed(A, n3, nb6):
    """2-norm condition number of a jointed matrix: with the signs of its body columns and of its joint rows flipped (which
    leaves the singular values alone) it is the symmetric [M K 0; K^T 0 J^T; 0 J 0], whose eigenvalues' moduli they are"""
    S = np.array(A)
    S[:, n3:n3 + nb6] *= -1.0
    S[n3 + nb6:] *= -1.0
    assert np.abs(S - S.T).max() <= 1e-13 * np.abs(S).max()              # (M itself is symmetric to rounding only)
    e = np.abs(np.linalg.eigvalsh(0.5 * (S + S.T)))
    return float(e.max() / e.min())


def pc_M(M, nblb, block):
    """M~ of the context's preconditioner: the per-body diagonal blocks of M (block_PC) or diag(M); the argument of schur_block_pc
    in tests/test_joints_gpu.py's redundant-loop test"""
    if not block:
        return np.diag(np.diag(M))
    Mt = np.zeros_like(M)
    for s in range(0, M.shape[0], 3 * nblb):
        Mt[s:s + 3 * nblb, s:s + 3 * nblb] = M[s:s + 3 * nblb, s:s + 3 * nblb]
    return Mt


def jointed_pc(M, K, J, nblb, block):
    """the right preconditioner of the jointed solve as a dense matrix: the exact inverse of the jointed matrix with M replaced
    by M~ -- one numpy inverse of the whole matrix, no Schur complement in it"""
    return np.linalg.inv(jointed_matrix(pc_M(M, nblb, block), K, J))


def gmres_right_pc(A, P, b, max_iter, rtol):
    """Right-preconditioned GMRES(max_iter) with the library's rules, what tests/torch_krylov.gmres_right_pc and
    test_native_gmres_equals_torch_gmres pin: x0 = 0, no restart, Arnoldi on A P with classical Gram-Schmidt applied twice, after
    every iteration k the least-squares residual |beta e1 - H_k y| / |b|, stop at the FIRST k at which it is < rtol (strictly),
    x = P V_k y.  A, P dense.  -> (x, iterations, residual estimate)"""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n, beta = b.size, float(np.linalg.norm(b))
    V, H = np.zeros((max_iter + 1, n)), np.zeros((max_iter + 1, max_iter))
    V[0] = b / beta
    e1 = np.zeros(max_iter + 1)
    e1[0] = beta
    m, y, res = max_iter, None, 1.0
    for j in range(max_iter):
        w = A @ (P @ V[j])
        for _ in range(2):
            h = V[:j + 1] @ w
            w = w - h @ V[:j + 1]
            H[:j + 1, j] += h
        H[j + 1, j] = np.linalg.norm(w)
        V[j + 1] = w / H[j + 1, j]
        y = np.linalg.lstsq(H[:j + 2, :j + 1], e1[:j + 2], rcond=None)[0]
        res = float(np.linalg.norm(H[:j + 2, :j + 1] @ y - e1[:j + 2]) / beta)
        if res < rtol:
            m = j + 1
            break
    return P @ (y @ V[:m]), m, res


def rhs_jointed(F, slip, c):
    return np.concatenate([np.asarray(slip).reshape(-1), -np.asarray(F).reshape(-1), np.asarray(c).reshape(-1)])


# ---- joint sets whose anchors scale with the body (chain_set and hub_set draw in +-0.6 whatever the body's size) -------------
def _radius(cfg):
    import body_shapes as bs
    return bs.radius(cfg)


def chain1(nb, cfg, X, seed):
    """the chain (i, i + 1) and ONE pivot, on body 0: nb joints; anchors uniform in +-R_b, the lab point R_b (0.3, 0.4, -0.2) from
    the body's centre"""
    Rb = _radius(cfg)
    body = np.array([[i, i + 1] for i in range(nb - 1)] + [[0, -1]])
    anchor = np.random.default_rng(seed).uniform(-Rb, Rb, (nb, 6))
    anchor[nb - 1, 3:] = np.asarray(X)[0] + Rb * np.array([0.3, 0.4, -0.2])
    return body, anchor


def hinged(nb, cfg, X, seed):
    """the chain, a second joint between the bodies 0 and 1 named in the other order, [1, 0] (with joint 0 an open hinge whose
    ends are swapped), and a pivot on the last body: nb + 1 joints, anchors as chain1's"""
    Rb = _radius(cfg)
    body = np.array([[i, i + 1] for i in range(nb - 1)] + [[1, 0], [nb - 1, -1]])
    anchor = np.random.default_rng(seed).uniform(-Rb, Rb, (nb + 1, 6))
    anchor[nb, 3:] = np.asarray(X)[nb - 1] + Rb * np.array([0.3, 0.4, -0.2])
    return body, anchor


def pivots(nb, cfg, X, Q, seed):
    """one pivot per body: anchors uniform in +-R_b, each lab point within +-0.5 of its anchor's lab position (never on it)"""
    Rb = _radius(cfg)
    rng = np.random.default_rng(seed)
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), unit(Q)
    body = np.array([[i, -1] for i in range(nb)])
    anchor = rng.uniform(-Rb, Rb, (nb, 6))
    off = rng.uniform(-0.5, 0.5, (nb, 3))
    for i in range(nb):
        anchor[i, 3:] = X[i] + rot(Q[i]) @ anchor[i, :3] + off[i]
    return body, anchor


# name: (shape, N_bod, wall, joint set, eta).  Lattices: body_shapes.lattice with seed 0; anchor seeds: 33 (chain_set), 35 (hub_set),
# 7 (chain1, hinged), 5 (pivots).  3 N_j rows, padded by the library to np = 32 ceil(3 N_j / 32)
SHAPE_CASES = {
    "J1w": ("trimer", 100, True, "chain_set", 1.0),       # 101 joints, 303 rows, np 320; 6 N_bod = 600 > N = 300
    "J1f": ("trimer", 100, False, "chain_set", 1.0),
    "J2": ("trimer", 172, False, "hub_set", 1.0),         # 171 joints, 513 rows, np 544 > 512: the second Cholesky panel
    "J3": ("trimer", 300, True, "chain1", 1.0),           # 300 joints, 900 rows, np 928; the system has order 5400
    "J4": ("tetra", 90, True, "pivots", 1.0),             # 90 joints, 270 rows, np 288; l_B = 0 everywhere
    "J5f": ("tetra", 100, False, "hinged", 1.0),          # 101 joints; an open hinge with swapped ends
    "J5w": ("bipyramid", 90, True, "hinged", 1.0),        # 91 joints
    "J6f": ("fib7", 43, False, "chain_set", 1.0),         # 44 joints, 132 rows, np 160; 3 N_blb = 21
    "J6w": ("fib7", 43, True, "chain_set", 1.0),
    "J7a": ("fib257", 2, True, "chain1", 1.0),            # 2 joints
    "J7b": ("fib257", 2, False, "hinged", 1.0),           # 3 joints
    "J7c": ("fib255", 3, False, "chain1", 1.0),           # 3 joints
    "J7d": ("fib513", 1, True, "chain1", 0.5),            # 1 joint
}


def joint_set(kind, nb, cfg, X, Q):
    if kind == "chain_set":
        return chain_set(nb, X, 33)
    if kind == "hub_set":
        return hub_set(nb, 35)
    if kind == "pivots":
        return pivots(nb, cfg, X, Q, 5)
    return {"chain1": chain1, "hinged": hinged}[kind](nb, cfg, X, 7)


def shape_case(name):
    """-> dict(cfg, X, Q, a, eta, nb, nblb, wall, body, anchor) of a named jointed configuration"""
    import body_shapes as bs
    sh, nb, wall, kind, eta = SHAPE_CASES[name]
    cfg = bs.shape(sh)
    X, Q = bs.lattice(nb, cfg, wall, 0)
    body, anchor = joint_set(kind, nb, cfg, X, Q)
    return {"cfg": cfg, "X": X, "Q": Q, "a": bs.A, "eta": eta, "nb": nb, "nblb": cfg.shape[0], "wall": wall, "body": body,
            "anchor": anchor}


# ---- the cap: 2048 pivots on 2048 trimers whose lattice is spread by CAP_SPREAD, so that the bodies are weakly coupled and the
# iteration count of the first 64 bodies alone stands for the whole (tests/test_joints_shapes_cpu.py checks that on 64 and 256)
CAP_JOINTS, CAP_SPREAD = 2048, 100.0


def cap_case(n_first=None):
    """the cap's configuration above a wall, or its first n_first bodies with their pivots"""
    import body_shapes as bs
    cfg = bs.trimer()
    X, Q = bs.lattice(CAP_JOINTS, cfg, True, 0)
    X[:, :2] *= CAP_SPREAD
    X[:, 2] = X[:, 2].min() + (X[:, 2] - X[:, 2].min()) * CAP_SPREAD          # the lowest layer stays where the lattice put it
    body, anchor = pivots(CAP_JOINTS, cfg, X, Q, 5)
    n = CAP_JOINTS if n_first is None else n_first
    return {"cfg": cfg, "X": X[:n], "Q": Q[:n], "a": bs.A, "eta": bs.ETA, "nb": n, "nblb": 3, "wall": True, "body": body[:n],
            "anchor": anchor[:n]}


def J_apply(X, Q, body, anchor, U):
    """J U by formula, no matrix: (u_A + w_A x l_A) - (u_B + w_B x l_B) per joint, flat (3 n)"""
    body, U = np.asarray(body).reshape(-1, 2), np.asarray(U, dtype=np.float64).reshape(-1, 6)
    lA, lB, _ = geometry(X, Q, body, anchor)
    a, b = body[:, 0], body[:, 1]
    out = U[a, :3] + np.cross(U[a, 3:], lA)
    two = b >= 0
    out[two] -= U[b[two], :3] + np.cross(U[b[two], 3:], lB[two])
    return out.reshape(-1)


def JT_apply(X, Q, body, anchor, phi, nb):
    """J^T phi by formula: the force +-phi_j and the torque l x (+-phi_j) of every joint end on its body, flat (6 nb)"""
    body, phi = np.asarray(body).reshape(-1, 2), np.asarray(phi, dtype=np.float64).reshape(-1, 3)
    lA, lB, _ = geometry(X, Q, body, anchor)
    out = np.zeros((nb, 6))
    np.add.at(out, (body[:, 0], slice(0, 3)), phi)
    np.add.at(out, (body[:, 0], slice(3, 6)), np.cross(lA, phi))
    two = body[:, 1] >= 0
    np.add.at(out, (body[two, 1], slice(0, 3)), -phi[two])
    np.add.at(out, (body[two, 1], slice(3, 6)), -np.cross(lB[two], phi[two]))
    return out.reshape(-1)


def inputs(nb, nblb, nj, seed):
    """random F, slip (0.1 sigma) and joint_rhs, drawn as tests/test_joints_gpu.py's _inputs draws them"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(6 * nb), 0.1 * rng.standard_normal(3 * nb * nblb), rng.standard_normal(3 * nj)


def cap_inputs(n_first=None):
    """the cap's right-hand side, or the part of it that belongs to the first n_first bodies and their pivots"""
    n = CAP_JOINTS if n_first is None else n_first
    F, slip, c = inputs(CAP_JOINTS, 3, CAP_JOINTS, 201)
    return F[:6 * n], slip[:9 * n], c[:3 * n]


# ---- a jointed configuration that gamma = 1 can step: every joint nearly closed ----------------------------------------------
def close_chain(nb, X, Q, seed, open_by):
    """chain_set's bodies and joints (the chain and a pivot on each end body) with every gap of the order open_by, as hinged_chain
    has them: end A's anchor is drawn in +-0.6, end B's is the same lab point seen from body B (a lever of about the lattice
    spacing) or, for a pivot, the lab point itself, displaced by a vector whose entries are +-(0.5 .. 1) open_by -- no gap is zero"""
    rng = np.random.default_rng(seed)
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), unit(Q)
    body = np.array([[i, i + 1] for i in range(nb - 1)] + [[0, -1], [nb - 1, -1]])
    anchor = np.zeros((nb + 1, 6))
    anchor[:, :3] = rng.uniform(-0.6, 0.6, (nb + 1, 3))
    delta = open_by * rng.uniform(0.5, 1.0, (nb + 1, 3)) * rng.choice([-1.0, 1.0], (nb + 1, 3))
    for j, (a, b) in enumerate(body):
        pB = X[a] + rot(Q[a]) @ anchor[j, :3] - delta[j]
        anchor[j, 3:] = rot(Q[b]).T @ (pB - X[b]) if b >= 0 else pB
    return body, anchor


STEP_DT, STEP_STEPS, STEP_OPEN_BY = 0.01, 3, 0.05


def step_case():
    """J1's bodies (100 trimers above a wall, lattice seed 0) on close_chain(seed 7): 101 joints, 303 rows, 6 N_bod > N, and gaps
    that three steps with gamma = 1 close without leaving the lattice"""
    import body_shapes as bs
    cfg = bs.trimer()
    X, Q = bs.lattice(100, cfg, True, 0)
    body, anchor = close_chain(100, X, Q, 7, STEP_OPEN_BY)
    return {"cfg": cfg, "X": X, "Q": Q, "a": bs.A, "eta": bs.ETA, "nb": 100, "nblb": 3, "wall": True, "body": body, "anchor": anchor}
