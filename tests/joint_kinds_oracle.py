"""numpy restatement of the joint kinds of include/rbl.h section 9 (ball, lock, axis), for the tests: the angular gap e, J with
the angular rows, the sigma ah ah^T block of an axis joint, the dense jointed solve, the exact preconditioner and the step with
the motor angles.  Ball rows, the dense M and K, the preconditioner's M~ and the GMRES are tests/joint_oracle.py's.  Nothing here
calls the library.

A joint set is a dict of rows: body (n, 2), kind (n,), anchor_a, anchor_b (n, 3), axis (n, 3; unit, in body A's frame), q_rel
(n, 4; unit, scalar first) -- the keyword arguments of set_joint_kinds."""
import numpy as np

import joint_oracle as jo

BALL, LOCK, AXIS = 0, 1, 2


def qmul(p, q):
    """Hamilton product, scalar first: R(p q) = R(p) R(q)"""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return np.concatenate([[p[0] * q[0] - p[1:] @ q[1:]], p[0] * q[1:] + q[0] * p[1:] + np.cross(p[1:], q[1:])])


def qconj(q):
    return np.asarray(q, dtype=np.float64) * [1.0, -1.0, -1.0, -1.0]


def qrot(angle, a):
    """the quaternion of a rotation by angle about the unit vector a"""
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * np.asarray(a, dtype=np.float64)])


def rotvec(d):
    """rotation vector of a quaternion, the short way round"""
    d = np.asarray(d, dtype=np.float64)
    if d[0] < 0.0:
        d = -d
    vn = np.linalg.norm(d[1:])
    return np.zeros(3) if vn == 0.0 else 2.0 * np.arctan2(vn, d[0]) / vn * d[1:]


def rows(body, kind, anchor_a=None, anchor_b=None, axis=None, q_rel=None):
    """a joint set from its parts, the missing ones zero (q_rel: the identity), the axes and q_rel normalised"""
    body = np.asarray(body).reshape(-1, 2)
    n = body.shape[0]
    r = dict(body=body, kind=np.asarray(kind, dtype=np.int32).reshape(n))
    for k, v, w in (("anchor_a", anchor_a, 3), ("anchor_b", anchor_b, 3), ("axis", axis, 3), ("q_rel", q_rel, 4)):
        r[k] = np.zeros((n, w)) if v is None else np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (n, w)))
    if q_rel is None:
        r["q_rel"][:, 0] = 1.0
    ang = r["kind"] != BALL
    r["axis"][ang] /= np.linalg.norm(r["axis"][ang], axis=1, keepdims=True)
    r["q_rel"] /= np.linalg.norm(r["q_rel"], axis=1, keepdims=True)
    return r


def concat(*sets):
    return {k: np.concatenate([s[k] for s in sets]) for k in ("body", "kind", "anchor_a", "anchor_b", "axis", "q_rel")}


def anchor6(r):
    return np.concatenate([r["anchor_a"], r["anchor_b"]], axis=1)


def geometry(X, Q, r, theta=None):
    """-> (ah (n, 3): R(Q_A) a of the angular joints, zero for a ball joint; gap (n, 3): p_A - p_B of a ball joint, the angular
    gap e of a lock joint -- the rotation vector of Q_A rot(theta a) q_rel Q_B^-1 -- and P e of an axis joint)"""
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), jo.unit(Q)
    n = r["body"].shape[0]
    theta = np.zeros(n) if theta is None else np.asarray(theta, dtype=np.float64)
    ah, gap = np.zeros((n, 3)), jo.geometry(X, Q, r["body"], anchor6(r))[2]
    for j, (a, b) in enumerate(r["body"]):
        if r["kind"][j] == BALL:
            continue
        ah[j] = jo.rot(Q[a]) @ r["axis"][j]
        th = theta[j] if r["kind"][j] == LOCK else 0.0
        qb = Q[b] if b >= 0 else np.array([1.0, 0.0, 0.0, 0.0])
        e = rotvec(qmul(qmul(qmul(Q[a], qrot(th, r["axis"][j])), r["q_rel"][j]), qconj(qb)))
        gap[j] = e - ah[j] * (ah[j] @ e) if r["kind"][j] == AXIS else e
    return ah, gap


def J_matrix(X, Q, r):
    """(3 n, 6 N_bod): a ball joint's rows are joint_oracle.J_matrix's; a lock joint's w_A - w_B; an axis joint's P (w_A - w_B),
    P = I - ah ah^T"""
    J = jo.J_matrix(X, Q, r["body"], anchor6(r))
    ah = geometry(X, Q, r)[0]
    for j, (a, b) in enumerate(r["body"]):
        if r["kind"][j] == BALL:
            continue
        G = np.eye(3) - (np.outer(ah[j], ah[j]) if r["kind"][j] == AXIS else 0.0)
        J[3 * j:3 * j + 3] = 0.0
        J[3 * j:3 * j + 3, 6 * a + 3:6 * a + 6] = G
        if b >= 0:
            J[3 * j:3 * j + 3, 6 * b + 3:6 * b + 6] = -G
    return J


def project(X, Q, r, c):
    """c with the component along ah taken out of every axis joint's rows"""
    ah = geometry(X, Q, r)[0]
    c = np.array(c, dtype=np.float64).reshape(-1, 3)
    for j in np.flatnonzero(r["kind"] == AXIS):
        c[j] -= ah[j] * (ah[j] @ c[j])
    return c.reshape(-1)


def D_matrix(X, Q, r, Mt, K, nblb):
    """(3 n, 3 n): sigma_j ah ah^T on the diagonal block of every axis joint, sigma_j the mean rotational diagonal entry of
    N_A^-1, N_b = K_b^T Mt_bb^-1 K_b with the preconditioner's Mt (joint_oracle.pc_M)"""
    ah = geometry(X, Q, r)[0]
    n = r["body"].shape[0]
    D = np.zeros((3 * n, 3 * n))
    for j in np.flatnonzero(r["kind"] == AXIS):
        a = r["body"][j, 0]
        s = slice(3 * nblb * a, 3 * nblb * (a + 1))
        Kb = K[s, 6 * a:6 * a + 6]
        Ninv = np.linalg.inv(Kb.T @ np.linalg.solve(Mt[s, s], Kb))
        D[3 * j:3 * j + 3, 3 * j:3 * j + 3] = np.trace(Ninv[3:, 3:]) / 3.0 * np.outer(ah[j], ah[j])
    return D


def jointed_matrix(M, K, J, D):
    """[M -K 0; K^T 0 J^T; 0 J -D]: the operator of the jointed solve with joint kinds"""
    A = jo.jointed_matrix(M, K, J)
    nj3 = J.shape[0]
    A[-nj3:, -nj3:] = -D
    return A


def dense_jointed(M, K, J, D, F, slip, c):
    """numpy.linalg.solve on the matrix above; c already projected -> (lambda, U, phi)"""
    n3, nb6 = M.shape[0], K.shape[1]
    x = np.linalg.solve(jointed_matrix(M, K, J, D), jo.rhs_jointed(F, slip, c))
    return x[:n3], x[n3:n3 + nb6], x[n3 + nb6:]


def jointed_pc(M, K, J, D, nblb, block):
    """the exact right preconditioner: the inverse of the jointed matrix with M replaced by M~.  Its joint Schur complement is
    S = J N^-1 J^T + D: the sigma ah ah^T term the library adds to S"""
    return np.linalg.inv(jointed_matrix(jo.pc_M(M, nblb, block), K, J, D))


def schur(M, K, J, D, nblb, block):
    return jo.schur_block_pc(jo.pc_M(M, nblb, block), K, J, nblb) + D


def step_rhs(X, Q, r, theta, rate, gamma, dt, v):
    """c = -(gamma / dt) gap + v - rate ah on the rows of the lock joints (before the projection)"""
    ah, gap = geometry(X, Q, r, theta)
    c = -(gamma / dt) * gap + np.asarray(v, dtype=np.float64).reshape(-1, 3)
    lock = r["kind"] == LOCK
    c[lock] -= np.asarray(rate, dtype=np.float64)[lock, None] * ah[lock]
    return c.reshape(-1)


def numpy_steps(orc, c, r, wall, F, slip, v, gamma, dt, rates):
    """the step restated: rates (steps, n) -- one row per step.  The dense solve at q^n with step_rhs, the oracle's evolve, then
    theta += rate dt -> (X, Q, theta)"""
    from oracle import oracle as O
    X, Q = np.array(c["X"]), O.normalize_quats(np.asarray(c["Q"], dtype=np.float64))
    theta = np.zeros(r["body"].shape[0])
    for rate in np.asarray(rates, dtype=np.float64):
        M, K = jo.dense_matrices(orc, c["cfg"], X, Q, c["a"], c["eta"], wall)
        J = J_matrix(X, Q, r)
        D = D_matrix(X, Q, r, jo.pc_M(M, c["cfg"].shape[0], True), K, c["cfg"].shape[0])
        crhs = project(X, Q, r, step_rhs(X, Q, r, theta, rate, gamma, dt, v))
        _, U, _ = dense_jointed(M, K, J, D, F, slip, crhs)
        X, Q = O.evolve(X, Q, U, dt)
        theta = theta + rate * dt
    return X, Q, theta


# ---- builders on a configuration: the rows of composed joints, as the library's hinge / weld / motor build them ------------
def _pair(X, Q, a, b, point, axis, kinds):
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), jo.unit(Q)
    RA = jo.rot(Q[a])
    qb = Q[b] if b >= 0 else np.array([1.0, 0.0, 0.0, 0.0])
    point = np.asarray(point, dtype=np.float64)
    r = rows([[a, b]] * len(kinds), kinds, axis=RA.T @ jo._unit(axis), q_rel=qmul(qconj(Q[a]), qb))
    r["anchor_a"][0] = RA.T @ (point - X[a])
    r["anchor_b"][0] = jo.rot(Q[b]).T @ (point - X[b]) if b >= 0 else point
    return r


def hinge(X, Q, a, b, point, axis):
    return _pair(X, Q, a, b, point, axis, [BALL, AXIS])


def weld(X, Q, a, b, point):
    return _pair(X, Q, a, b, point, [0.0, 0.0, 1.0], [BALL, LOCK])


def motor(X, Q, a, b, point, axis):
    return _pair(X, Q, a, b, point, axis, [BALL, LOCK])


def perturbed(r, seed, open_by):
    """the same joints a little open: every ball joint's anchor on B (or lab point) displaced and every q_rel turned by a vector
    whose entries are +-(0.5 .. 1) open_by"""
    rng = np.random.default_rng(seed)
    r = {k: np.array(v) for k, v in r.items()}
    n = r["body"].shape[0]
    d = open_by * rng.uniform(0.5, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    for j in range(n):
        if r["kind"][j] == BALL:
            r["anchor_b"][j] += d[j]
        else:
            w = np.linalg.norm(d[j])
            r["q_rel"][j] = qmul(r["q_rel"][j], qrot(w, d[j] / w))
    return r


# ---- the configurations of the GPU cases (tests/test_joint_kinds_gpu.py), shared with the CPU test of their matrices -------
def spread(nb, z0=3.0, seed=0, identity_first=False):
    """nb bodies on a line along (1, 0.2, 0.1), three units apart (shell_N_12 has radius 1.21), random orientations"""
    rng = np.random.default_rng(100 + seed)
    d = jo._unit([1.0, 0.2, 0.1])
    X = np.array([[0.0, 0.0, z0] + 3.0 * i * d for i in range(nb)])
    Q = jo.unit(rng.standard_normal((nb, 4)))
    if identity_first:
        Q[0] = [1.0, 0.0, 0.0, 0.0]
    return X, Q


def mid(X, a, b, off=(0.1, -0.2, 0.15)):
    return 0.5 * (X[a] + X[b]) + np.asarray(off)


def case_weld():
    """2 bodies welded at a point between them, q_rel a little off the configuration's"""
    X, Q = spread(2, seed=1)
    return X, Q, perturbed(weld(X, Q, 0, 1, mid(X, 0, 1)), 11, 0.05)


def case_hinge():
    """3 bodies: a BALL + AXIS hinge 0-1 about the lab's z, which is body 0's own (its orientation is the identity), a ball joint
    1-2 and a pivot on body 2 -> (X, Q, rows, the same with the hinge as two ball joints half a unit either side on its axis)"""
    X, Q = spread(3, seed=2, identity_first=True)
    p, z = mid(X, 0, 1), np.array([0.0, 0.0, 1.0])
    rest = rows([[1, 2], [2, -1]], [BALL, BALL], anchor_a=[[0.5, 0.1, -0.2], [0.3, 0.2, -0.4]],
                anchor_b=[[-0.3, 0.4, 0.1], X[2] + [0.5, -0.2, 0.6]])
    five = concat(hinge(X, Q, 0, 1, p, z), rest)
    two = concat(_pair(X, Q, 0, 1, p + 0.5 * z, z, [BALL]), _pair(X, Q, 0, 1, p - 0.5 * z, z, [BALL]), rest)
    return X, Q, five, two


def case_motor(lab):
    """a 2-body motor between the bodies 0 and 1, or body 0 driven against the lab (body 1 free beside it)"""
    X, Q = spread(2, seed=3)
    ax = [0.3, -0.5, 0.8]
    return X, Q, motor(X, Q, 0, -1 if lab else 1, X[0] + [0.4, 0.2, -0.3] if lab else mid(X, 0, 1), ax)


def case_mixed42():
    """4 shell_N_42 bodies: a weld 0-1, a hinge 1-2 with the bodies named [2, 1], a motor 3-lab and a ball joint 2-3"""
    X, Q = spread(4, z0=4.0, seed=4)
    r = concat(weld(X, Q, 0, 1, mid(X, 0, 1)), hinge(X, Q, 2, 1, mid(X, 1, 2), [0.2, 0.9, -0.4]),
               motor(X, Q, 3, -1, X[3] + [0.3, 0.3, 0.5], [1.0, 0.1, 0.2]),
               rows([[2, 3]], [BALL], anchor_a=[[0.4, 0.1, 0.2]], anchor_b=[[-0.5, 0.2, 0.1]]))
    return X, Q, perturbed(r, 12, 0.05)


def case_mixed5():
    """the four bodies and seven joints of case_mixed42 and a fifth body on a closed two-ball hinge to body 0, its second joint
    named [4, 0]: the ball joint's own special case -- mates, the redundant row and its eigenvalue -- inside a set with angular
    joints.  The dense matrix is singular by construction (that row): no dense reference, the bits are what is compared"""
    X, Q = spread(5, z0=4.0, seed=4)
    X4, Q4, r = case_mixed42()
    assert np.array_equal(X[:4], X4) and np.array_equal(Q[:4], Q4)
    X[4] = X[0] + [0.3, 3.2, 0.4]
    p, ax = mid(X, 0, 4), jo._unit([0.5, 0.1, 1.0])
    one, two = _pair(X, Q, 0, 4, p + 0.5 * ax, ax, [BALL]), _pair(X, Q, 4, 0, p - 0.5 * ax, ax, [BALL])
    return X, Q, concat(r, one, two)


def case_hub(nb=36):
    """a hub: body 0 carries a ball joint and an angular joint to every other body (lock and axis alternating, every third pair
    named with the hub second): 2 (nb - 1) = 70 ends on body 0.  Bodies on a 6 x 6 lattice, 3.5 apart"""
    rng = np.random.default_rng(105)
    X = np.array([[3.5 * (i % 6), 3.5 * (i // 6), 3.0 + 0.3 * ((i * 7) % 5)] for i in range(nb)])
    Q = jo.unit(rng.standard_normal((nb, 4)))
    sets = []
    for i in range(1, nb):
        a, b = (0, i) if i % 3 else (i, 0)
        p, ax = X[i] + rng.uniform(-0.5, 0.5, 3), rng.standard_normal(3)
        sets.append(weld(X, Q, a, b, p) if i % 2 else hinge(X, Q, a, b, p, ax))
    return X, Q, perturbed(concat(*sets), 13, 0.05)


def case_steps():
    """3 bodies for the step tests: a motor 0-1, a hinge 1-2 across, a pivot on body 0; every joint open by about 0.01"""
    X, Q = spread(3, seed=5)
    d = jo._unit([1.0, 0.2, 0.1])
    e = jo._unit(np.cross(d, [0.0, 0.0, 1.0]))
    X[2] = X[1] + 3.0 * e
    r = concat(motor(X, Q, 0, 1, mid(X, 0, 1, (0.0, 0.0, 0.0)), e), hinge(X, Q, 1, 2, mid(X, 1, 2, (0.0, 0.0, 0.0)), np.cross(e, d)),
               _pair(X, Q, 0, -1, X[0] + [-0.2, 0.3, 0.5], e, [BALL]))
    return X, Q, perturbed(r, 14, 0.01)


def case_driven():
    """2 bodies, a driven hinge between them, closed at the start"""
    X, Q = spread(2, seed=6)
    return X, Q, motor(X, Q, 0, 1, mid(X, 0, 1, (0.0, 0.0, 0.0)), [0.1, 0.3, 1.0])
