"""Rigid shapes with no structure file, and the dense reference of a configuration of them: the inputs of
tests/test_body_shapes_cpu.py and tests/test_body_shapes_gpu.py.  A helper -- no test in it.

Every shape is made of touching blobs of radius a (nearest neighbours 2a apart), centred on its mean:
    trimer (3)      equilateral triangle
    tetra (4)       regular tetrahedron
    bipyramid (5)   the trimer and two apices on its axis
    fib(n)          Fibonacci sphere scaled so that the smallest neighbour distance is 2a

CASES names the configurations the tests run, N_bod x shape.  G1-G9 are for the general (multi-launch) solver, S1-S5 are
shapes at the documented limits of the one-kernel solver (N <= 256 blobs, N_bod <= 64), E1-E4 the largest shapes of the
same families that the one-kernel solver does take: besides those two limits its vectors have to fit 150 KB of LDS, which S1, S2
and S4 do not (see small_fits and small_lds_bytes below).
"""
import functools

import numpy as np

A, ETA = 0.5, 1.0


def trimer(a=A):
    r = 2.0 * a / np.sqrt(3.0)
    ang = 2.0 * np.pi * np.arange(3) / 3.0
    return np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(3)], axis=1)


def tetra(a=A):
    return np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * (a / np.sqrt(2.0))


def bipyramid(a=A):
    h = 2.0 * a * np.sqrt(2.0 / 3.0)          # apex to every vertex of the triangle: sqrt(h^2 + (2a / sqrt 3)^2) = 2a
    return np.concatenate([trimer(a), [[0.0, 0.0, h], [0.0, 0.0, -h]]])


def min_distance(pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    best = np.inf
    for i0 in range(0, len(pts), 512):        # blocks of rows: 900 blobs need no 900 x 900 x 3 array at once
        d = np.linalg.norm(pts[i0:i0 + 512, None, :] - pts[None, :, :], axis=2)
        d[np.arange(d.shape[0]), i0 + np.arange(d.shape[0])] = np.inf
        best = min(best, d.min())
    return best


@functools.lru_cache(maxsize=None)
def _fib(n, a):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = np.pi * (1.0 + np.sqrt(5.0)) * k
    s = np.sqrt(1.0 - z * z)
    p = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    p -= p.mean(axis=0)
    return p * (2.0 * a / min_distance(p))


def fib(n, a=A):
    return _fib(int(n), float(a)).copy()


def shape(name, a=A):
    if name.startswith("fib"):
        return fib(int(name[3:]), a)
    return {"trimer": trimer, "tetra": tetra, "bipyramid": bipyramid}[name](a)


def radius(cfg):
    return float(np.linalg.norm(cfg, axis=1).max())


def lattice(n_bodies, cfg, wall, seed=0, a=A):
    """synth.make_config's jittered cubic lattice (x fastest, jitter +-0.1 per coordinate, random unit quaternions) with the spacing
    taken from the shape's own radius R_b, 2 (R_b + a) + 0.5: the bounding spheres of two bodies stay 0.3 apart.  Above a wall
    the lowest layer's centres sit at R_b + a + 0.3 +- 0.1, so the lowest blob clears z = a by 0.2 at least.  -> X, Q"""
    Rb = radius(cfg)
    side = int(np.ceil(n_bodies ** (1.0 / 3.0) - 1e-9))
    spacing = 2.0 * (Rb + a) + 0.5
    idx = np.arange(n_bodies)
    X = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1).astype(np.float64) * spacing
    X += np.random.default_rng(seed).uniform(-0.1, 0.1, X.shape)
    if wall:
        X[:, 2] += Rb + a + 0.2 + 0.1
    Q = np.random.default_rng(seed + 1).standard_normal((n_bodies, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return X, Q


def dense(orc, cfg, X, Q, a, eta, wall):
    """-> M (the oracle's rotne_prager_tensor, damped with orc.damp above a wall), K (oracle.K_matrix), the saddle matrix
    [[M, -K], [K^T, 0]] and the blob positions"""
    from oracle import oracle as onp
    cfg = onp.remove_mean(cfg)
    Qn = onp.normalize_quats(Q)
    r = orc.multi_body_pos(X, Qn, cfg)
    M = np.array(orc.rotne_prager_tensor(r, a, eta, wall))
    if wall:
        B = orc.damp(r, a)
        M = (B[:, None] * M) * B[None, :]
    K = onp.K_matrix(X, Qn, cfg)
    nb6 = K.shape[1]
    return M, K, np.block([[M, -K], [K.T, np.zeros((nb6, nb6))]]), r


def cond2(Amat, n3):
    """2-norm condition number of a saddle matrix [[M, -K], [K^T, 0]] with M of order n3: flipping the sign of its body rows makes
    it symmetric and leaves the singular values alone, which are then the moduli of that matrix's eigenvalues"""
    S = np.array(Amat)
    S[n3:] *= -1.0
    e = np.abs(np.linalg.eigvalsh(S))
    return float(e.max() / e.min())


# name: (shape, N_bod)
CASES = {
    "G1": ("trimer", 300),       # body rows exceed the blob-sized grid
    "G2": ("tetra", 100),
    "G3": ("bipyramid", 90),
    "G4": ("fib7", 43),          # N = 301, odd, small
    "G5": ("fib255", 3),         # N_blb = BT - 1
    "G6": ("fib256", 2),         # N_blb = BT
    "G7": ("fib257", 2),         # N_blb = BT + 1
    "G8": ("fib513", 1),         # one body, three passes of BT
    "G9": ("tetra", 65),         # one past the small solver's body limit
    "S1": ("tetra", 64),         # N = 256 and N_bod = 64 together
    "S2": ("fib256", 1),         # one body of 256 blobs
    "S3": ("trimer", 64),        # most body rows per blob
    "S4": ("fib7", 36),          # N = 252
    "S5": ("trimer", 1),         # smallest solvable system
    "E1": ("tetra", 49),         # the most tetrahedra the one-kernel solver takes at max_iter = 255 (196 blobs)
    "E2": ("fib238", 1),         # the largest single body it takes at max_iter = 255
    "E3": ("fib7", 30),          # the most 7-blob bodies it takes at max_iter = 255 (210 blobs)
    "E4": ("tetra", 51),         # the most tetrahedra it takes at max_iter = 100, with and without prescribed bodies (204 blobs)
}
# eta = 1 everywhere but at G8: one body of 513 blobs has cond(A) = 1.27e4 there, above the cap of 1e4 the inputs have to meet;
# the largest singular value is K's (lever arms up to 7.3), the smallest scales with M, so eta = 0.5 halves it
ETA_OF = {"G8": 0.5}
G_CASES = ["G%d" % i for i in range(1, 10)]
S_CASES = ["S%d" % i for i in range(1, 6)]
E_CASES = ["E1", "E2", "E3", "E4"]


def case(name, wall, seed=0):
    """-> dict(cfg, X, Q, a, eta, nb, nblb) of a named configuration; seed: the lattice's (replicas of an ensemble differ in it)"""
    sh, nb = CASES[name]
    cfg = shape(sh)
    X, Q = lattice(nb, cfg, wall, seed)
    return {"cfg": cfg, "X": X, "Q": Q, "a": A, "eta": ETA_OF.get(name, ETA), "nb": nb, "nblb": cfg.shape[0]}


# the ensembles of the GPU tests: case -> (replicas, max_iter); replica r is the case's lattice with seed 2 r.  S1, S2 and S4 are
# refused by the library (they do not fit the one-kernel solver's LDS); the iteration limits are ones at which the others fit
ENSEMBLES = {"S1": (5, 100), "S2": (3, 100), "S3": (2, 100), "S4": (3, 100), "S5": (300, 100),
             "S3x5": (5, 100), "E1": (6, 255), "E2": (3, 255), "E3": (3, 255), "E4": (2, 100)}


def ensemble_case(name):
    return name[:2]


def replica_seed(r):
    return 2 * r


# ---- the one-kernel solver's size rule (rbl_small.hip: rbl_gmres_small_fits), restated: tests/test_body_shapes_cpu.py holds it
# against the library's own host-side check (rbl_ensemble_set_config refuses what does not fit at max_iter = 1)
SMALL_LDS_MAX = 150 * 1024


def small_lds_bytes(nblb, nb, max_iter, mixed=False):
    N = nblb * nb
    n3, nb6, m = 3 * N, 6 * nb, max_iter
    nsys = n3 + nb6
    return 8 * (2 * n3 + 2 * N + N + 36 * nb + 3 * nsys + nb6 + 3 * (m + 2) + 2 * m + 8 + 16 * n3 + n3 + 6 * N +
                (m * (m + 1) // 2 if m <= 64 else 0) + (nb6 if mixed else 0))


def small_basis_bytes(nblb, nb, max_iter):
    """the Krylov basis: max_iter + 1 vectors; in LDS when it fits beside small_lds_bytes, else in the global workspace"""
    return 8 * (max_iter + 1) * (3 * nblb * nb + 6 * nb)


def small_work_doubles(nblb, nb, max_iter):
    """the global workspace of one replica (rbl_gmres_small_work_doubles): the basis | the packed triangular factor | 8 spare"""
    return (max_iter + 1) * (3 * nblb * nb + 6 * nb) + max_iter * (max_iter + 1) // 2 + 8


def small_fits(nblb, nb, max_iter, mixed=False):
    return nblb * nb <= 256 and nb <= 64 and 1 <= max_iter <= 255 and small_lds_bytes(nblb, nb, max_iter, mixed) <= SMALL_LDS_MAX


# ---- condition numbers of the saddle matrix, cond_2, measured by tests/test_body_shapes_cpu.py with this recipe (a = 0.5, eta = 1)
# and rounded up: the GPU tests' solution bounds, 10 cond(A) rtol, rest on them.  (case, wall) -> the largest over the lattice
# seeds in use (seed 0 for the single configurations, seeds 0 .. 5 for the replicas of an ensemble; S5: the first 8 of 300).
COND_A = {
    ("G1", False): 226,
    ("G1", True): 153,
    ("G2", False): 235,
    ("G2", True): 179,
    ("G3", False): 273,
    ("G3", True): 203,
    ("G4", False): 257,
    ("G4", True): 208,
    ("G5", False): 6.39e+03,
    ("G5", True): 6.39e+03,
    ("G6", False): 6.41e+03,
    ("G6", True): 6.41e+03,
    ("G7", False): 6.44e+03,
    ("G7", True): 6.44e+03,
    ("G8", False): 6.54e+03,
    ("G8", True): 6.54e+03,
    ("G9", False): 198,
    ("G9", True): 156,
    ("S1", False): 200,
    ("S1", True): 164,
    ("S2", False): 6.41e+03,
    ("S2", True): 6.41e+03,
    ("S3", False): 114,
    ("S3", True): 97.7,
    ("S4", False): 242,
    ("S4", True): 197,
    ("S5", False): 63.1,
    ("S5", True): 73.1,
    ("E1", False): 184,
    ("E1", True): 153,
    ("E2", False): 5.95e+03,
    ("E2", True): 5.95e+03,
    ("E3", False): 232,
    ("E3", True): 192,
    ("E4", False): 184,
    ("E4", True): 153,
}


# ---- condition numbers of the JOINTED matrix [M -K 0; K^T 0 J^T; 0 J 0] of tests/joint_oracle.SHAPE_CASES, cond_2, measured by
# tests/test_joints_shapes_cpu.py (joint_oracle.cond_jointed) and rounded up: the solution bounds 10 cond(A) rtol of
# tests/test_joints_shapes_gpu.py rest on them.  The cap on these inputs is 1e5
COND_JOINTED = {
    "J1w": 319,
    "J1f": 394,
    "J2": 720,
    "J3": 461,
    "J4": 218,
    "J5f": 6.07e+03,
    "J5w": 5.03e+03,
    "J6f": 715,
    "J6w": 850,
    "J7a": 5.82e+04,
    "J7b": 3.67e+04,
    "J7c": 1.95e+04,
    "J7d": 2.36e+04,
    "J1s": 3.24e+03,            # joint_oracle.step_case: the largest over the three configurations its reference steps solve at
}
