"""The inputs of tests/test_joints_shapes_gpu.py are sound before any kernel sees them, and the references it trusts are pinned
(tests/joint_oracle.py: SHAPE_CASES, the radius-scaled joint sets, the jointed matrix, its exact preconditioner, the numpy
restatement of the library's GMRES).  No device is touched.

For every case: no gap is zero and no hinge is closed (S is non-singular, no gauge row enters); cond_2 of the dense jointed matrix
is under the cap of 1e5 and is the figure recorded in body_shapes.COND_JOINTED, on which the GPU tests' solution bounds rest; the
smallest Cholesky pivot of the joint Schur complement (joint_oracle.schur_block_pc, for the block and for the diagonal M~) keeps
d^2 / S_ii >= 1e-3, twelve orders above the library's JT_PIVOT_TOL: no case is "redundant" by accident; and the reference
iteration counts at rtol = 1e-10 for the right-hand sides the GPU tests draw are the recorded ones (ITS_REF; +-1: another BLAS may
move the crossing of the threshold by one iteration).  The GPU tests compute their own reference counts; these records show
what they are expected to be and that every case converges well inside max_iter = 200.

Measured here (a = 0.5; eta = 1 but J7d's 0.5): cond(A) 218 .. 5.82e4; pivot ratios 0.040 (J5w, block) .. 0.996; the cap's
lattice (2048 trimers above a wall, spacing times joint_oracle.CAP_SPREAD = 100) needs 28 reference iterations with the diagonal
preconditioner for its first 64 bodies and 28 for its first 256.  At CAP_SPREAD = 10 the counts were 26 and 29, at 30: 27 and 28.
With the block preconditioner the count is small and still grows with the number of bodies at every spread tried (100: 3 and 5,
300: 3 and 4), so the cap case runs with the diagonal one.  The step case (joint_oracle.step_case) is followed through its three
reference steps and stays sound at each."""
import numpy as np
import pytest

import body_shapes as bs
import joint_oracle as jo

COND_CAP = 1e5
PIVOT_MIN = 1e-3
SEED = 101                                                  # of the right-hand sides, here and in tests/test_joints_shapes_gpu.py
# (case, block preconditioner) -> reference iterations at rtol 1e-10 for joint_oracle.inputs(..., SEED)
ITS_REF = {
    ("J1w", True): 27, ("J1w", False): 38, ("J1f", True): 29, ("J1f", False): 40, ("J2", True): 37, ("J2", False): 51,
    ("J3", True): 34, ("J3", False): 45, ("J4", True): 33, ("J4", False): 55, ("J5f", True): 31, ("J5f", False): 49,
    ("J5w", True): 26, ("J5w", False): 53, ("J6f", True): 31, ("J6f", False): 54, ("J6w", True): 29, ("J6w", False): 54,
    ("J7a", True): 22, ("J7a", False): 76, ("J7b", True): 24, ("J7b", False): 81, ("J7c", True): 27, ("J7c", False): 86,
    ("J7d", True): 1, ("J7d", False): 73,
}
CAP_ITS_REF = {64: 28, 256: 28}                             # diagonal preconditioner, joint_oracle.cap_inputs


def _matrices(orc, c):
    M, K = jo.dense_matrices(orc, c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["wall"])
    J = jo.J_matrix(c["X"], c["Q"], c["body"], c["anchor"])
    return M, K, J, jo.jointed_matrix(M, K, J)


def _pivot_ratio(M, K, J, nblb, block):
    S = jo.schur_block_pc(jo.pc_M(M, nblb, block), K, J, nblb)
    L = np.linalg.cholesky(S)
    return float((np.diag(L) ** 2 / np.diag(S)).min())


def _no_hinge_is_closed(c):
    """two joints between one pair of bodies: the distance of their anchors differs between the two bodies (the library's
    JT_HINGE_CLOSED is 1e-6 relative)"""
    body, anchor = c["body"], c["anchor"]
    seen = {}
    for j, (a, b) in enumerate(body):
        if b < 0:
            continue
        k = seen.setdefault((min(a, b), max(a, b)), j)
        if k == j:
            continue
        lA, lB, _ = jo.geometry(c["X"], c["Q"], body[[k, j]], anchor[[k, j]])
        same = body[k, 0] == a
        dA = lA[0] - (lA[1] if same else lB[1])
        dB = lB[0] - (lB[1] if same else lA[1])
        assert np.linalg.norm(dA - dB) > 1e-2 * np.linalg.norm(dA), (j, k)


def test_the_gmres_restatement_keeps_the_library_s_rules():
    rng = np.random.default_rng(3)
    n = 60
    A = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    b = rng.standard_normal(n)
    x, its, res = jo.gmres_right_pc(A, np.linalg.inv(A), b, 50, 1e-10)      # the exact inverse: one iteration
    assert its == 1 and res < 1e-10 and np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)
    P = np.diag(1.0 / np.diag(A))
    x, its, res = jo.gmres_right_pc(A, P, b, 50, 1e-10)
    true = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    assert 1 < its < 50 and res < 1e-10 and abs(true - res) <= 1e-13       # the estimate is the residual (x0 = 0, CGS2)
    x1, its1, res1 = jo.gmres_right_pc(A, P, b, 50, res)                    # "<", strictly: the iteration that only reaches rtol goes on
    assert its1 == its + 1 and res1 < res
    x2, its2, res2 = jo.gmres_right_pc(A, P, b, its - 1, 1e-10)             # max_iter: stops there, unconverged
    assert its2 == its - 1 and res2 >= 1e-10


def test_the_joint_sets_are_what_their_names_say():
    cfg = bs.shape("fib7")
    Rb = bs.radius(cfg)
    X, Q = bs.lattice(6, cfg, True)
    body, anchor = jo.chain1(6, cfg, X, 7)
    assert body.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, -1]]
    assert np.abs(anchor[:5]).max() <= Rb and np.abs(anchor[:5]).max() > 0.6 and np.allclose(anchor[5, 3:], X[0] + Rb * np.array([0.3, 0.4, -0.2]))
    body, anchor = jo.hinged(6, cfg, X, 7)
    assert body.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [1, 0], [5, -1]]
    assert np.allclose(anchor[6, 3:], X[5] + Rb * np.array([0.3, 0.4, -0.2]))
    body, anchor = jo.pivots(6, cfg, X, Q, 5)
    assert body.tolist() == [[i, -1] for i in range(6)]
    gap = jo.geometry(X, Q, body, anchor)[2]
    assert np.abs(gap).max() <= 0.5 and np.linalg.norm(gap, axis=1).min() > 1e-3 and np.abs(anchor[:, :3]).max() <= Rb
    # J by formula is J by matrix
    rng = np.random.default_rng(9)
    for bd, an in (jo.hinged(6, cfg, X, 7), (body, anchor)):
        J = jo.J_matrix(X, Q, bd, an)
        U, phi = rng.standard_normal(36), rng.standard_normal(3 * bd.shape[0])
        assert np.allclose(jo.J_apply(X, Q, bd, an, U), J @ U, rtol=0, atol=1e-13)
        assert np.allclose(jo.JT_apply(X, Q, bd, an, phi, 6), J.T @ phi, rtol=0, atol=1e-13)


def test_the_case_table_has_the_joint_counts_it_claims():
    want = {"J1w": 101, "J1f": 101, "J2": 171, "J3": 300, "J4": 90, "J5f": 101, "J5w": 91, "J6f": 44, "J6w": 44, "J7a": 2, "J7b": 3, "J7c": 3,
            "J7d": 1}
    assert set(want) == set(jo.SHAPE_CASES) == set(bs.COND_JOINTED) - {"J1s"}
    for name, nj in want.items():
        c = jo.shape_case(name)
        assert c["body"].shape == (nj, 2) and c["anchor"].shape == (nj, 6), name
    c = jo.shape_case("J2")
    assert np.sum(c["body"] == 0) == 171 and 3 * 171 > 512                  # all ends on one body; past the Cholesky's panel
    assert 6 * jo.shape_case("J1w")["nb"] > jo.shape_case("J1w")["nb"] * 3   # more body rows than blobs


@pytest.mark.parametrize("name", list(jo.SHAPE_CASES))
def test_inputs_are_sound_and_their_records_hold(orc, name):
    c = jo.shape_case(name)
    nb, nblb, nj = c["nb"], c["nblb"], c["body"].shape[0]
    gaps = np.linalg.norm(jo.geometry(c["X"], c["Q"], c["body"], c["anchor"])[2], axis=1)
    assert gaps.min() > 1e-3                                                # no gap is zero
    _no_hinge_is_closed(c)
    M, K, J, A = _matrices(orc, c)
    np.linalg.cholesky(M)
    cond = jo.cond_jointed(A, M.shape[0], K.shape[1])
    rec = bs.COND_JOINTED[name]
    F, slip, crhs = jo.inputs(nb, nblb, nj, SEED)
    b = jo.rhs_jointed(F, slip, crhs)
    out = []
    for block in (True, False):
        piv = _pivot_ratio(M, K, J, nblb, block)
        x, its, res = jo.gmres_right_pc(A, jo.jointed_pc(M, K, J, nblb, block), b, 200, 1e-10)
        out.append((piv, its))
        assert piv >= PIVOT_MIN, (name, block, piv)
        assert res < 1e-10 and abs(its - ITS_REF[(name, block)]) <= 1, (name, block, its)
        assert np.linalg.norm(A @ x - b) <= 1e-9 * np.linalg.norm(b)
    print("%s %3d x %3d blobs, %3d joints, order %4d: smallest gap %.3f  cond(A) %.4g (recorded %.3g)  pivot ratio block %.3f diagonal %.3f  "
          "reference iterations block %d diagonal %d" % (name, nb, nblb, nj, A.shape[0], gaps.min(), cond, rec, out[0][0], out[1][0], out[0][1], out[1][1]))
    assert cond <= COND_CAP
    assert 0.9 * rec <= cond <= rec <= COND_CAP                             # the record is an upper bound, and not a loose one


def test_the_cap_s_lattice_is_weakly_coupled(orc):
    """the spread of the cap's lattice: the reference iteration counts (diagonal preconditioner) of its first 64 and of its first
    256 bodies differ by at most one, so that the count of the first 64 can stand for all 2048 with a margin of two"""
    counts = {}
    for n in (64, 256):
        c = jo.cap_case(n)
        assert c["X"].shape == (n, 3) and c["body"].tolist() == [[i, -1] for i in range(n)]
        M, K, J, A = _matrices(orc, c)
        r = orc.multi_body_pos(c["X"], jo.unit(c["Q"]), c["cfg"] - c["cfg"].mean(axis=0)).reshape(-1, 3)
        assert r[:, 2].min() > c["a"] + 0.2                                 # above the wall
        if n == 64:
            cond, piv = jo.cond_jointed(A, M.shape[0], K.shape[1]), _pivot_ratio(M, K, J, 3, False)
            print("cap, first 64: cond(A) %.4g, pivot ratio %.3f" % (cond, piv))
            assert cond <= COND_CAP and piv >= PIVOT_MIN
        x, its, res = jo.gmres_right_pc(A, jo.jointed_pc(M, K, J, 3, False), jo.rhs_jointed(*jo.cap_inputs(n)), 200, 1e-10)
        assert res < 1e-10
        counts[n] = its
    print("cap, spread %g: reference iterations %s" % (jo.CAP_SPREAD, counts))
    assert abs(counts[64] - counts[256]) <= 1
    assert all(abs(counts[n] - CAP_ITS_REF[n]) <= 1 for n in counts)
    full = jo.cap_case()
    assert full["body"].shape == (2048, 2) and 3 * 2048 == 6144


def test_the_step_case_stays_sound_while_gamma_1_closes_its_gaps(orc):
    """joint_oracle.step_case, 100 trimers above a wall on a nearly closed chain, through the three reference steps of
    tests/test_joints_shapes_gpu.py (gamma = 1, dt = 0.01): at every configuration the blobs clear z = a by 0.2, blobs of different
    bodies stay more than 2a apart, M is positive definite and cond(A) is the recorded one (the largest of the three solves,
    rounded up; it moves by 2 % along the way).  Measured: gaps 0.049 .. 0.084, then <= 2.6e-3, then <= 8.9e-6; the bodies move by
    0.095, 0.0044 and 0.0025; cond(A) 3181, 3226, 3238."""
    from oracle import oracle as O
    c = jo.step_case()
    nb, nj = c["nb"], c["body"].shape[0]
    assert nj == 101 and 6 * nb > nb * c["nblb"]
    F, slip, _ = jo.inputs(nb, c["nblb"], nj, 42)
    X, Q = np.array(c["X"]), O.normalize_quats(c["Q"])
    owner = np.repeat(np.arange(nb), c["nblb"])
    conds, moves = [], []
    for s in range(jo.STEP_STEPS + 1):
        r = orc.multi_body_pos(X, Q, O.remove_mean(c["cfg"])).reshape(-1, 3)
        d = np.linalg.norm(r[:, None] - r[None], axis=2)
        d[owner[:, None] == owner[None]] = np.inf
        assert r[:, 2].min() > c["a"] + 0.2 and d.min() > 2 * c["a"] + 0.25, (s, r[:, 2].min(), d.min())
        gap = jo.geometry(X, Q, c["body"], c["anchor"])[2]
        if s == 0:
            g = np.linalg.norm(gap, axis=1)
            assert 0.5 * jo.STEP_OPEN_BY < g.min() and g.max() < 2 * jo.STEP_OPEN_BY         # nearly closed, none closed
        if s == jo.STEP_STEPS:
            break
        M, K = jo.dense_matrices(orc, c["cfg"], X, Q, c["a"], c["eta"], True)
        J = jo.J_matrix(X, Q, c["body"], c["anchor"])
        np.linalg.cholesky(M)
        conds.append(jo.cond_jointed(jo.jointed_matrix(M, K, J), M.shape[0], K.shape[1]))
        if s == 0:
            for block in (True, False):
                assert _pivot_ratio(M, K, J, c["nblb"], block) >= PIVOT_MIN
        _, U, _ = jo.dense_jointed(M, K, J, F, slip, -(1.0 / jo.STEP_DT) * gap.reshape(-1))
        Xn, Q = O.evolve(X, Q, U, jo.STEP_DT)
        moves.append(np.abs(Xn - X).max())
        X = Xn
    print("step case: cond(A) %s (recorded %.3g), largest move per step %s, largest gap at the end %.2e"
          % (["%.5g" % v for v in conds], bs.COND_JOINTED["J1s"], ["%.2e" % v for v in moves], np.linalg.norm(gap, axis=1).max()))
    assert moves[0] > 1e-2 and np.linalg.norm(gap, axis=1).max() < 1e-4      # the gaps were there and are closed
    rec = bs.COND_JOINTED["J1s"]
    assert 0.9 * rec <= max(conds) <= rec <= COND_CAP
