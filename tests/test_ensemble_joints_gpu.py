"""Hard joints in ensembles (include/rbl.h section 5: rbl_ensemble_solve_jointed / _step_jointed): the jointed saddle solve and
step of every replica in one launch of k_gmres_small_jt, for ball, lock and axis joints.  References: the dense numpy solve on
the oracle's M and K with tests/joint_kinds_oracle.py's rows, the numpy GMRES with the exact preconditioner on the DIAGONAL M~
(block=False: the one-kernel solver's), the numpy restatement of the step, and the single-context RigidBody.  Tolerances are
tests/test_joint_kinds_gpu.py's: two solutions of one system within 1e-7 relative, true residual and |J U - c| / |U| <= 1e-9,
iteration counts within one of the reference GMRES; max_iter = 100 and rtol = 1e-10 unless stated.

Which instantiation <WALL, VLDS> a shape selects, by the launcher's arithmetic (vectors + joint data + Krylov basis <= 150 KB puts
the basis in LDS; the triangular factor R is in LDS up to 64 iterations):
  weld, motors (2 bodies, 2 joints)        20 KB of vectors + 71 KB of basis at max_iter = 100: VLDS, R global
  hinge (3 bodies, 4 joints)               max_iter = 60: 42 KB + 66 KB: VLDS, R in LDS;  max_iter = 100: 30 KB + 109 KB: VLDS, R global
  case_steps' set (3 bodies, 5 joints)     31 KB + 111 KB: VLDS
  hub (9 bodies, 16 joints)                111 KB of vectors, the basis of 336 KB in global memory: <WALL, false>
  cfg 1 chain (10 bodies, 11 joints)       99 KB of vectors, the basis of 357 KB in global memory: <WALL, false>"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_kinds_oracle as jk  # noqa: E402
import joint_oracle as jo  # noqa: E402

BALL, LOCK, AXIS = jk.BALL, jk.LOCK, jk.AXIS
MAXIT, RTOL = 100, 1e-10
# iterations of jo.gmres_right_pc with jk.jointed_pc(..., block=False) at rtol 1e-10: (no wall, wall)
REF_ITERS = {"weld": (29, 30), "hinge": (34, 37), "steps": (37, 37), "hub": (50, 52), "chain": (53, 55)}


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _params():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return cfg, p["sep"] / 2.0


def _ens(X, Q, wall, dt=0.01):
    """an ensemble of the replicas X (R, nb, 3) -- or one, (nb, 3) -- and the dict the oracle helpers take for replica 0"""
    from rigid_body_light_amd import Ensemble
    cfg, a = _params()
    X, Q = np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    if X.ndim == 2:
        X, Q = X[None], Q[None]
    c = dict(cfg=cfg, X=np.array(X[0]), Q=np.array(Q[0]), a=a, eta=1.0)
    return c, Ensemble(cfg, X, Q, a, 1.0, dt, kBT=0.0, wall=wall)


def _inputs(nb, nj, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(6 * nb), 0.1 * rng.standard_normal(3 * nb * 12), rng.standard_normal(3 * nj)


def _reference(orc, c, r, wall, F, slip, crhs, count):
    M, K = jo.dense_matrices(orc, c["cfg"], c["X"], c["Q"], c["a"], c["eta"], wall)
    J = jk.J_matrix(c["X"], c["Q"], r)
    D = jk.D_matrix(c["X"], c["Q"], r, jo.pc_M(M, 12, False), K, 12)
    cp = jk.project(c["X"], c["Q"], r, crhs)
    lam, U, phi = jk.dense_jointed(M, K, J, D, F, slip, cp)
    its = None
    if count:
        A, P = jk.jointed_matrix(M, K, J, D), jk.jointed_pc(M, K, J, D, 12, False)
        its = jo.gmres_right_pc(A, P, jo.rhs_jointed(F, slip, cp), MAXIT, RTOL)[1]
    return lam, U, phi, its, M, K, J, D, cp


def _solve_and_compare(orc, c, ens, r, wall, seed, label, table=None, crhs=None, F=None, max_iter=MAXIT):
    """R = 1: set the joints, solve to 1e-10, hold lambda, U, phi against the dense solve, the count against the table (or, where
    the table has no row, the numpy GMRES run here), the true residual and the constraint"""
    nb, nj = c["X"].shape[0], r["body"].shape[0]
    ens.set_joint_kinds(**r)
    F0, slip, c0 = _inputs(nb, nj, seed)
    F = F0 if F is None else F
    crhs = c0 if crhs is None else crhs
    lam, U, phi, its, res = ens.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=max_iter, rtol=RTOL)
    assert lam.shape == (1, 36 * nb) and U.shape == (1, 6 * nb) and phi.shape == (1, 3 * nj) and its.shape == (1,)
    lam, U, phi, its, res = lam[0], U[0], phi[0], int(its[0]), float(res[0])
    lam_d, U_d, phi_d, its_d, M, K, J, D, cp = _reference(orc, c, r, wall, F, slip, crhs, table is None)
    ref = its_d if table is None else REF_ITERS[table][1 if wall else 0]
    x = np.concatenate([lam, U, phi])
    rr = jk.jointed_matrix(M, K, J, D) @ x - jo.rhs_jointed(F, slip, cp)
    true_res = np.linalg.norm(rr) / np.linalg.norm(jo.rhs_jointed(F, slip, cp))
    cons = np.linalg.norm(J @ U - cp) / np.linalg.norm(U)
    print("%s: %d joints, %d iterations (reference %d), residual %.2e, true %.2e, |J U - c| / |U| %.2e, rel. diff lambda %.2e U %.2e phi %.2e"
          % (label, nj, its, ref, res, true_res, cons, _rel(lam, lam_d), _rel(U, U_d), _rel(phi, phi_d)))
    assert 0 < its < max_iter and res < RTOL
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(phi, phi_d) <= 1e-7
    assert true_res <= 1e-9 and cons <= 1e-9
    assert abs(its - ref) <= 1
    return dict(F=F, slip=slip, c=crhs, cp=cp, lam=lam, U=U, phi=phi, its=its)


# ------------------------------------------------------------------------------------------------ 1: each kind against the dense solve
@pytest.mark.parametrize("wall", [False, True])
def test_a_weld(orc, wall):
    X, Q, r = jk.case_weld()
    c, ens = _ens(X, Q, wall)
    _solve_and_compare(orc, c, ens, r, wall, 11, "weld wall=%s" % wall, table="weld")


@pytest.mark.parametrize("wall", [False, True])
def test_a_weld_keeps_its_bits_where_the_basis_crosses_64_kb_of_lds(wall):
    """the weld's solve with max_iter = 40 and with 100: vectors, joint data and Krylov basis take 54 200 bytes of LDS at 40 and
    93 240 at 100, under and over the 64 KB a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize (the bytes from
    rbl_ensemble_joints_fit, the basis max_iter + 1 vectors of 3 N + 6 N_bod + 3 n_joints).  The solve converges to 1e-10 below
    both caps -- REF_ITERS: the numpy GMRES takes 29 / 30 iterations -- so lambda, U, phi, the counts and the residuals are the
    same bits"""
    import ctypes
    X, Q, r = jk.case_weld()
    _, ens = _ens(X, Q, wall)
    ens.set_joint_kinds(**r)
    caps, total = (40, MAXIT), []
    for m in caps:
        lds = ctypes.c_int64(0)
        assert ens.ctx.L.rbl_ensemble_joints_fit(12, 2, m, 2, ctypes.byref(lds)) == 1
        total.append(lds.value + 8 * (m + 1) * (72 + 12 + 6))
    assert total == [54200, 93240] and total[0] <= 64 * 1024 < total[1] <= 153600
    F, slip, crhs = _inputs(2, 2, 11)
    got = [ens.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=m, rtol=RTOL) for m in caps]
    its, res = int(got[0][3][0]), float(got[0][4][0])
    print("weld wall=%s, max_iter 40 and 100: %d iterations (reference %d), residual %.2e" % (wall, its, REF_ITERS["weld"][wall], res))
    assert 0 < its < caps[0] and abs(its - REF_ITERS["weld"][wall]) <= 1 and res < RTOL
    for p, q in zip(*got):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()


@pytest.mark.parametrize("max_iter", [60, 100])
@pytest.mark.parametrize("wall", [False, True])
def test_a_five_row_hinge_with_the_factor_in_lds_and_in_global_memory(orc, wall, max_iter):
    X, Q, five, _ = jk.case_hinge()
    c, ens = _ens(X, Q, wall)
    s = _solve_and_compare(orc, c, ens, five, wall, 21, "hinge wall=%s max_iter=%d" % (wall, max_iter), table="hinge", max_iter=max_iter)
    assert abs(s["c"][5]) > 1e-2 and s["cp"][5] == 0.0          # ah = (0, 0, 1) exactly: the right-hand side's part along it is ignored
    assert s["phi"].reshape(-1, 3)[1, 2] == 0.0


@pytest.mark.parametrize("wall", [False, True])
def test_the_step_tests_set_of_a_motor_a_hinge_and_a_pivot(orc, wall):
    X, Q, r = jk.case_steps()
    c, ens = _ens(X, Q, wall)
    _solve_and_compare(orc, c, ens, r, wall, 5, "case_steps wall=%s" % wall, table="steps")


@pytest.mark.parametrize("lab", [False, True])
@pytest.mark.parametrize("wall", [False, True])
def test_a_motor_with_the_steps_right_hand_side(orc, wall, lab):
    omega = 0.7
    X, Q, r = jk.case_motor(lab)
    c, ens = _ens(X, Q, wall)
    crhs = jk.step_rhs(X, Q, r, np.zeros(2), [0.0, omega], 1.0, 0.01, np.zeros(6))
    s = _solve_and_compare(orc, c, ens, r, wall, 31, "motor lab=%s wall=%s" % (lab, wall), crhs=crhs, F=np.zeros(12))
    U, ah = s["U"].reshape(2, 6), jk.geometry(X, Q, r)[0][1]
    dw = (0.0 if lab else U[1, 3:]) - U[0, 3:]
    assert np.linalg.norm(dw - omega * ah) <= 1e-9 * omega


@pytest.mark.parametrize("wall", [False, True])
def test_the_cfg1_chain_takes_the_global_basis(orc, wall):
    from rigid_body_light_amd import make_config
    cc = make_config(10, 12, wall)
    body, anchor = jo.chain_set(10, cc["X"], seed=81)
    assert body.shape[0] == 11
    r = jk.rows(body, np.zeros(11, dtype=np.int32), anchor_a=anchor[:, :3], anchor_b=anchor[:, 3:])
    c, ens = _ens(cc["X"], cc["Q"], wall)
    c["a"], c["eta"] = cc["a"], cc["eta"]
    assert c["a"] == _params()[1] and cc["eta"] == 1.0
    _solve_and_compare(orc, c, ens, r, wall, 82, "cfg 1 chain wall=%s" % wall, table="chain")


# ------------------------------------------------------------------------------------------------ 2: the hub
@pytest.mark.parametrize("wall", [False, True])
def test_a_hub_of_nine_bodies_with_sixteen_ends_on_one(orc, wall):
    X, Q, r = jk.case_hub(9)
    assert np.sum(r["body"] == 0) == 16 and sorted(set(r["kind"])) == [BALL, LOCK, AXIS]
    c, ens = _ens(X, Q, wall)
    s = _solve_and_compare(orc, c, ens, r, wall, 42, "hub wall=%s" % wall, table="hub")
    ah, phi = jk.geometry(X, Q, r)[0], s["phi"].reshape(-1, 3)
    along = max(abs(phi[j] @ ah[j]) / np.linalg.norm(phi[j]) for j in np.flatnonzero(r["kind"] == AXIS))
    print("   |phi . ah| / |phi| on the axis joints %.2e" % along)
    assert along <= 8 * np.finfo(float).eps


# ------------------------------------------------------------------------------------------------ 3: the closed two-ball hinge
@pytest.mark.parametrize("wall", [False, True])
def test_a_closed_two_ball_hinge_moves_like_the_five_row_hinge_and_like_the_single_context(wall):
    from rigid_body_light_amd import RigidBody
    X, Q, five, two = jk.case_hinge()
    c, ens = _ens(X, Q, wall)
    F, slip, crhs = _inputs(3, 4, 21)
    crhs[:6] = 0.0                                               # (the two hinges' own rows mean different things)
    ens.set_joint_kinds(**five)
    s5 = ens.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)
    ens.set_joint_kinds(two["body"], None, two["anchor_a"], two["anchor_b"])
    s2 = ens.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)
    rb = RigidBody(c["cfg"], X, Q, c["a"], 1.0, 0.01, wall_PC=wall, block_PC=False)
    rb.set_joints(two["body"], two["anchor_a"], two["anchor_b"])
    s1 = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)
    print("closed hinge wall=%s: five rows %d iterations, two balls %d, single context %d; U vs five %.2e, vs single %.2e; lambda %.2e, %.2e"
          % (wall, s5[3][0], s2[3][0], s1[3], _rel(s2[1][0], s5[1][0]), _rel(s2[1][0], s1[1]), _rel(s2[0][0], s5[0][0]), _rel(s2[0][0], s1[0])))
    assert s5[4][0] < RTOL and s2[4][0] < RTOL and s1[4] < RTOL
    assert _rel(s2[1][0], s5[1][0]) <= 1e-7 and _rel(s2[0][0], s5[0][0]) <= 1e-7
    assert _rel(s2[1][0], s1[1]) <= 1e-7 and _rel(s2[0][0], s1[0]) <= 1e-7


# ------------------------------------------------------------------------------------------------ 4: replicas are independent
def _turned(X, Q, angle, axis, shift):
    q = jk.qrot(angle, jo._unit(axis))
    Rm = jo.rot(q)
    return np.asarray(X) @ Rm.T + shift, np.array([jk.qmul(q, p) for p in jo.unit(Q)])


@pytest.mark.parametrize("wall", [False, True])
def test_every_replica_is_bitwise_the_ensemble_of_that_replica_alone(wall):
    X0, Q0, r = jk.case_steps()
    reps = [(X0, jo.unit(Q0)), _turned(X0, Q0, 0.01, [0.2, 1.0, -0.3], [0.01, -0.005, 0.02]),
            _turned(X0, Q0, -0.015, [1.0, 0.1, 0.4], [-0.008, 0.012, 0.015])]
    X, Q = np.array([p[0] for p in reps]), np.array([p[1] for p in reps])
    rng = np.random.default_rng(61)
    F, slip, crhs = rng.standard_normal((3, 18)), 0.1 * rng.standard_normal((3, 108)), rng.standard_normal((3, 15))
    rates, theta = np.zeros((3, 5)), np.zeros((3, 5))
    rates[:, 1], theta[:, 1] = [0.9, -0.4, 0.3], [0.0, 0.02, -0.03]

    def run(Xs, Qs, sel):
        _, ens = _ens(Xs, Qs, wall)
        ens.set_joint_kinds(**r)
        ens.set_joint_rates(rates[sel])
        ens.set_joint_angles(theta[sel])
        solved = ens.solve_jointed(F[sel], slip=slip[sel], joint_rhs=crhs[sel], max_iter=MAXIT, rtol=RTOL)
        stepped = ens.step_jointed(F[sel], slip=slip[sel], joint_velocity=0.1 * crhs[sel], gamma=0.5, max_iter=MAXIT, rtol=RTOL)
        assert (solved[4] < RTOL).all() and (stepped[2] < RTOL).all()
        return tuple(solved) + tuple(stepped) + tuple(ens.get_config()) + (ens.joint_state()[2],)

    together = run(X, Q, slice(0, 3))
    for k in range(3):
        alone = run(X[k:k + 1], Q[k:k + 1], slice(k, k + 1))
        for p, q in zip(together, alone):
            assert np.asarray(p)[k].tobytes() == np.asarray(q)[0].tobytes()
    assert np.array_equal(together[-1][:, 1], theta[:, 1] + rates[:, 1] * 0.01) and not np.array_equal(together[1][0], together[1][1])


# ------------------------------------------------------------------------------------------------ 5: steps
@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("wall", [False, True])
def test_ten_steps_of_two_replicas_against_the_numpy_restatement(orc, wall, gamma):
    """replica 0 follows tests/test_joint_kinds_gpu.py's protocol: the motor's rate changes sign after five steps, joint_velocity
    pulls the pivot along and asks the hinge for a rate about its free axis, which is ignored; replica 1 the same with other rates"""
    dt, steps = 0.01, 10
    X, Q, r = jk.case_steps()
    rng = np.random.default_rng(51)
    F, slip = rng.standard_normal(18), 0.1 * rng.standard_normal(108)
    v = np.zeros((5, 3))
    v[4] = [0.2, -0.1, 0.3]
    v[3] = 0.4 * jk.geometry(X, Q, r)[0][3] + [0.05, 0.0, -0.02]
    rates = np.zeros((2, steps, 5))
    rates[0, :5, 1], rates[0, 5:, 1] = 0.9, -0.6
    rates[1, :5, 1], rates[1, 5:, 1] = -0.4, 0.7
    c = None
    out = []
    for again in range(2):
        c, ens = _ens(np.array([X, X]), np.array([Q, Q]), wall, dt=dt)
        ens.set_joint_kinds(**r)
        for n in range(steps):
            ens.set_joint_rates(rates[:, n])
            phi, its, res = ens.step_jointed(F, slip=slip, joint_velocity=v, gamma=gamma, max_iter=MAXIT, rtol=RTOL)
            assert phi.shape == (2, 15) and (its > 0).all() and (its < MAXIT).all() and (res < RTOL).all()
        out.append(tuple(ens.get_config()) + tuple(ens.joint_state()))
    for p, q in zip(*out):                                       # a run of steps is repeatable to the bit
        assert p.tobytes() == q.tobytes()
    X1, Q1, gap, _, theta = out[0]
    for k in range(2):
        Xo, Qo, theta_o = jk.numpy_steps(orc, c, r, wall, F, slip, v, gamma, dt, rates[k])
        print("step_jointed wall=%s gamma=%.1f replica %d: |X - X_ref| %.2e, |Q - Q_ref| %.2e, moved %.2e, theta %r"
              % (wall, gamma, k, np.abs(X1[k] - Xo).max(), np.abs(Q1[k] - Qo).max(), np.abs(X1[k] - X).max(), theta[k, 1]))
        assert np.abs(X1[k] - Xo).max() <= 1e-7 and np.abs(Q1[k] - Qo).max() <= 1e-7
        assert np.array_equal(theta[k], theta_o) and theta[k, 1] != 0.0 and not theta[k, [0, 2, 3, 4]].any()
        assert np.abs(X1[k] - X).max() > 1e-3
        assert np.allclose(gap[k], jk.geometry(X1[k], Q1[k], r, theta[k])[1], rtol=0.0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 6: the driven hinge
def test_a_driven_hinge_keeps_its_gaps():
    """tests/test_joint_kinds_gpu.py's conditions: the largest gap of the last five of 40 steps is at most twice that of the
    steps 2 .. 6 (angular and translational), and halving dt divides the angular gap by between 2 and 8"""
    omega, steps = 1.0, 40
    X, Q, r = jk.case_driven()
    F = np.random.default_rng(52).standard_normal(12)
    last = {}
    for dt in (0.01, 0.005):
        _, ens = _ens(X, Q, True, dt=dt)
        ens.set_joint_kinds(**r)
        ens.set_joint_rates([0.0, omega])
        ang, lin = [], []
        for n in range(steps):
            _, its, res = ens.step_jointed(F, gamma=1.0, max_iter=MAXIT, rtol=RTOL)
            assert 0 < its[0] < MAXIT and res[0] < RTOL
            gap, _, theta = ens.joint_state()
            lin.append(np.linalg.norm(gap[0, 0]))
            ang.append(np.linalg.norm(gap[0, 1]))
        print("driven hinge dt=%g: angular gap steps 2-6 max %.3e, last five max %.3e; translational %.3e, %.3e; theta %.17g"
              % (dt, max(ang[1:6]), max(ang[-5:]), max(lin[1:6]), max(lin[-5:]), theta[0, 1]))
        assert max(ang[-5:]) <= 2.0 * max(ang[1:6]) and max(lin[-5:]) <= 2.0 * max(lin[1:6])
        assert abs(theta[0, 1] - omega * steps * dt) <= 1e-15 * steps
        last[dt] = max(ang[-5:])
    assert 2.0 <= last[0.01] / last[0.005] <= 8.0


# ------------------------------------------------------------------------------------------------ 7: the same bits
def _same(p, q):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(p, q))


@pytest.mark.parametrize("wall", [False, True])
def test_ball_joints_by_kind_none_and_by_explicit_zeros(wall):
    from rigid_body_light_amd import make_config
    cc = make_config(10, 12, wall)
    body, anchor = jo.chain_set(10, cc["X"], seed=81)
    F, slip, crhs = _inputs(10, 11, 93)
    out = []
    for kind in (None, np.zeros(11, dtype=np.int32)):
        _, ens = _ens(cc["X"], cc["Q"], wall)
        ens.set_joint_kinds(body, kind, anchor[:, :3], anchor[:, 3:])
        solved = ens.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)
        stepped = ens.step_jointed(F, slip=slip, gamma=0.0, max_iter=MAXIT, rtol=RTOL)
        assert solved[4][0] < RTOL and stepped[2][0] < RTOL
        out.append(tuple(solved) + tuple(stepped) + tuple(ens.get_config()))
    assert _same(*out)


@pytest.mark.parametrize("wall", [False, True])
def test_joints_off_or_never_set_and_the_other_entry_points(wall):
    X, Q, r = jk.case_steps()
    F, slip, _ = _inputs(3, 5, 95)
    nobody = np.zeros(3, dtype=bool)

    def others(ens):
        mixed = ens.solve_mixed([1], F, slip=slip, max_iter=MAXIT, rtol=RTOL)
        det = ens.step_deterministic(F, slip=slip, max_iter=MAXIT, rtol=RTOL)
        return tuple(mixed) + tuple(det) + tuple(ens.get_config())

    def brownian(ens):
        return tuple(ens.step_brownian(F, seed=3, slip=slip, max_iter=MAXIT, rtol=RTOL)) + tuple(ens.get_config())

    _, plain = _ens(X, Q, wall)
    unj = plain.solve_mixed(nobody, F, slip=slip, max_iter=MAXIT, rtol=RTOL)        # bitwise the unmasked one-kernel solve
    ref_step = tuple(plain.step_deterministic(F, slip=slip, max_iter=MAXIT, rtol=RTOL)) + tuple(plain.get_config())
    for state in ("never", "off"):
        _, ens = _ens(X, Q, wall)
        if state == "off":
            ens.set_joint_kinds(**r, on=False)
        lam, U, phi, its, res = ens.solve_jointed(F, slip=slip, max_iter=MAXIT, rtol=RTOL)
        assert phi.shape == (1, 0) and _same((lam, U, its, res), (unj[0], unj[1], unj[3], unj[4]))
        phi, its, res = ens.step_jointed(F, slip=slip, max_iter=MAXIT, rtol=RTOL)
        assert _same((its, res) + tuple(ens.get_config()), ref_step)
    # with joints set and on, every other entry point gives the bits it gives without them
    _, a = _ens(X, Q, wall)
    _, b = _ens(X, Q, wall)
    b.set_joint_kinds(**r)
    b.set_joint_rates([0.0, 0.5, 0.0, 0.0, 0.0])
    assert _same(others(a), others(b))
    from rigid_body_light_amd import Ensemble
    cfg, rad = _params()
    pair = [Ensemble(cfg, X[None], Q[None], rad, 1.0, 0.01, kBT=0.01, wall=wall) for _ in range(2)]
    pair[1].set_joint_kinds(**r)
    assert _same(brownian(pair[0]), brownian(pair[1]))
    assert not b.joint_kinds()["theta"].any() and b.joint_state(phi=False)[1] is None      # no jointed step ran: no motor turned


# ------------------------------------------------------------------------------------------------ 8: a redundant ring
def test_a_redundant_ring_is_refused_and_the_ensemble_serves_a_valid_set_afterwards():
    from rigid_body_light_amd._lib import RblError
    X, Q, body, anchor = jo.redundant_set()
    _, ens = _ens(np.array([X, X]), np.array([Q, Q]), True)
    ens.set_joint_kinds(body, None, anchor[:, :3], anchor[:, 3:])
    F = np.random.default_rng(71).standard_normal(12)
    before = ens.get_config()
    for call in (lambda: ens.solve_jointed(F, max_iter=MAXIT, rtol=RTOL), lambda: ens.step_jointed(F, max_iter=MAXIT, rtol=RTOL)):
        with pytest.raises(RblError, match=r"replica 0.*redundant"):
            call()
    assert _same(before, ens.get_config()) and not ens.joint_state(phi=False)[2].any()
    keep = [0, 4]                                                # one pivot and the joint between the bodies: no loop is left
    ens.set_joint_kinds(body[keep], None, anchor[keep, :3], anchor[keep, 3:])
    lam, U, phi, its, res = ens.solve_jointed(F, max_iter=MAXIT, rtol=RTOL)
    assert (res < RTOL).all() and (its < MAXIT).all() and phi.shape == (2, 6)
    phi, its, res = ens.step_jointed(F, max_iter=MAXIT, rtol=RTOL)
    assert (res < RTOL).all() and not _same(before, ens.get_config())


def test_a_failing_step_turns_no_motor():
    """the redundant ring and, on another pair of bodies, a running motor whose angle is not zero: theta advances when the step
    commits and only then.  The refused step leaves every replica's theta as it was set; the step of a valid set then adds rate dt"""
    from rigid_body_light_amd._lib import RblError
    dt = 0.01
    X2, Q2, body, anchor = jo.redundant_set()
    X, Q = np.concatenate([X2, [[8.0, 0.0, 4.0]]]), np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    ring = jk.rows(body, np.zeros(5, dtype=np.int32), anchor_a=anchor[:, :3], anchor_b=anchor[:, 3:])
    r = jk.concat(ring, jk.motor(X, Q, 1, 2, jk.mid(X, 1, 2), [0.0, 0.0, 1.0]))
    assert list(r["kind"]) == [BALL] * 6 + [LOCK]
    rates, theta = np.zeros((2, 7)), np.zeros((2, 7))
    rates[:, 6], theta[:, 6] = [0.8, -0.5], [0.05, -0.02]
    _, ens = _ens(np.array([X, X]), np.array([Q, Q]), True, dt=dt)
    ens.set_joint_kinds(**r)
    ens.set_joint_rates(rates)
    ens.set_joint_angles(theta)
    F = np.random.default_rng(72).standard_normal(18)
    before = ens.get_config()
    with pytest.raises(RblError, match=r"replica 0.*redundant"):
        ens.step_jointed(F, max_iter=MAXIT, rtol=RTOL)
    assert _same(before, ens.get_config()) and np.array_equal(ens.joint_state(phi=False)[2], theta)
    keep = [0, 4, 5, 6]                                          # a pivot, the joint 0-1 and the motor 1-2: no loop is left
    ens.set_joint_kinds(**{k: v[keep] for k, v in r.items()})
    assert not ens.joint_state(phi=False)[2].any()               # a new set: its angles and rates start at zero
    ens.set_joint_rates(rates[:, keep])
    ens.set_joint_angles(theta[:, keep])
    _, its, res = ens.step_jointed(F, gamma=0.5, max_iter=MAXIT, rtol=RTOL)
    assert (res < RTOL).all() and not _same(before, ens.get_config())
    assert np.array_equal(ens.joint_state()[2], theta[:, keep] + rates[:, keep] * dt)


def test_the_joint_table_follows_a_change_of_the_body_count():
    """rbl_ensemble_set_config with another N_bod at the same R: the device table holds N_bod + 1 row starts, so it is made again;
    solve, step and state are bitwise those of a fresh ensemble of the new shape (angles and rates start at zero in both)"""
    X, Q, r = jk.case_steps()
    X4, Q4 = np.concatenate([X, [X[0] + [0.0, -3.5, 0.5]]]), np.concatenate([jo.unit(Q), [[1.0, 0.0, 0.0, 0.0]]])
    F3, slip3, crhs = _inputs(3, 5, 97)
    F4, slip4, _ = _inputs(4, 5, 98)
    rate = [0.0, 0.6, 0.0, 0.0, 0.0]

    def run(ens):
        ens.set_joint_rates(rate)
        solved = ens.solve_jointed(F4, slip=slip4, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)
        stepped = ens.step_jointed(F4, slip=slip4, gamma=0.5, max_iter=MAXIT, rtol=RTOL)
        assert (solved[4] < RTOL).all() and (stepped[2] < RTOL).all()
        return tuple(solved) + tuple(stepped) + tuple(ens.get_config()) + tuple(ens.joint_state())

    for wall in (False, True):
        _, ens = _ens(X, Q, wall)
        ens.set_joint_kinds(**r)
        ens.set_joint_rates(rate)
        ens.set_joint_angles([0.0, 0.03, 0.0, 0.0, 0.0])
        assert ens.solve_jointed(F3, slip=slip3, joint_rhs=crhs, max_iter=MAXIT, rtol=RTOL)[4][0] < RTOL
        assert ens.step_jointed(F3, slip=slip3, gamma=0.5, max_iter=MAXIT, rtol=RTOL)[2][0] < RTOL
        ens.set_config(X4[None], Q4[None])
        assert ens.N_bodies == 4 and not ens.joint_state(phi=False)[2].any()
        _, fresh = _ens(X4, Q4, wall)
        fresh.set_joint_kinds(**r)
        assert _same(run(ens), run(fresh))


def test_the_state_querys_gaps_are_the_single_contexts():
    """k_ens_jt_geom and the single context's k_jt_geom hold the same statements in two places (rbl_joints_dev.hpp, rbl_joints.hip):
    their gaps on the five bodies of case_mixed5 -- all three kinds and a closed two-ball hinge.  A gap entry is a sum of at most
    four terms no larger than |X| < 16, each rounded once: two correct evaluations differ by less than 8 x eps x 16 / 2 = 1.5e-14"""
    from rigid_body_light_amd import RigidBody
    X, Q, r = jk.case_mixed5()
    c, ens = _ens(X, Q, True)
    ens.set_joint_kinds(**r)
    rb = RigidBody(c["cfg"], X, Q, c["a"], 1.0, 0.01, wall_PC=True, block_PC=False)
    rb.set_joint_kinds(**r)
    rb.solve_jointed(np.ones(30), max_iter=200, rtol=1e-8)      # (the single context's query wants a phi to hand back)
    mine, theirs = ens.joint_state(phi=False)[0][0], rb.joint_state()[0]
    print("gaps of case_mixed5: ensemble against single context, largest difference %.2e (bitwise: %s)"
          % (np.abs(mine - theirs).max(), mine.tobytes() == np.asarray(theirs).tobytes()))
    assert np.abs(X).max() < 16.0 and np.abs(mine - theirs).max() <= 1.5e-14
    assert np.allclose(mine, jk.geometry(X, Q, r)[1], rtol=0.0, atol=1e-12)


def test_sets_and_rates_are_checked_against_the_ensemble():
    from rigid_body_light_amd._lib import RblError
    X, Q, r = jk.case_steps()
    _, ens = _ens(np.array([X, X, X]), np.array([Q, Q, Q]), True)
    ens.set_joint_kinds(**r)
    with pytest.raises(ValueError):
        ens.set_joint_rates(np.zeros((2, 5)))                    # neither (n_joints,) nor (R, n_joints)
    with pytest.raises(RblError, match="sets must be 1 or R"):
        ens.ctx._chk(ens.ctx.L.rbl_ensemble_set_joint_rates(ens.ctx.h, np.zeros(10).ctypes.data, 2))
    with pytest.raises(RblError, match="only a lock joint"):
        ens.set_joint_rates([0.3, 0.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="local to a replica"):
        ens.set_joint_kinds(np.array([[0, 3]]), None, np.zeros(3), np.zeros(3))
    # the library's own refusal of a body index >= N_bod: the set stored past the wrapper's check (the context has no
    # configuration of its own, so rbl_set_joint_kinds stores it), then RBL_ERR_STATE (7) from the three calls, nothing moved
    ens.ctx.set_joint_kinds(np.array([[0, 1], [0, 3]]), np.zeros(2, dtype=np.int32), np.zeros(3), np.zeros(3))
    before = ens.get_config()
    for call in (lambda: ens.solve_jointed(np.zeros(18), max_iter=MAXIT, rtol=RTOL), lambda: ens.step_jointed(np.zeros(18), max_iter=MAXIT, rtol=RTOL)):
        with pytest.raises(RblError, match=r"joint 1 names body 3, a replica has 3 bodies.*status 7"):
            call()
    with pytest.raises(RblError, match=r"ensemble_joint_state: a joint names a body beyond the replica's 3.*status 7"):
        ens.joint_state(phi=False)
    assert _same(before, ens.get_config())


# ------------------------------------------------------------------------------------------------ 9: the force model inside the step
@pytest.mark.parametrize("wall", [False, True])
def test_the_step_adds_the_models_loads_and_the_flows_slip_at_q_n(wall):
    dt = 0.01
    X, Q, r = jk.case_steps()
    _, ens = _ens(np.array([X, X]), np.array([Q, Q]), wall, dt=dt)
    ens.set_joint_kinds(**r)
    ens.set_interactions(w=0.3, eps_blob=2.0, b_blob=0.5, eps_wall=3.0 if wall else 0.0, b_wall=0.4)
    G = np.zeros((3, 3))
    G[0, 2] = 0.4
    ens.set_background_flow(u0=[0.05, 0.0, 0.0] if not wall else [0.0, 0.0, 0.0], G=G)
    rng = np.random.default_rng(81)
    F, slip = rng.standard_normal((2, 18)), 0.1 * rng.standard_normal((2, 108))
    Fm, sm = ens.interaction_forces(), ens.flow_slip()
    assert np.abs(Fm).max() > 1e-3 and np.abs(sm).max() > 1e-3
    _, U, phi, _, res = ens.solve_jointed(F + Fm, slip=slip + sm, max_iter=MAXIT, rtol=RTOL)
    phi_s, its, res_s = ens.step_jointed(F, slip=slip, gamma=0.0, max_iter=MAXIT, rtol=RTOL)
    X1, Q1 = ens.get_config()
    # the whole U of the step from the update it made: X moved by dt u, Q turned by the rotation vector dt w (update_X_Q)
    Us = np.zeros((2, 3, 6))
    Us[:, :, :3] = (X1 - X[None]) / dt
    Q0 = jo.unit(Q)
    for k in range(2):
        for b in range(3):
            Us[k, b, 3:] = jk.rotvec(jk.qmul(Q1[k, b], jk.qconj(Q0[b]))) / dt
    U = U.reshape(2, 3, 6)
    print("force model in the step wall=%s: |U_step - U_solve| / |U| %.2e (translations %.2e, rotations %.2e), phi %.2e"
          % (wall, _rel(Us, U), _rel(Us[:, :, :3], U[:, :, :3]), _rel(Us[:, :, 3:], U[:, :, 3:]), _rel(phi_s, phi)))
    assert (res < RTOL).all() and (res_s < RTOL).all()
    assert _rel(Us, U) <= 1e-7 and _rel(Us[:, :, 3:], U[:, :, 3:]) <= 1e-7 and _rel(phi_s, phi) <= 1e-7


def test_a_set_that_does_not_fit_is_refused_with_the_reason():
    """16 x 12 blobs fit the one-kernel solver at max_iter = 100 and take 12 joints, not the 17 of a chain with two pivots; 19 x 12
    blobs fit at max_iter = 100 and not at 255, joints or none: RBL_ERR_SIZE both times, the two reasons told apart"""
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import RblError
    cc = make_config(16, 12, True)
    body, anchor = jo.chain_set(16, cc["X"], seed=83)
    _, ens = _ens(cc["X"], cc["Q"], True)
    ens.set_joint_kinds(body, None, anchor[:, :3], anchor[:, 3:])
    before = ens.get_config()
    for call in (ens.solve_jointed, ens.step_jointed):
        with pytest.raises(RblError, match=r"without joints, but not with the LDS of 17 joints.*status 4"):
            call(np.zeros(96), max_iter=MAXIT, rtol=RTOL)
    assert _same(before, ens.get_config())
    ens.set_joint_kinds(body[:12], None, anchor[:12, :3], anchor[:12, 3:])
    assert (ens.solve_jointed(np.ones(96), max_iter=MAXIT, rtol=1e-8)[4] < 1e-8).all()
    cc = make_config(19, 12, True)
    _, ens = _ens(cc["X"], cc["Q"], True)
    ens.set_joint_kinds([[0, 1]], None, np.zeros(3), np.zeros(3))
    with pytest.raises(RblError, match=r"beyond the one-kernel solver.*status 4"):
        ens.step_jointed(np.zeros(114), max_iter=255, rtol=RTOL)
    assert (ens.step_jointed(np.ones(114), gamma=0.0, max_iter=MAXIT, rtol=1e-8)[2] < 1e-8).all()
