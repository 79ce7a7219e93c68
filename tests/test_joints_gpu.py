"""Hard joints (include/rbl.h section 9) on the GPU: ball joints and pivots as constraints of the saddle solve.  Dense numpy
solutions of the 3 N + 6 N_bod + 3 N_j system on the oracle's M and K (tests/joint_oracle.py, whose J is pinned by
tests/test_joints_cpu.py), the residual through the public operators, the sign of phi, shapes away from the easy ones, the step
against a numpy restatement, joints off, a redundant loop, reproducibility.  Tolerances are those of tests/test_prescribed_gpu.py:
solves to rtol 1e-10 within 200 iterations, two solutions of one system within 1e-7, true residual below 1e-9 of the
right-hand side.

Iterations are printed by every test (run with -s) and asserted here only as "converged within max_iter"; the counts of the probe
set, the chain of forty and the hub are held against a reference GMRES, with larger joint sets and other body shapes, in
tests/test_joints_shapes_gpu.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_oracle as jo  # noqa: E402

WALL_BLOCK = [(False, False), (False, True), (True, False), (True, True)]


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _body(nb, nblb, wall, block, dt=0.01):
    from rigid_body_light_amd import RigidBody, make_config
    c = make_config(nb, nblb, wall)
    return c, RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt, wall_PC=wall, block_PC=block)


def _inputs(nb, nblb, nj, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(6 * nb), 0.1 * rng.standard_normal(3 * nb * nblb), rng.standard_normal(3 * nj)


def _solve_and_compare(orc, c, rb, body, anchor, wall, seed, label):
    """set the joints, solve with random F, slip and joint_rhs to 1e-10, compare with the dense solve -> everything a caller may
    want to look at further"""
    nb, nblb = c["X"].shape[0], c["cfg"].shape[0]
    nj = body.shape[0]
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    F, slip, crhs = _inputs(nb, nblb, nj, seed)
    lam, U, phi, its, res = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    M, K = jo.dense_matrices(orc, c["cfg"], c["X"], c["Q"], c["a"], c["eta"], wall)
    J = jo.J_matrix(c["X"], c["Q"], body, anchor)
    gaps = np.linalg.norm(jo.geometry(c["X"], c["Q"], body, anchor)[2], axis=1)
    lam_d, U_d, phi_d = jo.dense_jointed(M, K, J, F, slip, crhs)
    print("%s: %d joints, smallest gap %.3f, %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e phi %.2e"
          % (label, nj, gaps.min(), its, res, _rel(lam, lam_d), _rel(U, U_d), _rel(phi, phi_d)))
    assert gaps.min() > 1e-3                                   # no gap is zero
    assert phi.shape == (3 * nj,) and 0 < its < 200 and res < 1e-10
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(phi, phi_d) <= 1e-7
    return dict(F=F, slip=slip, c=crhs, lam=lam, U=U, phi=phi, J=J, its=its, res=res)


# ------------------------------------------------------------------------------------------------------------ 1: dense parity
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_dense_parity_and_residual_through_the_public_operators(orc, wall, block):
    c, rb = _body(4, 12, wall, block)
    body, anchor = jo.probe_set(c["cfg"], c["X"])
    s = _solve_and_compare(orc, c, rb, body, anchor, wall, seed=31, label="probe set wall=%s block=%s" % (wall, block))
    # the residual of the three blocks through apply_saddle and a numpy J rebuilt from get_config
    X, Q = rb.get_config()
    J = jo.J_matrix(X, Q, body, anchor)
    n3 = s["lam"].size
    top = rb.apply_saddle(np.concatenate([s["lam"], s["U"]]))
    r = np.concatenate([top[:n3] - s["slip"], top[n3:] + J.T @ s["phi"] + s["F"], J @ s["U"] - s["c"]])
    true_res = np.linalg.norm(r) / np.linalg.norm(np.concatenate([s["slip"], s["F"], s["c"]]))
    print("   true residual %.2e" % true_res)
    assert true_res <= 1e-9


# ------------------------------------------------------------------------------------------------------------ 2: sign, consistency
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_phi_is_a_load_in_the_convention_of_F_body(orc, wall, block):
    c, rb = _body(4, 12, wall, block)
    body, anchor = jo.probe_set(c["cfg"], c["X"])
    s = _solve_and_compare(orc, c, rb, body, anchor, wall, seed=32, label="sign wall=%s block=%s" % (wall, block))
    X, Q = rb.get_config()
    J = jo.J_matrix(X, Q, body, anchor)
    x, its0, res0 = rb.solve_saddle(np.concatenate([s["slip"], -(s["F"] + J.T @ s["phi"])]), max_iter=200, rtol=1e-10)
    n3 = s["lam"].size
    cons = np.linalg.norm(J @ s["U"] - s["c"]) / np.linalg.norm(s["U"])
    print("   solve_saddle with F + J^T phi: %d iterations, rel. diff lambda %.2e U %.2e; |J U - c| / |U| %.2e"
          % (its0, _rel(x[:n3], s["lam"]), _rel(x[n3:], s["U"]), cons))
    assert res0 < 1e-10 and _rel(x[:n3], s["lam"]) <= 1e-7 and _rel(x[n3:], s["U"]) <= 1e-7
    assert cons <= 1e-9
    # the load on body 0 is joint 0's force at its anchor there: +phi_0 and the torque l_A x phi_0
    lA = jo.geometry(X, Q, body, anchor)[0]
    load = (J.T @ s["phi"]).reshape(-1, 6)[0]
    assert np.allclose(load[:3], s["phi"][:3], rtol=1e-14) and np.allclose(load[3:], np.cross(lA[0], s["phi"][:3]), rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------ 3: shapes
def test_a_chain_of_forty_with_two_pivots(orc):
    """41 joints: 123 joint rows, no multiple of 16 or 64; the padded Schur complement has 128"""
    c, rb = _body(40, 12, True, True)
    body, anchor = jo.chain_set(40, c["X"], seed=33)
    assert body.shape[0] == 41
    _solve_and_compare(orc, c, rb, body, anchor, True, seed=34, label="chain of 40, wall, block")


@pytest.mark.parametrize("wall,block", [(False, True), (True, False)])
def test_a_hub_with_more_than_sixty_four_ends_on_one_body(orc, wall, block):
    c, rb = _body(71, 12, wall, block)
    body, anchor = jo.hub_set(71, seed=35)
    assert np.sum(body == 0) == 70
    _solve_and_compare(orc, c, rb, body, anchor, wall, seed=36, label="hub of 71 wall=%s block=%s" % (wall, block))


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_three_larger_shells_with_a_hinge_and_a_pivot(orc, wall, block):
    c, rb = _body(3, 42, wall, block)
    rng = np.random.default_rng(37)
    body = np.array([[0, 1], [1, 2], [2, 1], [0, -1]])
    anchor = rng.uniform(-0.6, 0.6, (4, 6))
    anchor[0, :3], anchor[2, 3:] = jo.blob(c["cfg"], 5), jo.blob(c["cfg"], 17)
    anchor[3, 3:] = c["X"][0] + [0.4, -0.3, 0.5]
    _solve_and_compare(orc, c, rb, body, anchor, wall, seed=38, label="3 x shell_N_42 wall=%s block=%s" % (wall, block))


# ------------------------------------------------------------------------------------------------------------ 4: the step
MODEL = dict(w=0.2, eps_wall=1.0, b_wall=0.1, eps_blob=0.0, b_blob=0.1)      # weight and the wall term


def _chain_body(wall, block, dt, model, seed=41):
    from rigid_body_light_amd import RigidBody, load_structure
    p, cfg = load_structure(12)
    X, Q, body, anchor = jo.hinged_chain(seed)
    rb = RigidBody(cfg, X, Q, p["sep"] / 2.0, 1.0, dt, wall_PC=wall, block_PC=block)
    if model:
        rb.set_interactions(**MODEL)
        rb.set_bonds([[0, 2]], [0.3, 0.0, 0.2], [-0.1, 0.4, 0.0], 2.0, 4.0)
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    return dict(cfg=cfg, X=X, Q=Q, a=p["sep"] / 2.0, eta=1.0), rb, body, anchor


def _numpy_steps(orc, c, body, anchor, wall, F, slip, v, gamma, dt, steps, loads=None):
    """the step restated: the dense jointed solve with c = -(gamma / dt) gap + v at q^n, then the oracle's evolve.  loads(X, Q):
    the force model's share of the body loads at q^n, reference convention (None: no model)"""
    from oracle import oracle as O
    X, Q = np.array(c["X"]), O.normalize_quats(np.asarray(c["Q"], dtype=np.float64))
    for _ in range(steps):
        M, K = jo.dense_matrices(orc, c["cfg"], X, Q, c["a"], c["eta"], wall)
        J = jo.J_matrix(X, Q, body, anchor)
        gap = jo.geometry(X, Q, body, anchor)[2].reshape(-1)
        Ft = F if loads is None else F + loads(X, Q)
        _, U, _ = jo.dense_jointed(M, K, J, Ft, slip, -(gamma / dt) * gap + v)
        X, Q = O.evolve(X, Q, U, dt)
    return X, Q


@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("wall,block,model", [(False, False, False), (False, True, False), (True, True, False), (True, False, True),
                                              (True, True, True)])
def test_ten_steps_against_the_numpy_restatement(orc, wall, block, model, gamma):
    dt, steps = 0.01, 10
    c, rb, body, anchor = _chain_body(wall, block, dt, model)
    rng = np.random.default_rng(42)
    F, slip = rng.standard_normal(18), 0.1 * rng.standard_normal(108)
    v = np.zeros(12)
    v[3:6] = [0.2, -0.1, 0.3]                                   # one joint is being pulled apart at this rate
    loads = None
    if model:                                                    # the model's loads from a second context moved to the reference's q^n
        _, ref, _, _ = _chain_body(wall, block, dt, model)

        def loads(X, Q):
            ref.set_config(X, Q)
            return np.asarray(ref.interaction_forces()).reshape(-1)
        assert np.abs(loads(c["X"], c["Q"])).max() > 1e-3
    Xo, Qo = _numpy_steps(orc, c, body, anchor, wall, F, slip, v, gamma, dt, steps, loads)
    its_all = []
    for _ in range(steps):
        phi, its, res = rb.step_jointed(F, slip=slip, joint_velocity=v.reshape(-1, 3), gamma=gamma, max_iter=200, rtol=1e-10)
        assert 0 < its < 200 and res < 1e-10 and phi.shape == (12,)
        its_all.append(its)
    X1, Q1 = rb.get_config()
    print("step_jointed wall=%s block=%s model=%s gamma=%.1f: iterations %s; |X - X_ref| %.2e, |Q - Q_ref| %.2e, moved %.2e"
          % (wall, block, model, gamma, its_all, np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max(), np.abs(X1 - c["X"]).max()))
    assert np.abs(X1 - Xo).max() <= 1e-7 and np.abs(Q1 - Qo).max() <= 1e-7
    assert np.abs(X1 - c["X"]).max() > 1e-3                       # it did move


def test_the_relaxation_closes_the_gaps_the_plain_constraint_leaves_open():
    dt, steps = 0.01, 50
    F = np.random.default_rng(43).standard_normal(18)
    largest = {}
    for gamma in (1.0, 0.0):
        _, rb, body, anchor = _chain_body(True, True, dt, False)
        for _ in range(steps):
            _, its, res = rb.step_jointed(F, gamma=gamma, max_iter=200, rtol=1e-10)
            assert 0 < its < 200 and res < 1e-10
        gap, _ = rb.joint_state()
        X, Q = rb.get_config()
        assert np.allclose(gap, jo.geometry(X, Q, body, anchor)[2], rtol=0.0, atol=1e-12)
        largest[gamma] = np.linalg.norm(gap, axis=1).max()
    print("largest gap after %d steps of dt = %g: gamma = 1: %.3e, gamma = 0: %.3e" % (steps, dt, largest[1.0], largest[0.0]))
    assert largest[1.0] < largest[0.0]


# ------------------------------------------------------------------------------------------------------------ 5: joints off
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_joints_off_is_the_plain_solve_and_step_and_joints_on_changes_no_other_call(wall, block):
    nb, nblb = 10, 12
    c, _ = _body(nb, nblb, wall, block)
    body, anchor = jo.chain_set(nb, c["X"], seed=51)
    F, slip, _ = _inputs(nb, nblb, 1, seed=52)
    out = {}
    for state in ("never", "off", "on"):
        _, rb = _body(nb, nblb, wall, block)
        if state != "never":
            rb.set_joints(body, anchor[:, :3], anchor[:, 3:], on=state == "on")
        x, its0, res0 = rb.solve_saddle(np.concatenate([slip, -F]), max_iter=200, rtol=1e-10)
        mixed = rb.solve_mixed([1, 4], F, slip=slip, max_iter=200, rtol=1e-10)
        if state != "on":
            lam, U, phi, its, res = rb.solve_jointed(F, slip=slip, max_iter=200, rtol=1e-10)
            n3 = lam.size
            print("joints %s wall=%s block=%s: solve_jointed %d iterations, solve_saddle %d; rel. diff lambda %.2e U %.2e"
                  % (state, wall, block, its, its0, _rel(lam, x[:n3]), _rel(U, x[n3:])))
            assert phi.size == 0 and res < 1e-10 and _rel(lam, x[:n3]) <= 1e-7 and _rel(U, x[n3:]) <= 1e-7
            _, rb2 = _body(nb, nblb, wall, block)
            if state == "off":
                rb2.set_joints(body, anchor[:, :3], anchor[:, 3:], on=False)
            phi2, its2, _ = rb2.step_jointed(F, slip=slip, max_iter=200, rtol=1e-10)
            assert phi2.size == 0 and its2 > 0
            stepped = rb2.get_config()
        its_s, res_s = rb.step_deterministic(F, slip=slip, max_iter=200, rtol=1e-10)
        Xs, Qs = rb.get_config()
        if state != "on":
            assert np.abs(Xs - stepped[0]).max() <= 1e-7 and np.abs(Qs - stepped[1]).max() <= 1e-7
        out[state] = (x, its0, res0) + tuple(mixed) + (its_s, res_s, Xs, Qs)
    for state in ("off", "on"):                                  # bitwise what they are on a context without joints
        for p, q in zip(out["never"], out[state]):
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), state


# ------------------------------------------------------------------------------------------------------------ 6: a redundant loop
@pytest.mark.parametrize("block", [False, True])
def test_a_redundant_loop_is_reported_and_the_context_goes_on(orc, block):
    from rigid_body_light_amd import RigidBody, load_structure
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    X, Q, body, anchor = jo.redundant_set()
    M, K = jo.dense_matrices(orc, cfg, X, Q, a, 1.0, False)
    S = jo.schur_block_pc(M if block else np.diag(np.diag(M)), K, jo.J_matrix(X, Q, body, anchor), 12)
    ev = np.linalg.eigvalsh(S)
    print("reference S: smallest eigenvalues %s, largest %.3f" % (np.array2string(ev[:3], precision=2), ev[-1]))
    assert ev[0] <= 0.0                                           # singular in numpy: exactly, not nearly
    rb = RigidBody(cfg, X, Q, a, 1.0, 0.01, wall_PC=False, block_PC=block)
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    F = np.random.default_rng(61).standard_normal(12)
    with pytest.raises(RuntimeError, match="redundant") as e:
        rb.solve_jointed(F, max_iter=200, rtol=1e-10)
    assert "not positive definite" in str(e.value)
    X0, Q0 = (np.array(v) for v in rb.get_config())
    with pytest.raises(RuntimeError, match="redundant"):
        rb.step_jointed(F, max_iter=200, rtol=1e-10)
    X1, Q1 = rb.get_config()
    assert np.array_equal(X0, X1) and np.array_equal(Q0, Q1)     # a failed step does not advance
    with pytest.raises(RuntimeError, match="no jointed solve"):
        rb.joint_state()
    # a valid set on the same context: one pivot a body and the joint, its anchors taken off the common line (on it the joint's
    # row along the line would still say 0 = 0: a point on the line through a pivot never moves along it)
    keep = [0, 2, 4]
    body, anchor = body[keep], anchor[keep].copy()
    anchor[2, 1], anchor[2, 5] = 0.5, 0.5
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    lam, U, phi, its, res = rb.solve_jointed(F, max_iter=200, rtol=1e-10)
    J = jo.J_matrix(X, Q, body, anchor)
    lam_d, U_d, phi_d = jo.dense_jointed(M, K, J, F, np.zeros(M.shape[0]), np.zeros(9))
    print("   afterwards: %d iterations, rel. diff U %.2e phi %.2e" % (its, _rel(U, U_d), _rel(phi, phi_d)))
    assert 0 < its < 200 and res < 1e-10 and _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(phi, phi_d) <= 1e-7


@pytest.mark.parametrize("block", [False, True])
def test_a_hinge_to_the_lab_is_expected_redundancy_and_solves(orc, block):
    """two pivots on one body hold the distance between their anchors twice: the one redundant row a hinge always has.  The solve
    goes through, the body turns about the line through the pivots and nothing else, and lambda and U are those of the
    minimum-norm solution of the (singular, consistent) dense system"""
    from rigid_body_light_amd import RigidBody, load_structure
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    X, Q, body, anchor = jo.redundant_set()
    body, anchor = body[:2], anchor[:2]                           # body 0 on its two pivots, body 1 free beside it
    rb = RigidBody(cfg, X, Q, a, 1.0, 0.01, wall_PC=False, block_PC=block)
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    F = np.random.default_rng(62).standard_normal(12)
    lam, U, phi, its, res = rb.solve_jointed(F, max_iter=200, rtol=1e-10)
    M, K = jo.dense_matrices(orc, cfg, X, Q, a, 1.0, False)
    J = jo.J_matrix(X, Q, body, anchor)
    n3 = M.shape[0]
    A = np.zeros((n3 + 12 + 6,) * 2)
    A[:n3, :n3], A[:n3, n3:n3 + 12], A[n3:n3 + 12, :n3] = M, -K, K.T
    A[n3:n3 + 12, n3 + 12:], A[n3 + 12:, n3:n3 + 12] = J.T, J
    x = np.linalg.lstsq(A, np.concatenate([np.zeros(n3), -F, np.zeros(6)]), rcond=1e-12)[0]
    print("lab hinge block=%s: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e, U of the hinged body %s"
          % (block, its, res, _rel(lam, x[:n3]), _rel(U, x[n3:n3 + 12]), np.array2string(U[:6], precision=4)))
    assert 0 < its < 200 and res < 1e-10
    assert _rel(lam, x[:n3]) <= 1e-7 and _rel(U, x[n3:n3 + 12]) <= 1e-7
    assert np.abs(U[[0, 1, 2, 4, 5]]).max() <= 1e-9 * np.abs(U).max() and abs(U[3]) > 1e-3      # it turns about x, the pivots' line
    load = (J.T @ phi).reshape(2, 6)
    assert np.abs(load[1]).max() == 0.0 and np.abs(load[0]).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------ 7: the same bits
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_two_calls_give_the_same_bits_and_the_state_query_returns_them(wall, block):
    nb, nblb = 10, 12
    c, rb = _body(nb, nblb, wall, block)
    body, anchor = jo.chain_set(nb, c["X"], seed=71)
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    j = rb.joints()
    assert j["on"] and np.array_equal(j["body"], body) and np.array_equal(j["anchor_a"], anchor[:, :3]) and np.array_equal(j["anchor_b"], anchor[:, 3:])
    F, slip, crhs = _inputs(nb, nblb, body.shape[0], seed=72)
    with pytest.raises(RuntimeError, match="no jointed solve"):
        rb.joint_state()
    first = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    second = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    _, rb2 = _body(nb, nblb, wall, block)
    rb2.set_joints(body, anchor[:, :3], anchor[:, 3:])
    third = rb2.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    for p, q, r in zip(first, second, third):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes() == np.asarray(r).tobytes()
    gap, phi = rb.joint_state()
    assert gap.shape == phi.shape == (body.shape[0], 3) and np.array_equal(phi.reshape(-1), first[2])
    assert np.allclose(gap, jo.geometry(c["X"], c["Q"], body, anchor)[2], rtol=0.0, atol=1e-13)
    # a step moves the bodies: the gaps follow the configuration, phi is the step's
    phi_s, its, res = rb.step_jointed(F, slip=slip, gamma=0.0, max_iter=200, rtol=1e-10)
    gap2, phi2 = rb.joint_state()
    X, Q = rb.get_config()
    assert np.array_equal(phi2.reshape(-1), phi_s) and np.allclose(gap2, jo.geometry(X, Q, body, anchor)[2], rtol=0.0, atol=1e-13)
    assert np.abs(gap2 - gap).max() > 0.0
    rb.set_joints(body[:3], anchor[:3, :3], anchor[:3, 3:])          # another joint set: its phi does not exist yet
    with pytest.raises(RuntimeError, match="no jointed solve"):
        rb.joint_state()


# The second shape, 17 x shell_N_162 = 2754 blobs: a blob vector is 66 096 bytes, the smallest from the shipped structures above the
# 64 KB at which the host form's copies go through the staging buffer, synchronously; below it (10 x 12) both forms copy
# asynchronously.  Iterations to 1e-8 there, before the two forms shared their code and since: 24 with the joints, 13 with
# them off (printed; max_iter 200 is more than twice the larger and below 254).
def _device_form_gives_the_host_form_s_bits(ctx, c, nb, nblb, max_iter, rtol):
    import torch
    body, anchor = jo.chain_set(nb, c["X"], seed=81)
    ctx.set_joints(body, anchor[:, :3], anchor[:, 3:])
    j = ctx.joints()
    assert j["on"] and np.array_equal(j["body"], body) and np.array_equal(j["anchor_b"], anchor[:, 3:])
    F, slip, crhs = _inputs(nb, nblb, body.shape[0], seed=82)
    lam, U, phi, its, res = ctx.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=max_iter, rtol=rtol)
    dev = [torch.tensor(v, dtype=torch.float64, device="cuda:0") for v in (F, slip, crhs)]
    out = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0") for n in (lam.size, U.size, phi.size)]
    its_d, res_d = ctx.solve_jointed_dev(*(t.data_ptr() for t in dev), max_iter, rtol, *(t.data_ptr() for t in out))
    ctx.sync_check()
    torch.cuda.synchronize()
    print("device form against host form, %d x %d: %d iterations to %.0e, residual %.2e" % (nb, nblb, its, rtol, res))
    assert (its_d, res_d) == (its, res) and 0 < its < max_iter and res < rtol
    for host, d in zip((lam, U, phi), out):
        assert host.tobytes() == d.cpu().numpy().tobytes()
    gap, phi_s = ctx.joint_state()
    assert np.array_equal(phi_s.reshape(-1), phi) and np.allclose(gap, jo.geometry(c["X"], c["Q"], body, anchor)[2], rtol=0.0, atol=1e-13)
    # without slip, joint_rhs and lambda
    its2, _ = ctx.solve_jointed_dev(dev[0].data_ptr(), None, None, max_iter, rtol, None, out[1].data_ptr(), out[2].data_ptr())
    ctx.sync_check()
    assert np.array_equal(out[1].cpu().numpy(), ctx.solve_jointed(F, max_iter=max_iter, rtol=rtol)[1]) and its2 > 0
    # the joints switched off and a slip given: the plain solve of both forms
    ctx.set_joints(body, anchor[:, :3], anchor[:, 3:], on=False)
    lam0, U0, phi0, its0, res0 = ctx.solve_jointed(F, slip=slip, max_iter=max_iter, rtol=rtol)
    out0 = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0") for n in (lam0.size, U0.size)]
    its0_d, res0_d = ctx.solve_jointed_dev(dev[0].data_ptr(), dev[1].data_ptr(), None, max_iter, rtol, out0[0].data_ptr(), out0[1].data_ptr(), None)
    ctx.sync_check()
    torch.cuda.synchronize()
    print("   joints off: %d iterations, residual %.2e" % (its0, res0))
    assert (its0_d, res0_d) == (its0, res0) and 0 < its0 < max_iter and res0 < rtol and phi0.size == 0
    for host, d in zip((lam0, U0), out0):
        assert host.tobytes() == d.cpu().numpy().tobytes()
    return F


def test_the_device_form_gives_the_host_form_s_bits_and_an_ensemble_context_is_refused():
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext, RblError
    for nb, nblb, max_iter, rtol in ((10, 12, 200, 1e-10), (17, 162, 200, 1e-8)):
        c = make_config(nb, nblb, True)
        ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
        try:
            ctx._chk(ctx.L.rbl_set_blk_pc(ctx.h, 1))
            ctx.set_config(c["X"], c["Q"])
            F = _device_form_gives_the_host_form_s_bits(ctx, c, nb, nblb, max_iter, rtol)
            if nb == 10:
                # a context that holds an ensemble: refused before any work
                ctx.ensemble_set_config(c["X"][None], c["Q"][None])
                with pytest.raises(RblError, match="ensemble"):
                    ctx.solve_jointed(F, max_iter=200, rtol=1e-10)
                with pytest.raises(RblError, match="ensemble"):
                    ctx.step_jointed(F, max_iter=200, rtol=1e-10)
        finally:
            ctx.close()


@pytest.mark.parametrize("wall,block", [(False, True), (True, True), (True, False)])
def test_poisoned_workspaces_change_no_bit(monkeypatch, wall, block):
    """every workspace filled with NaN patterns at every reserve (the hook of tests/test_poisoned_workspace_gpu.py): a jointed
    solve and step that read a slot they never wrote would differ from the clean run, or fail"""
    nb, nblb = 10, 12
    out = []
    for poison in (False, True):
        monkeypatch.setenv("RBL_POISON_WORKSPACE", "1" if poison else "0")
        c, rb = _body(nb, nblb, wall, block)
        assert rb.cb.get_option("poison_workspace") == int(poison)
        body, anchor = jo.chain_set(nb, c["X"], seed=91)
        body = np.concatenate([body, [[3, 2]]])                                      # and a hinge
        anchor = np.concatenate([anchor, np.random.default_rng(92).uniform(-0.6, 0.6, (1, 6))])
        rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
        F, slip, crhs = _inputs(nb, nblb, body.shape[0], seed=93)
        solved = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
        stepped = rb.step_jointed(F, slip=slip, gamma=0.0, max_iter=200, rtol=1e-10)
        out.append(tuple(solved) + tuple(stepped) + tuple(rb.get_config()) + tuple(rb.joint_state()))
        assert solved[4] < 1e-10 and stepped[2] < 1e-10
    for p, q in zip(*out):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()
