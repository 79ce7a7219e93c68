"""Joint kinds (include/rbl.h section 9: ball, lock, axis) on the GPU: welds, five-row hinges and motors in the jointed solve and
step.  Dense numpy solutions on the oracle's M and K with the angular rows of tests/joint_kinds_oracle.py (pinned by
tests/test_joint_kinds_cpu.py), the iteration count against a numpy GMRES with the exact preconditioner, the kinematics each
composition promises, the step against a numpy restatement with the motor angles, and the bits.  Tolerances are those of
tests/test_joints_gpu.py: solves to rtol 1e-10 within 200 iterations, two solutions of one system within 1e-7, true residual
and |J U - c| / |U| below 1e-9, iteration counts within one of the reference GMRES."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_kinds_oracle as jk  # noqa: E402
import joint_oracle as jo  # noqa: E402

WALL_BLOCK = [(False, False), (False, True), (True, False), (True, True)]
BALL, LOCK, AXIS = jk.BALL, jk.LOCK, jk.AXIS


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _body(X, Q, wall, block, nblb=12, dt=0.01):
    from rigid_body_light_amd import RigidBody, load_structure
    p, cfg = load_structure(nblb)
    c = dict(cfg=cfg, X=np.array(X), Q=np.array(Q), a=p["sep"] / 2.0, eta=1.0)
    return c, RigidBody(cfg, X, Q, c["a"], 1.0, dt, wall_PC=wall, block_PC=block)


def _inputs(nb, nblb, nj, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(6 * nb), 0.1 * rng.standard_normal(3 * nb * nblb), rng.standard_normal(3 * nj)


def _reference(orc, c, r, wall, block, F, slip, crhs, count=True):
    """the dense solve and, with count, the numpy GMRES with the exact preconditioner -> (lambda, U, phi, iterations or None,
    J, c with the axis joints' rows projected)"""
    nblb = c["cfg"].shape[0]
    M, K = jo.dense_matrices(orc, c["cfg"], c["X"], c["Q"], c["a"], c["eta"], wall)
    J = jk.J_matrix(c["X"], c["Q"], r)
    D = jk.D_matrix(c["X"], c["Q"], r, jo.pc_M(M, nblb, block), K, nblb)
    cp = jk.project(c["X"], c["Q"], r, crhs)
    lam, U, phi = jk.dense_jointed(M, K, J, D, F, slip, cp)
    its = None
    if count:
        A, P = jk.jointed_matrix(M, K, J, D), jk.jointed_pc(M, K, J, D, nblb, block)
        its = jo.gmres_right_pc(A, P, jo.rhs_jointed(F, slip, cp), 200, 1e-10)[1]
    return lam, U, phi, its, J, cp


def _solve_and_compare(orc, c, rb, r, wall, block, seed, label, crhs=None, F=None, count=True):
    """set the joints, solve to 1e-10, hold lambda, U, phi against the dense solve, the iteration count against the reference
    GMRES, the residual through the public operators and the constraint -> everything a caller may look at further"""
    nb, nblb, nj = c["X"].shape[0], c["cfg"].shape[0], r["body"].shape[0]
    rb.set_joint_kinds(**r)
    F0, slip, c0 = _inputs(nb, nblb, nj, seed)
    F = F0 if F is None else F
    crhs = c0 if crhs is None else crhs
    lam, U, phi, its, res = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    lam_d, U_d, phi_d, its_d, J, cp = _reference(orc, c, r, wall, block, F, slip, crhs, count)
    top = rb.apply_saddle(np.concatenate([lam, U]))
    n3 = lam.size
    rr = np.concatenate([top[:n3] - slip, top[n3:] + J.T @ phi + F, J @ U - cp])
    true_res = np.linalg.norm(rr) / np.linalg.norm(np.concatenate([slip, F, cp]))
    cons = np.linalg.norm(J @ U - cp) / np.linalg.norm(U)
    print("%s: %d joints, %d iterations (reference %s), residual %.2e, true %.2e, |J U - c| / |U| %.2e, rel. diff lambda %.2e U %.2e phi %.2e"
          % (label, nj, its, its_d, res, true_res, cons, _rel(lam, lam_d), _rel(U, U_d), _rel(phi, phi_d)))
    assert phi.shape == (3 * nj,) and 0 < its < 200 and res < 1e-10
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(phi, phi_d) <= 1e-7
    assert true_res <= 1e-9 and cons <= 1e-9
    if count:
        assert abs(its - its_d) <= 1
    return dict(F=F, slip=slip, c=crhs, cp=cp, lam=lam, U=U, phi=phi, J=J, its=its, res=res)


# ------------------------------------------------------------------------------------------------------------ 1: the weld
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_a_weld_solves_like_the_dense_system_and_moves_as_one_body(orc, wall, block):
    X, Q, r = jk.case_weld()
    c, rb = _body(X, Q, wall, block)
    _solve_and_compare(orc, c, rb, r, wall, block, seed=11, label="weld wall=%s block=%s" % (wall, block))
    # closed (both anchors one lab point, q_rel the configuration's) and with no joint_rhs: one rigid body under random loads
    r0 = jk.weld(X, Q, 0, 1, jk.mid(X, 0, 1))
    s = _solve_and_compare(orc, c, rb, r0, wall, block, seed=12, label="   closed", crhs=np.zeros(6))
    U = s["U"].reshape(2, 6)
    rigid = np.concatenate([U[0, :3] + np.cross(U[0, 3:], X[1] - X[0]), U[0, 3:]])
    print("   |U_B - rigid| / |U| %.2e" % (np.linalg.norm(U[1] - rigid) / np.linalg.norm(U)))
    assert np.linalg.norm(U[1] - rigid) <= 1e-9 * np.linalg.norm(U) and np.linalg.norm(U[0, 3:]) > 1e-3
    # the builders of the package give the same rows, and q_rel = None takes the configuration's
    mine = rb.weld(0, 1, jk.mid(X, 0, 1))
    rb.set_joint_kinds(mine["body"], mine["kind"], mine["anchor_a"], mine["anchor_b"], axis=mine["axis"])
    k = rb.joint_kinds()
    assert k["by_kinds"] and np.allclose(k["q_rel"][1], r0["q_rel"][1], rtol=0.0, atol=1e-14) and np.allclose(k["anchor_b"], r0["anchor_b"], rtol=0.0, atol=1e-13)
    again = rb.solve_jointed(s["F"], slip=s["slip"], max_iter=200, rtol=1e-10)
    assert _rel(again[1], s["U"]) <= 1e-7


# ------------------------------------------------------------------------------------------------------------ 2: the hinge
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_a_five_row_hinge(orc, wall, block):
    """BALL + AXIS between the bodies 0 and 1, a ball joint 1-2, a pivot on body 2.  The hinge's axis is the lab's z and body 0
    is not rotated, so ah = (0, 0, 1) exactly: there the projection that removes phi's component along ah, and the one that
    ignores joint_rhs's, leave an exact zero (for a general ah: the rounding of one projection, a few 1e-16 |phi|, which the hub
    and the 42-blob case below bound)"""
    X, Q, five, two = jk.case_hinge()
    c, rb = _body(X, Q, wall, block)
    s = _solve_and_compare(orc, c, rb, five, wall, block, seed=21, label="hinge wall=%s block=%s" % (wall, block))
    assert abs(s["c"][5]) > 1e-2 and s["cp"][5] == 0.0          # the right-hand side did have a component along the axis
    phi = s["phi"].reshape(-1, 3)
    assert phi[1, 2] == 0.0 and np.dot(phi[1], [0.0, 0.0, 1.0]) == 0.0 and np.abs(phi[1, :2]).max() > 1e-3
    # the component of joint_rhs along the axis is ignored: the same bits with it zeroed
    first = rb.solve_jointed(s["F"], slip=s["slip"], joint_rhs=s["c"], max_iter=200, rtol=1e-10)
    zeroed = np.array(s["c"])
    zeroed[5] = 0.0
    second = rb.solve_jointed(s["F"], slip=s["slip"], joint_rhs=zeroed, max_iter=200, rtol=1e-10)
    for p, q in zip(first, second):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()
    assert first[2].tobytes() == s["phi"].tobytes()
    # the two-ball hinge on the same axis under the same loads: the same motion
    crhs = np.array(s["c"])
    crhs[:6] = 0.0                                               # (the two hinges' own rows mean different things)
    U5 = rb.solve_jointed(s["F"], slip=s["slip"], joint_rhs=crhs, max_iter=200, rtol=1e-10)
    rb.set_joints(two["body"], two["anchor_a"], two["anchor_b"])
    U2 = rb.solve_jointed(s["F"], slip=s["slip"], joint_rhs=crhs, max_iter=200, rtol=1e-10)
    print("   five rows: %d iterations, two ball joints: %d; rel. diff U %.2e lambda %.2e" % (U5[3], U2[3], _rel(U5[1], U2[1]), _rel(U5[0], U2[0])))
    assert U5[4] < 1e-10 and U2[4] < 1e-10 and _rel(U5[1], U2[1]) <= 1e-7 and _rel(U5[0], U2[0]) <= 1e-7
    w = (U5[1].reshape(3, 6)[0, 3:] - U5[1].reshape(3, 6)[1, 3:])
    assert np.abs(w[:2]).max() <= 1e-9 * np.linalg.norm(U5[1]) and abs(w[2]) > 1e-3       # it turns about z and nothing else


# ------------------------------------------------------------------------------------------------------------ 3: the motor
@pytest.mark.parametrize("lab", [False, True])
@pytest.mark.parametrize("wall,block", [(False, True), (True, False), (True, True)])
def test_a_motor_turns_body_b_at_plus_omega_about_the_axis_and_loads_nothing_else(orc, wall, block, lab):
    """no external load: F = 0, joint_rhs what the step sets for a closed motor with the rate Omega, -Omega ah on the lock's rows.
    Between two bodies J^T phi is an internal load: its forces and its torques about the origin sum to zero.  Against the lab the
    reaction is the lab's: there the free body beside the motor carries no load at all"""
    omega = 0.7
    X, Q, r = jk.case_motor(lab)
    c, rb = _body(X, Q, wall, block)
    crhs = jk.step_rhs(X, Q, r, np.zeros(2), [0.0, omega], 1.0, 0.01, np.zeros(6))
    ah = jk.geometry(X, Q, r)[0][1]
    assert np.allclose(crhs[3:], -omega * ah, rtol=0.0, atol=1e-12)
    s = _solve_and_compare(orc, c, rb, r, wall, block, seed=31, label="motor lab=%s wall=%s block=%s" % (lab, wall, block), crhs=crhs,
                           F=np.zeros(12))
    U = s["U"].reshape(2, 6)
    dw = (0.0 if lab else U[1, 3:]) - U[0, 3:]
    print("   |w_B - w_A - Omega ah| %.2e" % np.linalg.norm(dw - omega * ah))
    assert np.linalg.norm(dw - omega * ah) <= 1e-9 * omega
    load = (s["J"].T @ s["phi"]).reshape(2, 6)
    size = np.abs(load).max()
    assert size > 1e-3
    if lab:
        assert np.abs(load[1]).max() == 0.0
    else:
        about = load[:, 3:] + np.cross(X, load[:, :3])           # the torques about the origin, body by body
        force, torque = load[:, :3].sum(axis=0), about.sum(axis=0)
        print("   sum of forces %.2e of %.2e, of torques about the origin %.2e of %.2e" % (np.abs(force).max(), size, np.abs(torque).max(), np.abs(about).max()))
        assert np.abs(force).max() <= 1e-12 * size and np.abs(torque).max() <= 1e-12 * np.abs(about).max()
    # one step with the rate set does the same: phi is the solve's to the gaps' rounding, theta advances by Omega dt
    rb.set_joint_rates([0.0, omega])
    phi_s, its, res = rb.step_jointed(np.zeros(12), slip=s["slip"], gamma=1.0, max_iter=200, rtol=1e-10)
    gap, phi2, theta = rb.joint_state()
    assert res < 1e-10 and _rel(phi_s, s["phi"]) <= 1e-7 and np.array_equal(phi2.reshape(-1), phi_s)
    assert theta[0] == 0.0 and theta[1] == omega * 0.01 and np.array_equal(rb.joint_kinds()["theta"], theta)


# ------------------------------------------------------------------------------------------------------------ 4: larger
def test_four_shell_42_bodies_with_all_three_kinds(orc):
    X, Q, r = jk.case_mixed42()
    assert sorted(set(r["kind"])) == [BALL, LOCK, AXIS]
    c, rb = _body(X, Q, True, True, nblb=42)
    s = _solve_and_compare(orc, c, rb, r, True, True, seed=41, label="4 x shell_N_42, weld + hinge + motor + ball")
    ah = jk.geometry(X, Q, r)[0]
    phi = s["phi"].reshape(-1, 3)
    along = max(abs(phi[j] @ ah[j]) / np.linalg.norm(phi[j]) for j in np.flatnonzero(r["kind"] == AXIS))
    print("   |phi . ah| / |phi| on the axis joint %.2e" % along)
    # phi_out = phi - ah d^, d^ the computed ah . phi: d^ is off by at most 3 eps |phi|, the subtraction adds 2 eps |phi| along ah,
    # and numpy's own dot product here 3 eps |phi|: 8 eps |phi| at the worst
    assert along <= 8 * np.finfo(float).eps


@pytest.mark.parametrize("wall,block", [(False, True), (True, False)])
def test_a_hub_with_seventy_joint_ends_of_mixed_kinds(orc, wall, block):
    """body 0 carries a ball joint and a lock or axis joint to each of 35 others: 70 ends on one body, two passes of k_jt_tail's
    lanes and its LDS tree sum, torque-only and projected ends among them; 70 joints, 210 rows, np = 224"""
    X, Q, r = jk.case_hub()
    assert np.sum(r["body"] == 0) == 70 and (r["kind"] == LOCK).sum() > 10 and (r["kind"] == AXIS).sum() > 10
    c, rb = _body(X, Q, wall, block)
    s = _solve_and_compare(orc, c, rb, r, wall, block, seed=42, label="hub wall=%s block=%s" % (wall, block))
    ah = jk.geometry(X, Q, r)[0]
    phi = s["phi"].reshape(-1, 3)
    assert max(abs(phi[j] @ ah[j]) / np.linalg.norm(phi[j]) for j in np.flatnonzero(r["kind"] == AXIS)) <= 8 * np.finfo(float).eps


# ------------------------------------------------------------------------------------------------------------ 5: steps
@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("wall,block", [(False, True), (True, False), (True, True)])
def test_ten_steps_against_the_numpy_restatement(orc, wall, block, gamma):
    """a motor 0-1 whose rate changes sign after five steps, a hinge 1-2, a pivot on body 0, every joint open by about 0.01;
    joint_velocity pulls the pivot along and asks the hinge for a rate about its free axis, which is ignored"""
    dt, steps = 0.01, 10
    X, Q, r = jk.case_steps()
    c, rb = _body(X, Q, wall, block, dt=dt)
    rb.set_joint_kinds(**r)
    rng = np.random.default_rng(51)
    F, slip = rng.standard_normal(18), 0.1 * rng.standard_normal(108)
    v = np.zeros((5, 3))
    v[4] = [0.2, -0.1, 0.3]
    v[3] = 0.4 * jk.geometry(X, Q, r)[0][3] + [0.05, 0.0, -0.02]
    rates = np.zeros((steps, 5))
    rates[:5, 1], rates[5:, 1] = 0.9, -0.6
    Xo, Qo, theta_o = jk.numpy_steps(orc, c, r, wall, F, slip, v, gamma, dt, rates)
    its_all = []
    for n in range(steps):
        rb.set_joint_rates(rates[n])
        phi, its, res = rb.step_jointed(F, slip=slip, joint_velocity=v, gamma=gamma, max_iter=200, rtol=1e-10)
        assert 0 < its < 200 and res < 1e-10 and phi.shape == (15,)
        its_all.append(its)
    X1, Q1 = rb.get_config()
    gap, _, theta = rb.joint_state()
    print("step_jointed wall=%s block=%s gamma=%.1f: iterations %s; |X - X_ref| %.2e, |Q - Q_ref| %.2e, moved %.2e, theta %r"
          % (wall, block, gamma, its_all, np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max(), np.abs(X1 - X).max(), theta[1]))
    assert np.abs(X1 - Xo).max() <= 1e-7 and np.abs(Q1 - Qo).max() <= 1e-7
    assert np.array_equal(theta, theta_o) and theta[1] != 0.0 and not theta[[0, 2, 3, 4]].any()
    assert np.abs(X1 - X).max() > 1e-3
    assert np.allclose(gap, jk.geometry(X1, Q1, r, theta)[1], rtol=0.0, atol=1e-12)     # the state query's gaps, angular rows included


def _relative_angle(Q, r, j):
    """the angle by which body B has turned relative to body A about the lock joint j's axis since q_rel was taken"""
    a, b = r["body"][j]
    d = jk.qmul(jk.qmul(jk.qconj(jo.unit(Q)[a]), jo.unit(Q)[b]), jk.qconj(r["q_rel"][j]))      # = rot(angle a), seen from A
    return float(jk.rotvec(d) @ r["axis"][j])


def test_a_driven_hinge_keeps_its_angular_gap_and_turns_by_omega_n_dt():
    """40 steps of a motor between two bodies under random loads at gamma = 1, rate 1, with dt = 0.01 and dt = 0.005.  With
    gamma = 1 a step takes the gap it finds out to first order and leaves the second-order error of its own explicit rotation
    update, O((|w| dt)^2), whatever it found: the angular gap neither accumulates nor decays.  Asserted, in the form of the
    translational gaps: the largest gap of the last five steps is at most twice the largest of the steps 2 .. 6; halving dt
    divides it by about four (between 2 and 8); and the relative angle about the axis is Omega n dt to within the gap.

    Measured (one MI355X), dt = 0.01: angular gap 6.32e-7 after the first step, at most 6.13e-7 over the steps 2 .. 6 and 6.84e-7
    over the last five; translational gap 3.64e-5 and 3.59e-5; relative angle - Omega n dt 1.5e-11.  dt = 0.005: 1.58e-7, 1.56e-7,
    1.26e-7; 9.10e-6 and 9.07e-6; 1.0e-12.  Ratio of the last-five gaps 5.4."""
    omega, steps = 1.0, 40
    X, Q, r = jk.case_driven()
    F = np.random.default_rng(52).standard_normal(12)
    last = {}
    for dt in (0.01, 0.005):
        c, rb = _body(X, Q, True, True, dt=dt)
        rb.set_joint_kinds(**r)
        rb.set_joint_rates([0.0, omega])
        ang, lin = [], []
        for n in range(steps):
            _, its, res = rb.step_jointed(F, gamma=1.0, max_iter=200, rtol=1e-10)
            assert 0 < its < 200 and res < 1e-10
            gap, _, theta = rb.joint_state()
            lin.append(np.linalg.norm(gap[0]))
            ang.append(np.linalg.norm(gap[1]))
        Q1 = rb.get_config()[1]
        turned = _relative_angle(Q1, r, 1)
        print("driven hinge dt=%g: angular gap after step 1 %.3e, steps 2-6 max %.3e, last five max %.3e; translational %.3e, %.3e; "
              "theta %.17g, relative angle - Omega n dt %.3e" % (dt, ang[0], max(ang[1:6]), max(ang[-5:]), max(lin[1:6]), max(lin[-5:]),
                                                                 theta[1], turned - omega * steps * dt))
        assert max(ang[-5:]) <= 2.0 * max(ang[1:6]) and max(lin[-5:]) <= 2.0 * max(lin[1:6])
        assert abs(theta[1] - omega * steps * dt) <= 1e-15 * steps
        assert abs(turned - omega * steps * dt) <= ang[-1] + 10.0 * ang[-1] ** 2 + 1e-12     # first order in e: exactly e . ah
        last[dt] = max(ang[-5:])
    assert 2.0 <= last[0.01] / last[0.005] <= 8.0


# ------------------------------------------------------------------------------------------------------------ 6: the same bits
def _ball_set(c, nb):
    body, anchor = jo.chain_set(nb, c["X"], seed=91)
    body = np.concatenate([body, [[3, 2]]])                                          # and a two-ball hinge
    anchor = np.concatenate([anchor, np.random.default_rng(92).uniform(-0.6, 0.6, (1, 6))])
    return body, anchor


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_ball_joints_through_set_joint_kinds_give_the_bits_of_set_joints(wall, block):
    from rigid_body_light_amd import make_config
    nb, nblb = 10, 12
    c = make_config(nb, nblb, wall)
    body, anchor = _ball_set(c, nb)
    F, slip, crhs = _inputs(nb, nblb, body.shape[0], seed=93)
    out = []
    for kinds in (False, True):
        _, rb = _body(c["X"], c["Q"], wall, block)
        if kinds:
            rb.set_joint_kinds(body, np.zeros(body.shape[0], dtype=np.int32), anchor[:, :3], anchor[:, 3:])
            assert rb.joint_kinds()["by_kinds"] and not rb.joint_kinds()["kind"].any()
        else:
            rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
        solved = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
        stepped = rb.step_jointed(F, slip=slip, gamma=1.0, max_iter=200, rtol=1e-10)
        state = rb.joint_state()
        assert len(state) == (3 if kinds else 2) and solved[4] < 1e-10 and stepped[2] < 1e-10
        out.append(tuple(solved) + tuple(stepped) + tuple(rb.get_config()) + tuple(state[:2]))
    for p, q in zip(*out):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()


def _mixed_run(rb, r, F, slip, crhs):
    rb.set_joint_kinds(**r)
    rates = np.where(r["kind"] == LOCK, 0.5, 0.0)
    rb.set_joint_rates(rates)
    solved = rb.solve_jointed(F, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    stepped = rb.step_jointed(F, slip=slip, gamma=1.0, max_iter=200, rtol=1e-10)
    assert solved[4] < 1e-10 and stepped[2] < 1e-10
    return tuple(solved) + tuple(stepped) + tuple(rb.get_config()) + tuple(rb.joint_state())


@pytest.mark.parametrize("wall,block", [(False, True), (True, True), (True, False)])
def test_two_calls_and_poisoned_workspaces_change_no_bit(monkeypatch, wall, block):
    """the mixed set of the 42-blob case on 12-blob bodies and a closed two-ball hinge to a fifth body (its redundant row is
    found and given its eigenvalue inside a set with angular joints): two calls on one context, a second context, and a
    context whose workspaces are filled with NaN patterns at every reserve (the hook of tests/test_poisoned_workspace_gpu.py) -- a
    kernel of the KINDS instantiations that read a slot it never wrote would differ, or fail"""
    X, Q, r = jk.case_mixed5()
    F, slip, crhs = _inputs(5, 12, r["body"].shape[0], seed=94)
    crhs[-6:] = 0.0                                              # (the closed hinge's redundant row takes no right-hand side)
    out = []
    for poison in (False, False, True):
        monkeypatch.setenv("RBL_POISON_WORKSPACE", "1" if poison else "0")
        _, rb = _body(X, Q, wall, block)
        assert rb.cb.get_option("poison_workspace") == int(poison)
        out.append(_mixed_run(rb, r, F, slip, crhs))
        if not poison:
            rb.set_config(X, Q)                                  # the same context again, from the same configuration
            out.append(_mixed_run(rb, r, F, slip, crhs))
    for other in out[1:]:
        for p, q in zip(out[0], other):
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes()


# ------------------------------------------------------------------------------------------------------------ 7: other entry points
@pytest.mark.parametrize("wall,block", [(False, True), (True, False)])
def test_every_other_entry_point_ignores_the_kinds(wall, block):
    X, Q, r = jk.case_mixed42()
    F, slip, _ = _inputs(4, 12, 1, seed=95)
    out = {}
    for state in ("never", "on"):
        _, rb = _body(X, Q, wall, block)
        if state == "on":
            rb.set_joint_kinds(**r)
            rb.set_joint_rates(np.where(r["kind"] == LOCK, 0.5, 0.0))
        x, its0, res0 = rb.solve_saddle(np.concatenate([slip, -F]), max_iter=200, rtol=1e-10)
        mixed = rb.solve_mixed([1, 3], F, slip=slip, max_iter=200, rtol=1e-10)
        its_s, res_s = rb.step_deterministic(F, slip=slip, max_iter=200, rtol=1e-10)
        out[state] = (x, its0, res0) + tuple(mixed) + (its_s, res_s) + tuple(rb.get_config())
        if state == "on":
            assert not rb.joint_kinds()["theta"].any()           # step_deterministic is no jointed step: no motor turned
    for p, q in zip(out["never"], out["on"]):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()


def test_an_ensemble_context_refuses_the_jointed_calls_with_kinds_set():
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext, RblError
    c = make_config(4, 12, True)
    ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.set_config(c["X"], c["Q"])
        from rigid_body_light_amd import _lib as lib
        rows = lib.joint_rows(ctx.weld(0, 1, 0.5 * (c["X"][0] + c["X"][1])), ctx.motor(2, -1, c["X"][2], [0.0, 0.0, 1.0]))
        ctx.set_joint_kinds(**rows)
        assert list(ctx.joint_kinds()["kind"]) == [BALL, LOCK, BALL, LOCK]
        F = np.random.default_rng(96).standard_normal(24)
        lam, U, phi, its, res = ctx.solve_jointed(F, max_iter=200, rtol=1e-10)
        assert res < 1e-10 and len(ctx.joint_state()) == 3
        ctx.ensemble_set_config(c["X"][None], c["Q"][None])
        with pytest.raises(RblError, match="ensemble"):
            ctx.solve_jointed(F, max_iter=200, rtol=1e-10)
        with pytest.raises(RblError, match="ensemble"):
            ctx.step_jointed(F, max_iter=200, rtol=1e-10)
    finally:
        ctx.close()
