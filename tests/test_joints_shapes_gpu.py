"""Hard joints (include/rbl.h section 9) away from the shapes they were written at: joint sets of 90 .. 300 joints on 3-, 4-, 5- and
7-blob bodies and of 1 .. 3 joints on bodies of 255 .. 513 blobs (tests/joint_oracle.SHAPE_CASES, whose inputs
tests/test_joints_shapes_cpu.py holds sound), the cap of 2048 joints, and time steps at 303 joint rows.  What the cases reach is listed in DESIGN.md section 5b.

Every context is created with its workspaces poisoned and every output starts as NaN (the conventions of
tests/test_body_shapes_gpu.py).  References are numpy on the oracle's dense M and K: numpy.linalg.solve on the jointed matrix,
and a right-preconditioned GMRES with the library's stopping rule whose preconditioner is the dense inverse of the jointed
matrix with M replaced by the context's M~ (joint_oracle.gmres_right_pc, jointed_pc).

Asserted per solve, at rtol = 1e-10 and max_iter = 200:
    residual estimate < 1e-10; true residual through apply_saddle and a numpy J rebuilt from get_config <= 1e-9;
    lambda, U and phi within 10 cond(A) rtol of the dense solve, cond(A) from body_shapes.COND_JOINTED (never from a GPU result);
    |J U - c| / |U| <= 1e-9;
    |iterations - reference iterations| <= 1.
The last is the one assertion that sees the preconditioner: GMRES uses S^-1 = (J N^-1 J^T)^-1 only as a right preconditioner, so a
wrong block of N^-1, of S or of its inverse leaves lambda, U and phi right and only costs iterations.  Two correct
implementations can differ by one iteration, at the stopping threshold."""
import functools
import time

import numpy as np
import pytest

import body_shapes as bs
import joint_oracle as jo
from test_body_shapes_gpu import _ctx, _dev, _frozen, _nan, _oracle, _rel

pytestmark = pytest.mark.gpu
RTOL, MAX_ITER, SEED = 1e-10, 200, 101                     # SEED: the right-hand sides of tests/test_joints_shapes_cpu.py's records


# ---------------------------------------------------------------------------------------------------------------- references
def _reference(c, seed):
    """-> dict(M, K, J, A, F, slip, crhs, b, sol = (lambda, U, phi)) on the oracle's matrices: read-only"""
    M, K = jo.dense_matrices(_oracle(), c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["wall"])
    J = jo.J_matrix(c["X"], c["Q"], c["body"], c["anchor"])
    A = jo.jointed_matrix(M, K, J)
    F, slip, crhs = jo.inputs(c["X"].shape[0], c["cfg"].shape[0], c["body"].shape[0], seed)
    b = jo.rhs_jointed(F, slip, crhs)
    sol = jo.dense_jointed(M, K, J, F, slip, crhs)
    _frozen(M, K, J, A, F, slip, crhs, b, *sol)
    return dict(M=M, K=K, J=J, A=A, F=F, slip=slip, crhs=crhs, b=b, sol=sol, its={})


def _reference_iterations(c, ref, block):
    if block not in ref["its"]:
        P = jo.jointed_pc(ref["M"], ref["K"], ref["J"], c["cfg"].shape[0], block)
        _, its, res = jo.gmres_right_pc(ref["A"], P, ref["b"], MAX_ITER, RTOL)
        assert res < RTOL
        ref["its"][block] = its
    return ref["its"][block]


@functools.lru_cache(maxsize=None)
def _shape_ref(name):
    c = jo.shape_case(name)
    return c, _reference(c, SEED)


@functools.lru_cache(maxsize=None)
def _small_ref(which, wall):
    """the three joint sets of tests/test_joints_gpu.py on shell_N_12 bodies, with that file's seeds"""
    from rigid_body_light_amd import make_config
    nb, seed = {"probe": (4, 31), "chain40": (40, 34), "hub71": (71, 36)}[which]
    c = dict(make_config(nb, 12, wall))
    if which == "probe":
        body, anchor = jo.probe_set(c["cfg"], c["X"])
    elif which == "chain40":
        body, anchor = jo.chain_set(40, c["X"], seed=33)
    else:
        body, anchor = jo.hub_set(71, seed=35)
    c.update(wall=wall, body=body, anchor=anchor)
    return c, _reference(c, seed)


# ---------------------------------------------------------------------------------------------------------------- the solve
def _solve(ctx, ref):
    """solve_jointed_dev into NaN outputs -> (lambda, U, phi, iterations, residual estimate)"""
    n3, nb6, nj3 = ref["slip"].size, ref["F"].size, ref["crhs"].size
    dF, ds, dc = _dev(ref["F"]), _dev(ref["slip"]), _dev(ref["crhs"])
    lam, U, phi = _nan(n3), _nan(nb6), _nan(nj3)
    its, res = ctx.solve_jointed_dev(dF.data_ptr(), ds.data_ptr(), dc.data_ptr(), MAX_ITER, RTOL, lam.data_ptr(), U.data_ptr(), phi.data_ptr())
    ctx.sync_check()
    return lam.cpu().numpy(), U.cpu().numpy(), phi.cpu().numpy(), its, res


def _true_residual(ctx, c, ref, lam, U, phi):
    """the three blocks through apply_saddle and J by formula at the configuration the context holds"""
    nb = c["X"].shape[0]
    X, Q = ctx.get_config(nb)
    n3 = lam.size
    dx, top = _dev(np.concatenate([lam, U])), _nan(n3 + 6 * nb)
    ctx.apply_saddle(dx.data_ptr(), top.data_ptr())
    ctx.sync_check()
    top = top.cpu().numpy()
    JU = jo.J_apply(X, Q, c["body"], c["anchor"], U)
    r = np.concatenate([top[:n3] - ref["slip"], top[n3:] + jo.JT_apply(X, Q, c["body"], c["anchor"], phi, nb) + ref["F"], JU - ref["crhs"]])
    return float(np.linalg.norm(r) / np.linalg.norm(ref["b"])), float(np.linalg.norm(JU - ref["crhs"]) / np.linalg.norm(U))


def _check(tag, c, ref, block, bound, twice=False):
    ctx = _ctx(c, c["wall"], block)
    try:
        ctx.set_joints(c["body"], c["anchor"][:, :3], c["anchor"][:, 3:])
        lam, U, phi, its, res = _solve(ctx, ref)
        again = _solve(ctx, ref) if twice else None
        true_res, cons = _true_residual(ctx, c, ref, lam, U, phi)
    finally:
        ctx.close()
    its_ref = _reference_iterations(c, ref, block)
    e = [_rel(v, w) for v, w in zip((lam, U, phi), ref["sol"])]
    print("%s %s: %d joints, %d iterations (reference %d), residual estimate %.2e, true %.2e, |J U - c| / |U| %.2e; rel. diff lambda %.2e U %.2e "
          "phi %.2e = %.1e of the bound %.1e" % (tag, "block" if block else "diagonal", c["body"].shape[0], its, its_ref, res, true_res, cons,
                                                  e[0], e[1], e[2], max(e) / bound, bound))
    assert np.isfinite(lam).all() and np.isfinite(U).all() and np.isfinite(phi).all(), tag
    assert 0 < its < MAX_ITER and res < RTOL, tag
    assert true_res <= 1e-9 and cons <= 1e-9, tag
    assert max(e) <= bound, tag
    assert abs(its - its_ref) <= 1, (tag, its, its_ref)
    if twice:
        for p, q in zip((lam, U, phi, its, res), again):
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), tag


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("block", [True, False], ids=["block", "diagonal"])
@pytest.mark.parametrize("name", list(jo.SHAPE_CASES))
def test_jointed_solve_vs_dense_solve_and_reference_iterations(name, block):
    """J1 .. J7 of joint_oracle.SHAPE_CASES with both preconditioners; the block one on J1w, J2 and J7b twice, for the same bits.

    Measured (one MI355X): the iteration count equals the reference's in all 26 solves (1 .. 86 iterations); residual estimate and
    true residual agree, 9.9e-11 at worst; |J U - c| / |U| 2.2e-11 at worst (J7d, diagonal); lambda, U, phi 3.3e-10 from the dense solve
    at worst (J5f, diagonal), 9.9e-4 of the bound at worst (J4, diagonal).  With k_jt_inverse updating only the first row a thread owns,
    or k_jt_mirror without its second block in x (scratch builds), J1w and J1f take 2 .. 7 iterations more and fail on that alone."""
    c, ref = _shape_ref(name)
    _check(name, c, ref, block, 10 * bs.COND_JOINTED[name] * RTOL, twice=block and name in ("J1w", "J2", "J7b"))


@pytest.mark.parametrize("which,wall,block", [("probe", False, False), ("probe", False, True), ("probe", True, False), ("probe", True, True),
                                              ("chain40", True, True), ("hub71", False, True), ("hub71", True, False)])
def test_reference_iterations_on_the_sets_of_the_first_joint_tests(which, wall, block):
    """probe_set on 4 x 12 (its open hinge included), chain_set(40) and hub_set(71) as tests/test_joints_gpu.py runs them, with
    that file's bound of 1e-7 on the solution, and the iteration count against the reference's"""
    c, ref = _small_ref(which, wall)
    _check("%s wall=%s" % (which, wall), c, ref, block, 1e-7)


# ---------------------------------------------------------------------------------------------------------------- a step
def _steps(c, block, F, slip, steps):
    """steps of step_jointed with gamma = 1 on a poisoned context -> (X, Q, iterations per step)"""
    nb, nj = c["nb"], c["body"].shape[0]
    ctx = _ctx(c, c["wall"], block)
    its_all = []
    try:
        ctx.set_joints(c["body"], c["anchor"][:, :3], c["anchor"][:, 3:])
        for _ in range(steps):
            phi, its, res = ctx.step_jointed(F, slip=slip, gamma=1.0, max_iter=MAX_ITER, rtol=RTOL)
            assert 0 < its < MAX_ITER and res < RTOL and phi.shape == (3 * nj,) and np.isfinite(phi).all()
            its_all.append(its)
        X1, Q1 = ctx.get_config(nb)
    finally:
        ctx.close()
    return X1, Q1, its_all


def test_three_steps_of_two_hinged_257_blob_bodies_against_the_numpy_restatement():
    """step_jointed with gamma = 1 on J7b (2 x fib257 in free space, a chain joint, a second joint between the same bodies named in the
    other order, a pivot; block preconditioner: the shared body-frame factor) for three steps of dt = 0.01, against
    tests/test_joints_gpu.py's _numpy_steps.  gamma = 1 asks the first step to close gaps of up to 12 (anchors drawn in +-R_b): the
    bodies move by 6.3, 3.4 and 4.7 and end up overlapping, the hinge may count as closed afterwards, and cond(A) grows along the way
    (3.7e4, 3.6e5, 7.4e5 in the restatement) -- so configurations are compared, not iteration counts.

    Bound: the step test of tests/test_joints_gpu.py allows 1e-7 on X and Q at rtol 1e-10 for 12-blob bodies, which is the rule of
    this section, 10 cond(A) rtol, at the cond(A) of about 1e2 that well-separated 12-blob bodies have; here the same rule with the
    recorded cond(A) of q^0 in its place: 10 x 3.67e4 x 1e-10 = 3.7e-5, absolute, on X and Q after the three steps.

    Measured (one MI355X): |X - X_ref| 9.6e-12, |Q - Q_ref| 1.4e-12; 24, 72 and 76 iterations.

    The step-only code at 303 joint rows and 6 N_bod > N is the business of the two tests below."""
    import test_joints_gpu as tj
    c, _ = _shape_ref("J7b")
    nb, nj = c["nb"], c["body"].shape[0]
    F, slip, _ = jo.inputs(nb, c["nblb"], nj, 42)
    dt, steps = 0.01, 3                                    # (dt: the contexts of test_body_shapes_gpu._ctx)
    bound = 10 * bs.COND_JOINTED["J7b"] * RTOL
    Xo, Qo = tj._numpy_steps(_oracle(), c, c["body"], c["anchor"], False, F, slip, np.zeros(3 * nj), 1.0, dt, steps)
    X1, Q1, its_all = _steps(c, True, F, slip, steps)
    ex, eq = np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max()
    print("J7b, three steps: iterations %s; |X - X_ref| %.2e, |Q - Q_ref| %.2e (bound %.1e), moved %.2e" % (its_all, ex, eq, bound, np.abs(X1 - c["X"]).max()))
    assert ex <= bound and eq <= bound
    assert np.abs(X1 - c["X"]).max() > 1e-3                 # it did move


def test_the_one_step_J1w_can_take_against_the_numpy_restatement():
    """step_jointed with gamma = 1 on J1w (100 trimers above a wall, 101 joints, block preconditioner): k_jt_step_rhs with two
    blocks (303 rows), and jt_geom, jt_rhs, jt_solve and the update with 6 N_bod = 600 > N = 300.  ONE step: J1w's gaps are of the
    order of the lattice (up to 11.5), gamma = 1 asks the step to close them, the bodies move by up to 6.6, and afterwards blobs
    lie at z = 0.27 < a and inside each other, where M is no longer positive definite -- a second step is rightly refused with
    RBL_ERR_NOT_SPD and is no test.  The first is solved at q^0, which tests/test_joints_shapes_cpu.py holds sound.

    Bound: 10 cond(A) rtol with the recorded cond(A) of q^0 = 3.2e-7, absolute, on X and Q (the rule of
    test_three_steps_of_two_hinged_257_blob_bodies_against_the_numpy_restatement).

    Measured (one MI355X): |X - X_ref| 2.4e-10, |Q - Q_ref| 1.2e-10; 27 iterations."""
    import test_joints_gpu as tj
    c, _ = _shape_ref("J1w")
    nj = c["body"].shape[0]
    F, slip, _ = jo.inputs(c["nb"], c["nblb"], nj, 42)
    bound = 10 * bs.COND_JOINTED["J1w"] * RTOL
    Xo, Qo = tj._numpy_steps(_oracle(), c, c["body"], c["anchor"], True, F, slip, np.zeros(3 * nj), 1.0, 0.01, 1)
    X1, Q1, its = _steps(c, True, F, slip, 1)
    ex, eq = np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max()
    print("J1w, one step: iterations %s; |X - X_ref| %.2e, |Q - Q_ref| %.2e (bound %.1e), moved %.2e" % (its, ex, eq, bound, np.abs(X1 - c["X"]).max()))
    assert ex <= bound and eq <= bound
    assert np.abs(X1 - c["X"]).max() > 1e-3


@pytest.mark.parametrize("block", [True, False], ids=["block", "diagonal"])
def test_three_steps_of_a_nearly_closed_chain_of_one_hundred_trimers(block):
    """joint_oracle.step_case: J1's bodies on a chain whose gaps are 0.05 .. 0.08 (close_chain; the pattern of hinged_chain), so that
    three steps with gamma = 1 and dt = 0.01 close them -- to 2.6e-3, then 8.9e-6 -- while the bodies move by 0.095, 0.0044 and
    0.0025 and stay where tests/test_joints_shapes_cpu.py finds every configuration sound (above the wall, apart, M positive
    definite).  303 joint rows, 6 N_bod > N, levers of the lattice spacing on the B ends.  First the solve at q^0 with everything
    _check asserts, the iteration count included; then the three steps against _numpy_steps.

    Bound on X and Q after the steps: 10 cond(A) rtol, absolute, with the largest cond(A) of the three solves as recorded in
    body_shapes.COND_JOINTED["J1s"] (3.24e3: 3.2e-6); the same for the solve.

    Measured (one MI355X): |X - X_ref| 3.2e-12, |Q - Q_ref| 1.4e-12 at worst; 25, 23, 22 iterations with the block preconditioner,
    36, 35, 34 with the diagonal one; the solve at q^0 takes the reference's 24 and 35 and is 1.1e-4 of its bound from the dense one."""
    import test_joints_gpu as tj
    c = jo.step_case()
    nj = c["body"].shape[0]
    bound = 10 * bs.COND_JOINTED["J1s"] * RTOL
    _check("J1s", c, _reference(c, SEED), block, bound)
    F, slip, _ = jo.inputs(c["nb"], c["nblb"], nj, 42)
    Xo, Qo = tj._numpy_steps(_oracle(), c, c["body"], c["anchor"], True, F, slip, np.zeros(3 * nj), 1.0, jo.STEP_DT, jo.STEP_STEPS)
    X1, Q1, its = _steps(c, block, F, slip, jo.STEP_STEPS)
    ex, eq = np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max()
    gap = np.linalg.norm(jo.geometry(X1, Q1, c["body"], c["anchor"])[2], axis=1).max()
    print("J1s %s, three steps: iterations %s; |X - X_ref| %.2e, |Q - Q_ref| %.2e (bound %.1e), moved %.2e, largest gap left %.2e"
          % ("block" if block else "diagonal", its, ex, eq, bound, np.abs(X1 - c["X"]).max(), gap))
    assert ex <= bound and eq <= bound
    assert np.abs(X1 - c["X"]).max() > 1e-2 and gap < 1e-4      # it moved, and the gaps are closed


# ---------------------------------------------------------------------------------------------------------------- the cap
def test_two_thousand_and_forty_eight_pivots():
    """rbl_set_joints' cap: 2048 pivots on 2048 trimers above a wall, np = 6144 -- a column of S^-1 fills 48 KB of LDS, a thread of
    k_jt_inverse owns 24 rows, S and S^-1 take 302 MB each.  The dense system would have order 36 864: no dense reference.
    Asserted: convergence at rtol 1e-10; the true residual <= 1e-9 through apply_saddle with J applied by formula; |J U - c| / |U|
    <= 1e-9; and the iteration count against the reference's count for the FIRST 64 bodies of the same lattice, anchors and
    right-hand side (order 1152), with a margin of +2: one for the stopping threshold, one because the count of a weakly coupled
    suspension may grow by one with the number of bodies (tests/test_joints_shapes_cpu.py: 28 for 64 bodies, 28 for 256).
    Diagonal preconditioner: with the block one the count is 3 .. 5 and still grows with the number of bodies.

    Measured (one MI355X): 29 iterations against 28, residual 8.1e-11, |J U - c| / |U| 3.3e-14; 0.3 s up to the end of the solve (2.1 s as
    the first test of a process)."""
    c = jo.cap_case()
    F, slip, crhs = jo.cap_inputs()
    ref = dict(F=F, slip=slip, crhs=crhs, b=jo.rhs_jointed(F, slip, crhs))
    t0 = time.perf_counter()
    ctx = _ctx(c, True, False)
    try:
        ctx.set_joints(c["body"], c["anchor"][:, :3], c["anchor"][:, 3:])
        lam, U, phi, its, res = _solve(ctx, ref)
        t1 = time.perf_counter()
        true_res, cons = _true_residual(ctx, c, ref, lam, U, phi)
    finally:
        ctx.close()
    c64 = jo.cap_case(64)
    M, K = jo.dense_matrices(_oracle(), c64["cfg"], c64["X"], c64["Q"], c64["a"], c64["eta"], True)
    J = jo.J_matrix(c64["X"], c64["Q"], c64["body"], c64["anchor"])
    _, its_ref, res_ref = jo.gmres_right_pc(jo.jointed_matrix(M, K, J), jo.jointed_pc(M, K, J, 3, False), jo.rhs_jointed(*jo.cap_inputs(64)),
                                            MAX_ITER, RTOL)
    print("2048 pivots: %d iterations (reference for the first 64 bodies: %d), residual estimate %.2e, true %.2e, |J U - c| / |U| %.2e; "
          "context, joints and solve %.2f s, the whole test %.2f s" % (its, its_ref, res, true_res, cons, t1 - t0, time.perf_counter() - t0))
    assert res_ref < RTOL
    assert np.isfinite(lam).all() and np.isfinite(U).all() and np.isfinite(phi).all()
    assert 0 < its < MAX_ITER and res < RTOL
    assert true_res <= 1e-9 and cons <= 1e-9
    assert its_ref - 1 <= its <= its_ref + 2, (its, its_ref)
