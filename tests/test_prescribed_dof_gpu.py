"""Prescribed kinematics per velocity component (include/rbl.h section 7, the _dof entry points) on the GPU: any of a body's six
lab-frame velocity components held or driven while the others stay free.  Dense numpy solutions on the oracle's matrices, the
residual through the public operators (also with more than 256 blobs per body), the preconditioner as the exact inverse of one
body's block, the reduction to solve_mixed, the round trip through a mobility solve, the step, reproducibility, poisoned
workspaces and the example.  Systems, helpers and tolerances are those of test_prescribed_gpu.py: solves to rtol 1e-10, the
residual estimate < 1e-10, two solutions of one system within 1e-7, the true residual <= 1e-9, F = -K^T lambda to 1e-12.

Iterations are printed by every test (run with -s), and asserted only as "converged within max_iter" -- except where the
preconditioner is the exact inverse of the whole system (one body), which GMRES must show by converging in at most 2."""
import subprocess
import sys

import numpy as np
import pytest

import test_poisoned_workspace_gpu as pw
import test_prescribed_gpu as t

pytestmark = pytest.mark.gpu
ROOT = t.ROOT
WALL_BLOCK, MODEL = t.WALL_BLOCK, t.MODEL
NB, NBLB = 10, 12
MASKS = ("rotations", "translations_147", "z", "random")


def _mask(which, nb=NB):
    P = np.zeros((nb, 6), dtype=bool)
    if which == "none":
        pass
    elif which == "rotations":
        P[:, 3:] = True
    elif which == "translations_147":
        P[[1, 4, 7], :3] = True
    elif which == "z":
        P[:, 2] = True
    elif which == "random":
        P = np.random.default_rng(31).random((nb, 6)) < 0.5
        P[2], P[5], P[8] = False, True, True               # an all-free body, a fully prescribed one, ...
        P[8, 4] = False                                    # ... and one with a single free component
        n = P.sum(axis=1)
        assert (n == 0).any() and (n == 6).any() and (n == 5).any() and ((n > 0) & (n < 5)).any()
    else:
        raise KeyError(which)
    return P


def _body_in(P, F, Up):
    return np.where(P, Up, F).reshape(-1)


def _dense_dof(M, K, P, F, Up, slip):
    """numpy.linalg.solve on [[M, -K[:, free]], [K[:, free]^T, 0]] -> (lambda, U, F), all components"""
    n3 = M.shape[0]
    free = ~P.reshape(-1)
    Kf, Kp = K[:, free], K[:, ~free]
    nf = Kf.shape[1]
    A = np.block([[M, -Kf], [Kf.T, np.zeros((nf, nf))]])
    x = np.linalg.solve(A, np.concatenate([slip + Kp @ Up.reshape(-1)[~free], -F.reshape(-1)[free]]))
    lam = x[:n3]
    U = np.array(Up, dtype=np.float64).reshape(-1)
    U[free] = x[n3:]
    Fo = np.array(F, dtype=np.float64).reshape(-1)
    Fo[~free] = -(Kp.T @ lam)
    return lam, U, Fo


# ---- 1. dense parity ------------------------------------------------------------------------------------------------------------
def _dense_parity(orc, wall, block, which):
    c, rb = t._body(NB, NBLB, wall, block)
    M, K = t._dense_matrices(orc, c, c["X"], c["Q"], wall)
    P = _mask(which)
    F, Up, slip = t._inputs(NB, NBLB, seed=11)
    lam, U, Fo, its, res = rb.solve_mixed_dof(P, _body_in(P, F, Up), slip=slip, max_iter=200, rtol=1e-10)
    lam_d, U_d, F_d = _dense_dof(M, K, P, F, Up, slip)
    print("dense parity wall=%s block=%s mask=%s (%d of %d components): %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e F %.2e"
          % (wall, block, which, int(P.sum()), P.size, its, res, t._rel(lam, lam_d), t._rel(U, U_d), t._rel(Fo, F_d)))
    assert 0 < its < 200 and res < 1e-10
    assert t._rel(lam, lam_d) <= 1e-7 and t._rel(U, U_d) <= 1e-7 and t._rel(Fo, F_d) <= 1e-7
    assert np.array_equal(U.reshape(NB, 6)[P], Up[P]) and np.array_equal(Fo.reshape(NB, 6)[~P], F[~P])      # echoed, bitwise


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_dense_parity(orc, wall, block, which):
    _dense_parity(orc, wall, block, which)


# ---- 2. the true residual through apply_M / K_dot / KT_dot ------------------------------------------------------------------------
def _operator_residual(rb, P, body_in, slip, lam, U, Fo):
    nb = P.shape[0]
    free = ~P.reshape(-1)
    r = rb.get_blob_positions().reshape(-1)
    bi = body_in.reshape(-1)
    top = rb.apply_M(lam, r) - rb.K_dot(U).reshape(-1) - slip
    ktl = rb.KT_dot(lam).reshape(-1)
    bot = (ktl + bi)[free]
    rhs = np.concatenate([slip + rb.K_dot(np.where(free, 0.0, bi)).reshape(-1), bi[free]])
    res = np.linalg.norm(np.concatenate([top, bot])) / np.linalg.norm(rhs)
    ferr = t._rel(Fo.reshape(-1)[~free], -ktl[~free]) if P.any() else 0.0
    assert np.array_equal(U.reshape(-1)[~free], bi[~free]) and np.array_equal(Fo.reshape(-1)[free], bi[free])
    return res, ferr


def _residual_case(nb, nblb, wall, block, P, seed, label):
    c, rb = t._body(nb, nblb, wall, block)
    F, Up, slip = t._inputs(nb, nblb, seed)
    bi = _body_in(P, F, Up)
    lam, U, Fo, its, res = rb.solve_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
    true_res, ferr = _operator_residual(rb, P, bi, slip, lam, U, Fo)
    print("%s wall=%s block=%s, %d of %d components prescribed: %d iterations, estimate %.2e, true residual %.2e, F_p error %.2e"
          % (label, wall, block, int(P.sum()), P.size, its, res, true_res, ferr))
    assert 0 < its < 200 and res < 1e-10
    assert true_res <= 1e-9 and ferr <= 1e-12


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_residual_through_the_public_operators(wall, block, which):
    _residual_case(NB, NBLB, wall, block, _mask(which), seed=12, label="residual 10 x 12, mask " + which)


@pytest.mark.parametrize("wall", [False, True])
def test_residual_with_642_blobs_per_body(wall):
    """N_blb > 256: the stride loops of the tails run three times with a ragged last pass (642 = 2 x 256 + 130); in free space the
    body-frame factor without tables, i.e. blk_solve and the block tail"""
    P = np.zeros((2, 6), dtype=bool)
    P[0, 3:] = True                                        # rotations of body 0
    P[1, 2] = True                                         # z of body 1
    _residual_case(2, 642, wall, True, P, seed=23, label="residual 2 x 642")


# ---- 3. the preconditioner is the exact inverse of a body's block ------------------------------------------------------------------
def _one_body_masks():
    out = []
    for comp in range(6):
        P = np.zeros((1, 6), dtype=bool)
        P[0, comp] = True
        out.append(("component %d" % comp, P))
    P = np.zeros((1, 6), dtype=bool)
    P[0, 3:] = True
    return out + [("rotations", P)]


def _exact_inverse(rb, label):
    F, Up, slip = t._inputs(1, rb.blobs_per_body, seed=24)
    for name, P in _one_body_masks():
        lam, U, Fo, its, res = rb.solve_mixed_dof(P, _body_in(P, F, Up), slip=slip, max_iter=20, rtol=1e-10)
        print("%s, mask %s: %d iterations, residual %.2e" % (label, name, its, res))
        assert 0 < its <= 2 and res < 1e-10, (label, name, its, res)


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("nblb", [12, 42])
def test_one_body_converges_in_two_iterations(nblb, wall):
    """one body: the block preconditioner with the masked factor is the inverse of the whole constrained matrix (free space: through
    the body-frame tables, the shared factor rotated to the lab frame before the mask cuts it)"""
    c, rb = t._body(1, nblb, wall, True)
    _exact_inverse(rb, "one shell of %d, wall=%s" % (nblb, wall))


def test_one_irregular_body_converges_in_two_iterations():
    """as above in free space with a body of no symmetry: a shell's K^T M^-1 K is isotropic, so rotating its factor the wrong way
    would go unseen; this one's is not"""
    from rigid_body_light_amd import RigidBody
    rng = np.random.default_rng(25)
    a = 0.3
    cfg = np.array([[0.0, 0.0, 0.0], [0.7, 0.0, 0.0], [1.3, 0.3, 0.0], [0.1, 0.8, 0.2], [0.2, 0.1, 0.9], [1.0, 0.9, 0.7], [-0.6, 0.2, 0.5]])
    Q = rng.standard_normal((1, 4))
    Q /= np.linalg.norm(Q)
    rb = RigidBody(cfg, np.array([[0.3, -0.2, 0.5]]), Q, a, 1.0, 0.01, wall_PC=False, block_PC=True)
    _exact_inverse(rb, "one irregular body of 7 blobs, free space")


# ---- 4. reduction to what exists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_whole_body_masks_reduce_to_solve_mixed(wall, block):
    """whole rows of the mask: the same kernels on the same bit sets and the same factor values (the masked factor of an all-free
    body is a copy of the context's, a fully prescribed body reads none), so solve_mixed's results bit for bit"""
    c, rb = t._body(NB, NBLB, wall, block)
    F, Up, slip = t._inputs(NB, NBLB, seed=26)
    for name, p in t._sets(NB).items():                    # none, bodies 1 4 7, all
        bi = t._body_in(p, F, Up)
        want = rb.solve_mixed(p, bi, slip=slip, max_iter=200, rtol=1e-10)
        got = rb.solve_mixed_dof(np.repeat(p[:, None], 6, axis=1), bi, slip=slip, max_iter=200, rtol=1e-10)
        bitwise = all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))
        diffs = [t._rel(x, y) for x, y in zip(got[:3], want[:3])]
        print("reduction wall=%s block=%s, whole bodies '%s': %d iterations (solve_mixed %d), rel. diff lambda %.1e U %.1e F %.1e, bitwise equal: %s"
              % (wall, block, name, got[3], want[3], diffs[0], diffs[1], diffs[2], bitwise))
        assert 0 < got[3] < 200 and got[3] == want[3]
        assert max(diffs) <= 1e-12
        assert bitwise


# ---- 5. round trip through a mobility solve ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_round_trip_through_a_mobility_solve(wall, block):
    c, rb = t._body(NB, NBLB, wall, block)
    n3 = 3 * NB * NBLB
    F, _, slip = t._inputs(NB, NBLB, seed=27)
    x, its0, res0 = rb.solve_saddle(np.concatenate([slip, -F.reshape(-1)]), max_iter=200, rtol=1e-10)
    lam0, U0 = x[:n3], x[n3:].reshape(NB, 6)
    P = _mask("random")
    lam, U, Fo, its, res = rb.solve_mixed_dof(P, _body_in(P, F, U0), slip=slip, max_iter=200, rtol=1e-10)
    print("round trip wall=%s block=%s: solve_saddle %d iterations, solve_mixed_dof %d; rel. diff lambda %.2e U %.2e F %.2e, F on the prescribed components %.2e"
          % (wall, block, its0, its, t._rel(lam, lam0), t._rel(U, U0), t._rel(Fo, F), t._rel(Fo.reshape(NB, 6)[P], F[P])))
    assert 0 < its < 200 and res < 1e-10 and res0 < 1e-10
    assert t._rel(lam, lam0) <= 1e-7 and t._rel(U, U0) <= 1e-7 and t._rel(Fo, F) <= 1e-7
    assert t._rel(Fo.reshape(NB, 6)[P], F[P]) <= 1e-7


# ---- 6. the step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_step_is_the_solve_then_the_update(wall, block):
    c, rb = t._body(NB, NBLB, wall, block)
    _, twin = t._body(NB, NBLB, wall, block)
    P = _mask("random")
    P[5, 3:] = False                                       # body 5: the three translations held, the rotation free under its torque
    F, Up, slip = t._inputs(NB, NBLB, seed=28)
    Up[5, :3] = 0.0
    bi = _body_in(P, F, Up)
    X0, Q0 = (np.array(v) for v in rb.get_config())
    lam, U, Fs, its, res = twin.solve_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
    twin.evolve_rigid_bodies(U)
    Fo, its_s, res_s = rb.step_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
    (X1, Q1), (Xt, Qt) = rb.get_config(), twin.get_config()
    print("step_mixed_dof wall=%s block=%s: %d iterations (the solve: %d); |X - X_twin| %.2e, |Q - Q_twin| %.2e; held body's |dQ| %.2e"
          % (wall, block, its_s, its, np.abs(X1 - Xt).max(), np.abs(Q1 - Qt).max(), np.abs(Q1[5] - Q0[5]).max()))
    assert 0 < its_s < 200 and res_s < 1e-10 and its_s == its
    assert np.array_equal(Fo, Fs)
    assert np.abs(X1 - Xt).max() <= 1e-14 and np.abs(Q1 - Qt).max() <= 1e-14
    assert np.array_equal(X1[5], X0[5]) and np.abs(Q1[5] - Q0[5]).max() > 1e-6      # held in place, bitwise, while it turns
    assert np.abs(X1[2] - X0[2]).max() > 1e-5                                      # the all-free body moved


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_force_model_enters_the_free_components_only(wall, block):
    """model on: the step solves the system whose free components carry body_in plus the model's loads, -K^T f_phys =
    interaction_forces(), and whose prescribed components are untouched -- bitwise what solve_mixed_dof returns when handed those
    loads (the whole-body test of test_prescribed_gpu.py, component by component)"""
    from oracle import oracle as O
    dt = 0.01
    P = _mask("random")
    F, Up, slip = t._inputs(NB, NBLB, seed=29)
    bi = _body_in(P, F, Up).reshape(NB, 6)
    c, rb = t._body(NB, NBLB, wall, block, dt=dt)
    rb.set_interactions(**MODEL)
    share = rb.interaction_forces().reshape(NB, 6)
    assert np.abs(share[P]).max() > 1e-3 and np.abs(share[~P]).max() > 1e-3      # the model does load prescribed components too
    bi_model = np.where(P, bi, bi + share)
    lam, U, Fs, its, res = rb.solve_mixed_dof(P, bi_model, slip=slip, max_iter=200, rtol=1e-10)
    assert np.array_equal(U.reshape(NB, 6)[P], Up[P])                            # prescribed velocities: bitwise body_in
    X0, Q0 = (np.array(v) for v in rb.get_config())
    Fo, its_s, res_s = rb.step_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
    print("model on, mask random, wall=%s block=%s: %d iterations; |F_step - F_solve| %.2e" % (wall, block, its_s, np.abs(Fo - Fs).max()))
    assert 0 < its_s < 200 and res_s < 1e-10
    assert its_s == its and res_s == res and np.array_equal(Fo, Fs)              # the same system: the same bits
    assert np.array_equal(Fo.reshape(NB, 6)[~P], bi_model[~P])                   # free loads echoed WITH the model's share
    Xo, Qo = O.evolve(X0, Q0, U, dt)
    X1, Q1 = rb.get_config()
    assert np.abs(X1 - Xo).max() <= 1e-14 and np.abs(Q1 - Qo).max() <= 1e-14     # the step moved the bodies with that U
    # with the model's loads added to the prescribed slots too the answer would differ by far more than rounding
    _, rb2 = t._body(NB, NBLB, wall, block, dt=dt)
    _, U_bad, _, _, _ = rb2.solve_mixed_dof(P, bi + share, slip=slip, max_iter=200, rtol=1e-10)
    assert t._rel(U_bad, U) > 1e-4


# ---- 7. reproducibility, unwritten memory --------------------------------------------------------------------------------------------
def test_reproducible_call_to_call():
    for wall, block in WALL_BLOCK:
        c, rb = t._body(NB, NBLB, wall, block)
        P = _mask("random")
        F, Up, slip = t._inputs(NB, NBLB, seed=30)
        a = rb.solve_mixed_dof(P, _body_in(P, F, Up), slip=slip, max_iter=200, rtol=1e-10)
        b = rb.solve_mixed_dof(P, _body_in(P, F, Up), slip=slip, max_iter=200, rtol=1e-10)
        print("two calls wall=%s block=%s: %d iterations" % (wall, block, a[3]))
        assert 0 < a[3] < 200
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_poisoned_workspaces(wall, block):
    """test_poisoned_workspace_gpu.py's pattern: the same inputs through a fresh object with every workspace poisoned and through
    one without -- the same iteration counts, bitwise the same outputs; a tail that reads a slot nobody wrote (the masked factors of
    a body, a ragged pass) fails.  The solve with device pointers too, into outputs that are NaN beforehand."""
    from rigid_body_light_amd import make_config
    c = make_config(NB, NBLB, wall)
    P = _mask("random")
    F, Up, slip = t._inputs(NB, NBLB, seed=32)
    bi = _body_in(P, F, Up)

    def fn(poison):
        rb = pw._body(poison, c["cfg"], c["X"], c["Q"], c["a"], wall, block)
        lam, U, Fo, its, res = rb.solve_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
        Fs, its_s, res_s = rb.step_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
        X, Q = rb.get_config()
        return dict(lam=lam, U=U, F=Fo, its=int(its), res=float(res), Fs=Fs, its_s=int(its_s), res_s=float(res_s), X=np.asarray(X), Q=np.asarray(Q))
    out = pw._twice(fn)
    print("poisoned workspaces wall=%s block=%s: %d iterations" % (wall, block, out["its"]))
    assert 0 < out["its"] < 200


def test_dev_form_equals_the_host_form():
    from rigid_body_light_amd._lib import DeviceContext, lib
    wall = True
    c, rb = t._body(NB, NBLB, wall, True)
    P = _mask("random")
    F, Up, slip = t._inputs(NB, NBLB, seed=33)
    bi = _body_in(P, F, Up)
    host = rb.solve_mixed_dof(P, bi, slip=slip, max_iter=200, rtol=1e-10)
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=pw._stream())
    lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_config(c["X"], c["Q"])
    d_bi, d_slip = pw._dev(bi), pw._dev(slip)
    d_lam, d_U, d_F = pw._nan(3 * NB * NBLB), pw._nan(6 * NB), pw._nan(6 * NB)
    its, res = ctx.solve_mixed_dof_dev(P, d_bi.data_ptr(), d_slip.data_ptr(), 200, 1e-10, d_lam.data_ptr(), d_U.data_ptr(), d_F.data_ptr())
    ctx.sync_check()
    print("device form: %d iterations (host form %d)" % (its, host[3]))
    assert 0 < its < 200 and its == host[3] and res == host[4]
    for got, want in zip((d_lam, d_U, d_F), host[:3]):
        assert np.array_equal(got.cpu().numpy(), want)
    ctx.close()


# ---- 8. the example ----------------------------------------------------------------------------------------------------------------
def test_microroller_example_rolls_the_way_it_spins():
    cmd = [sys.executable, "examples/microroller.py", "--steps", "3", "--omega"]
    procs = [subprocess.Popen(cmd + [om], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for om in ("10.0", "-10.0")]
    ux = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, out[-2000:] + err[-2000:]
        rows = [l.split() for l in out.splitlines() if l.startswith("step ")]
        assert len(rows) == 3
        vals = np.array([[float(v) for v in r[1:]] for r in rows])
        assert np.all(np.isfinite(vals))
        assert "rolling velocity along x" in out
        ux.append(vals[:, 2])
        print("microroller: mean U_x per step %s, torque about y %s, iterations %s" % (vals[:, 2], vals[:, 5], vals[:, 6]))
    assert np.all(ux[0] > 0.0) and np.all(ux[1] < 0.0)       # a shell spinning about +y above the wall rolls towards +x
    assert np.all(np.abs(ux[0]) > 1e-4 * 10.0) and np.all(np.abs(ux[1]) > 1e-4 * 10.0)      # far above the solves' 1e-8: not rounding
