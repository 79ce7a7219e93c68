"""Prescribed kinematics (include/rbl.h section 7) on the GPU: bodies that are held or driven while the others stay free, and the
loads that takes.  Dense numpy solutions on the oracle's matrices, the residual through the public operators, the round trip
through a mobility solve, the resistance matrix, the physics of a held body, the step, the cfg 2 / cfg 3 sizes, reproducibility,
poisoned workspaces and the example.  Tolerances are those tests/test_host_boundary_gpu.py uses for solve_saddle: solves to
rtol 1e-10, residual < 1e-9 of the right-hand side, two solutions of one system within 1e-7.

Iterations to 1e-10 are printed by every test (run with -s), never asserted beyond "converged within max_iter"."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL_BLOCK = [(False, False), (False, True), (True, False), (True, True)]
MODEL = dict(w=0.2, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.1)


def _body(nb, nblb, wall, block, dt=0.01):
    from rigid_body_light_amd import RigidBody, make_config
    c = make_config(nb, nblb, wall)
    return c, RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt, wall_PC=wall, block_PC=block)


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _sets(nb):
    return {"none": np.zeros(nb, dtype=bool), "three": np.isin(np.arange(nb), [1, 4, 7]), "all": np.ones(nb, dtype=bool)}


def _inputs(nb, nblb, seed, slip_scale=0.1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nb, 6)), rng.standard_normal((nb, 6)), slip_scale * rng.standard_normal(3 * nb * nblb)


def _dense_matrices(orc, c, X, Q, wall):
    """M (B M B with the wall, as apply_M applies it) and K of a configuration, built as test_host_boundary_gpu.py builds them"""
    from oracle import oracle as O
    cfg = c["cfg"] - c["cfg"].mean(axis=0)
    Qn = O.normalize_quats(np.asarray(Q, dtype=np.float64).reshape(-1, 4))
    r = orc.multi_body_pos(X, Qn, cfg)
    K = O.K_matrix(X, Qn, cfg)
    M = orc.rotne_prager_tensor(r, c["a"], c["eta"], wall)
    if wall:
        B = orc.damp(r, c["a"])
        M = B[:, None] * M * B[None, :]
    return M, K


def _dense_mixed(M, K, p, F, Up, slip):
    """numpy.linalg.solve on the constrained matrix [M -K_f; K_f^T 0] -> (lambda, U (all bodies), F (all bodies))"""
    nb = p.size
    n3 = M.shape[0]
    colf = np.repeat(~p, 6)
    Kf, Kp = K[:, colf], K[:, ~colf]
    nf6 = Kf.shape[1]
    A = np.block([[M, -Kf], [Kf.T, np.zeros((nf6, nf6))]])
    rhs = np.concatenate([slip + Kp @ Up[p].reshape(-1), -F[~p].reshape(-1)])
    x = np.linalg.solve(A, rhs)
    lam = x[:n3]
    U = np.array(Up, dtype=np.float64)
    U[~p] = x[n3:].reshape(-1, 6)
    Fo = np.array(F, dtype=np.float64)
    Fo[p] = -(Kp.T @ lam).reshape(-1, 6)
    return lam, U.reshape(-1), Fo.reshape(-1)


def _body_in(p, F, Up):
    return np.where(p[:, None], Up, F).reshape(-1)


def _dense_parity(orc, wall, block, which):
    nb, nblb = 10, 12
    c, rb = _body(nb, nblb, wall, block)
    M, K = _dense_matrices(orc, c, c["X"], c["Q"], wall)
    p = _sets(nb)[which]
    F, Up, slip = _inputs(nb, nblb, seed=11)
    lam, U, Fo, its, res = rb.solve_mixed(p, _body_in(p, F, Up), slip=slip, max_iter=200, rtol=1e-10)
    lam_d, U_d, F_d = _dense_mixed(M, K, p, F, Up, slip)
    print("dense parity wall=%s block=%s p=%s: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e F %.2e"
          % (wall, block, which, its, res, _rel(lam, lam_d), _rel(U, U_d), _rel(Fo, F_d)))
    assert 0 < its < 200 and res < 1e-10
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(Fo, F_d) <= 1e-7
    assert np.array_equal(U.reshape(nb, 6)[p], Up[p]) and np.array_equal(Fo.reshape(nb, 6)[~p], F[~p])      # echoed


@pytest.mark.parametrize("which", ["none", "three", "all"])
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_dense_parity_cfg1(orc, wall, block, which):
    _dense_parity(orc, wall, block, which)


def _operator_residual(rb, p, body_in, slip, lam, U, Fo):
    """the system through apply_M / K_dot / KT_dot -> (|residual| / |rhs|, rel. error of F = -K^T lambda on prescribed bodies)"""
    nb = p.size
    r = rb.get_blob_positions().reshape(-1)
    bi = body_in.reshape(nb, 6)
    top = rb.apply_M(lam, r) - rb.K_dot(U).reshape(-1) - slip
    ktl = rb.KT_dot(lam).reshape(nb, 6)
    bot = (ktl + bi)[~p].reshape(-1)
    Up = np.where(p[:, None], bi, 0.0).reshape(-1)
    rhs = np.concatenate([slip + rb.K_dot(Up).reshape(-1), bi[~p].reshape(-1)])
    res = np.linalg.norm(np.concatenate([top, bot])) / np.linalg.norm(rhs)
    Fp = Fo.reshape(nb, 6)[p]
    ferr = _rel(Fp, -ktl[p]) if p.any() else 0.0
    return res, ferr


def _residual_case(nb, nblb, wall, block, p, seed, label):
    c, rb = _body(nb, nblb, wall, block)
    F, Up, slip = _inputs(nb, nblb, seed)
    bi = _body_in(p, F, Up)
    lam, U, Fo, its, res = rb.solve_mixed(p, bi, slip=slip, max_iter=200, rtol=1e-10)
    true_res, ferr = _operator_residual(rb, p, bi, slip, lam, U, Fo)
    print("%s wall=%s block=%s, %d of %d prescribed: %d iterations, estimate %.2e, true residual %.2e, F_p error %.2e"
          % (label, wall, block, int(p.sum()), nb, its, res, true_res, ferr))
    assert 0 < its < 200 and res < 1e-10
    assert true_res <= 1e-9 and ferr <= 1e-12
    return rb, (lam, U, Fo, its, res)


@pytest.mark.parametrize("which", ["none", "three", "all"])
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_residual_through_the_public_operators(wall, block, which):
    _residual_case(10, 12, wall, block, _sets(10)[which], seed=12, label="residual cfg 1")


def _round_trip(nb, nblb, wall, block, p, seed, label):
    c, rb = _body(nb, nblb, wall, block)
    n3 = 3 * nb * nblb
    F, _, slip = _inputs(nb, nblb, seed)
    x, its0, res0 = rb.solve_saddle(np.concatenate([slip, -F.reshape(-1)]), max_iter=200, rtol=1e-10)
    lam0, U0 = x[:n3], x[n3:].reshape(nb, 6)
    lam, U, Fo, its, res = rb.solve_mixed(p, _body_in(p, F, U0), slip=slip, max_iter=200, rtol=1e-10)
    print("%s wall=%s block=%s, %d of %d prescribed: solve_saddle %d iterations, solve_mixed %d; rel. diff lambda %.2e U %.2e F %.2e"
          % (label, wall, block, int(p.sum()), nb, its0, its, _rel(lam, lam0), _rel(U, U0), _rel(Fo, F)))
    assert 0 < its < 200 and res < 1e-10 and res0 < 1e-10
    assert _rel(lam, lam0) <= 1e-7 and _rel(U, U0) <= 1e-7 and _rel(Fo, F) <= 1e-7


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_round_trip_through_a_mobility_solve(wall, block):
    nb = 10
    half = np.zeros(nb, dtype=bool)
    half[np.random.default_rng(5).permutation(nb)[:nb // 2]] = True
    _round_trip(nb, 12, wall, block, half, seed=13, label="round trip cfg 1")
    _round_trip(nb, 12, wall, block, np.zeros(nb, dtype=bool), seed=14, label="nobody prescribed == solve_saddle")


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_resistance_matrix_is_the_inverse_of_the_mobility_matrix(wall, block):
    c, rb = _body(10, 12, wall, block)
    R, its = rb.body_resistance_matrix(max_iter=200, rtol=1e-10)
    N, _ = rb.body_mobility_matrix(max_iter=200, rtol=1e-11)
    nR = np.linalg.norm(R)
    sym, inv = np.linalg.norm(R - R.T) / nR, np.linalg.norm(R @ N - np.eye(60))     # (the whole 60 x 60 difference, not normalised)
    emin = np.linalg.eigvalsh(0.5 * (R + R.T)).min()
    print("resistance matrix wall=%s block=%s: iterations %d..%d, asymmetry %.2e, |R N - I|_F %.2e, smallest eigenvalue %.3e"
          % (wall, block, its.min(), its.max(), sym, inv, emin))
    assert R.shape == (60, 60) and np.all(its > 0) and np.all(its < 200)
    assert sym <= 1e-7 and emin > 0.0 and inv <= 1e-6
    Rc, _ = rb.body_resistance_matrix(max_iter=200, rtol=1e-10, columns=[2, 40])
    assert Rc.shape == (60, 2) and np.array_equal(Rc, R[:, [2, 40]])


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_no_flow_at_a_held_body(wall, block):
    """one shell held next to a free one under load: the fluid is at rest on the held body's blobs and moves with K U on the
    free body's (no slip on both), to the bound test_velocity_field_gpu.py puts on no slip"""
    from rigid_body_light_amd import RigidBody, load_structure
    params, cfg = load_structure(162)
    a = params["sep"] / 2.0
    Rb = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()) + a
    X = np.array([[0.0, 0.0, Rb + a], [2.0 * Rb + 1.5 * a, 0.3 * Rb, Rb + 2.0 * a]])
    Q = np.array([[1.0, 0.0, 0.0, 0.0], [0.8, 0.0, 0.6, 0.0]])
    rb = RigidBody(cfg, X, Q, a, 1.0, 0.01, wall_PC=wall, block_PC=block)
    nblb = rb.blobs_per_body
    bi = np.zeros((2, 6))
    bi[1] = [0.3, -0.2, -1.0, 0.1, 0.5, -0.2]                   # body 0 held (U = 0), body 1 free under this load
    lam, U, F, its, res = rb.solve_mixed([0], bi, max_iter=200, rtol=1e-10)
    u = rb.velocity_field(rb.get_blob_positions(), lam).reshape(2, nblb, 3)
    KU = rb.K_dot(U).reshape(2, nblb, 3)
    speed = np.linalg.norm(KU[1])
    print("held body wall=%s block=%s: %d iterations; |u| on the held body / free body's blob speed %.2e, free body no slip %.2e, load on the held body %s"
          % (wall, block, its, np.linalg.norm(u[0]) / speed, _rel(u[1], KU[1]), np.array2string(F[:6], precision=4)))
    assert 0 < its < 200 and res < 1e-10
    assert not np.any(U[:6]) and not np.any(KU[0])
    assert np.linalg.norm(u[0]) <= 1e-8 * speed and _rel(u[1], KU[1]) <= 1e-8
    assert np.linalg.norm(F[:6]) > 1e-3 * np.linalg.norm(bi[1])      # holding it takes a load


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_step_mixed_against_the_numpy_restatement(orc, wall, block):
    from oracle import oracle as O
    nb, nblb = 10, 12
    c, rb = _body(nb, nblb, wall, block)
    dt = 0.01
    M, K = _dense_matrices(orc, c, c["X"], c["Q"], wall)
    p = _sets(nb)["three"]
    F, Up, slip = _inputs(nb, nblb, seed=15)
    bi = _body_in(p, F, Up)
    _, U_d, F_d = _dense_mixed(M, K, p, F, Up, slip)
    Fo, its, res = rb.step_mixed(p, bi, slip=slip, max_iter=200, rtol=1e-10)
    X1, Q1 = rb.get_config()
    Xo, Qo = O.evolve(c["X"], O.normalize_quats(np.asarray(c["Q"], dtype=np.float64)), U_d, dt)
    print("step_mixed wall=%s block=%s: %d iterations; |X - X_ref| %.2e, |Q - Q_ref| %.2e, rel. diff F %.2e"
          % (wall, block, its, np.abs(X1 - Xo).max(), np.abs(Q1 - Qo).max(), _rel(Fo, F_d)))
    assert 0 < its < 200 and res < 1e-10
    assert np.abs(X1 - Xo).max() <= 1e-7 and np.abs(Q1 - Qo).max() <= 1e-7 and _rel(Fo, F_d) <= 1e-7
    # five steps: body 1 held, body 4 driven without rotation, the others free under their loads
    c, rb = _body(nb, nblb, wall, block)
    p = np.isin(np.arange(nb), [1, 4])
    bi = np.array(F)
    bi[1] = 0.0
    bi[4] = [0.3, -0.2, 0.1, 0.0, 0.0, 0.0]
    X0, Q0 = (np.array(v) for v in rb.get_config())
    Xprev = X0
    for step in range(5):
        _, its, res = rb.step_mixed(p, bi, max_iter=200, rtol=1e-10)
        assert 0 < its < 200 and res < 1e-10
        Xs = np.array(rb.get_config()[0])
        # X += dt U: one rounding of the sum (half an ulp of |X|, 1.1e-16 relative); the difference of the two neighbours is exact
        assert np.abs((Xs[4] - Xprev[4]) - dt * bi[4, :3]).max() <= 1e-15 * np.abs(Xs[4]).max()
        Xprev = Xs
    X5, Q5 = rb.get_config()
    assert np.array_equal(X5[1], X0[1]) and np.abs(Q5[1] - Q0[1]).max() <= 1e-15
    assert np.abs(X5[0] - X0[0]).max() > 1e-4                        # the free ones moved


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_step_mixed_with_the_force_model(wall, block):
    nb, nblb = 10, 12
    F, Up, _ = _inputs(nb, nblb, seed=16)
    none, everyone = np.zeros(nb, dtype=bool), np.ones(nb, dtype=bool)
    # nobody prescribed: the deterministic step, model included
    _, rb1 = _body(nb, nblb, wall, block)
    _, rb2 = _body(nb, nblb, wall, block)
    rb1.set_interactions(**MODEL)
    rb2.set_interactions(**MODEL)
    its1, _ = rb1.step_deterministic(F.reshape(-1), max_iter=200, rtol=1e-10)
    _, its2, _ = rb2.step_mixed(none, F.reshape(-1), max_iter=200, rtol=1e-10)
    (Xa, Qa), (Xb, Qb) = rb1.get_config(), rb2.get_config()
    print("model on, nobody prescribed, wall=%s block=%s: step_deterministic %d iterations, step_mixed %d; |dX| %.2e |dQ| %.2e"
          % (wall, block, its1, its2, np.abs(Xa - Xb).max(), np.abs(Qa - Qb).max()))
    assert np.abs(Xa - Xb).max() <= 1e-7 and np.abs(Qa - Qb).max() <= 1e-7
    # everybody prescribed: no free body feels the model -- bitwise the model-off run
    out = []
    for on in (False, True):
        _, rb = _body(nb, nblb, wall, block)
        if on:
            rb.set_interactions(**MODEL)
        lam, U, Fs, its, res = rb.solve_mixed(everyone, Up.reshape(-1), max_iter=200, rtol=1e-10)
        Fo, its_s, res_s = rb.step_mixed(everyone, Up.reshape(-1), max_iter=200, rtol=1e-10)
        X, Q = rb.get_config()
        out.append((lam, U, Fs, Fo, X, Q, its, its_s))
    for a, b in zip(*out):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.array_equal(out[0][2], out[0][3])                      # the step's F is the solve's


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_force_model_enters_the_free_bodies_only(wall, block):
    """model on, three bodies prescribed: the step leaves the prescribed velocities alone (U echoed: they advance by dt U exactly
    as without the model) and solves the free bodies with their loads plus the model's, -K^T f_phys = interaction_forces(), in
    the free slots -- bitwise what solve_mixed returns when it is handed those loads"""
    nb, nblb, dt = 10, 12, 0.01
    p = _sets(nb)["three"]
    F, Up, slip = _inputs(nb, nblb, seed=22)
    bi = _body_in(p, F, Up).reshape(nb, 6)
    c, rb = _body(nb, nblb, wall, block, dt=dt)
    rb.set_interactions(**MODEL)
    share = rb.interaction_forces().reshape(nb, 6)
    assert np.abs(share[p]).max() > 1e-3 and np.abs(share[~p]).max() > 1e-3      # the model does load prescribed bodies too
    bi_model = np.where(p[:, None], bi, bi + share)
    lam, U, Fs, its, res = rb.solve_mixed(p, bi_model, slip=slip, max_iter=200, rtol=1e-10)
    assert np.array_equal(U.reshape(nb, 6)[p], Up[p])                            # prescribed velocities: bitwise body_in
    X0, Q0 = (np.array(v) for v in rb.get_config())
    Fo, its_s, res_s = rb.step_mixed(p, bi, slip=slip, max_iter=200, rtol=1e-10)
    print("model on, 3 of 10 prescribed, wall=%s block=%s: %d iterations; |F_step - F_solve| %.2e"
          % (wall, block, its_s, np.abs(Fo - Fs).max()))
    assert its_s == its and res_s == res and np.array_equal(Fo, Fs)              # the same system: the same bits
    assert np.array_equal(Fo.reshape(nb, 6)[~p], bi_model[~p])                   # free loads echoed WITH the model's share
    from oracle import oracle as O
    Xo, Qo = O.evolve(X0, Q0, U, dt)
    X1, Q1 = rb.get_config()
    assert np.abs(X1 - Xo).max() <= 1e-14 and np.abs(Q1 - Qo).max() <= 1e-14     # the step moved the bodies with that U
    assert np.abs((X1[p] - X0[p]) - dt * Up[p, :3]).max() <= 1e-15 * np.abs(X1).max()
    # without the mask (model loads added to the prescribed slots too) the answer would differ by far more than rounding
    _, rb2 = _body(nb, nblb, wall, block, dt=dt)
    _, U_bad, _, _, _ = rb2.solve_mixed(p, bi + share, slip=slip, max_iter=200, rtol=1e-10)
    assert _rel(U_bad, U) > 1e-4


def test_cfg2_residual_round_trip_and_reproducibility():
    nb, nblb = 50, 162
    p = np.zeros(nb, dtype=bool)
    p[np.random.default_rng(6).permutation(nb)[:10]] = True
    rb, first = _residual_case(nb, nblb, True, True, p, seed=17, label="residual cfg 2")
    F, Up, slip = _inputs(nb, nblb, seed=17)
    again = rb.solve_mixed(p, _body_in(p, F, Up), slip=slip, max_iter=200, rtol=1e-10)
    for a, b in zip(first, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()     # two calls: bitwise equal
    _round_trip(nb, nblb, True, True, p, seed=18, label="round trip cfg 2")


def test_cfg3_one_solve_residual():
    nb, nblb = 200, 642
    p = np.zeros(nb, dtype=bool)
    p[np.random.default_rng(7).permutation(nb)[:50]] = True
    _residual_case(nb, nblb, True, True, p, seed=19, label="residual cfg 3")


def test_small_systems_reproducible_call_to_call():
    for wall, block in WALL_BLOCK:
        c, rb = _body(10, 12, wall, block)
        p = _sets(10)["three"]
        F, Up, slip = _inputs(10, 12, seed=20)
        a = rb.solve_mixed(p, _body_in(p, F, Up), slip=slip, max_iter=200, rtol=1e-10)
        b = rb.solve_mixed(p, _body_in(p, F, Up), slip=slip, max_iter=200, rtol=1e-10)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


_POISON_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from oracle import Oracle
import test_prescribed_gpu as t
from rigid_body_light_amd import RigidBody, make_config
c = make_config(2, 12, False)
assert RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 0.01).cb.get_option("poison_workspace") == 1
orc = Oracle()
for wall, block in t.WALL_BLOCK:
    for which in ("none", "three", "all"):
        t._dense_parity(orc, wall, block, which)
print("ALL OK")
"""


def test_dense_parity_with_poisoned_workspaces():
    """every device workspace filled with NaN at each reserve (RBL_POISON_WORKSPACE=1, a child process): a read of memory
    nobody wrote fails the dense parity"""
    env = dict(os.environ, RBL_POISON_WORKSPACE="1")
    p = subprocess.run([sys.executable, "-c", _POISON_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout


# The second shape, 17 x shell_N_162 = 2754 blobs: a blob vector is 66 096 bytes, the smallest from the shipped structures above the
# 64 KB at which the host form's copies go through the staging buffer, synchronously; below it (10 x 12) both forms copy
# asynchronously.  Iterations to 1e-8 there, before the two forms shared their code and since: 18 (printed; max_iter 200 is
# more than twice that and below 254).
def _dev_form_equals_the_host_form(nb, nblb, max_iter, rtol):
    import torch
    from rigid_body_light_amd._lib import DeviceContext, lib
    wall = True
    c, rb = _body(nb, nblb, wall, True)
    p = _sets(nb)["three"]
    F, Up, slip = _inputs(nb, nblb, seed=21)
    bi = _body_in(p, F, Up)
    host = rb.solve_mixed(p, bi, slip=slip, max_iter=max_iter, rtol=rtol)
    print("dev form against host form, %d x %d: %d iterations to %.0e, residual %.2e" % (nb, nblb, host[3], rtol, host[4]))
    assert 0 < host[3] < max_iter and host[4] < rtol
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
    lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_config(c["X"], c["Q"])
    dev = torch.device("cuda:0")
    d_bi, d_slip = torch.from_numpy(bi).to(dev), torch.from_numpy(slip).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    d_lam, d_U, d_F = nan(3 * nb * nblb), nan(6 * nb), nan(6 * nb)
    its, res = ctx.solve_mixed_dev(p, d_bi.data_ptr(), d_slip.data_ptr(), max_iter, rtol, d_lam.data_ptr(), d_U.data_ptr(), d_F.data_ptr())
    ctx.sync_check()
    assert its == host[3] and res == host[4]
    for got, want in zip((d_lam, d_U, d_F), host[:3]):
        assert np.array_equal(got.cpu().numpy(), want)
    lam_h, U_h, F_h, its_h, _ = ctx.solve_mixed(p, bi, max_iter=max_iter, rtol=rtol, slip=slip)
    assert its_h == its and np.array_equal(lam_h, host[0]) and np.array_equal(U_h, host[1]) and np.array_equal(F_h, host[2])
    ctx.close()


def test_dev_form_equals_the_host_form():
    _dev_form_equals_the_host_form(10, 12, 200, 1e-10)
    _dev_form_equals_the_host_form(17, 162, 200, 1e-8)


def test_cost_per_iteration_at_cfg3_is_the_unconstrained_solve_s():
    """tools/bench_prescribed.py at cfg 3 (wall, block preconditioner, rtol 1e-8; solve_saddle in the same process is the
    yardstick): a mixed iteration is the same pair product (20.5 of ~22 ms) with one pass over the per-body factors; 5 % are
    allowed for a possible second pass and 5 % for the lost fusions -> ms per iteration <= 1.10 x the unconstrained solve's."""
    import json
    p = subprocess.run([sys.executable, "tools/bench_prescribed.py", "--cfgs", "cfg3", "--rounds", "3"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["cfg3"]
    for case in ("mixed_none", "mixed_quarter", "mixed_all"):
        print("cfg 3 %s: %d iterations, %.3f ms per iteration, %.4f x solve_saddle's %.3f"
              % (case, d[case]["iterations"], d[case]["ms_per_iter"], d[case]["ms_per_iter_ratio"], d["solve_saddle"]["ms_per_iter"]))
        assert 0 < d[case]["iterations"] < 200
        assert d[case]["ms_per_iter_ratio"] <= 1.10


def test_held_and_driven_example():
    p = subprocess.run([sys.executable, "examples/held_and_driven.py", "--steps", "4"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l.split() for l in p.stdout.splitlines() if l.startswith("step ")]
    assert len(rows) == 4
    vals = np.array([[float(v) for v in r[2:]] for r in rows])
    assert vals.shape[1] >= 7 and np.all(np.isfinite(vals))
    assert np.all(np.abs(vals[:, 1]) > 0.0)                           # dragging takes a force along the drag
