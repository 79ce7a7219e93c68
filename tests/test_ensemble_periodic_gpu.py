"""Ensembles in a periodic cell (include/rbl.h section 5: rbl_ensemble_set_periodic; Ensemble.set_cell) on the GPU: the image sum
inside the one-kernel solver against dense numpy solves on tests/periodic_oracle.py's matrices, the masked solves, the deterministic
step against the single context with its own cell, the Brownian step against a numpy restatement of the scheme on the oracle's
matrices, the one-step covariance, the bitwise properties, the minimum-image forces per replica, and the errors.

Tolerances are the project's own for the same comparisons (head of tests/test_periodic_gpu.py): 1e-7 relative for a solve to rtol
1e-10 against the dense solve, 1e-7 for what contains the difference quotient, the bound of test_pair_forces_by_minimum_image
(1e-12) for forces.  Iteration counts are printed (run with -s) and asserted only as "converged within max_iter" = 200: the
image-free diagonal preconditioner's count in a cell is whatever it is.

The shapes: A 4 tetrahedra (16 blobs: even N, one row block of the pair sweep), B 3 trimers (9: odd N, no half offset), C one body of
7 blobs alone (every image term is an own-image term), D 10 x shell_N_12 (120: two row blocks, the second ragged, and the half
offset of an even N), E 2 x 65 blobs (130: three row blocks, the last of two lanes; beyond the dense oracle, so against the single
context)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ETA = 1.0
SOLVE = dict(max_iter=200, rtol=1e-10)


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _ens(cfg, a, X, Q, dt=0.01, kBT=1.0, wall=True):
    from rigid_body_light_amd import Ensemble
    return Ensemble(cfg, np.asarray(X), np.asarray(Q), a, ETA, dt, kBT=kBT, wall=wall)


def _stack(cases):
    return np.stack([c["X"] for c in cases]), np.stack([c["Q"] for c in cases])


def _case_A(s):
    return pc.layers("tetra", 4, 2, 2, seed=s)


def _D_replicas():
    """D itself and two copies with the bodies displaced by up to 0.05"""
    c = pc.layer10()
    rng = np.random.default_rng(51)
    X = np.stack([c["X"], c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape), c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape)])
    return c, X, np.stack([c["Q"]] * 3)


@pytest.fixture(scope="module")
def D(orc):
    """10 x shell_N_12 in layer10()'s cell as three replicas, with the dense B M_per B of every replica for images (1, 1) and (2, 1):
    every pair evaluated once, shared by the tests below, never written to"""
    from oracle import oracle as O
    c, X, Q = _D_replicas()
    cfg = O.remove_mean(c["cfg"])
    M, K = [], []
    for r in range(3):
        Qn = O.normalize_quats(Q[r])
        pos = orc.multi_body_pos(X[r], Qn, cfg)
        T = po.image_terms(orc, pos, c["a"], ETA, c["L"], (2, 1))
        B = orc.damp(pos.reshape(-1), c["a"])
        M.append({(1, 1): po.truncated(T, (1, 1), B), (2, 1): po.truncated(T, (2, 1), B)})
        K.append(O.K_matrix(X[r], Qn, cfg))
        for m in M[-1].values():
            m.setflags(write=False)
    return dict(c=c, X=X, Q=Q, M=M, K=K)


def _dense_saddle(M, K, F, slip):
    n3, nb6 = M.shape[0], K.shape[1]
    x = np.linalg.solve(np.block([[M, -K], [K.T, np.zeros((nb6, nb6))]]), np.concatenate([slip, -F]))
    return x[:n3], x[n3:]


def _np_masked(M, K, P6, body_in, slip):
    """the masked system of include/rbl.h section 7 on M: P6 (N_bod, 6) bool, body_in (6 N_bod,) -> (lambda, U, F)"""
    n3 = M.shape[0]
    free = ~P6.reshape(-1)
    Kf, Kp = K[:, free], K[:, ~free]
    nf = Kf.shape[1]
    x = np.linalg.solve(np.block([[M, -Kf], [Kf.T, np.zeros((nf, nf))]]), np.concatenate([slip + Kp @ body_in[~free], -body_in[free]]))
    U, F = body_in.copy(), body_in.copy()
    U[free] = x[n3:]
    F[~free] = -(Kp.T @ x[:n3])
    return x[:n3], U, F


def _inputs(R, nb, n3, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, 6 * nb)), 0.1 * rng.standard_normal((R, n3))


def _free_solve(ens, F, slip):
    nb = ens.N_bodies
    lam, U, _, its, res = ens.solve_mixed(np.zeros(nb, dtype=bool), F, slip=slip, **SOLVE)
    assert (its > 0).all() and (its < SOLVE["max_iter"]).all() and (res < SOLVE["rtol"]).all(), (its, res)
    return lam, U, its


# ------------------------------------------------------------------------------------------------------ 1: the operator, by the solve
CASES_1 = [("A", (1, 1), "xy"), ("A", (2, 1), "xy"), ("A", (16, 1), "xy"), ("A", (1, 0), "x"), ("A", (0, 3), "y"), ("B", (1, 1), "xy"),
           ("C", (1, 1), "xy")]


@pytest.mark.parametrize("name,images,axes", CASES_1)
def test_solve_against_the_dense_solve_with_M_per(orc, name, images, axes):
    build = {"A": _case_A, "B": lambda s: pc.layers("trimer", 3, 3, 1, seed=s), "C": lambda s: pc.layers("fib7", 1, 1, 1, seed=s, extra=(1, 1))}[name]
    cases = [build(s) for s in (0, 1, 2)]
    c = cases[0]
    L = (c["L"][0] if "x" in axes else 0.0, c["L"][1] if "y" in axes else 0.0)
    X, Q = _stack(cases)
    R, nb, n3 = 3, X.shape[1], 3 * X.shape[1] * c["nblb"]
    F, slip = _inputs(R, nb, n3, 61)
    ens = _ens(c["cfg"], c["a"], X, Q)
    lam_open, U_open, _ = _free_solve(ens, F, slip)
    ens.set_cell(L[0], L[1], images=images)
    assert ens.cell() == dict(on=True, Lx=L[0], Ly=L[1], images=images)
    lam, U, its = _free_solve(ens, F, slip)
    lam2, U2, _ = _free_solve(ens, F, slip)
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2)    # one summation order
    for r in range(R):
        M, K, pos = po.dense_matrices(orc, cases[r]["cfg"], X[r], Q[r], c["a"], ETA, L, images)
        lam_d, U_d = _dense_saddle(M, K, F[r], slip[r])
        print("%s seed %d, cell %.2f x %.2f, images %s: %d iterations, rel. diff lambda %.2e U %.2e, against the open system %.2e"
              % (name, r, L[0], L[1], images, its[r], _rel(lam[r], lam_d), _rel(U[r], U_d), _rel(U[r], U_open[r])))
        assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7
        if name == "C":                                           # one body alone: what the cell adds is its own images, and they count
            assert _rel(U[r], U_open[r]) > 1e-3
        if name == "A":                                           # the own-image term alone is seen: without it the answer is another
            T = po.image_terms(orc, pos, c["a"], ETA, L, images)
            B = orc.damp(pos.reshape(-1), c["a"])
            own = np.zeros_like(M)
            for pq, t in T.items():
                if pq != (0, 0):
                    for i in range(n3 // 3):
                        own[3 * i:3 * i + 3, 3 * i:3 * i + 3] += t[3 * i:3 * i + 3, 3 * i:3 * i + 3]
            _, U_no = _dense_saddle(M - B[:, None] * own * B[None, :], K, F[r], slip[r])
            assert _rel(U[r], U_no) > 1e-4, _rel(U[r], U_no)
    ens.close()


@pytest.mark.parametrize("images", [(1, 1), (2, 1)])
def test_solve_on_two_row_blocks_against_the_dense_solve(D, images):
    c = D["c"]
    F, slip = _inputs(3, 10, 360, 62)
    ens = _ens(c["cfg"], c["a"], D["X"], D["Q"])
    ens.set_cell(c["L"][0], c["L"][1], images=images)
    lam, U, its = _free_solve(ens, F, slip)
    for r in range(3):
        lam_d, U_d = _dense_saddle(D["M"][r][images], D["K"][r], F[r], slip[r])
        print("D replica %d, images %s: %d iterations, rel. diff lambda %.2e U %.2e" % (r, images, its[r], _rel(lam[r], lam_d), _rel(U[r], U_d)))
        assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7
    ens.close()


# ------------------------------------------------------------------------------------------------------ 2: masks
def test_masked_solves_against_the_masked_system_on_M_per(orc):
    cases = [_case_A(s) for s in (0, 1, 2)]
    c = cases[0]
    L, images = c["L"], (1, 1)
    X, Q = _stack(cases)
    R, nb, n3 = 3, 4, 48
    rng = np.random.default_rng(63)
    body_in, slip = rng.standard_normal((R, 6 * nb)), 0.1 * rng.standard_normal((R, n3))
    ens = _ens(c["cfg"], c["a"], X, Q)
    ens.set_cell(L[0], L[1], images=images)
    held = np.zeros((nb, 6), dtype=bool); held[0] = True          # body 0 held
    zheld = np.zeros((nb, 6), dtype=bool); zheld[:, 2] = True     # z of every body held
    bi_held = body_in.copy().reshape(R, nb, 6); bi_held[:, 0] = 0.0
    bi_z = body_in.copy().reshape(R, nb, 6); bi_z[:, :, 2] = 0.0
    out_b = ens.solve_mixed(held[:, 0], bi_held.reshape(R, -1), slip=slip, **SOLVE)
    out_z = ens.solve_mixed_dof(zheld, bi_z.reshape(R, -1), slip=slip, **SOLVE)
    for label, P6, bi, (lam, U, Fo, its, res) in (("body 0 held", held, bi_held, out_b), ("z held", zheld, bi_z, out_z)):
        assert (its > 0).all() and (its < 200).all() and (res < 1e-10).all()
        for r in range(R):
            M, K, _ = po.dense_matrices(orc, c["cfg"], X[r], Q[r], c["a"], ETA, L, images)
            lam_d, U_d, F_d = _np_masked(M, K, P6, bi[r].reshape(-1), slip[r])
            print("%s, replica %d: %d iterations, rel. diff lambda %.2e U %.2e F %.2e" % (label, r, its[r], _rel(lam[r], lam_d), _rel(U[r], U_d), _rel(Fo[r], F_d)))
            assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7 and _rel(Fo[r], F_d) <= 1e-7
    ens.close()


# ------------------------------------------------------------------------------------------------------ 3: the deterministic step
def _single_step(c, X, Q, L, images, F, slip, dt):
    from rigid_body_light_amd import RigidBody
    rb = RigidBody(c["cfg"], X, Q, c["a"], ETA, dt, wall_PC=True, block_PC=False)
    rb.set_periodic(L[0], L[1], images=images)
    its, res = rb.step_deterministic(F, slip=slip, **SOLVE)
    assert 0 < its < 200 and res < 1e-10
    X1, Q1 = rb.get_config()
    return np.asarray(X1).reshape(-1, 3), np.asarray(Q1).reshape(-1, 4), its


@pytest.mark.parametrize("name", ["D", "E"])
def test_deterministic_step_equals_the_single_context_step_in_its_cell(name):
    if name == "D":
        c, X, Q = _D_replicas()
    else:
        c = pc.layers("fib65", 2, 2, 1)
        X = np.stack([c["X"], c["X"] + np.random.default_rng(52).uniform(-0.05, 0.05, c["X"].shape)])
        Q = np.stack([c["Q"]] * 2)
    R, nb = X.shape[0], X.shape[1]
    n3 = 3 * nb * c["cfg"].shape[0]
    assert n3 == (360 if name == "D" else 390)
    dt, L, images = 0.01, c["L"], (1, 1)
    F, slip = _inputs(R, nb, n3, 64)
    ens = _ens(c["cfg"], c["a"], X, Q, dt=dt)
    ens.set_cell(L[0], L[1], images=images)
    its, res = ens.step_deterministic(F, slip=slip, **SOLVE)
    assert (its > 0).all() and (its < 200).all() and (res < 1e-10).all()
    Xe, Qe = ens.get_config()
    ens.close()
    Qn = Q / np.linalg.norm(Q, axis=2, keepdims=True)
    for r in range(R):
        Xs, Qs, its_s = _single_step(c, X[r], Q[r], L, images, F[r], slip[r], dt)
        moved_X, moved_Q = np.abs(Xs - X[r]).max(), np.abs(Qs - Qn[r]).max()
        print("%s replica %d: %d iterations (single context %d), X differs by %.2e of a displacement of %.2e, Q by %.2e of %.2e"
              % (name, r, its[r], its_s, np.abs(Xe[r] - Xs).max() / moved_X, moved_X, np.abs(Qe[r] - Qs).max() / moved_Q, moved_Q))
        assert moved_X > 1e-4 and np.abs(Xe[r] - Xs).max() <= 1e-7 * moved_X and np.abs(Qe[r] - Qs).max() <= 1e-7 * moved_Q


def test_the_unmasked_step_keeps_its_bits_where_the_basis_crosses_64_kb_of_lds():
    """2 x shell_N_12 in a cell, three replicas, the unmasked k_gmres_small_per: with max_iter = 40 the vectors and the Krylov basis
    take 51 184 bytes of LDS, with max_iter = 100 87 344 (body_shapes' restatement of the launcher's arithmetic), more than the
    64 KB a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize and less than the solver's 153 600.  The step converges
    to 1e-10 below both caps -- the numpy GMRES with the diagonal preconditioner on B M_per B (joint_oracle.gmres_right_pc) takes 28
    iterations for each of the three replicas -- so both calls do the same arithmetic: iteration counts, residuals and the new
    configurations are the same bits"""
    import body_shapes as bs
    from rigid_body_light_amd.synth import make_config
    c = make_config(2, 12, True)
    s = pc.spacing(c["a"])
    rng = np.random.default_rng(71)
    R, caps = 3, (40, 100)
    X = np.stack([c["X"]] + [c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape) for _ in range(R - 1)])
    F, slip = rng.standard_normal((R, 12)), 0.1 * rng.standard_normal((R, 72))
    total = [bs.small_lds_bytes(12, 2, m) + bs.small_basis_bytes(12, 2, m) for m in caps]
    assert total == [51184, 87344] and total[0] <= 64 * 1024 < total[1] <= bs.SMALL_LDS_MAX
    got = []
    for m in caps:
        ens = _ens(c["cfg"], c["a"], X, np.stack([c["Q"]] * R))
        ens.set_cell(2.0 * s, s + 0.7, images=(1, 1))
        its, res = ens.step_deterministic(F, slip=slip, max_iter=m, rtol=1e-10)
        got.append((its, res) + tuple(ens.get_config()))
        ens.close()
    its, res = got[0][:2]
    print("2 bodies in a cell, max_iter 40 and 100: %s iterations, residual estimates <= %.1e" % (its.tolist(), res.max()))
    assert (its > 0).all() and (its < caps[0]).all() and (res < 1e-10).all()
    for p, q in zip(*got):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()
    assert np.abs(got[0][2] - X).max() > 1e-4                  # the replicas moved


# ------------------------------------------------------------------------------------------------------ 4: the Brownian step
def _np_brownian_step(orc, cfg, X, Qn, a, L, images, dt, kBT, P6, body_in, slip, W, split_rand, delta=1e-4):
    """the stochastic midpoint step of rbl_ensemble.hip restated on the oracle's matrices of the cell: the root from
    numpy.linalg.cholesky(B M_per B), the drift from the difference quotient at q +- delta / 2 dq with po.dense_M, the masked
    midpoint solve -> (X, Q, F)"""
    from oracle import oracle as O
    n3 = slip.size
    W1, W2, Wr = W[:n3], W[n3:2 * n3], W[2 * n3:]
    assert np.array_equal(P6[:, 3:].any(axis=1), P6[:, 3:].all(axis=1))
    Df = (~P6).reshape(-1).astype(np.float64)
    M = po.dense_M(orc, orc.multi_body_pos(X, Qn, cfg), a, ETA, L, images)
    Lc = np.linalg.cholesky(M)
    mw1, mw2 = Lc @ W1, Lc @ W2
    Kinv = O.Kinv_matrix(X, Qn, cfg)
    dq = Df * (Kinv @ Wr)
    Xp, Qp = O.update_X_Q(X, Qn, 0.5 * delta * dq)
    Xm, Qm = O.update_X_Q(X, Qn, -0.5 * delta * dq)
    rfd = (po.dense_M(orc, orc.multi_body_pos(Xp, Qp, cfg), a, ETA, L, images) @ Wr
           - po.dense_M(orc, orc.multi_body_pos(Xm, Qm, cfg), a, ETA, L, images) @ Wr) / delta
    if split_rand:
        c1, c2 = 2.0 * np.sqrt(kBT / dt), np.sqrt(kBT / dt)
        BI = c2 * (mw1 - mw2)
    else:
        c1 = c2 = np.sqrt(2.0 * kBT / dt)
        BI = c2 * mw1
    s = slip - kBT * rfd - BI
    Up = np.where(P6.reshape(-1), body_in, 0.0)
    Xh, Qh = O.update_X_Q(X, Qn, Df * (0.5 * dt * c1) * (Kinv @ mw1) + (1.0 - Df) * (0.5 * dt) * Up)
    Mh = po.dense_M(orc, orc.multi_body_pos(Xh, Qh, cfg), a, ETA, L, images)
    _, U, F = _np_masked(Mh, O.K_matrix(Xh, Qh, cfg), P6, body_in, s)
    Xn, Qn1 = O.evolve(X, Qn, U, dt)
    return Xn, Qn1, F


@pytest.mark.parametrize("split_rand", [True, False])
@pytest.mark.parametrize("mask", ["free", "body", "z"])
def test_brownian_step_with_injected_noise_against_the_numpy_restatement(orc, split_rand, mask):
    from oracle import oracle as O
    cases = [_case_A(s) for s in (0, 1, 2)]
    c = cases[0]
    L, images, dt, kBT = c["L"], (1, 1), 0.01, 1.0
    X, Q = _stack(cases)
    R, nb, n3 = 3, 4, 48
    rng = np.random.default_rng(65)
    body_in, slip, W = rng.standard_normal((R, nb, 6)), 0.1 * rng.standard_normal((R, n3)), rng.standard_normal((R, 3 * n3))
    P6 = np.zeros((nb, 6), dtype=bool)
    if mask == "body":
        P6[0] = True
        body_in[:, 0] = [0.02, 0.0, 0.01, 0.0, 0.03, 0.0]         # driven
    elif mask == "z":
        P6[:, 2] = True
        body_in[:, :, 2] = 0.0
    body_in = body_in.reshape(R, 6 * nb)
    ens = _ens(c["cfg"], c["a"], X, Q, dt=dt, kBT=kBT)
    ens.set_cell(L[0], L[1], images=images)
    kw = dict(W=W, split_rand=split_rand, slip=slip, **SOLVE)
    if mask == "free":
        its, res = ens.step_brownian(body_in, **kw)
        Fo = None
    elif mask == "body":
        Fo, its, res = ens.step_brownian_mixed(P6[:, 0], body_in, **kw)
    else:
        Fo, its, res = ens.step_brownian_mixed_dof(P6, body_in, **kw)
    assert (its > 0).all() and (its < 200).all() and (res < 1e-10).all()
    Xe, Qe = ens.get_config()
    ens.close()
    cfg = O.remove_mean(c["cfg"])
    for r in range(R):
        Qn = O.normalize_quats(Q[r])
        Xn, Qn1, F_d = _np_brownian_step(orc, cfg, X[r], Qn, c["a"], L, images, dt, kBT, P6, body_in[r], slip[r], W[r], split_rand)
        moved_X, moved_Q = np.abs(Xn - X[r]).max(), np.abs(Qn1 - Qn).max()
        print("A %s split_rand=%s replica %d: %d iterations, X differs by %.2e of a displacement of %.2e, Q by %.2e of %.2e"
              % (mask, split_rand, r, its[r], np.abs(Xe[r] - Xn).max() / moved_X, moved_X, np.abs(Qe[r] - Qn1).max() / moved_Q, moved_Q))
        assert np.abs(Xe[r] - Xn).max() <= 1e-7 * moved_X and np.abs(Qe[r] - Qn1).max() <= 1e-7 * moved_Q
        if Fo is not None:
            pres = P6.reshape(-1)
            assert _rel(Fo[r][pres], F_d[pres]) <= 1e-7


# ------------------------------------------------------------------------------------------------------ 5: the covariance
def test_one_step_covariance_is_2_kBT_dt_N_of_the_cell(orc):
    """the statistic and the bound of tests/test_ensemble_gpu.py::test_one_step_covariance_is_2_kBT_dt_N, with
    N = (K^T M_per^-1 K)^-1 from the oracle: many replicas from one configuration of A"""
    c = _case_A(0)
    R, dt, kBT, nb, L, images = 4096, 1e-3, 1.0, 4, c["L"], (1, 1)
    X0, Q0 = c["X"], c["Q"] / np.linalg.norm(c["Q"], axis=1, keepdims=True)
    ens = _ens(c["cfg"], c["a"], np.repeat(X0[None], R, axis=0), np.repeat(Q0[None], R, axis=0), dt=dt, kBT=kBT)
    ens.set_cell(L[0], L[1], images=images)
    its, res = ens.step_brownian(np.zeros(6 * nb), seed=2025, max_iter=100, rtol=1e-12)
    assert (its < 100).all()
    X, Q = ens.get_config()
    ens.close()
    D = []
    for b in range(nb):
        dX = X[:, b] - X0[b]
        q, q0 = Q[:, b], Q0[b] * [1, -1, -1, -1]                  # q_rel = q (x) q0^-1
        w = q[:, 0] * q0[0] - q[:, 1:] @ q0[1:]
        v = q[:, :1] * q0[1:] + q0[0] * q[:, 1:] + np.cross(q[:, 1:], q0[1:])
        s = np.linalg.norm(v, axis=1)
        rot = (2 * np.arctan2(s, w) / np.where(s > 0, s, 1.0))[:, None] * v
        D.append(np.concatenate([dX, rot], axis=1))
    Cov = np.cov(np.concatenate(D, axis=1).T) / (2 * kBT * dt)
    M, K, _ = po.dense_matrices(orc, c["cfg"], X0, Q0, c["a"], ETA, L, images)
    N = np.linalg.inv(K.T @ np.linalg.solve(M, K))
    worst = 0.0
    for i in range(6 * nb):
        for j in range(6 * nb):
            se = np.sqrt((N[i, i] * N[j, j] + N[i, j] ** 2) / (R - 1))
            worst = max(worst, abs(Cov[i, j] - N[i, j]) / se)
            assert abs(Cov[i, j] - N[i, j]) <= 5 * se, (i, j, Cov[i, j], N[i, j], se)
    print("one-step covariance of A in its cell: the worst entry is %.2f standard errors off" % worst)


# ------------------------------------------------------------------------------------------------------ 6: bitwise properties on D
MODEL = dict(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)    # 2 R_body + r_cut = 3.6 <= L / 2


def _D_ens(X, Q, cell=(1, 1), dt=0.01, model=True):
    c = pc.layer10()
    ens = _ens(c["cfg"], c["a"], X, Q, dt=dt)
    if model:
        ens.set_interactions(**MODEL)
    if cell is not None:
        ens.set_cell(c["L"][0], c["L"][1], images=cell)
    return ens


def _two_steps(ens, F, slip, W):
    """a deterministic and a Brownian step -> the configurations after each, the forces before"""
    FT = ens.interaction_forces()
    ens.step_deterministic(F, slip=slip, max_iter=200, rtol=1e-8)
    a = ens.get_config()
    ens.step_brownian(F, W=W, slip=slip, max_iter=200, rtol=1e-8)
    b = ens.get_config()
    return FT, a[0], a[1], b[0], b[1]


def test_two_calls_agree_and_a_replica_does_not_see_the_others():
    _, X, Q = _D_replicas()
    R, nb, n3 = 3, 10, 360
    F, slip = _inputs(R, nb, n3, 66)
    W = np.random.default_rng(67).standard_normal((R, 3 * n3))
    outs = []
    for _ in range(2):
        ens = _D_ens(X, Q)
        outs.append(_two_steps(ens, F, slip, W))
        ens.close()
    for p, q in zip(*outs):
        assert np.array_equal(p, q)                               # two calls on the same input
    assert np.abs(outs[0][3] - X).max() > 1e-4 and np.abs(outs[0][0]).max() > 1e-3
    for r in range(R):                                            # replica r of R = 3 is the R = 1 call
        ens = _D_ens(X[r:r + 1], Q[r:r + 1])
        one = _two_steps(ens, F[r:r + 1], slip[r:r + 1], W[r:r + 1])
        ens.close()
        for p, q in zip(outs[0], one):
            assert np.array_equal(p[r], q[0]), r
    X2, Q2 = X.copy(), Q.copy()                                   # another replica 1 leaves replica 0's forces and steps alone
    X2[1] += np.random.default_rng(68).uniform(-0.05, 0.05, X2[1].shape)
    ens = _D_ens(X2, Q2)
    other = _two_steps(ens, F, slip, W)
    ens.close()
    for p, q in zip(outs[0], other):
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[2], q[2]) and not np.array_equal(p[1], q[1])


@pytest.mark.parametrize("family", ["deterministic", "brownian", "masked deterministic", "masked brownian"])
def test_a_run_of_five_steps_is_five_one_step_calls_bitwise(family):
    _, X, Q = _D_replicas()
    R, nb, n3, steps = 3, 10, 360, 5
    F, slip = _inputs(R, nb, n3, 69)
    F *= 0.3
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 2] = True
    body_in = F.copy().reshape(R, nb, 6)
    body_in[mask] = [0.02, 0.0, 0.01, 0.0, 0.03, 0.0]
    body_in = body_in.reshape(R, 6 * nb)
    kw = dict(max_iter=200, rtol=1e-8)
    brownian, masked = "brownian" in family, "masked" in family
    ens = _D_ens(X, Q)
    cfgs, its = [], []
    for n in range(steps):
        if masked and brownian:
            it = ens.step_brownian_mixed(mask, body_in, seed=40 + n, slip=slip, **kw)[1]
        elif masked:
            it = ens.step_mixed(mask, body_in, slip=slip, **kw)[1]
        elif brownian:
            it = ens.step_brownian(F, seed=40 + n, slip=slip, **kw)[0]
        else:
            it = ens.step_deterministic(F, slip=slip, **kw)[0]
        assert (it < 200).all()
        its.append(it); cfgs.append(ens.get_config())
    ens.close()
    ens = _D_ens(X, Q)
    if masked:
        out = ens.run(steps, prescribed=mask, body_in=body_in, brownian=brownian, seed=40, stride=1, slip=slip, **kw)
    else:
        out = ens.run(steps, F=F, brownian=brownian, seed=40, stride=1, slip=slip, **kw)
    Xr, Qr = ens.get_config()
    ens.close()
    print("%s run in the cell: %s iterations over %d steps" % (family, out.iters_sum, steps))
    assert np.array_equal(Xr, cfgs[-1][0]) and np.array_equal(Qr, cfgs[-1][1])
    assert out.X.shape == (steps, R, nb, 3)
    for k in range(steps):                                        # a frame per step
        assert np.array_equal(out.X[k], cfgs[k][0]) and np.array_equal(out.Q[k], cfgs[k][1]), k
    assert np.array_equal(out.iters_sum, np.sum(its, axis=0)) and np.array_equal(out.accepted, np.full(R, steps))
    assert np.abs(Xr - X).max() > 1e-4


def test_a_cell_switched_off_is_a_cell_never_set_bitwise():
    _, X, Q = _D_replicas()
    F, slip = _inputs(3, 10, 360, 70)
    W = np.random.default_rng(71).standard_normal((3, 1080))
    c = pc.layer10()
    outs = []
    for with_cell in (False, True, "on"):
        ens = _D_ens(X, Q, cell=None)
        if with_cell:
            ens.set_cell(c["L"][0], c["L"][1], images=(2, 1))
        if with_cell is True:
            ens.set_cell(c["L"][0], c["L"][1], images=(2, 1), on=False)
            assert ens.cell() == dict(on=False, Lx=c["L"][0], Ly=c["L"][1], images=(2, 1))
        outs.append(_two_steps(ens, F, slip, W))
        ens.close()
    for p, q in zip(outs[0], outs[1]):
        assert np.array_equal(p, q)
    assert not np.array_equal(outs[0][1], outs[2][1])             # ... and the cell that is on does change the step


def test_a_lattice_translation_of_one_body_leaves_the_solve_alone():
    """body 3 of every replica moved by (2 Lx, -Ly): U changes by no more than the bound of the single context's translation test
    (tests/test_periodic_gpu.py: 1e-12, the rounding of the larger coordinates); coordinates stay unwrapped"""
    c, X, Q = _D_replicas()
    F, slip = _inputs(3, 10, 360, 72)
    X1 = X.copy()
    X1[:, 3, 0] += 2.0 * c["L"][0]
    X1[:, 3, 1] -= c["L"][1]
    U = []
    for Xc in (X, X1):
        ens = _D_ens(Xc, Q, model=False)
        U.append(ens.solve_mixed(np.zeros(10, dtype=bool), F, slip=slip, max_iter=200, rtol=1e-13)[1])
        assert np.array_equal(ens.get_config()[0], Xc)
        ens.close()
    print("U after a lattice translation of one body: rel. change %.2e" % _rel(U[1], U[0]))
    assert _rel(U[1], U[0]) <= 1e-12


# ------------------------------------------------------------------------------------------------------ 7: forces
@pytest.mark.parametrize("which", ["steric", "table"])
def test_interaction_forces_per_replica_by_minimum_image(which):
    c, X, Q = _D_replicas()
    X, Q = X[:2], Q[:2]
    a, L = c["a"], c["L"]
    steric = (1.5, 0.1, 2.0 * a + 2.0) if which == "steric" else None
    table = pc.PAIR_TABLE if which == "table" else None
    ens = _D_ens(X, Q, model=False)
    if steric:
        ens.set_interactions(eps_blob=steric[0], b_blob=steric[1], r_cut=steric[2], **pc.BUILTIN)
    else:
        ens.set_pair_table(*table)
    FT, E = ens.interaction_forces(), ens.interaction_energy()
    assert np.array_equal(FT, ens.interaction_forces())
    for r in range(2):
        pos = pc.blob_positions(c["cfg"], X[r], Q[r])
        ref = po.force_model(pos, X[r], 12, a, L, builtin=pc.BUILTIN if steric else None, steric=steric, table=table)
        print("%s, replica %d: body forces / torques rel. error %.2e, energy %.2e (%d direct pairs, %d through a boundary)"
              % (which, r, _rel(-FT[r], ref["FT"]), abs(E[r] - ref["E"]) / abs(ref["E"]), ref["direct"], ref["through"]))
        assert ref["through"] > 0 and np.abs(ref["FT"]).max() > 1e-3
        assert _rel(-FT[r], ref["FT"]) <= 1e-12 and abs(E[r] - ref["E"]) <= 1e-12 * abs(ref["E"])
    # a cell too small for the cutoff: RBL_ERR_ARG naming the length and the bound; the ensemble stays usable
    from rigid_body_light_amd._lib import RblError
    ens.set_cell(7.0, L[1], images=(1, 1))
    with pytest.raises(RblError, match=r"periodic cell too small: Lx = 7\.0.*status 11"):
        ens.interaction_forces()
    ens.set_cell(L[0], L[1], images=(1, 1))
    assert np.array_equal(ens.interaction_forces(), FT)
    ens.close()


# ------------------------------------------------------------------------------------------------------ 8: errors
def test_an_overlap_through_the_boundary_names_its_replica_and_moves_nobody():
    from rigid_body_light_amd._lib import RblError
    cases = [_case_A(s) for s in (0, 1, 2)]
    c = cases[0]
    X, Q = _stack(cases)
    Q = Q / np.linalg.norm(Q, axis=2, keepdims=True)
    X[1, 1] = X[1, 0] + [c["L"][0], 0.0, 0.0]                     # replica 1: body 1 is body 0's image through the x boundary,
    Q[1, 1] = Q[1, 0]                                             # blob on blob; in the open system they are a cell apart
    F = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], 4)
    ens = _ens(c["cfg"], c["a"], X, Q)
    its, _ = ens.step_deterministic(F, max_iter=100, rtol=1e-8)   # the open system steps
    assert (its < 100).all()
    ens.set_config(X, Q)
    ens.set_cell(c["L"][0], c["L"][1], images=(1, 1))
    for step in ("det", "brown"):
        with pytest.raises(RblError) as e:
            if step == "det":
                ens.step_deterministic(F, max_iter=100, rtol=1e-8)
            else:
                ens.step_brownian(F, seed=1, max_iter=100, rtol=1e-8)
        assert "[rbl status 1]" in str(e.value) and "replica 1" in str(e.value), str(e.value)
        Xc, Qc = ens.get_config()
        assert np.array_equal(Xc, X) and np.array_equal(Qc, Q)    # no replica moved
    out = ens.run(3, F=F, brownian=False, on_error="reject", max_iter=100, rtol=1e-8)
    assert np.array_equal(out.rejected, [0, 3, 0]) and np.array_equal(out.accepted, [3, 0, 3]) and np.array_equal(out.first_status, [0, 1, 0])
    Xc, _ = ens.get_config()
    assert np.array_equal(Xc[1], X[1]) and np.abs(Xc[0] - X[0]).max() > 0.0
    ens.close()


def test_refusals_with_the_cell_on_and_the_single_context_cell_as_before():
    from rigid_body_light_amd import RigidBody
    from rigid_body_light_amd._lib import RblError
    c = _case_A(0)
    X, Q = _stack([c, _case_A(1)])
    F = np.zeros(24)
    # wall off with the cell on: found at use
    free = _ens(c["cfg"], c["a"], X, Q, wall=False)
    free.set_cell(c["L"][0], c["L"][1])
    for call in (lambda: free.step_deterministic(F), lambda: free.step_brownian(F, seed=1), lambda: free.run(2, F=F)):
        with pytest.raises(RblError, match=r"periodic.*wall.*status 7"):
            call()
    free.set_cell(c["L"][0], c["L"][1], on=False)
    free.step_deterministic(F)
    free.close()
    ens = _ens(c["cfg"], c["a"], X, Q)
    ens.set_cell(c["L"][0], c["L"][1])
    # the jointed calls
    for call in (lambda: ens.solve_jointed(F), lambda: ens.step_jointed(F), lambda: ens.joint_state(phi=False)):
        with pytest.raises(RblError, match=r"periodic.*status 7"):
            call()
    # the single context's cell on the same context: still refused, still reported off
    with pytest.raises(RblError, match=r"set_periodic: not offered for ensembles.*status 7"):
        ens.ctx.set_periodic(c["L"][0], c["L"][1])
    assert ens.ctx.periodic() == dict(on=False, Lx=0.0, Ly=0.0, images=(0, 0))
    # a new R keeps the cell; what is offered works with it: the flow term, the moments, the bond state (unwrapped)
    ens.set_config(X[:1], Q[:1])
    assert ens.cell() == dict(on=True, Lx=c["L"][0], Ly=c["L"][1], images=(1, 1)) and ens.R == 1
    ens.set_config(X, Q)
    ens.set_background_flow(G=np.array([[0.0, 0.0, 0.3], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    assert ens.flow_slip().shape == (2, 48) and np.abs(ens.flow_slip()).max() > 0.0
    ens.record_moments()
    ens.set_bonds([[0, 1]], [ens.blob_anchor(0)], [ens.blob_anchor(1)], k=1.0, l0=1.0)
    length = ens.bond_state()[0]
    ens.step_deterministic(F, max_iter=200)
    assert ens.step_moments().shape == (2, 4, 3, 3) and length.shape == (2, 1)
    Rm = ens.body_resistance_matrix(max_iter=200, rtol=1e-10)
    assert Rm.shape == (2, 24, 24) and np.linalg.eigvalsh(0.5 * (Rm[0] + Rm[0].T)).min() > 0.0
    ens.close()
    # the single context's dense build with ITS cell on stays refused
    rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], ETA, 0.01, wall_PC=True)
    rb.set_periodic(c["L"][0], c["L"][1])
    with pytest.raises(RuntimeError, match="periodic"):
        rb.dense_mobility(c["r"], scale_damp=True)


# ------------------------------------------------------------------------------------------------------ 9: the example
def test_example_ensemble_periodic_layer_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_periodic_layer.py"), "--replicas", "8", "--steps", "20",
                          "--stride", "10"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "mean height" in out.stdout and "closest centres" in out.stdout
