"""Replica ensembles with held or driven bodies on the GPU (include/rbl.h section 5, rbl_ensemble_*_mixed): every replica solves
and steps as a single context at its configuration does (rbl_solve_mixed, rbl_step_mixed, rbl_step_brownian_mixed with the
dense root), a prescribed body moves by exactly dt U_p, nobody prescribed is bitwise the unmasked ensemble step, everybody
prescribed gives the resistance matrix, the force model loads the free bodies only, the one-step covariance of a free body next
to a held one is 2 kBT dt (R_ff)^-1, errors leave everything where it was, results are reproducible and read no unwritten
memory, and the example runs.  Bounds are those of test_prescribed_gpu.py and test_brownian_mixed_gpu.py between two solvers of
one system (1e-7), with both sides solved to rtol 1e-12.  Figures are printed before they are asserted (run with -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_ensemble_gpu import _configs, _ensemble, _model, _packed, _shell12, _single  # noqa: E402

IT, RTOL = 250, 1e-12


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _masks(R, nb, seed):
    """a different set in every replica: none, one, a few, ..., all but one, all"""
    rng = np.random.default_rng(seed)
    m = np.zeros((R, nb), dtype=bool)
    counts = [0, 1, nb - 1, nb] + [int(k) for k in rng.integers(2, nb - 1, size=max(R - 4, 0))]
    for r in range(R):
        m[r, rng.permutation(nb)[:counts[r % len(counts)]]] = True
    return m


def _inputs(R, nb, mask, seed, held_every=3):
    """loads for the free bodies, velocities of speed <= 1 for the driven ones (every third prescribed body is held), slip"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, nb, 6))
    Up = rng.uniform(-1.0, 1.0, (R, nb, 6)) / np.sqrt(3.0)
    k = 0
    for r in range(R):
        for b in range(nb):
            if mask[r, b]:
                if k % held_every == 0:
                    Up[r, b] = 0.0
                k += 1
    bi = np.where(mask[:, :, None], Up, F)
    slip = 0.1 * rng.standard_normal((R, 36 * nb))
    return bi.reshape(R, 6 * nb), slip


def _step_mixed_single(s, mask, body_in, slip, max_iter, rtol):
    """rbl_step_mixed on a DeviceContext -> (F, iterations)"""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    b = np.ascontiguousarray(body_in, dtype=np.float64).reshape(-1)
    sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64)
    F = np.zeros(b.size)
    it, res = C.c_int(0), C.c_double(0.0)
    s._chk(s.L.rbl_step_mixed(s.h, m.ctypes.data, b.ctypes.data, None if sl is None else sl.ctypes.data, int(max_iter), float(rtol),
                              F.ctypes.data, C.byref(it), C.byref(res)))
    return F, it.value


# ---- 1. the solve ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wall", [False, True])
def test_solve_equals_the_single_context_solve_per_replica(wall):
    from rigid_body_light_amd import RigidBody
    from test_prescribed_gpu import _operator_residual
    c = _shell12()
    R, nb = 7, 10
    X0, Q0 = _configs(R, nb, wall)
    mask = _masks(R, nb, 31)
    assert len({tuple(m) for m in mask}) == R                                         # the mask differs between replicas
    bi, slip = _inputs(R, nb, mask, 32)
    ens = _ensemble(c, X0, Q0, wall)
    lam, U, F, its, res = ens.ensemble_solve_mixed(mask, bi, max_iter=IT, rtol=RTOL, slip=slip)
    Xa, Qa = ens.ensemble_get_config()
    assert np.array_equal(Xa, X0)                                                     # nothing moves
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall)
        lam1, U1, F1, it1, res1 = s.solve_mixed(mask[r], bi[r], max_iter=IT, rtol=RTOL, slip=slip[r])
        s.close()
        rb = RigidBody(c["cfg"], X0[r], Q0[r], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=False)
        true_res, ferr = _operator_residual(rb, mask[r], bi[r], slip[r], lam[r], U[r], F[r])
        print("solve wall=%s replica %d, %d of %d prescribed: %d iterations (single context %d), estimate %.2e, true residual %.2e; "
              "rel. diff lambda %.2e U %.2e F %.2e" % (wall, r, int(mask[r].sum()), nb, its[r], it1, res[r], true_res,
                                                       _rel(lam[r], lam1), _rel(U[r], U1), _rel(F[r], F1)))
        assert 0 < its[r] < IT and res[r] < RTOL and res1 < RTOL
        assert _rel(lam[r], lam1) <= 1e-7 and _rel(U[r], U1) <= 1e-7 and _rel(F[r], F1) <= 1e-7
        assert true_res <= 1e-9 and ferr <= 1e-12
        p = mask[r]
        assert np.array_equal(U[r].reshape(nb, 6)[p], bi[r].reshape(nb, 6)[p])         # echoed
        assert np.array_equal(F[r].reshape(nb, 6)[~p], bi[r].reshape(nb, 6)[~p])
    ens.close()


# ---- 2. the steps ---------------------------------------------------------------------------------------------------------------

def _check_steps(c, ens, X0, Q0, mask, bi, F, Xfirst, single_steps, label):
    R, nb, dt = mask.shape[0], mask.shape[1], c["dt"]
    Xe, Qe = ens.ensemble_get_config()
    held = mask & ~np.any(bi.reshape(R, nb, 6) != 0.0, axis=2)
    assert held.any() and (mask & ~held).any()
    for r in range(R):
        s = _single(c, X0[r], Q0[r], True)
        Fs = single_steps(s, r)
        Xs, Qs = s.get_config(nb)
        s.close()
        print("%s replica %d, %d of %d prescribed: |X - single| %.2e |Q - single| %.2e, rel. diff F %.2e"
              % (label, r, int(mask[r].sum()), nb, np.abs(Xe[r] - Xs).max(), np.abs(Qe[r] - Qs).max(), _rel(F[r], Fs)))
        assert np.abs(Xe[r] - Xs).max() <= 1e-7 and np.abs(Qe[r] - Qs).max() <= 1e-7
        assert _rel(F[r], Fs) <= 1e-7
        p = mask[r]
        Up = bi[r].reshape(nb, 6)
        # X += dt U_p: one rounding of the sum (half an ulp of |X|), as test_brownian_mixed_gpu.py checks it
        if p.any():
            assert np.abs((Xfirst[r][p] - X0[r][p]) - dt * Up[p, :3]).max() <= 1e-15 * np.abs(Xfirst[r]).max()
        assert np.array_equal(Xe[r][held[r]], X0[r][held[r]])                          # a held body does not move
        if (~p).any():
            assert np.linalg.norm(Xe[r][~p] - X0[r][~p]) > 1e-5                        # the free ones did


def test_deterministic_steps_equal_single_context_steps():
    c = _shell12()
    R, nb, wall = 7, 10, True
    X0, Q0 = _configs(R, nb, wall)
    mask = _masks(R, nb, 41)
    bi, slip = _inputs(R, nb, mask, 42)
    ens = _ensemble(c, X0, Q0, wall)
    Xfirst = None
    for n in range(3):
        F, its, res = ens.ensemble_step_mixed(mask, bi, max_iter=IT, rtol=RTOL, slip=slip)
        assert np.all(its > 0) and np.all(its < IT) and np.all(res < RTOL)
        if n == 0:
            Xfirst = ens.ensemble_get_config()[0]

    def single(s, r):
        for _ in range(3):
            Fs, it = _step_mixed_single(s, mask[r], bi[r], slip[r], IT, RTOL)
            assert 0 < it < IT
        return Fs
    _check_steps(c, ens, X0, Q0, mask, bi, F, Xfirst, single, "step_mixed")
    ens.close()


@pytest.mark.parametrize("split_rand", [True, False])
def test_brownian_steps_equal_single_context_steps_with_injected_noise(split_rand):
    c = _shell12()
    R, nb, wall = 7, 10, True
    X0, Q0 = _configs(R, nb, wall)
    mask = _masks(R, nb, 51)
    bi, slip = _inputs(R, nb, mask, 52)
    Ws = [np.random.default_rng(53 + n).standard_normal((R, 9 * 12 * nb)) for n in range(3)]
    ens = _ensemble(c, X0, Q0, wall)
    Xfirst = None
    for n, W in enumerate(Ws):
        F, its, res = ens.ensemble_step_brownian_mixed(mask, bi, W=W, split_rand=split_rand, max_iter=IT, rtol=RTOL, slip=slip)
        assert np.all(its > 0) and np.all(its < IT) and np.all(res < RTOL)
        if n == 0:
            Xfirst = ens.ensemble_get_config()[0]

    def single(s, r):
        for W in Ws:
            Fs, it, _ = s.step_brownian_mixed(mask[r], bi[r], max_iter=IT, rtol=RTOL, slip=slip[r], W=W[r], method=0,
                                              split_rand=split_rand)
            assert 0 < it < IT
        return Fs
    _check_steps(c, ens, X0, Q0, mask, bi, F, Xfirst, single, "step_brownian_mixed split=%s" % split_rand)
    ens.close()


# ---- 3. nobody prescribed -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [False, True])
@pytest.mark.parametrize("noise", ["none", "seeded", "injected"])
def test_nobody_prescribed_is_bitwise_the_unmasked_step(noise, model):
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 61)
    mdl = _model(c["a"]) if model else None
    rng = np.random.default_rng(62)
    F = rng.standard_normal((R, 6 * nb))
    slip = 0.1 * rng.standard_normal((R, 36 * nb))
    Ws = [rng.standard_normal((R, 9 * 12 * nb)) for _ in range(3)]
    mask = np.zeros((R, nb), dtype=bool)
    a, b = _ensemble(c, X0, Q0, wall, dt=1e-3, model=mdl), _ensemble(c, X0, Q0, wall, dt=1e-3, model=mdl)
    for n in range(3):
        if noise == "none":
            Fo, ita, resa = a.ensemble_step_mixed(mask, F, max_iter=80, rtol=1e-10, slip=slip)
            itb, resb = b.ensemble_step_deterministic(F, max_iter=80, rtol=1e-10, slip=slip)
        else:
            kw = dict(W=Ws[n]) if noise == "injected" else dict(seed=70 + n)
            Fo, ita, resa = a.ensemble_step_brownian_mixed(mask, F, max_iter=80, rtol=1e-10, slip=slip, **kw)
            itb, resb = b.ensemble_step_brownian(F, max_iter=80, rtol=1e-10, slip=slip, **kw)
        assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.all(ita > 0)
        (Xa, Qa), (Xb, Qb) = a.ensemble_get_config(), b.ensemble_get_config()
        assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)
    assert np.abs(Xa - X0).max() > 1e-5
    if not model:
        assert np.array_equal(Fo, F)                                                  # free loads echoed
    a.close()
    b.close()


# ---- 4. everybody prescribed ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wall", [False, True])
def test_resistance_matrix_of_every_replica(wall):
    from rigid_body_light_amd import Ensemble, RigidBody
    c = _shell12()
    R, nb = 3, 3
    X0, Q0 = _configs(R, nb, wall)
    ens = Ensemble(c["cfg"], X0, Q0, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=wall)
    Rm = ens.body_resistance_matrix(max_iter=IT, rtol=RTOL)
    ens.close()
    assert Rm.shape == (R, 6 * nb, 6 * nb)
    for r in range(R):
        rb = RigidBody(c["cfg"], X0[r], Q0[r], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=False)
        R1, its = rb.body_resistance_matrix(max_iter=IT, rtol=RTOL)
        sym = np.linalg.norm(Rm[r] - Rm[r].T) / np.linalg.norm(Rm[r])
        emin = np.linalg.eigvalsh(0.5 * (Rm[r] + Rm[r].T)).min()
        print("resistance matrix wall=%s replica %d: rel. diff to the single system %.2e, asymmetry %.2e, smallest eigenvalue %.3e"
              % (wall, r, _rel(Rm[r], R1), sym, emin))
        assert _rel(Rm[r], R1) <= 1e-7 and sym <= 1e-7 and emin > 0.0
    assert _rel(Rm[0], Rm[1]) > 1e-3                                                   # distinct configurations


# ---- 5. the force model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("brownian", [False, True])
def test_force_model_enters_the_free_bodies_only(brownian):
    """model on: the step of a model-free ensemble that is handed interaction_forces() in the free slots and zeros elsewhere --
    the same system, the same bits (the single-context test_force_model_enters_the_free_bodies_only)"""
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 9)
    model = _model(c["a"])
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 1] = True
    mask[::2, 3] = True
    on, off = _ensemble(c, X0, Q0, wall, dt=1e-3, model=model), _ensemble(c, X0, Q0, wall, dt=1e-3)
    share = on.ensemble_interaction_forces()[0].reshape(R, nb, 6)
    assert np.abs(share[mask]).max() > 1e-3 and np.abs(share[~mask]).max() > 1e-3      # the model loads prescribed bodies too
    handed = np.where(mask[:, :, None], 0.0, share).reshape(R, 6 * nb)
    W = np.random.default_rng(10).standard_normal((R, 9 * 12 * nb))
    if brownian:
        Fa, ita, resa = on.ensemble_step_brownian_mixed(mask, np.zeros(6 * nb), W=W, max_iter=IT, rtol=1e-10)
        Fb, itb, resb = off.ensemble_step_brownian_mixed(mask, handed, W=W, max_iter=IT, rtol=1e-10)
    else:
        Fa, ita, resa = on.ensemble_step_mixed(mask, np.zeros(6 * nb), max_iter=IT, rtol=1e-10)
        Fb, itb, resb = off.ensemble_step_mixed(mask, handed, max_iter=IT, rtol=1e-10)
    assert np.all(ita > 0) and np.all(ita < IT)
    assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.array_equal(Fa, Fb)
    (Xa, Qa), (Xb, Qb) = on.ensemble_get_config(), off.ensemble_get_config()
    assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)
    assert np.array_equal(Xa[mask], X0[mask]) and np.abs(Xa[~mask] - X0[~mask]).max() > 1e-6
    assert np.array_equal(Fa.reshape(R, nb, 6)[~mask], handed.reshape(R, nb, 6)[~mask])   # free loads echoed WITH the model's share
    assert np.abs(Fa.reshape(R, nb, 6)[mask]).max() > 1e-3                              # holding takes a load
    pairs = 0
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall, dt=1e-3, model=model)
        s.interaction_forces()
        pairs += s.interaction_stats()[1]
        s.close()
    assert pairs > 0                                                                   # the steric model was exercised
    on.close()
    off.close()


# ---- 6. statistics --------------------------------------------------------------------------------------------------------------

def test_one_step_covariance_next_to_a_held_body_is_2_kBT_dt_Ntilde():
    """free space, two shells at z = 10 a surface gap of 0.3 apart, body 1 held, 4096 identical replicas, one seeded step: the
    covariance of body 0's displacement is 2 kBT dt Ntilde, Ntilde = (R_ff)^-1, within 5 standard errors per entry
    (test_one_step_covariance_is_2_kBT_dt_N's se) -- and the sample can tell Ntilde from the mobility N of the all-free pair:
    |Ntilde_xx - N_xx| >= 10 se"""
    from rigid_body_light_amd import RigidBody
    c = _shell12()
    R, dt, kBT = 4096, 1e-3, 1.0
    Rb = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
    X0 = np.array([[0.3, -0.1, 10.0], [0.3 + 2 * (Rb + c["a"]) + 0.3, -0.1, 10.0]])
    Q0 = np.array([[0.9, 0.1, 0.3, -0.2], [0.9, 0.1, 0.3, -0.2]])
    Q0 /= np.linalg.norm(Q0, axis=1, keepdims=True)
    ens = _ensemble(c, np.repeat(X0[None], R, axis=0), np.repeat(Q0[None], R, axis=0), False, kBT=kBT, dt=dt)
    F, its, res = ens.ensemble_step_brownian_mixed([0, 1], np.zeros(12), seed=2024, max_iter=120, rtol=1e-12)
    X, Q = ens.ensemble_get_config()
    ens.close()
    assert np.all(its > 0) and np.all(its < 120)
    assert np.array_equal(X[:, 1], np.repeat(X0[1][None], R, axis=0))                  # held
    dX = X[:, 0] - X0[0]
    q, q0 = Q[:, 0], Q0[0] * [1, -1, -1, -1]    # q_rel = q (x) q0^-1
    w = q[:, 0] * q0[0] - q[:, 1:] @ q0[1:]
    v = q[:, :1] * q0[1:] + q0[0] * q[:, 1:] + np.cross(q[:, 1:], q0[1:])
    s = np.linalg.norm(v, axis=1)
    rot = (2 * np.arctan2(s, w) / np.where(s > 0, s, 1.0))[:, None] * v
    D = np.concatenate([dX, rot], axis=1)
    Cv = np.cov(D.T) / (2 * kBT * dt)
    rb = RigidBody(c["cfg"], X0, Q0, a=c["a"], eta=c["eta"], dt=dt)
    Rfull, _ = rb.body_resistance_matrix(max_iter=200, rtol=1e-12)
    N, _ = rb.body_mobility_matrix(max_iter=200, rtol=1e-12)
    Nt = np.linalg.inv(Rfull[:6, :6])
    se_xx = np.sqrt(2 * Nt[0, 0] ** 2 / (R - 1))
    print("Ntilde_xx %.6f, N_xx %.6f (%.1f %% apart), sample %.6f, se %.6f (%.1f %%)"
          % (Nt[0, 0], N[0, 0], 100 * abs(Nt[0, 0] - N[0, 0]) / N[0, 0], Cv[0, 0], se_xx, 100 * se_xx / Nt[0, 0]))
    worst = 0.0
    for i in range(6):
        for j in range(6):
            se = np.sqrt((Nt[i, i] * Nt[j, j] + Nt[i, j] ** 2) / (R - 1))
            worst = max(worst, abs(Cv[i, j] - Nt[i, j]) / se)
    print("largest deviation of an entry of the covariance: %.2f se" % worst)
    assert abs(Nt[0, 0] - N[0, 0]) >= 10 * se_xx                                       # held can be told from free
    for i in range(6):
        for j in range(6):
            se = np.sqrt((Nt[i, i] * Nt[j, j] + Nt[i, j] ** 2) / (R - 1))
            assert abs(Cv[i, j] - Nt[i, j]) <= 5 * se, (i, j, Cv[i, j], Nt[i, j], se)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------

def test_errors_leave_every_replica_and_the_single_configuration_unchanged():
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, nb, wall = 4, 3, True
    X0, Q0 = _configs(R, nb, wall)
    ens = _ensemble(c, X0, Q0, wall)
    Xs0, Qs0 = X0[0] + 5.0, Q0[1]
    ens.set_config(Xs0, Qs0)                    # the context's own single-system configuration
    Xa, Qa = ens.ensemble_get_config()
    mask = np.zeros((R, nb), dtype=np.uint8)
    mask[:, 2] = 1
    bi = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], nb)
    bi[12:] = [0.3, 0.0, 0.0, 0.0, 0.0, 0.0]    # body 2 driven along x
    for bad, code in (("overlap", 1), ("below", 2)):
        Xb, Qb = Xa.copy(), Qa.copy()
        if bad == "overlap":
            Xb[2, 1], Qb[2, 1] = Xb[2, 0], Qb[2, 0]   # two bodies of replica 2 on top of each other: every blob coincides
        else:
            Xb[1, 0, 2] = -0.5                  # a body of replica 1 below the wall
        ens.ensemble_set_config(Xb, Qb)
        for step in ("det", "brown"):
            with pytest.raises(RblError) as e:
                if step == "det":
                    ens.ensemble_step_mixed(mask, bi, max_iter=40, rtol=1e-8)
                else:
                    ens.ensemble_step_brownian_mixed(mask, bi, seed=1, max_iter=40, rtol=1e-8)
            assert "[rbl status %d]" % code in str(e.value)
            assert ("replica %d" % (2 if bad == "overlap" else 1)) in str(e.value)
            Xc, Qc = ens.ensemble_get_config()
            assert np.array_equal(Xc, Xb) and np.array_equal(Qc, Qb)
    ens.ensemble_set_config(Xa, Qa)
    two = mask.copy()
    two[3, 0] = 2
    for call in (lambda: ens.ensemble_step_mixed(two, bi), lambda: ens.ensemble_step_brownian_mixed(two, bi, seed=1),
                 lambda: ens.ensemble_solve_mixed(two, bi)):
        with pytest.raises(RblError) as e:
            call()
        assert "[rbl status 11]" in str(e.value) and "0 or 1" in str(e.value)
    Xc, Qc = ens.ensemble_get_config()
    assert np.array_equal(Xc, Xa) and np.array_equal(Qc, Qa)
    ens.ensemble_step_brownian_mixed(mask, bi, seed=3, max_iter=40, rtol=1e-8)
    ens.ensemble_step_mixed(mask, bi, max_iter=40, rtol=1e-8)
    Xsn, Qsn = ens.get_config(nb)
    assert np.array_equal(Xsn, Xs0) and np.allclose(Qsn, Qs0 / np.linalg.norm(Qs0, axis=1, keepdims=True), rtol=0, atol=1e-15)
    with pytest.raises(RblError) as e:         # beyond the one-kernel solver's iteration limit
        ens.ensemble_step_mixed(mask, bi, max_iter=256, rtol=1e-8)
    assert "[rbl status 4]" in str(e.value)
    ens.close()


def test_a_shape_that_fits_unmasked_but_not_with_the_mask_is_a_size_error_that_says_so():
    """58 bodies of 3 blobs with max_iter = 63: the one-kernel solver's vectors take 151 000 of its 153 600 bytes of LDS, the mask's
    6 N_bod doubles (2 784 bytes) no longer fit beside them (small_lds_base_bytes, rbl_small.hip)"""
    from rigid_body_light_amd._lib import DeviceContext, RblError
    import torch
    nb, R = 58, 2
    cfg = np.array([[0.6, 0.0, 0.0], [-0.3, 0.52, 0.0], [-0.3, -0.52, 0.0]])
    ens = DeviceContext(0.5, 1.0, True, cfg=cfg, dt=0.01, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    X = np.zeros((R, nb, 3))
    X[:, :, 0] = 4.0 * (np.arange(nb) % 8)
    X[:, :, 1] = 4.0 * (np.arange(nb) // 8)
    X[:, :, 2] = 3.0
    Q = np.zeros((R, nb, 4))
    Q[:, :, 0] = 1.0
    ens.ensemble_set_config(X, Q)
    F = np.zeros((R, 6 * nb))
    F[:, 2::6] = -1.0
    its, res = ens.ensemble_step_deterministic(F, max_iter=63, rtol=1e-6)             # the unmasked step fits and runs
    assert np.all(its > 0) and np.all(np.isfinite(res))
    mask = np.zeros((R, nb), dtype=bool)
    for call in (lambda: ens.ensemble_step_mixed(mask, F, max_iter=63, rtol=1e-6),
                 lambda: ens.ensemble_step_brownian_mixed(mask, F, seed=1, max_iter=63, rtol=1e-6),
                 lambda: ens.ensemble_solve_mixed(mask, F, max_iter=63, rtol=1e-6)):
        with pytest.raises(RblError) as e:
            call()
        assert "[rbl status 4]" in str(e.value) and "without prescribed bodies" in str(e.value)
    ens.ensemble_step_mixed(mask, F, max_iter=40, rtol=1e-6)                         # fewer iterations: the mask fits again
    ens.close()


# ---- 8. reproducibility, poisoned workspaces -----------------------------------------------------------------------------------

def _run(poison):
    from rigid_body_light_amd._lib import DeviceContext
    from test_poisoned_workspace_gpu import _poison_env
    import torch
    R, nb, wall = 5, 5, True
    c, X0, Q0 = _packed(R, nb, 81)
    mask = _masks(R, nb, 82)
    bi, slip = _inputs(R, nb, mask, 83)
    bi *= 0.2
    with _poison_env(poison):
        ens = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=1e-3, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    assert ens.get_option("poison_workspace") == int(poison)
    ens.ensemble_set_config(X0, Q0)
    ens.set_interactions(**_model(c["a"]))
    out = list(ens.ensemble_solve_mixed(mask, bi, max_iter=120, rtol=1e-10, slip=slip))
    for n in range(2):
        out += list(ens.ensemble_step_brownian_mixed(mask, bi, seed=90 + n, max_iter=120, rtol=1e-10, slip=slip))
        out += list(ens.ensemble_step_brownian_mixed(mask, bi, seed=90 + n, split_rand=False, max_iter=120, rtol=1e-10))
    out += list(ens.ensemble_step_mixed(mask, bi, max_iter=120, rtol=1e-10, slip=slip))
    out += list(ens.ensemble_get_config())
    ens.close()
    return out


def test_same_seed_same_bits_and_no_read_of_unwritten_memory():
    a, b, p = _run(False), _run(False), _run(True)
    assert all(np.all(np.isfinite(x)) for x in a)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                                                    # two runs with the same seed
    for x, y in zip(a, p):
        assert np.array_equal(x, y)                                                    # poisoned workspaces: the same bits


# ---- 9. the example -------------------------------------------------------------------------------------------------------------

def test_example_ensemble_microrheology_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_microrheology.py"), "--replicas", "32", "--steps",
                          "20"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith("step ")]
    assert len(rows) == 20
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.all(np.isfinite(vals))
    assert len([l for l in out.stdout.splitlines() if l.startswith("mean drag")]) == 1 and "standard error" in out.stdout
