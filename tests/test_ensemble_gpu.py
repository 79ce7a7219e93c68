"""Ensembles of independent replicas on the GPU (include/rbl.h section 5, rbl_ensemble.hip): every replica steps as a single
context at its configuration would (deterministic and Brownian, with injected and with seeded noise, with the force model),
replicas do not interact, the one-step covariance is 2 kBT dt N, errors leave every replica where it was, and the example runs.
Single-context comparisons use a fresh context with the block preconditioner off: it takes the one-kernel solver too."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import random_positions  # noqa: E402


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _single(c, X, Q, wall, kBT=1.0, dt=None, model=None):
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"] if dt is None else dt, kBT=kBT, stream_ptr=_stream())
    ctx.set_config(X, Q)
    if model:
        ctx.set_interactions(**model)
    return ctx


def _ensemble(c, X, Q, wall, kBT=1.0, dt=None, model=None):
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"] if dt is None else dt, kBT=kBT, stream_ptr=_stream())
    ctx.ensemble_set_config(X, Q)
    if model:
        ctx.set_interactions(**model)
    return ctx


def _shell12():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return {"cfg": cfg, "a": p["sep"] / 2.0, "eta": 1.0, "dt": 0.01}


def _configs(R, nb, wall, spread=10.0):
    """R distinct seeded configurations of nb shell_N_12 bodies (random_positions style, centres >= 4 apart)"""
    X, Q = np.zeros((R, nb, 3)), np.zeros((R, nb, 4))
    for r in range(R):
        x, q = random_positions(nb, wall=wall, seed=100 + r, min_dist=4.0)
        if wall:
            x[:, 2] += 1.5
        X[r], Q[r] = x, q
    return X, Q


@pytest.mark.parametrize("wall", [False, True])
def test_deterministic_replicas_equal_single_context_steps(wall):
    c = _shell12()
    R, nb = 7, 10
    X0, Q0 = _configs(R, nb, wall)
    F = np.random.default_rng(1).standard_normal((R, 6 * nb))
    ens = _ensemble(c, X0, Q0, wall)
    its = [ens.ensemble_step_deterministic(F, max_iter=60, rtol=1e-10)[0] for _ in range(3)]
    Xe, Qe = ens.ensemble_get_config()
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall)
        for n in range(3):
            it, _ = s.step_deterministic(F[r], max_iter=60, rtol=1e-10)
            assert it == its[n][r]
        Xs, Qs = s.get_config(nb)
        assert np.abs(Xe[r] - Xs).max() <= 1e-12
        assert np.abs(Qe[r] - Qs).max() <= 1e-12
        s.close()
    ens.close()


@pytest.mark.parametrize("split_rand", [True, False])
def test_brownian_replicas_equal_single_context_steps_with_injected_noise(split_rand):
    c = _shell12()
    R, nb, wall = 5, 10, True
    X0, Q0 = _configs(R, nb, wall)
    n3 = 3 * nb * 12
    rng = np.random.default_rng(2)
    F = rng.standard_normal((R, 6 * nb))
    Ws = [rng.standard_normal((R, 3 * n3)) for _ in range(3)]
    ens = _ensemble(c, X0, Q0, wall)
    for W in Ws:
        ens.ensemble_step_brownian(F, W=W, split_rand=split_rand, max_iter=80, rtol=1e-12)
    Xe, Qe = ens.ensemble_get_config()
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall)
        for W in Ws:
            s.step_brownian(F[r], max_iter=80, rtol=1e-12, W=W[r], method=0, split_rand=split_rand)
        Xs, Qs = s.get_config(nb)
        assert np.abs(Xe[r] - Xs).max() <= 1e-10
        assert np.abs(Qe[r] - Qs).max() <= 1e-10
        s.close()
    ens.close()


def test_seeded_noise_replica_zero_reproducibility_and_independence():
    c = _shell12()
    R, nb, wall = 6, 4, True
    X0, Q0 = _configs(1, nb, wall)
    X0, Q0 = np.repeat(X0, R, axis=0), np.repeat(Q0, R, axis=0)
    F = np.zeros(6 * nb)
    runs = []
    for _ in range(2):
        ens = _ensemble(c, X0, Q0, wall)
        for n in range(2):
            ens.ensemble_step_brownian(F, seed=77 + n, max_iter=80, rtol=1e-12)
        runs.append(ens.ensemble_get_config())
        ens.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])   # bitwise
    s = _single(c, X0[0], Q0[0], wall)
    for n in range(2):
        s.step_brownian(F, max_iter=80, rtol=1e-12, seed=77 + n, method=0)
    Xs, Qs = s.get_config(nb)
    assert np.abs(runs[0][0][0] - Xs).max() <= 1e-10
    assert np.abs(runs[0][1][0] - Qs).max() <= 1e-10
    s.close()
    X = runs[0][0]
    for r in range(1, R):                      # same start, own counters: every replica ends elsewhere
        assert np.abs(X[r] - X[0]).max() > 1e-6


def _model(a):
    return dict(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=2 * a + 20 * 0.05)


def test_replicas_do_not_interact():
    """every replica at the SAME place with the same noise and the force model on: copies that saw each other would overlap
    (an error) or push each other (a difference)"""
    c = _shell12()
    R, nb, wall = 8, 3, True
    X0, Q0 = _configs(1, nb, wall)
    X0[0, 1] = X0[0, 0] + [1.2, 0.3, 0.0]       # two bodies inside each other's cut-off
    n3 = 3 * nb * 12
    W1 = np.random.default_rng(4).standard_normal(3 * n3)
    F = np.zeros(6 * nb)
    ens = _ensemble(c, np.repeat(X0, R, axis=0), np.repeat(Q0, R, axis=0), wall, model=_model(c["a"]))
    ens.ensemble_step_brownian(F, W=np.tile(W1, (R, 1)), max_iter=80, rtol=1e-12)
    Xe, Qe = ens.ensemble_get_config()
    for r in range(1, R):
        assert np.array_equal(Xe[r], Xe[0]) and np.array_equal(Qe[r], Qe[0])
    s = _single(c, X0[0], Q0[0], wall, model=_model(c["a"]))
    s.step_brownian(F, max_iter=80, rtol=1e-12, W=W1, method=0)
    Xs, Qs = s.get_config(nb)
    assert np.abs(Xe[0] - Xs).max() <= 1e-10 and np.abs(Qe[0] - Qs).max() <= 1e-10
    s.close()
    ens.close()


def _packed(R, nb, seed):
    """replicas of nb shell_N_12 bodies in a row above the wall, the even ones packed (neighbouring shells a fraction of a blob
    radius apart: well inside the steric cut-off), the odd ones spread beyond it"""
    c = _shell12()
    Rb = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
    rng = np.random.default_rng(seed)
    X, Q = np.zeros((R, nb, 3)), np.zeros((R, nb, 4))
    for r in range(R):
        gap = 2 * (Rb + c["a"]) + (0.3 if r % 2 == 0 else 2.0)
        X[r, :, 0] = np.arange(nb) * gap
        X[r, :, 2] = Rb + 2.0 * c["a"]
        X[r] += rng.uniform(-0.05, 0.05, (nb, 3)) * [1, 1, 0]
        q = rng.standard_normal((nb, 4))
        Q[r] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return c, X, Q


def test_forces_per_replica_equal_single_context_forces_and_steps():
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 9)
    model = _model(c["a"])
    ens = _ensemble(c, X0, Q0, wall, dt=1e-3, model=model)
    FTe, Ee = ens.ensemble_interaction_forces()
    n3 = 3 * nb * 12
    rng = np.random.default_rng(5)
    F = rng.standard_normal((R, 6 * nb))
    Ws = [rng.standard_normal((R, 3 * n3)) for _ in range(2)]
    for W in Ws:
        ens.ensemble_step_brownian(F, W=W, max_iter=80, rtol=1e-12)
    Xe, Qe = ens.ensemble_get_config()
    packed_pairs = 0
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall, dt=1e-3, model=model)
        f, FT = s.interaction_forces()
        E = s.interaction_energy()
        packed_pairs += s.interaction_stats()[1]
        assert np.abs(FTe[r] + FT).max() <= 1e-12 * max(1.0, np.abs(FT).max())   # reference convention: -K^T f_phys
        assert abs(Ee[r] - E) <= 1e-12 * max(1.0, abs(E))
        for W in Ws:
            s.step_brownian(F[r], max_iter=80, rtol=1e-12, W=W[r], method=0)
        Xs, Qs = s.get_config(nb)
        assert np.abs(Xe[r] - Xs).max() <= 1e-10 and np.abs(Qe[r] - Qs).max() <= 1e-10
        s.close()
    assert packed_pairs > 0                    # the steric model was exercised
    ens.close()


def test_one_step_covariance_is_2_kBT_dt_N():
    from rigid_body_light_amd import RigidBody
    c = _shell12()
    R, dt, kBT = 4096, 1e-3, 1.0
    X0 = np.array([[0.3, -0.1, 10.0]])     # every blob above z = a: the dense root's damping B (reference :668) is the identity
    Q0 = np.array([[0.9, 0.1, 0.3, -0.2]]); Q0 /= np.linalg.norm(Q0)
    ens = _ensemble(c, np.repeat(X0[None], R, axis=0), np.repeat(Q0[None], R, axis=0), False, kBT=kBT, dt=dt)
    ens.ensemble_step_brownian(np.zeros(6), seed=2024, max_iter=80, rtol=1e-12)
    X, Q = ens.ensemble_get_config()
    ens.close()
    dX = X[:, 0] - X0[0]
    q, q0 = Q[:, 0], Q0[0] * [1, -1, -1, -1]    # q_rel = q (x) q0^-1
    w = q[:, 0] * q0[0] - q[:, 1:] @ q0[1:]
    v = q[:, :1] * q0[1:] + q0[0] * q[:, 1:] + np.cross(q[:, 1:], q0[1:])
    s = np.linalg.norm(v, axis=1)
    rot = (2 * np.arctan2(s, w) / np.where(s > 0, s, 1.0))[:, None] * v
    D = np.concatenate([dX, rot], axis=1)
    C = np.cov(D.T) / (2 * kBT * dt)
    rb = RigidBody(c["cfg"], X0, Q0, a=c["a"], eta=c["eta"], dt=dt)
    N, _ = rb.body_mobility_matrix(rtol=1e-12)
    for i in range(6):
        for j in range(6):
            se = np.sqrt((N[i, i] * N[j, j] + N[i, j] ** 2) / (R - 1))
            assert abs(C[i, j] - N[i, j]) <= 5 * se, (i, j, C[i, j], N[i, j], se)


def test_errors_leave_every_replica_and_the_single_configuration_unchanged():
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, nb, wall = 4, 3, True
    X0, Q0 = _configs(R, nb, wall)
    ens = _ensemble(c, X0, Q0, wall)
    Xs0, Qs0 = X0[0] + 5.0, Q0[1]
    ens.set_config(Xs0, Qs0)                    # the context's own single-system configuration
    Xa, Qa = ens.ensemble_get_config()
    F = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], nb)   # a nonzero right-hand side: the solver applies M (and meets the overlap)
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
                    ens.ensemble_step_deterministic(F, max_iter=40, rtol=1e-8)
                else:
                    ens.ensemble_step_brownian(F, seed=1, max_iter=40, rtol=1e-8)
            assert "[rbl status %d]" % code in str(e.value)
            assert ("replica %d" % (2 if bad == "overlap" else 1)) in str(e.value)
            Xc, Qc = ens.ensemble_get_config()
            assert np.array_equal(Xc, Xb) and np.array_equal(Qc, Qb)
    ens.ensemble_set_config(Xa, Qa)
    ens.ensemble_step_brownian(F, seed=3, max_iter=40, rtol=1e-8)
    ens.ensemble_step_deterministic(F, max_iter=40, rtol=1e-8)
    Xsn, Qsn = ens.get_config(nb)
    assert np.array_equal(Xsn, Xs0) and np.allclose(Qsn, Qs0 / np.linalg.norm(Qs0, axis=1, keepdims=True), rtol=0, atol=1e-15)
    with pytest.raises(RblError) as e:         # beyond the one-kernel solver's iteration limit
        ens.ensemble_step_deterministic(F, max_iter=256, rtol=1e-8)
    assert "[rbl status 4]" in str(e.value)
    ens.close()


def test_python_ensemble_broadcasts_forces_and_checks_shapes():
    from rigid_body_light_amd import Ensemble
    c = _shell12()
    R, nb = 3, 2
    X0, Q0 = _configs(R, nb, True)
    ens = Ensemble(c["cfg"], X0, Q0, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=True)
    with pytest.raises(ValueError):
        ens.step_deterministic(np.zeros(5))
    with pytest.raises(ValueError):
        ens.step_brownian(np.zeros((R, 6 * nb)), W=np.zeros((R, 7)))
    it1, _ = ens.step_deterministic(np.tile([0, 0, -1.0, 0, 0, 0], nb))
    Xa, _ = ens.get_config()
    ens.set_config(X0, Q0)
    it2, _ = ens.step_deterministic(np.tile([0, 0, -1.0, 0, 0, 0], (R, nb)))
    Xb, _ = ens.get_config()
    assert np.array_equal(Xa, Xb) and np.array_equal(it1, it2) and it1.shape == (R,)
    ens.set_interactions(w=0.2, eps_wall=1.0, b_wall=0.1)
    assert ens.interaction_forces().shape == (R, 6 * nb) and ens.interaction_energy().shape == (R,)
    ens.close()


def test_example_ensemble_gibbs_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_gibbs.py"), "--replicas", "32", "--steps", "60",
                          "--burn", "20"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "mean" in out.stdout and "var" in out.stdout
