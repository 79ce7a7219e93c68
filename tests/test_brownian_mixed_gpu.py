"""The Brownian midpoint step with prescribed bodies (include/rbl.h section 7) on the GPU.

The scheme, restated in numpy below (`_np_rhs_mid`, `_np_step`) on the oracle's matrices.  p: 0/1 per body; D_f, D_p select the six
slots of the free / prescribed bodies; Kinv = (K^T K)^-1 K^T; W = [W1 | W2 | W_rfd]:
  3. M^{1/2}W1 (and M^{1/2}W2 with split_rand) at q^n -- M of ALL blobs, the mask does not enter;
  4. dq = D_f Kinv W_rfd,  M_RFD = (1/delta)[M(q + delta/2 dq) - M(q - delta/2 dq)] W_rfd;
  5. s = slip - kBT M_RFD - BI   (split: c1 = 2 sqrt(kBT/dt), c2 = sqrt(kBT/dt), BI = c2 (M^{1/2}W1 - M^{1/2}W2); else
     c1 = c2 = sqrt(2 kBT/dt), BI = c2 M^{1/2}W1);
  6. q^{n+1/2} = q^n displaced by D_f (dt/2) c1 Kinv M^{1/2}W1 + D_p (dt/2) U_p;
  7. at q^{n+1/2}: [M -K_f; K_f^T 0][lambda; U_f] = [s + K_p U_p; -F_f],  F_p = -K_p^T lambda;
  8. from q^n: evolve_X_Q(U), a prescribed body by exactly dt U_p.
Tolerances are those of the all-free counterparts (test_RHS_and_Midpoint_vs_oracle, test_brownian_step_vs_dense_numpy) and of
test_prescribed_gpu.py.  Iteration counts are printed (run with -s), never asserted beyond "converged within max_iter"."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KBT = 1.0                                   # the wrapper's fixed value
MODEL = dict(w=0.2, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.1)
MASKS = {"none": ([], []), "one held": ([1], []), "one held, one driven": ([1], [2])}


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _case(wall, nb=4, seed=220):
    """4 x shell_N_12 at random places (above the wall: lifted), noise, slip, loads and prescribed velocities"""
    from conftest import random_positions
    X, Q = random_positions(nb, wall=wall, seed=seed)
    if wall:
        X[:, 2] += 1.4
    n3 = 36 * nb
    rng = np.random.default_rng(seed + 1)
    return X, Q, rng.standard_normal(3 * n3), 0.1 * rng.standard_normal(n3), rng.standard_normal((nb, 6)), 0.5 * rng.standard_normal((nb, 6))


def _mask_and_body_in(which, F, Up):
    held, driven = MASKS[which]
    nb = F.shape[0]
    p = np.isin(np.arange(nb), held + driven)
    bi = np.array(F)
    bi[held] = 0.0
    bi[driven] = Up[driven]
    return p, bi


def _solver(cfg, X, Q, wall, block, dt=0.01, a=1.0, eta=1.0):
    from rigid_body_light_amd import RigidBody
    return RigidBody(cfg, X, Q, a=a, eta=eta, dt=dt, wall_PC=wall, block_PC=block)


def _dense_M_K(orc, cfg, X, Qn, a, eta, wall):
    """M (B M B with the wall, as apply_M applies it) and K of a configuration; cfg centred"""
    from oracle import oracle as O
    r = orc.multi_body_pos(X, Qn, cfg)
    K = O.K_matrix(X, Qn, cfg)
    M = orc.rotne_prager_tensor(r, a, eta, wall)
    if wall:
        B = orc.damp(r, a)
        M = B[:, None] * M * B[None, :]
    return M, K


def _np_rhs_mid(orc, cfg, X, Qn, a, eta, wall, dt, kBT, p, body_in, slip, W, split_rand, delta=1.0e-4):
    """steps 3-6 -> (s, X_half, Q_half)"""
    from oracle import oracle as O
    n3 = slip.size
    W1, W2, Wr = W[:n3], W[n3:2 * n3], W[2 * n3:]
    Df = np.repeat(~p, 6).astype(np.float64)
    r = orc.multi_body_pos(X, Qn, cfg)
    mw1 = orc.M_half_W(r, a, eta, wall, W1)
    Kinv = O.Kinv_matrix(X, Qn, cfg)
    dq = Df * (Kinv @ Wr)
    Xp, Qp = O.update_X_Q(X, Qn, 0.5 * delta * dq)
    Xm, Qm = O.update_X_Q(X, Qn, -0.5 * delta * dq)
    rfd = (orc.apply_M(Wr, orc.multi_body_pos(Xp, Qp, cfg), a, eta, wall) - orc.apply_M(Wr, orc.multi_body_pos(Xm, Qm, cfg), a, eta, wall)) / delta
    if split_rand:
        c1, c2 = 2.0 * np.sqrt(kBT / dt), np.sqrt(kBT / dt)
        BI = c2 * (mw1 - orc.M_half_W(r, a, eta, wall, W2))
    else:
        c1 = c2 = np.sqrt(2.0 * kBT / dt)
        BI = c2 * mw1
    s = slip - kBT * rfd - BI
    Up = np.where(p[:, None], body_in.reshape(-1, 6), 0.0).reshape(-1)
    Xh, Qh = O.update_X_Q(X, Qn, Df * (0.5 * dt * c1) * (Kinv @ mw1) + (1.0 - Df) * (0.5 * dt) * Up)
    return s, Xh, Qh


def _np_mixed(M, K, p, body_in, slip):
    """numpy.linalg.solve on [M -K_f; K_f^T 0] -> (U of all bodies, F of all bodies), as test_prescribed_gpu._dense_mixed"""
    n3 = M.shape[0]
    bi = body_in.reshape(-1, 6)
    colf = np.repeat(~p, 6)
    Kf, Kp = K[:, colf], K[:, ~colf]
    nf6 = Kf.shape[1]
    A = np.block([[M, -Kf], [Kf.T, np.zeros((nf6, nf6))]])
    x = np.linalg.solve(A, np.concatenate([slip + Kp @ bi[p].reshape(-1), -bi[~p].reshape(-1)]))
    U, F = np.array(bi), np.array(bi)
    U[~p] = x[n3:].reshape(-1, 6)
    F[p] = -(Kp.T @ x[:n3]).reshape(-1, 6)
    return U.reshape(-1), F.reshape(-1)


def _np_step(orc, cfg, X, Qn, a, eta, wall, dt, kBT, p, body_in, slip, W, split_rand=True):
    """steps 1-8 -> (X, Q, F, U)"""
    from oracle import oracle as O
    s, Xh, Qh = (slip, X, Qn) if kBT <= 1e-10 else _np_rhs_mid(orc, cfg, X, Qn, a, eta, wall, dt, kBT, p, body_in, slip, W, split_rand)
    M, K = _dense_M_K(orc, cfg, Xh, Qh, a, eta, wall)
    U, F = _np_mixed(M, K, p, body_in, s)
    Xn, Qn1 = O.evolve(X, Qn, U, dt)
    return Xn, Qn1, F, U


# ---- 1. right-hand side and predictor -------------------------------------------------------------------------------------------

def _rhs_case(orc, shell12, wall, split_rand, which):
    from oracle import oracle as O
    nb, dt = 4, 0.01
    X, Q, W, slip, F, Up = _case(wall)
    p, bi = _mask_and_body_in(which, F, Up)
    rb = _solver(shell12, X, Q, wall, False, dt=dt)
    args0 = [v.copy() for v in (p, bi, slip, W)]
    s, Xh, Qh = rb.RHS_and_Midpoint_mixed(p, bi, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    for v, v0 in zip((p, bi, slip, W), args0):
        assert np.array_equal(v, v0)                                                   # arguments untouched
    Qn = O.normalize_quats(Q)
    s_r, Xr, Qr = _np_rhs_mid(orc, O.remove_mean(shell12), X, Qn, 1.0, 1.0, wall, dt, KBT, p, bi, slip, W, split_rand)
    print("rhs wall=%s split=%s mask=%s: rel. error of s %.2e, |X_half - ref| %.2e, |Q_half - ref| %.2e"
          % (wall, split_rand, which, _rel(s, s_r), np.abs(Xh.reshape(-1, 3) - Xr).max(), np.abs(Qh.reshape(-1, 4) - Qr).max()))
    assert _rel(s, s_r) < 1e-8                      # the difference quotient carries 1e-15/delta of product rounding
    np.testing.assert_allclose(Xh.reshape(-1, 3), Xr, rtol=0, atol=1e-11)
    np.testing.assert_allclose(Qh.reshape(-1, 4), Qr, rtol=0, atol=1e-11)
    held, driven = MASKS[which]
    for b in held:                                  # a held body stays, a driven one sits at its own half step
        assert np.array_equal(Xh.reshape(-1, 3)[b], X[b])
    for b in driven:
        assert np.abs(Xh.reshape(-1, 3)[b] - (X[b] + 0.5 * dt * Up[b, :3])).max() <= 1e-15 * np.abs(X[b]).max()
    X1, Q1 = rb.get_config()
    assert np.array_equal(X1.reshape(-1, 3), X) and np.allclose(Q1.reshape(-1, 4), Qn, rtol=0, atol=1e-15)   # nothing committed


@pytest.mark.parametrize("which", list(MASKS))
@pytest.mark.parametrize("split_rand", [True, False])
@pytest.mark.parametrize("wall", [False, True])
def test_rhs_and_predictor_against_the_numpy_restatement(orc, shell12, wall, split_rand, which):
    _rhs_case(orc, shell12, wall, split_rand, which)


# ---- 2. the whole step ----------------------------------------------------------------------------------------------------------

def _step_case(orc, shell12, wall, block):
    from oracle import oracle as O
    nb, dt = 4, 0.01
    X, Q, W, slip, F, Up = _case(wall, seed=230)
    which = "one held, one driven"
    (held,), (driven,) = MASKS[which]
    p, bi = _mask_and_body_in(which, F, Up)
    rb = _solver(shell12, X, Q, wall, block, dt=dt)
    Fo, its, res = rb.step_brownian_mixed(p, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-11)
    Xg, Qg = rb.get_config()
    Qn = O.normalize_quats(Q)
    Xr, Qr, Fr, Ur = _np_step(orc, O.remove_mean(shell12), X, Qn, 1.0, 1.0, wall, dt, KBT, p, bi, slip, W)
    Fo, Fr = Fo.reshape(nb, 6), Fr.reshape(nb, 6)
    print("step wall=%s block=%s: %d iterations, residual %.2e; |X - ref| %.2e, |Q - ref| %.2e, rel. error of the loads on the prescribed bodies %.2e"
          % (wall, block, its, res, np.abs(Xg - Xr).max(), np.abs(Qg - Qr).max(), _rel(Fo[p], Fr[p])))
    assert 0 < its < 200 and res < 1e-11
    np.testing.assert_allclose(Xg, Xr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(Qg, Qr, rtol=0, atol=1e-9)
    assert _rel(Fo[p], Fr[p]) <= 1e-7
    assert np.array_equal(Fo[~p], bi[~p])                                              # free loads echoed
    # X += dt U_p: one rounding of the sum (half an ulp of |X|)
    assert np.abs((Xg[driven] - X[driven]) - dt * Up[driven, :3]).max() <= 1e-15 * np.abs(Xg[driven]).max()
    assert np.array_equal(Xg[held], X[held]) and np.abs(Qg[held] - Qn[held]).max() <= 1e-15
    assert np.linalg.norm(Xg[~p] - X[~p]) > 1e-4                                       # the free ones did move


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("wall", [False, True])
def test_whole_step_against_the_dense_numpy_step(orc, shell12, wall, block):
    _step_case(orc, shell12, wall, block)


# ---- 3. limits ------------------------------------------------------------------------------------------------------------------

def _raw(shell12, X, Q, kBT, wall, block, dt=0.01):
    import rigid_body_light_amd as rbl
    cm = rbl.c_rigid.CManyBodies()
    cm.setParameters(1.0, dt, kBT, 1.0, shell12)
    cm.setWallPC(wall)
    cm.setBlkPC(block)
    cm.setConfig(X.reshape(-1), Q.reshape(-1))
    cm.set_K_mats()
    return cm


@pytest.mark.parametrize("wall", [False, True])
def test_zero_temperature_is_step_mixed(shell12, wall):
    from rigid_body_light_amd._lib import DeviceContext
    X, Q, W, slip, F, Up = _case(wall, seed=240)
    p, bi = _mask_and_body_in("one held, one driven", F, Up)
    mask = p.astype(np.uint8)
    a, b = _raw(shell12, X, Q, 0.0, wall, True), _raw(shell12, X, Q, 0.0, wall, True)
    va, vb = (DeviceContext.borrow(cm.handle(), 1.0, shell12) for cm in (a, b))       # the views' methods; a and b own the contexts
    Fa, ita, _ = va.step_brownian_mixed(mask, bi.reshape(-1), slip=slip, W=W, seed=0, method="cholesky", split_rand=True, delta=1e-4,
                                        max_iter=200, rtol=1e-10)
    Fb, itb, _ = vb.step_mixed(mask, bi.reshape(-1), slip=slip, max_iter=200, rtol=1e-10)
    (Xa, Qa), (Xb, Qb) = a.getConfig(), b.getConfig()
    assert ita == itb and 0 < ita < 200
    assert np.abs(Xa - Xb).max() <= 1e-14 and np.abs(Qa - Qb).max() <= 1e-14 and np.abs(Fa - Fb).max() <= 1e-14 * np.abs(Fb).max()
    s, Xh, Qh = va.RHS_and_Midpoint_mixed(mask, bi.reshape(-1), slip, W)
    assert np.array_equal(s, slip) and np.array_equal(Xh, Xa) and np.array_equal(Qh, Qa)


@pytest.mark.parametrize("wall", [False, True])
def test_nothing_prescribed_is_step_brownian(shell12, wall):
    X, Q, W, slip, F, _ = _case(wall, seed=250)
    a, b = _solver(shell12, X, Q, wall, True), _solver(shell12, X, Q, wall, True)
    Fo, ita, resa = a.step_brownian_mixed([], F, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    itb, resb = b.step_brownian(F.reshape(-1), slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    (Xa, Qa), (Xb, Qb) = a.get_config(), b.get_config()
    print("nobody prescribed wall=%s: step_brownian_mixed %d iterations, step_brownian %d; |dX| %.2e |dQ| %.2e"
          % (wall, ita, itb, np.abs(Xa - Xb).max(), np.abs(Qa - Qb).max()))
    assert resa < 1e-10 and resb < 1e-10
    np.testing.assert_allclose(Xa, Xb, rtol=0, atol=1e-7)
    np.testing.assert_allclose(Qa, Qb, rtol=0, atol=1e-7)
    assert np.array_equal(Fo, F.reshape(-1)) and np.linalg.norm(Xa - X) > 1e-4


@pytest.mark.parametrize("split_rand", [False, True])
@pytest.mark.parametrize("wall", [False, True])
def test_nothing_prescribed_is_RHS_and_Midpoint_bitwise(shell12, wall, split_rand):
    """The all-free right-hand side is the mixed one with no mask, stated once in the library: with nobody prescribed s, X_half and
    Q_half are the bits of RHS_and_Midpoint's top block and predictor.  (The whole steps of the neighbouring test go through two
    GMRES drivers and keep their atol.)"""
    X, Q, W, slip, F, _ = _case(wall, seed=250)
    a, b = _solver(shell12, X, Q, wall, True), _solver(shell12, X, Q, wall, True)
    s, Xh, Qh = a.RHS_and_Midpoint_mixed([], F, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    rhs, Xr, Qr = b.RHS_and_Midpoint(slip, F.reshape(-1), W=W, method="cholesky", split_rand=split_rand)
    Xh, Qh, Xr, Qr = (np.asarray(v).reshape(-1) for v in (Xh, Qh, Xr, Qr))
    print("nobody prescribed wall=%s split=%s: |ds| %.2e |dX_half| %.2e |dQ_half| %.2e"
          % (wall, split_rand, np.abs(s - rhs[:s.size]).max(), np.abs(Xh - Xr).max(), np.abs(Qh - Qr).max()))
    assert np.array_equal(s, rhs[:s.size]) and np.array_equal(rhs[s.size:], -F.reshape(-1))
    assert np.array_equal(Xh, Xr) and np.array_equal(Qh, Qr)
    assert np.linalg.norm(Xh - X.reshape(-1)) > 1e-4                                  # a predictor that moved


def test_seeded_noise_is_reproducible(shell12):
    X, Q, _, slip, F, Up = _case(True, seed=260)
    p, bi = _mask_and_body_in("one held, one driven", F, Up)
    out = []
    for seed in (7, 7, 8):
        rb = _solver(shell12, X, Q, True, True)
        Fo, its, res = rb.step_brownian_mixed(p, bi, slip=slip, seed=seed, method="cholesky", max_iter=200, rtol=1e-10)
        s = rb.RHS_and_Midpoint_mixed(p, bi, slip=slip, seed=seed)[0]
        out.append((Fo, *rb.get_config(), s))
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)
    for x, y in zip(out[0], out[2]):
        assert not np.array_equal(x, y)


@pytest.mark.parametrize("with_slip", [True, False])
def test_dev_form_of_the_rhs_equals_the_host_form(shell12, with_slip):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    wall, dt, nb = True, 0.01, 4
    X, Q, W, slip, F, Up = _case(wall, seed=270)
    p, bi = _mask_and_body_in("one held, one driven", F, Up)
    rb = _solver(shell12, X, Q, wall, False, dt=dt)
    s, Xh, Qh = rb.RHS_and_Midpoint_mixed(p, bi, slip=slip if with_slip else None, W=W, method="cholesky")
    ctx = DeviceContext(1.0, 1.0, wall, cfg=shell12, dt=dt, kBT=KBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(X, Q)
    dev = torch.device("cuda:0")
    d_bi, d_slip, d_W = (torch.from_numpy(np.ascontiguousarray(v).reshape(-1)).to(dev) for v in (bi, slip, W))
    d_s = torch.full((36 * nb,), float("nan"), dtype=torch.float64, device=dev)
    Xd, Qd = ctx.RHS_and_Midpoint_mixed_dev(p, d_bi.data_ptr(), d_slip.data_ptr() if with_slip else None, d_W.data_ptr(), 0, 0, True,
                                            1e-4, d_s.data_ptr())
    ctx.sync_check()
    assert np.array_equal(d_s.cpu().numpy(), s)
    assert np.array_equal(Xd.reshape(-1), Xh.reshape(-1)) and np.array_equal(Qd.reshape(-1), Qh.reshape(-1))
    assert np.array_equal(d_bi.cpu().numpy(), bi.reshape(-1)) and np.array_equal(d_W.cpu().numpy(), W)     # inputs untouched
    # the ctypes form of the whole step is the extension's
    ctx2 = DeviceContext(1.0, 1.0, wall, cfg=shell12, dt=dt, kBT=KBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx2.set_config(X, Q)
    F1, it1, _ = ctx2.step_brownian_mixed(p, bi, max_iter=200, rtol=1e-10, slip=slip, W=W, method=0)
    F2, it2, _ = rb.step_brownian_mixed(p, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    Xc, Qc = ctx2.get_config(nb)
    Xr, Qr = rb.get_config()
    assert it1 == it2 and np.array_equal(F1, F2) and np.array_equal(Xc, Xr.reshape(-1, 3)) and np.array_equal(Qc, Qr.reshape(-1, 4))
    ctx.close()
    ctx2.close()


# ---- 4. the force model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wall,block", [(False, True), (True, False), (True, True)])
def test_force_model_enters_the_free_bodies_only(wall, block):
    """model on, three bodies prescribed: the step solves the free bodies with their loads plus the model's at q^n,
    -K^T f_phys = interaction_forces(), in the free slots and leaves the prescribed velocities alone -- bitwise the step of a
    model-free object that is handed those loads"""
    from rigid_body_light_amd import RigidBody, make_config
    nb, nblb, dt = 10, 12, 0.01
    c = make_config(nb, nblb, wall)
    rng = np.random.default_rng(22)
    F, Up, slip, W = rng.standard_normal((nb, 6)), 0.5 * rng.standard_normal((nb, 6)), 0.1 * rng.standard_normal(3 * nb * nblb), \
        rng.standard_normal(9 * nb * nblb)
    p = np.isin(np.arange(nb), [1, 4, 7])
    bi = np.where(p[:, None], Up, F)
    new = lambda: RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt, wall_PC=wall, block_PC=block)
    rb = new()
    rb.set_interactions(**MODEL)
    share = rb.interaction_forces().reshape(nb, 6)
    assert np.abs(share[p]).max() > 1e-3 and np.abs(share[~p]).max() > 1e-3           # the model does load prescribed bodies too
    bi_model = np.where(p[:, None], bi, bi + share)
    X0 = np.array(rb.get_config()[0])
    Fo, its, res = rb.step_brownian_mixed(p, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    rb2 = new()
    Fs, its2, res2 = rb2.step_brownian_mixed(p, bi_model, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    print("model on, 3 of 10 prescribed, wall=%s block=%s: %d iterations; |F_model - F_handed| %.2e" % (wall, block, its, np.abs(Fo - Fs).max()))
    assert 0 < its < 200 and its == its2 and res == res2 and np.array_equal(Fo, Fs)     # the same system: the same bits
    assert np.array_equal(Fo.reshape(nb, 6)[~p], bi_model[~p])                          # free loads echoed WITH the model's share
    (X1, Q1), (X2, Q2) = rb.get_config(), rb2.get_config()
    assert np.array_equal(X1, X2) and np.array_equal(Q1, Q2)
    assert np.abs((X1[p] - X0[p]) - dt * Up[p, :3]).max() <= 1e-15 * np.abs(X1).max()
    # without the mask (model loads added to the prescribed slots too) the bodies would go elsewhere
    rb3 = new()
    rb3.step_brownian_mixed(p, bi + share, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    assert np.abs(rb3.get_config()[0] - X1).max() > 1e-6


# ---- 5. poisoned workspaces -----------------------------------------------------------------------------------------------------

_POISON_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from oracle import Oracle
import test_brownian_mixed_gpu as t
from rigid_body_light_amd import RigidBody, load_structure, make_config
c = make_config(2, 12, False)
assert RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 0.01).cb.get_option("poison_workspace") == 1
orc, shell12 = Oracle(), load_structure(12)[1]
t._rhs_case(orc, shell12, True, True, "one held, one driven")
t._step_case(orc, shell12, True, True)
print("ALL OK")
"""


def test_rhs_and_step_with_poisoned_workspaces():
    """every device workspace filled with NaN at each reserve (RBL_POISON_WORKSPACE=1, a child process): a read of memory
    nobody wrote fails tests 1 and 2"""
    env = dict(os.environ, RBL_POISON_WORKSPACE="1")
    p = subprocess.run([sys.executable, "-c", _POISON_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout


# ---- 6. sizes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb,nblb", [(50, 162), (200, 642)])
def test_one_step_at_cfg2_and_cfg3(nb, nblb):
    from rigid_body_light_amd import RigidBody, make_config
    c = make_config(nb, nblb, True)
    rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True, block_PC=True)
    p = np.zeros(nb, dtype=bool)
    p[np.random.default_rng(6).permutation(nb)[:nb // 4]] = True
    bi = np.random.default_rng(8).standard_normal((nb, 6))
    bi[p] = 0.0                                                                        # a quarter of the bodies held
    X0 = np.array(rb.get_config()[0])
    F, its, res = rb.step_brownian_mixed(p, bi, seed=3, method="lanczos_pc", max_iter=100, rtol=1e-8)
    X1 = rb.get_config()[0]
    print("%d x %d blobs, %d held: %d iterations, residual %.2e, largest load on a held body %.3e"
          % (nb, nblb, int(p.sum()), its, res, np.abs(F.reshape(nb, 6)[p]).max()))
    assert 0 < its < 100 and res < 1e-8
    assert np.array_equal(X1[p], X0[p]) and np.all(np.isfinite(X1)) and np.all(np.isfinite(F))
    assert np.abs(X1[~p] - X0[~p]).max() > 1e-6 and np.abs(F.reshape(nb, 6)[p]).max() > 0.0


# ---- 7. the statistics of the step ----------------------------------------------------------------------------------------------

def _velocity(X0, Q0, X1, Q1, dt):
    """the (translation, rotation) velocity that evolve_X_Q turned into the move q0 -> q1"""
    from oracle import oracle as O
    dq = O.quat_mul(Q1, np.array([Q0[0], -Q0[1], -Q0[2], -Q0[3]]))
    if dq[0] < 0:
        dq = -dq
    v = np.linalg.norm(dq[1:])
    om = np.zeros(3) if v == 0.0 else (2.0 * np.arctan2(v, dq[0]) / v) * dq[1:]
    return np.concatenate([X1 - X0, om]) / dt


def _statistics(orc, shell12, Up, S=6400):
    from oracle import oracle as O
    from rigid_body_light_amd import load_structure
    a = load_structure(12)[0]["sep"] / 2.0
    eta, dt, wall = 1.0, 0.01, True
    cfg = O.remove_mean(shell12)
    X = np.array([[0.0, 0.0, 1.6], [2.4, 0.0, 1.5]])
    Qn = O.normalize_quats(np.random.default_rng(5).standard_normal((2, 4)))
    p = np.array([True, False])
    bi = np.zeros((2, 6))
    bi[0] = Up
    # oracle quantities
    free1 = slice(6, 12)

    def N_tilde(Xc, Qc, pres):
        M, K = _dense_M_K(orc, cfg, Xc, Qc, a, eta, wall)
        Kf = K[:, np.repeat(~pres, 6)]
        return np.linalg.inv(Kf.T @ np.linalg.solve(M, Kf))

    def divergence(pres, rows, coords, h=1e-5):
        """kBT sum_k d N_{.k} / d q_k over the coordinates `coords` (slots among all 12), rows `rows` of N"""
        d = np.zeros(6)
        free_slots = np.flatnonzero(np.repeat(~pres, 6))
        for k in coords:
            e = np.zeros(12)
            e[k] = h
            Np = N_tilde(*O.update_X_Q(X, Qn, e), pres)
            Nm = N_tilde(*O.update_X_Q(X, Qn, -e), pres)
            col = int(np.flatnonzero(free_slots == k)[0])
            d += KBT * (Np[rows, col] - Nm[rows, col]) / (2.0 * h)
        return d
    Nt = N_tilde(X, Qn, p)
    d = divergence(p, slice(0, 6), range(6, 12))
    d_allfree = divergence(np.array([False, False]), free1, range(12))
    M, K = _dense_M_K(orc, cfg, X, Qn, a, eta, wall)
    U_det = _np_mixed(M, K, p, bi.reshape(-1), np.zeros(M.shape[0]))[0][free1]
    # sampling
    rb = _solver(shell12, X, Qn, wall, True, dt=dt, a=a, eta=eta)
    rng = np.random.default_rng(7)
    e, o = np.zeros((S, 6)), np.zeros((S, 6))
    worst_its = 0
    for i in range(S):
        W = rng.standard_normal(216)
        U = []
        for sign in (1.0, -1.0):
            rb.set_config(X, Qn)
            _, its, res = rb.step_brownian_mixed(p, bi, W=sign * W, method="cholesky", max_iter=100, rtol=1e-10)
            assert 0 < its < 100 and res < 1e-10
            worst_its = max(worst_its, its)
            X1, Q1 = rb.get_config()
            U.append(_velocity(X[1], Qn[1], X1[1], Q1[1], dt))
        e[i], o[i] = 0.5 * (U[0] + U[1]), 0.5 * (U[0] - U[1])
    se = e.std(axis=0) / np.sqrt(S)
    dev = (e.mean(axis=0) - U_det - d) / se
    ratio = (o * o).mean(axis=0) * dt / (2.0 * KBT) / np.diag(Nt)
    return dict(dev=dev, se=se, d=d, d_allfree=d_allfree, ratio=ratio, U_det=U_det, its=worst_its)


@pytest.mark.parametrize("name,Up", [("held", (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)), ("driven", (0.5, 0.0, 0.0, 0.0, 0.0, 0.3))])
def test_drift_and_covariance_of_the_free_body(orc, shell12, name, Up):
    """Two shell_N_12 above the wall (a = sep/2, eta = 1, kBT = 1, dt = 0.01, X = [[0, 0, 1.6], [2.4, 0, 1.5]],
    Q = default_rng(5) normalised), body 0 prescribed, body 1 free with F = 0, cholesky roots, block preconditioner, rtol 1e-10.
    S = 6400 noise vectors from default_rng(7), each used as W and -W from the same configuration: e = (U(W) + U(-W))/2 carries
    the drift, o = (U(W) - U(-W))/2 the noise.  With Ntilde = (K_f^T M^-1 K_f)^-1 from the oracle's dense matrices,
    d = kBT sum_k d Ntilde_{.k} / d q_k (central differences, h = 1e-5, over the free body's coordinates) and U_det the dense
    noise-free solve at q^n:
      (a) |mean(e) - U_det - d| <= 4 s.e. in every component, s.e. = std(e)/sqrt(S);
      (b) power: |d_z| >= 10 s.e. and |d_x - d_x^{all free}| >= 4 s.e. (the divergence with nobody prescribed);
      (c) diag(mean(o o^T)) dt/(2 kBT) within 4 sqrt(2/S) = 7.07 % of diag(Ntilde).
    The numpy restatement of the scheme meets these on the same inputs (deviations <= 1.16 s.e. held, <= 1.29 s.e. driven, power
    9.5 s.e. in x and 23.6 in z, variance ratios 0.988-1.033); leaving the RFD term out misses d_z by 26 s.e., ignoring the hold
    gives 1.364 Ntilde_xx.  S is not halved: the 12 800 steps of one case take well under five minutes (the time is printed)."""
    S = 6400
    t0 = time.perf_counter()
    r = _statistics(orc, shell12, np.array(Up), S=S)
    wall_s = time.perf_counter() - t0
    fmt = lambda v: np.array2string(np.asarray(v), precision=3, suppress_small=False)
    print("statistics, body 0 %s: deviations (s.e.) %s; d %s; d_allfree %s; s.e. %s; variance ratios %s; U_det %s; at most %d iterations; %.1f s"
          % (name, fmt(r["dev"]), fmt(r["d"]), fmt(r["d_allfree"]), fmt(r["se"]), fmt(r["ratio"]), fmt(r["U_det"]), r["its"], wall_s))
    assert np.all(np.abs(r["dev"]) <= 4.0)                                                         # (a)
    assert abs(r["d"][2]) >= 10.0 * r["se"][2] and abs(r["d"][0] - r["d_allfree"][0]) >= 4.0 * r["se"][0]   # (b)
    assert np.all(np.abs(r["ratio"] - 1.0) <= 4.0 * np.sqrt(2.0 / S))                              # (c)


# ---- 8. the example, and the cost ----------------------------------------------------------------------------------------------

def test_probe_microrheology_example():
    p = subprocess.run([sys.executable, "examples/probe_microrheology.py", "--steps", "6"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l.split() for l in p.stdout.splitlines() if l.startswith("step ")]
    assert len(rows) == 6
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.all(np.isfinite(vals))
    mean = [l for l in p.stdout.splitlines() if l.startswith("mean drag")]
    assert len(mean) == 1


def test_cost_with_nobody_prescribed_at_cfg3_is_step_brownian_s():
    """tools/bench_brownian_mixed.py at cfg 3 (wall, block preconditioner, lanczos_pc roots to 1e-3, GMRES to 1e-8; step_brownian
    in the same process is the yardstick): with nobody prescribed the two steps do the same roots and RFD products and differ by
    the mixed solve's unfused tails, for which the project allows 10 % per iteration (test_prescribed_gpu.py) -> ms per step of
    mixed_none <= 1.10 x step_brownian's."""
    p = subprocess.run([sys.executable, "tools/bench_brownian_mixed.py", "--cfgs", "cfg3", "--rounds", "3"], cwd=ROOT, capture_output=True,
                       text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["cfg3"]
    for case in ("step_brownian", "mixed_none", "mixed_quarter", "mixed_all_but_one"):
        print("cfg 3 %s: %.1f ms per step, %d iterations, %.3f ms per iteration" % (case, d[case]["ms"], d[case]["iterations"], d[case]["ms_per_iter"]))
        assert 0 < d[case]["iterations"] < 200
    print("cfg 3 mixed_none / step_brownian: %.4f" % d["mixed_none"]["ms_ratio"])
    assert d["mixed_none"]["ms_ratio"] <= 1.10
