"""The Brownian midpoint step with prescribed velocity components on the GPU (include/rbl.h sections 5 and 7:
rbl_RHS_and_Midpoint_mixed_dof(_dev), rbl_step_brownian_mixed_dof, rbl_ensemble_step_brownian_mixed_dof), for the masks in which
every body's three rotation entries are all 0 or all 1.

The scheme, restated in numpy below (`_np_rhs_mid6`, `_np_mixed6`, `_np_step6`) on the oracle's matrices.  P: 0/1 per body and
lab-frame component; D_p = diag(P), D_f = I - D_p over the 6 N_bod slots; Kinv = (K^T K)^-1 K^T; W = [W1 | W2 | W_rfd]:
  1. M^{1/2}W1 (and M^{1/2}W2 with split_rand) at q^n -- M of ALL blobs, the mask does not enter;
  2. dq = D_f Kinv W_rfd,  M_RFD = (1/delta)[M(q + delta/2 dq) - M(q - delta/2 dq)] W_rfd,  s = slip - kBT M_RFD - BI
     (split: c1 = 2 sqrt(kBT/dt), c2 = sqrt(kBT/dt), BI = c2 (M^{1/2}W1 - M^{1/2}W2); else c1 = c2 = sqrt(2 kBT/dt), BI = c2 M^{1/2}W1);
  3. q^{n+1/2} = q^n displaced by D_f (dt/2) c1 Kinv M^{1/2}W1 + D_p (dt/2) U_p, in one update_X_Q;
  4. at q^{n+1/2}: [M -K D_f; D_f K^T  D_p][lambda; U] = [s + K D_p U_in; -D_f F_in],  F_p = -D_p K^T lambda;
  5. from q^n: evolve_X_Q(U), a prescribed component by exactly dt U_p.
Tolerances are those of test_brownian_mixed_gpu.py (right-hand side, predictor, whole step, statistics) and of
test_ensemble_mixed_gpu.py (an ensemble replica against the single context); nothing is wider here.  Figures are printed before they
are asserted (run with -s); iteration counts are printed, never asserted beyond "converged within max_iter"."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_brownian_mixed_gpu import KBT, _case, _dense_M_K, _raw, _rel, _solver  # noqa: E402
from test_ensemble_gpu import _configs, _ensemble, _model, _packed, _shell12, _single  # noqa: E402

IT, RTOL = 250, 1e-12                       # the ensemble comparisons, as test_ensemble_mixed_gpu.py
MASKS = ("z of all", "a rotation driven", "held and whole", "nothing")


def _mask6(which, nb):
    """-> (P bool (nb, 6), held bool (nb, 6): the prescribed components whose velocity is zero)"""
    P, held = np.zeros((nb, 6), dtype=bool), np.zeros((nb, 6), dtype=bool)
    if which == "z of all":                                 # a quasi-2D layer: U_z = 0 for every body
        P[:, 2] = held[:, 2] = True
    elif which == "a rotation driven":                      # a roller: body 1 turns as told, its translation is free
        P[1, 3:] = True
    elif which == "held and whole":                         # a trapped probe (body 1, free to turn) and a wholly driven body (2)
        P[1, :3] = held[1, :3] = True
        P[2] = True
    elif which == "mixed":                                  # all three kinds at once
        P[:, 2] = held[:, 2] = True
        P[0, 3:] = True
        P[1, :3] = held[1, :3] = True
    else:
        assert which == "nothing"
    return P, held


def _body_in6(P, held, F, Up):
    return np.where(held, 0.0, np.where(P, Up, F))


def _np_rhs_mid6(orc, cfg, X, Qn, a, eta, wall, dt, kBT, P, body_in, slip, W, split_rand, delta=1.0e-4):
    """steps 1-3 -> (s, X_half, Q_half)"""
    from oracle import oracle as O
    n3 = slip.size
    W1, W2, Wr = W[:n3], W[n3:2 * n3], W[2 * n3:]
    Df = (~P).reshape(-1).astype(np.float64)
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
    Up = np.where(P, body_in.reshape(-1, 6), 0.0).reshape(-1)
    Xh, Qh = O.update_X_Q(X, Qn, Df * (0.5 * dt * c1) * (Kinv @ mw1) + (1.0 - Df) * (0.5 * dt) * Up)
    return s, Xh, Qh


def _np_mixed6(M, K, P, body_in, slip):
    """numpy.linalg.solve on [M -K_f; K_f^T 0] with K_f = the free COLUMNS of K -> (U of all slots, F of all slots)"""
    n3 = M.shape[0]
    bi = body_in.reshape(-1)
    colf = ~P.reshape(-1)
    Kf, Kp = K[:, colf], K[:, ~colf]
    nf = Kf.shape[1]
    A = np.block([[M, -Kf], [Kf.T, np.zeros((nf, nf))]])
    x = np.linalg.solve(A, np.concatenate([slip + Kp @ bi[~colf], -bi[colf]]))
    U, F = np.array(bi), np.array(bi)
    U[colf] = x[n3:]
    F[~colf] = -(Kp.T @ x[:n3])
    return U, F


def _np_step6(orc, cfg, X, Qn, a, eta, wall, dt, kBT, P, body_in, slip, W, split_rand=True):
    """steps 1-5 -> (X, Q, F, U)"""
    from oracle import oracle as O
    s, Xh, Qh = (slip, X, Qn) if kBT <= 1e-10 else _np_rhs_mid6(orc, cfg, X, Qn, a, eta, wall, dt, kBT, P, body_in, slip, W, split_rand)
    M, K = _dense_M_K(orc, cfg, Xh, Qh, a, eta, wall)
    U, F = _np_mixed6(M, K, P, body_in, s)
    Xn, Qn1 = O.evolve(X, Qn, U, dt)
    return Xn, Qn1, F, U


# ---- 1. right-hand side, predictor and whole step against the restatement ------------------------------------------------------------

def _rhs_compare(orc, cfg, a, X, Q, W, slip, P, held, F, Up, wall, split_rand, tag, whole_body=False):
    """RHS_and_Midpoint_mixed_dof (whole_body: RHS_and_Midpoint_mixed with the bodies whose rows of P are set) against the
    restatement -> what the call returned"""
    from oracle import oracle as O
    dt = 0.01
    bi = _body_in6(P, held, F, Up)
    rb = _solver(cfg, X, Q, wall, False, dt=dt, a=a)
    args0 = [v.copy() for v in (P, bi, slip, W)]
    if whole_body:
        assert np.array_equal(P, np.repeat(P[:, :1], 6, axis=1))
        got = rb.RHS_and_Midpoint_mixed(P[:, 0].copy(), bi, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    else:
        got = rb.RHS_and_Midpoint_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    s, Xh, Qh = got
    for v, v0 in zip((P, bi, slip, W), args0):
        assert np.array_equal(v, v0)                                                   # arguments untouched
    Qn = O.normalize_quats(Q)
    s_r, Xr, Qr = _np_rhs_mid6(orc, O.remove_mean(cfg), X, Qn, a, 1.0, wall, dt, KBT, P, bi, slip, W, split_rand)
    Xh, Qh = Xh.reshape(-1, 3), Qh.reshape(-1, 4)
    print("rhs wall=%s split=%s %s: rel. error of s %.2e, |X_half - ref| %.2e, |Q_half - ref| %.2e"
          % (wall, split_rand, tag, _rel(s, s_r), np.abs(Xh - Xr).max(), np.abs(Qh - Qr).max()))
    assert _rel(s, s_r) < 1e-8                      # the difference quotient carries 1e-15/delta of product rounding
    np.testing.assert_allclose(Xh, Xr, rtol=0, atol=1e-11)
    np.testing.assert_allclose(Qh, Qr, rtol=0, atol=1e-11)
    # a held translation component stays, a driven one sits at its own half step; a body whose rotation is held keeps Q
    assert np.array_equal(Xh[held[:, :3]], X[held[:, :3]])
    drv = P[:, :3] & ~held[:, :3]
    if drv.any():
        assert np.abs(Xh[drv] - (X[drv] + 0.5 * dt * Up[:, :3][drv])).max() <= 1e-15 * np.abs(X).max()
    if (~P[:, :3]).any():
        assert np.linalg.norm(Xh - X) > 1e-4                                           # the free ones did move
    X1, Q1 = rb.get_config()
    assert np.array_equal(X1.reshape(-1, 3), X) and np.allclose(Q1.reshape(-1, 4), Qn, rtol=0, atol=1e-15)   # nothing committed
    return got


def _rhs_case6(orc, shell12, wall, split_rand, which):
    X, Q, W, slip, F, Up = _case(wall)
    P, held = _mask6(which, 4)
    _rhs_compare(orc, shell12, 1.0, X, Q, W, slip, P, held, F, Up, wall, split_rand, "mask=%s" % which)


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("split_rand", [True, False])
@pytest.mark.parametrize("wall", [False, True])
def test_rhs_and_predictor_against_the_numpy_restatement(orc, shell12, wall, split_rand, which):
    _rhs_case6(orc, shell12, wall, split_rand, which)


@pytest.mark.parametrize("shape,nb", [("fib257", 2), ("fib7", 3)])
@pytest.mark.parametrize("wall", [False, True])
def test_rhs_and_predictor_at_bodies_of_257_and_of_7_blobs(orc, wall, shape, nb):
    """The comparison above where the sums kernel's loop over a body's blobs is not the 12-blob one: 257 blobs are one past the
    workgroup's 256 threads (a second pass with one live lane), 7 are fewer than the threads and odd.  At each structure a
    whole-body mask (body 0, driven) through the whole-body call and a component mask (z of every body held, the rotation of
    body 1 driven) through the _dof call; and whole rows through _dof are the whole-body call's bits."""
    import body_shapes as bs
    cfg = bs.shape(shape)
    X, Q = bs.lattice(nb, cfg, wall, seed=3)
    n3 = 3 * nb * cfg.shape[0]
    rng = np.random.default_rng(257)
    W, slip, F, Up = rng.standard_normal(3 * n3), 0.1 * rng.standard_normal(n3), rng.standard_normal((nb, 6)), 0.5 * rng.standard_normal((nb, 6))
    none = np.zeros((nb, 6), dtype=bool)
    Pw = none.copy()
    Pw[0] = True
    tag = "%d x %s " % (nb, shape)
    whole = _rhs_compare(orc, cfg, bs.A, X, Q, W, slip, Pw, none, F, Up, wall, True, tag + "body 0, whole-body call", whole_body=True)
    rows = _rhs_compare(orc, cfg, bs.A, X, Q, W, slip, Pw, none, F, Up, wall, True, tag + "body 0, whole rows")
    for x, y in zip(rows, whole):
        assert np.array_equal(x, y)
    P, held = none.copy(), none.copy()
    P[:, 2] = held[:, 2] = True
    P[1, 3:] = True
    _rhs_compare(orc, cfg, bs.A, X, Q, W, slip, P, held, F, Up, wall, True, tag + "z of all, rotation of body 1")


def _check_step(tag, nb, dt, X, Qn, P, held, bi, Up, Xg, Qg, Fo, its, res, ref):
    Xr, Qr, Fr, Ur = ref
    Fo, Fr = Fo.reshape(nb, 6), Fr.reshape(nb, 6)
    relF = _rel(Fo[P], Fr[P]) if P.any() else 0.0
    print("step %s: %d iterations, residual %.2e; |X - ref| %.2e, |Q - ref| %.2e, rel. error of the loads on the prescribed components %.2e"
          % (tag, its, res, np.abs(Xg - Xr).max(), np.abs(Qg - Qr).max(), relF))
    assert 0 < its < 200 and res < 1e-11
    np.testing.assert_allclose(Xg, Xr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(Qg, Qr, rtol=0, atol=1e-9)
    assert relF <= 1e-7
    assert np.array_equal(Fo[~P], bi[~P])                                              # free loads echoed
    # X += dt U_p: one rounding of the sum (half an ulp of |X|)
    drv = P[:, :3] & ~held[:, :3]
    if drv.any():
        assert np.abs((Xg[drv] - X[drv]) - dt * Up[:, :3][drv]).max() <= 1e-15 * np.abs(Xg).max()
    assert np.array_equal(Xg[held[:, :3]], X[held[:, :3]])
    whole_held = held[:, 3:].all(axis=1)
    assert np.abs(Qg[whole_held] - Qn[whole_held]).max(initial=0.0) <= 1e-15
    if (~P[:, :3]).any():
        assert np.linalg.norm(Xg - X) > 1e-4                                           # the free components did move


def _step_case6(orc, shell12, wall, block, which):
    from oracle import oracle as O
    nb, dt = 4, 0.01
    X, Q, W, slip, F, Up = _case(wall, seed=230)
    P, held = _mask6(which, nb)
    bi = _body_in6(P, held, F, Up)
    rb = _solver(shell12, X, Q, wall, block, dt=dt)
    Fo, its, res = rb.step_brownian_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-11)
    Xg, Qg = rb.get_config()
    Qn = O.normalize_quats(Q)
    ref = _np_step6(orc, O.remove_mean(shell12), X, Qn, 1.0, 1.0, wall, dt, KBT, P, bi, slip, W)
    _check_step("wall=%s block=%s mask=%s" % (wall, block, which), nb, dt, X, Qn, P, held, bi, Up, Xg, Qg, Fo, its, res, ref)


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("wall", [False, True])
def test_whole_step_against_the_dense_numpy_step(orc, shell12, wall, block, which):
    _step_case6(orc, shell12, wall, block, which)


def test_rhs_and_step_at_three_shells_of_162_blobs(orc):
    """162 blobs a body: fewer than the body kernels' 256 threads, yet more than one wave -- their loop over the blobs runs once with
    idle lanes and the sums cross waves in the workgroup reduction.  All three kinds of mask at once."""
    from oracle import oracle as O
    from rigid_body_light_amd import RigidBody, make_config
    nb, nblb, wall, dt = 3, 162, True, 0.01
    c = make_config(nb, nblb, wall)
    X, Q, a, eta = np.array(c["X"]).reshape(nb, 3), np.array(c["Q"]).reshape(nb, 4), c["a"], c["eta"]
    n3 = 3 * nb * nblb
    rng = np.random.default_rng(162)
    W, slip, F, Up = rng.standard_normal(3 * n3), 0.1 * rng.standard_normal(n3), rng.standard_normal((nb, 6)), 0.5 * rng.standard_normal((nb, 6))
    P, held = _mask6("mixed", nb)
    bi = _body_in6(P, held, F, Up)
    Qn = O.normalize_quats(Q)
    cfg = O.remove_mean(c["cfg"])
    rb = RigidBody(c["cfg"], X, Q, a=a, eta=eta, dt=dt, wall_PC=wall, block_PC=True)
    s, Xh, Qh = rb.RHS_and_Midpoint_mixed_dof(P, bi, slip=slip, W=W, method="cholesky")
    s_r, Xr, Qr = _np_rhs_mid6(orc, cfg, X, Qn, a, eta, wall, dt, KBT, P, bi, slip, W, True)
    print("rhs 3 x 162: rel. error of s %.2e, |X_half - ref| %.2e, |Q_half - ref| %.2e"
          % (_rel(s, s_r), np.abs(Xh.reshape(-1, 3) - Xr).max(), np.abs(Qh.reshape(-1, 4) - Qr).max()))
    assert _rel(s, s_r) < 1e-8
    np.testing.assert_allclose(Xh.reshape(-1, 3), Xr, rtol=0, atol=1e-11)
    np.testing.assert_allclose(Qh.reshape(-1, 4), Qr, rtol=0, atol=1e-11)
    Fo, its, res = rb.step_brownian_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-11)
    Xg, Qg = rb.get_config()
    ref = _np_step6(orc, cfg, X, Qn, a, eta, wall, dt, KBT, P, bi, slip, W)
    _check_step("3 x 162", nb, dt, X, Qn, P, held, bi, Up, Xg, Qg, Fo, its, res, ref)


# ---- 2. bitwise identities -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [[1, 2], [0], [0, 1, 2, 3]])
@pytest.mark.parametrize("wall", [False, True])
def test_whole_rows_are_bitwise_the_whole_body_calls(shell12, wall, rows):
    """rows all-or-none: the right-hand side, the predictor and the step are the whole-body calls' bits -- configuration, F,
    iteration count.  (No row at all is the next test's case: there the step is step_brownian's bits, from which
    step_brownian_mixed with nobody prescribed differs in the last digits -- two GMRES drivers, test_brownian_mixed_gpu.py's
    test_nothing_prescribed_is_step_brownian; the right-hand side and the predictor with no row are all three calls' bits.)"""
    nb = 4
    X, Q, W, slip, F, Up = _case(wall, seed=280)
    p = np.isin(np.arange(nb), rows)
    bi = np.where(p[:, None], Up, F)
    if rows:
        bi[rows[0]] = 0.0                                                              # one held, the others driven
    P = np.repeat(p[:, None], 6, axis=1)
    a, b = _solver(shell12, X, Q, wall, True), _solver(shell12, X, Q, wall, True)
    for split_rand in (True, False):
        ra = a.RHS_and_Midpoint_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", split_rand=split_rand)
        rb_ = b.RHS_and_Midpoint_mixed(p, bi, slip=slip, W=W, method="cholesky", split_rand=split_rand)
        for x, y in zip(ra, rb_):
            assert np.array_equal(x, y)
    for n in range(2):
        Fa, ita, resa = a.step_brownian_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
        Fb, itb, resb = b.step_brownian_mixed(p, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
        (Xa, Qa), (Xb, Qb) = a.get_config(), b.get_config()
        print("whole rows %s wall=%s step %d: %d / %d iterations, |dX| %.2e |dQ| %.2e |dF| %.2e"
              % (rows, wall, n, ita, itb, np.abs(Xa - Xb).max(), np.abs(Qa - Qb).max(), np.abs(Fa - Fb).max()))
        assert ita == itb and 0 < ita < 200 and resa == resb
        assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb) and np.array_equal(Fa, Fb)
    assert np.linalg.norm(Xa - X) > 1e-4 or len(rows) == nb


@pytest.mark.parametrize("split_rand", [False, True])
@pytest.mark.parametrize("wall", [False, True])
def test_nothing_prescribed_is_step_brownian_bitwise(shell12, wall, split_rand):
    """With no component prescribed the right-hand side and the predictor are RHS_and_Midpoint's bits (and RHS_and_Midpoint_mixed's)
    and the step is step_brownian's: configuration and iteration count.  The library hands such a call to the all-free step; the
    masked solve with an empty mask would agree with it to rounding only (measured here before that: 6 iterations each, |dX|
    1.8e-15, |dQ| 5.6e-17)."""
    nb = 4
    X, Q, W, slip, F, _ = _case(wall, seed=250)
    P = np.zeros((nb, 6), dtype=bool)
    a, b = _solver(shell12, X, Q, wall, True), _solver(shell12, X, Q, wall, True)
    s, Xh, Qh = a.RHS_and_Midpoint_mixed_dof(P, F, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    rhs, Xr, Qr = b.RHS_and_Midpoint(slip, F.reshape(-1), W=W, method="cholesky", split_rand=split_rand)
    sm, Xm, Qm = b.RHS_and_Midpoint_mixed([], F, slip=slip, W=W, method="cholesky", split_rand=split_rand)
    Xh, Qh, Xr, Qr, Xm, Qm = (np.asarray(v).reshape(-1) for v in (Xh, Qh, Xr, Qr, Xm, Qm))
    assert np.array_equal(s, rhs[:s.size]) and np.array_equal(Xh, Xr) and np.array_equal(Qh, Qr)
    assert np.array_equal(s, sm) and np.array_equal(Xh, Xm) and np.array_equal(Qh, Qm)
    Fo, ita, resa = a.step_brownian_mixed_dof(P, F, slip=slip, W=W, method="cholesky", split_rand=split_rand, max_iter=200, rtol=1e-10)
    itb, resb = b.step_brownian(F.reshape(-1), slip=slip, W=W, method="cholesky", split_rand=split_rand, max_iter=200, rtol=1e-10)
    (Xa, Qa), (Xb, Qb) = a.get_config(), b.get_config()
    print("nothing prescribed wall=%s split=%s: step_brownian_mixed_dof %d iterations, step_brownian %d; |dX| %.2e |dQ| %.2e"
          % (wall, split_rand, ita, itb, np.abs(Xa - Xb).max(), np.abs(Qa - Qb).max()))
    assert np.array_equal(Fo, F.reshape(-1)) and np.linalg.norm(Xa - X) > 1e-4
    assert ita == itb and np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)


@pytest.mark.parametrize("wall", [False, True])
def test_zero_temperature_is_step_mixed_dof_bitwise(shell12, wall):
    from rigid_body_light_amd._lib import DeviceContext
    nb = 4
    X, Q, W, slip, F, Up = _case(wall, seed=240)
    P, held = _mask6("mixed", nb)
    bi = _body_in6(P, held, F, Up).reshape(-1)
    mask = P.astype(np.uint8).reshape(-1)
    a, b = _raw(shell12, X, Q, 0.0, wall, True), _raw(shell12, X, Q, 0.0, wall, True)
    va, vb = (DeviceContext.borrow(cm.handle(), 1.0, shell12) for cm in (a, b))       # the views' methods; a and b own the contexts
    Fa, ita, resa = va.step_brownian_mixed_dof(mask, bi, slip=slip, W=W, seed=0, method="cholesky", split_rand=True, delta=1e-4,
                                               max_iter=200, rtol=1e-10)
    Fb, itb, resb = vb.step_mixed_dof(mask, bi, slip=slip, max_iter=200, rtol=1e-10)
    (Xa, Qa), (Xb, Qb) = a.getConfig(), b.getConfig()
    assert ita == itb and 0 < ita < 200 and resa == resb
    assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb) and np.array_equal(Fa, Fb)
    s, Xh, Qh = va.RHS_and_Midpoint_mixed_dof(mask, bi, slip, W)
    assert np.array_equal(s, slip) and np.array_equal(Xh, Xa) and np.array_equal(Qh, Qa)


@pytest.mark.parametrize("with_slip", [True, False])
def test_dev_form_equals_the_host_form(shell12, with_slip):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    wall, dt, nb = True, 0.01, 4
    X, Q, W, slip, F, Up = _case(wall, seed=270)
    P, held = _mask6("mixed", nb)
    bi = _body_in6(P, held, F, Up)
    rb = _solver(shell12, X, Q, wall, False, dt=dt)
    s, Xh, Qh = rb.RHS_and_Midpoint_mixed_dof(P, bi, slip=slip if with_slip else None, W=W, method="cholesky")
    ctx = DeviceContext(1.0, 1.0, wall, cfg=shell12, dt=dt, kBT=KBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(X, Q)
    dev = torch.device("cuda:0")
    d_bi, d_slip, d_W = (torch.from_numpy(np.ascontiguousarray(v).reshape(-1)).to(dev) for v in (bi, slip, W))
    d_s = torch.full((36 * nb,), float("nan"), dtype=torch.float64, device=dev)
    Xd, Qd = ctx.RHS_and_Midpoint_mixed_dof_dev(P, d_bi.data_ptr(), d_slip.data_ptr() if with_slip else None, d_W.data_ptr(), 0, 0, True,
                                                1e-4, d_s.data_ptr())
    ctx.sync_check()
    assert np.array_equal(d_s.cpu().numpy(), s)
    assert np.array_equal(Xd.reshape(-1), Xh.reshape(-1)) and np.array_equal(Qd.reshape(-1), Qh.reshape(-1))
    assert np.array_equal(d_bi.cpu().numpy(), bi.reshape(-1)) and np.array_equal(d_W.cpu().numpy(), W)     # inputs untouched
    # the ctypes form of the whole step is the extension's
    ctx2 = DeviceContext(1.0, 1.0, wall, cfg=shell12, dt=dt, kBT=KBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx2.set_config(X, Q)
    F1, it1, _ = ctx2.step_brownian_mixed_dof(P, bi, max_iter=200, rtol=1e-10, slip=slip, W=W, method=0)
    F2, it2, _ = rb.step_brownian_mixed_dof(P, bi, slip=slip, W=W, method="cholesky", max_iter=200, rtol=1e-10)
    Xc, Qc = ctx2.get_config(nb)
    Xr, Qr = rb.get_config()
    assert it1 == it2 and np.array_equal(F1, F2) and np.array_equal(Xc, Xr.reshape(-1, 3)) and np.array_equal(Qc, Qr.reshape(-1, 4))
    ctx.close()
    ctx2.close()


def test_seeded_noise_is_reproducible(shell12):
    nb = 4
    X, Q, _, slip, F, Up = _case(True, seed=260)
    P, held = _mask6("mixed", nb)
    bi = _body_in6(P, held, F, Up)
    out = []
    for seed in (7, 7, 8):
        rb = _solver(shell12, X, Q, True, True)
        Fo, its, res = rb.step_brownian_mixed_dof(P, bi, slip=slip, seed=seed, method="cholesky", max_iter=200, rtol=1e-10)
        s = rb.RHS_and_Midpoint_mixed_dof(P, bi, slip=slip, seed=seed)[0]
        out.append((Fo, *rb.get_config(), s))
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)
    for x, y in zip(out[0], out[2]):
        assert not np.array_equal(x, y)


# ---- 3. exactness --------------------------------------------------------------------------------------------------------------------

def _velocities(X0, Q0, X1, Q1, dt):
    """the (translation, rotation) velocities that evolve_X_Q turned into the moves q0 -> q1, for arrays of bodies (..., 3), (..., 4):
    test_brownian_mixed_gpu._velocity, vectorised (q_rel = q1 (x) q0^-1, rotation vector 2 atan2(|v|, w) v/|v|)"""
    w0, v0 = Q0[..., :1], -Q0[..., 1:]
    w1, v1 = Q1[..., :1], Q1[..., 1:]
    w = w1 * w0 - np.sum(v1 * v0, axis=-1, keepdims=True)
    v = w1 * v0 + w0 * v1 + np.cross(v1, v0)
    sgn = np.where(w < 0.0, -1.0, 1.0)
    w, v = sgn * w, sgn * v
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    om = np.where(n > 0.0, 2.0 * np.arctan2(n, w) / np.where(n > 0.0, n, 1.0), 0.0) * v
    return np.concatenate([X1 - X0, om], axis=-1) / dt


def test_held_components_stay_bit_for_bit_and_driven_ones_advance_by_dt_Up(shell12):
    """five steps, wall: body 0 has its three translations held and turns freely, every body has z held, body 2 has its rotation
    driven and its x driven: X[0] and every X[:, 2] keep their bits while Q[0] changes; X[2, 0] advances by dt U_p to one rounding
    of the sum per step; the rotation read back from the move is Omega_p to the rounding of the quaternion product (a few ulp of
    1, divided by dt = 0.01: 1e-12 is a hundred times that)."""
    from oracle import oracle as O
    nb, dt, wall = 4, 0.01, True
    X, Q, _, slip, F, Up = _case(wall, seed=290)
    P = np.zeros((nb, 6), dtype=bool)
    P[:, 2] = True
    P[0, :3] = True
    P[2, 3:] = True
    P[2, 0] = True
    bi = np.where(P, 0.0, F)
    bi[2, 3:] = [0.0, 3.0, 0.0]
    bi[2, 0] = 0.7
    rb = _solver(shell12, X, Q, wall, True, dt=dt)
    Xp, Qp = X.copy(), O.normalize_quats(Q)
    for n in range(5):
        Fo, its, res = rb.step_brownian_mixed_dof(P, bi, slip=slip, seed=40 + n, method="cholesky", max_iter=200, rtol=1e-10)
        assert 0 < its < 200
        Xn, Qn = (np.array(v) for v in rb.get_config())
        assert np.array_equal(Xn[0], X[0]) and np.array_equal(Xn[:, 2], X[:, 2])       # bit for bit, from the first configuration on
        assert np.abs(Qn[0] - Qp[0]).max() > 1e-6                                      # while it turns
        assert abs((Xn[2, 0] - Xp[2, 0]) - dt * 0.7) <= 1e-15 * np.abs(Xn).max()
        V = _velocities(Xp, Qp, Xn, Qn, dt)
        print("step %d: %d iterations; |Omega - Omega_p| of the driven body %.2e; free x, y moved by up to %.2e"
              % (n, its, np.abs(V[2, 3:] - bi[2, 3:]).max(), np.abs(Xn[1:, :2] - Xp[1:, :2]).max()))
        assert np.abs(V[2, 3:] - bi[2, 3:]).max() <= 1e-12
        assert np.abs(Xn[1, :2] - Xp[1, :2]).min() > 1e-6 and np.abs(Xn[3, :2] - Xp[3, :2]).min() > 1e-6
        Xp, Qp = Xn, Qn


# ---- 4. ensembles --------------------------------------------------------------------------------------------------------------------

def _ens_masks(R, nb, seed):
    """(R, nb, 6) admissible masks, another kind from replica to replica: all free, whole rows only, z of all, a rotation driven and a
    translation held, then random admissible rows"""
    rng = np.random.default_rng(seed)
    P = np.zeros((R, nb, 6), dtype=bool)
    for r in range(R):
        k = r % 5
        if k == 1:
            P[r, rng.integers(nb)] = True
        elif k == 2:
            P[r, :, 2] = True
        elif k == 3:
            P[r, 0, 3:] = True
            P[r, nb - 1, :3] = True
        elif k == 4:
            P[r, :, :3] = rng.random((nb, 3)) < 0.5
            P[r, :, 3:] = (rng.random(nb) < 0.5)[:, None]
    assert not P[0].any() and set(P[1].sum(axis=1).tolist()) <= {0, 6} and P[1].any()
    return P


def _ens_inputs(P, seed, nblb=12):
    R, nb = P.shape[:2]
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, nb, 6))
    Up = rng.uniform(-1.0, 1.0, (R, nb, 6)) / np.sqrt(3.0)
    Up[:, :, 2] = np.where(rng.random((R, nb)) < 0.5, 0.0, Up[:, :, 2])                # some components held
    bi = np.where(P, Up, F)
    slip = 0.1 * rng.standard_normal((R, 3 * nblb * nb))
    return bi.reshape(R, 6 * nb), slip


@pytest.mark.parametrize("split_rand", [True, False])
@pytest.mark.parametrize("R,nb,steps,sample", [(5, 3, 3, None), (200, 2, 1, [0, 1, 2, 3, 4, 127, 128, 199])])
def test_every_replica_is_the_single_context_step(R, nb, steps, sample, split_rand):
    """15 bodies (not a multiple of the per-body kernels' 256 threads) and 400 bodies (two blocks; replicas 127 and 128 sit on either
    side of the boundary): every compared replica against rbl_step_brownian_mixed_dof(cholesky) at its configuration with its slice
    of W, within test_ensemble_mixed_gpu.py's 1e-7 between two solvers of one system"""
    c = _shell12()
    wall, dt = True, c["dt"]
    X0, Q0 = _configs(R, nb, wall)
    P = _ens_masks(R, nb, 71)
    assert len({m.tobytes() for m in P[:5]}) == 5
    bi, slip = _ens_inputs(P, 72)
    Ws = [np.random.default_rng(73 + n).standard_normal((R, 9 * 12 * nb)) for n in range(steps)]
    ens = _ensemble(c, X0, Q0, wall)
    Xfirst = None
    for n, W in enumerate(Ws):
        F, its, res = ens.ensemble_step_brownian_mixed_dof(P, bi, W=W, split_rand=split_rand, max_iter=IT, rtol=RTOL, slip=slip)
        assert np.all(its > 0) and np.all(its < IT) and np.all(res < RTOL)
        if n == 0:
            Xfirst = ens.ensemble_get_config()[0]
    Xe, Qe = ens.ensemble_get_config()
    ens.close()
    s = _single(c, X0[0], Q0[0], wall)
    for r in (range(R) if sample is None else sample):
        s.set_config(X0[r], Q0[r])
        for W in Ws:
            Fs, it, _ = s.step_brownian_mixed_dof(P[r], bi[r], max_iter=IT, rtol=RTOL, slip=slip[r], W=W[r], method=0, split_rand=split_rand)
            assert 0 < it < IT
        Xs, Qs = s.get_config(nb)
        print("R=%d replica %d, %d of %d components prescribed, split=%s: |X - single| %.2e |Q - single| %.2e, rel. diff F %.2e"
              % (R, r, int(P[r].sum()), 6 * nb, split_rand, np.abs(Xe[r] - Xs).max(), np.abs(Qe[r] - Qs).max(), _rel(F[r], Fs)))
        assert np.abs(Xe[r] - Xs).max() <= 1e-7 and np.abs(Qe[r] - Qs).max() <= 1e-7
        assert _rel(F[r], Fs) <= 1e-7
        Pt, Up = P[r][:, :3], bi[r].reshape(nb, 6)[:, :3]
        if Pt.any():                                                                   # X += dt U_p: one rounding of the sum
            assert np.abs((Xfirst[r][Pt] - X0[r][Pt]) - dt * Up[Pt]).max() <= 1e-15 * np.abs(Xfirst[r]).max()
        hold = Pt & (Up == 0.0)
        assert np.array_equal(Xe[r][hold], X0[r][hold])
        if (~Pt).any():
            assert np.linalg.norm(Xe[r][~Pt] - X0[r][~Pt]) > 1e-5
    s.close()


@pytest.mark.parametrize("per", [6, 1])
def test_258_trimers_with_masks_that_differ_lane_by_lane(per):
    """43 replicas of 6 trimers: 258 bodies, so the second workgroup of the one-thread-per-body kernels has two live lanes, and 3
    blobs a body.  Replica r holds z of the bodies in r's bits and drives the whole of body r % 6: neighbouring lanes of the masked
    predictor kernel hold free bodies, bodies with z alone, whole bodies -- a mask decoded for one lane and used by another gives
    another configuration.  per = 6: that mask through ensemble_step_brownian_mixed_dof; per = 1: its whole-body part alone through
    ensemble_step_brownian_mixed.  One step, injected noise; every replica against the single-context step at its configuration
    within the 1e-7 of test_every_replica_is_the_single_context_step."""
    import body_shapes as bs
    R, nb, wall = 43, 6, True
    cfg = bs.trimer()
    c = {"cfg": cfg, "a": bs.A, "eta": bs.ETA, "dt": 0.01}
    X0, Q0 = (np.stack(v) for v in zip(*(bs.lattice(nb, cfg, wall, seed=bs.replica_seed(r)) for r in range(R))))
    whole = np.arange(nb)[None, :] == (np.arange(R) % nb)[:, None]
    P = np.zeros((R, nb, 6), dtype=bool)
    if per == 6:
        P[:, :, 2] = ((np.arange(R)[:, None] >> np.arange(nb)[None, :]) & 1).astype(bool)
    P[whole] = True
    kinds = {int(k) for k in np.unique((P * (1 << np.arange(6))).sum(axis=2))}
    assert kinds == ({0, 4, 63} if per == 6 else {0, 63}) and len({m.tobytes() for m in P}) == (R if per == 6 else nb)
    bi, slip = _ens_inputs(P, 92, nblb=3)
    W = np.random.default_rng(93).standard_normal((R, 9 * 3 * nb))
    ens = _ensemble(c, X0, Q0, wall)
    if per == 6:
        F, its, res = ens.ensemble_step_brownian_mixed_dof(P, bi, W=W, max_iter=IT, rtol=RTOL, slip=slip)
    else:
        F, its, res = ens.ensemble_step_brownian_mixed(whole, bi, W=W, max_iter=IT, rtol=RTOL, slip=slip)
    assert np.all(its > 0) and np.all(its < IT) and np.all(res < RTOL)
    Xe, Qe = ens.ensemble_get_config()
    ens.close()
    s = _single(c, X0[0], Q0[0], wall)
    worst = np.zeros(3)
    for r in range(R):
        s.set_config(X0[r], Q0[r])
        if per == 6:
            Fs, it, _ = s.step_brownian_mixed_dof(P[r], bi[r], max_iter=IT, rtol=RTOL, slip=slip[r], W=W[r], method=0)
        else:
            Fs, it, _ = s.step_brownian_mixed(whole[r], bi[r], max_iter=IT, rtol=RTOL, slip=slip[r], W=W[r], method=0)
        assert 0 < it < IT
        Xs, Qs = s.get_config(nb)
        worst = np.maximum(worst, [np.abs(Xe[r] - Xs).max(), np.abs(Qe[r] - Qs).max(), _rel(F[r], Fs)])
        assert np.abs(Xe[r] - Xs).max() <= 1e-7 and np.abs(Qe[r] - Qs).max() <= 1e-7, r
        assert _rel(F[r], Fs) <= 1e-7, r
        Pt, Up = P[r][:, :3], bi[r].reshape(nb, 6)[:, :3]
        assert np.abs((Xe[r][Pt] - X0[r][Pt]) - c["dt"] * Up[Pt]).max() <= 1e-15 * np.abs(Xe[r]).max()   # X += dt U_p: one rounding
        assert np.linalg.norm(Xe[r][~Pt] - X0[r][~Pt]) > 1e-5
    s.close()
    print("258 trimers, per=%d: worst |X - single| %.2e |Q - single| %.2e, rel. diff F %.2e" % (per, *worst))


@pytest.mark.parametrize("R,nb", [(5, 3), (200, 2)])
def test_whole_rows_in_every_replica_are_bitwise_the_whole_body_ensemble_step(R, nb):
    from test_ensemble_mixed_gpu import _inputs
    c = _shell12()
    wall = True
    X0, Q0 = _configs(R, nb, wall)
    mask = ((np.arange(R)[:, None] >> np.arange(nb)[None, :]) & 1).astype(bool)       # replica r prescribes the bodies in r's bits
    assert not mask[0].any() and mask[2 ** nb - 1].all() if R >= 2 ** nb else mask.any()
    bi, slip = _inputs(R, nb, mask, 82)
    P = np.repeat(mask[:, :, None], 6, axis=2)
    a, b = _ensemble(c, X0, Q0, wall), _ensemble(c, X0, Q0, wall)
    for n in range(2):
        kw = dict(seed=90 + n) if n else dict(W=np.random.default_rng(83).standard_normal((R, 9 * 12 * nb)))
        Fa, ita, resa = a.ensemble_step_brownian_mixed_dof(P, bi, max_iter=120, rtol=1e-10, slip=slip, **kw)
        Fb, itb, resb = b.ensemble_step_brownian_mixed(mask, bi, max_iter=120, rtol=1e-10, slip=slip, **kw)
        (Xa, Qa), (Xb, Qb) = a.ensemble_get_config(), b.ensemble_get_config()
        print("whole rows R=%d step %d: |dX| %.2e |dQ| %.2e |dF| %.2e" % (R, n, np.abs(Xa - Xb).max(), np.abs(Qa - Qb).max(), np.abs(Fa - Fb).max()))
        assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.all(ita > 0) and np.all(ita < 120)
        assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb) and np.array_equal(Fa, Fb)
    assert np.abs(Xa - X0).max() > 1e-5
    a.close()
    b.close()


def test_an_inadmissible_mask_in_one_replica_is_refused_names_it_and_moves_nobody():
    c = _shell12()
    R, nb, wall, k = 5, 3, True, 3
    X0, Q0 = _configs(R, nb, wall)
    P = _ens_masks(R, nb, 71)
    bi, slip = _ens_inputs(P, 72)
    ens = _ensemble(c, X0, Q0, wall)
    bad = P.copy()
    bad[k, 1, 3:] = [True, False, True]
    bad[4, 0, 3:] = [False, True, False]                                               # a later offender: the first is named
    with pytest.raises(ValueError) as e:                                               # the Python layer, before the library
        ens.ensemble_step_brownian_mixed_dof(bad, bi, seed=1, max_iter=40, rtol=1e-8)
    assert "replica %d, body 1" % k in str(e.value)
    # the library itself
    m = np.ascontiguousarray(bad, dtype=np.uint8)
    F, its, res = np.zeros((R, 6 * nb)), np.zeros(R, dtype=np.int32), np.zeros(R)
    call = lambda mm: ens.L.rbl_ensemble_step_brownian_mixed_dof(ens.h, mm.ctypes.data, bi.ctypes.data, slip.ctypes.data, None, 1, 1, 1e-4, 40,
                                                                 1e-8, F.ctypes.data, its.ctypes.data, res.ctypes.data)
    assert call(m) == 11
    msg = ens.L.rbl_last_error(ens.h).decode()
    assert msg == str(e.value), (msg, str(e.value))
    assert msg.startswith("ensemble_step_brownian_mixed_dof: replica %d, body 1: the rotation is partly prescribed" % k)
    two = np.ascontiguousarray(P, dtype=np.uint8)
    two[2, 1, 0] = 2
    assert call(two) == 11 and "0 or 1" in ens.L.rbl_last_error(ens.h).decode()
    Xc, Qc = ens.ensemble_get_config()
    assert np.array_equal(Xc, X0) and np.allclose(Qc, Q0, rtol=0, atol=1e-15) and not its.any()
    F1, it1, _ = ens.ensemble_step_brownian_mixed_dof(P, bi, seed=1, max_iter=120, rtol=1e-8, slip=slip)       # the repaired call runs
    assert np.all(it1 > 0) and np.all(it1 < 120) and np.abs(ens.ensemble_get_config()[0] - X0).max() > 1e-6
    ens.close()


def test_force_model_enters_the_free_components_only():
    """model on: the Brownian step of a model-free ensemble that is handed interaction_forces() in the free slots and zeros in the
    prescribed ones -- the same system, the same bits, per replica (test_force_model_enters_the_free_components_only of
    test_ensemble_dof_gpu.py, with noise)"""
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 9)
    model = _model(c["a"])
    P = np.zeros((R, nb, 6), dtype=bool)
    P[:, :, :3] = np.random.default_rng(12).random((R, nb, 3)) < 0.5
    P[:, 1] = True                                          # a fully prescribed body, an all-free one, a roller, in every replica
    P[:, 2] = False
    P[:, 3] = [False, False, False, True, True, True]
    on, off = _ensemble(c, X0, Q0, wall, dt=1e-3, model=model), _ensemble(c, X0, Q0, wall, dt=1e-3)
    share = on.ensemble_interaction_forces()[0].reshape(R, nb, 6)
    assert np.abs(share[P]).max() > 1e-3 and np.abs(share[~P]).max() > 1e-3          # the model loads prescribed components too
    handed = np.where(P, 0.0, share).reshape(R, 6 * nb)
    W = np.random.default_rng(10).standard_normal((R, 9 * 12 * nb))
    Fa, ita, resa = on.ensemble_step_brownian_mixed_dof(P, np.zeros(6 * nb), W=W, max_iter=IT, rtol=1e-10)
    Fb, itb, resb = off.ensemble_step_brownian_mixed_dof(P, handed, W=W, max_iter=IT, rtol=1e-10)
    print("model on, component masks, Brownian: iterations %s; |F_on - F_handed| %.2e" % (ita, np.abs(Fa - Fb).max()))
    assert np.all(ita > 0) and np.all(ita < IT)
    assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.array_equal(Fa, Fb)
    (Xa, Qa), (Xb, Qb) = on.ensemble_get_config(), off.ensemble_get_config()
    assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)
    assert np.array_equal(Xa[:, 1], X0[:, 1]) and np.abs(Xa[:, 2] - X0[:, 2]).max() > 1e-6
    assert np.array_equal(Fa.reshape(R, nb, 6)[~P], handed.reshape(R, nb, 6)[~P])      # free loads echoed WITH the model's share
    assert np.abs(Fa.reshape(R, nb, 6)[P]).max() > 1e-3                                # holding takes a load
    # with the model's loads handed to the prescribed slots too they would be read as velocities: far more than rounding
    off.ensemble_set_config(X0, Q0)
    Fbad = off.ensemble_step_brownian_mixed_dof(P, share.reshape(R, 6 * nb), W=W, max_iter=IT, rtol=1e-10)[0]
    assert _rel(Fbad, Fa) > 1e-4
    on.close()
    off.close()


# ---- 5. poisoned workspaces ----------------------------------------------------------------------------------------------------------

_POISON_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from oracle import Oracle
import test_brownian_dof_gpu as t
from rigid_body_light_amd import RigidBody, load_structure, make_config
c = make_config(2, 12, False)
assert RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 0.01).cb.get_option("poison_workspace") == 1
orc, shell12 = Oracle(), load_structure(12)[1]
t._rhs_case6(orc, shell12, True, True, "mixed")
t._step_case6(orc, shell12, True, True, "mixed")
print("ALL OK")
"""


def test_rhs_and_step_with_poisoned_workspaces():
    """every device workspace filled with NaN at each reserve (RBL_POISON_WORKSPACE=1, a child process): a read of memory
    nobody wrote fails tests 1 and 2"""
    env = dict(os.environ, RBL_POISON_WORKSPACE="1")
    p = subprocess.run([sys.executable, "-c", _POISON_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout


# ---- 6. the statistics of the step -----------------------------------------------------------------------------------------------------

_STAT = {}


def _stat_oracle(orc):
    """the configuration and what the oracle says about it, computed once and shared by the three masks: N_tilde and the divergence
    for any mask, on demand"""
    if _STAT:
        return _STAT
    from oracle import oracle as O
    c = _shell12()
    a, eta, wall = c["a"], 1.0, True
    cfg = O.remove_mean(c["cfg"])
    X = np.array([[0.0, 0.0, 1.6], [2.4, 0.0, 1.5]])
    Qn = O.normalize_quats(np.random.default_rng(5).standard_normal((2, 4)))

    def N_tilde(Xc, Qc, free):
        M, K = _dense_M_K(orc, cfg, Xc, Qc, a, eta, wall)
        Kf = K[:, free]
        return np.linalg.inv(Kf.T @ np.linalg.solve(M, Kf))

    def divergence(free, h=1e-5):
        """kBT sum_{k free} d N_{.k} / d q_k by central differences through update_X_Q -> one entry per free slot"""
        slots = np.flatnonzero(free)
        d = np.zeros(slots.size)
        for col, k in enumerate(slots):
            e = np.zeros(12)
            e[k] = h
            Np = N_tilde(*O.update_X_Q(X, Qn, e), free)
            Nm = N_tilde(*O.update_X_Q(X, Qn, -e), free)
            d += KBT * (Np[:, col] - Nm[:, col]) / (2.0 * h)
        return d
    everyone = np.ones(12, dtype=bool)
    _STAT.update(c=c, a=a, eta=eta, wall=wall, cfg=cfg, X=X, Qn=Qn, N_tilde=N_tilde, divergence=divergence, d_allfree=divergence(everyone))
    return _STAT


def _statistics(orc, P, bi, steps=100):
    st = _stat_oracle(orc)
    c, X, Qn, dt = st["c"], st["X"], st["Qn"], 0.01
    R, half = 256, 128
    free = ~P.reshape(-1)
    Nt = st["N_tilde"](X, Qn, free)
    d = st["divergence"](free)
    M, K = _dense_M_K(orc, st["cfg"], X, Qn, st["a"], st["eta"], st["wall"])
    U_det = _np_mixed6(M, K, P, bi.reshape(-1), np.zeros(M.shape[0]))[0][free]
    X0, Q0 = np.repeat(X[None], R, axis=0), np.repeat(Qn[None], R, axis=0)
    ens = _ensemble(c, X0, Q0, st["wall"], kBT=KBT, dt=dt)
    rng = np.random.default_rng(7)
    e, o = np.zeros((steps * half, int(free.sum()))), np.zeros((steps * half, int(free.sum())))
    worst_its = 0
    for n in range(steps):
        W = rng.standard_normal((half, 216))                                           # pair by pair
        ens.ensemble_set_config(X0, Q0)
        _, its, res = ens.ensemble_step_brownian_mixed_dof(P, bi.reshape(-1), W=np.concatenate([W, -W]), max_iter=200, rtol=1e-10)
        assert np.all(its > 0) and np.all(its < 200) and np.all(res < 1e-10)
        worst_its = max(worst_its, int(its.max()))
        X1, Q1 = ens.ensemble_get_config()
        U = _velocities(X0, Q0, X1, Q1, dt).reshape(R, 12)[:, free]
        e[n * half:(n + 1) * half] = 0.5 * (U[:half] + U[half:])
        o[n * half:(n + 1) * half] = 0.5 * (U[:half] - U[half:])
    ens.close()
    S = steps * half
    se = e.std(axis=0) / np.sqrt(S)
    full = lambda v: _scatter(v, free)                                                 # by slot among all 12, nan where prescribed
    return dict(S=S, free=free, se=full(se), dev=full((e.mean(axis=0) - U_det - d) / se), d=full(d), d_allfree=st["d_allfree"],
                ratio=full((o * o).mean(axis=0) * dt / (2.0 * KBT) / np.diag(Nt)), its=worst_its)


def _scatter(v, free):
    out = np.full(free.size, np.nan)
    out[free] = v
    return out


def _stat_case(name):
    P, bi = np.zeros((2, 6), dtype=bool), np.zeros((2, 6))
    if name == "z of both held":
        P[:, 2] = True
    elif name == "rotation of body 1 driven":
        P[1, 3:] = True
        bi[1, 3:] = [0.0, 3.0, 0.0]
    else:
        assert name == "translation of body 0 held"
        P[0, :3] = True
    return P, bi


@pytest.mark.parametrize("name", ["z of both held", "rotation of body 1 driven", "translation of body 0 held"])
def test_drift_and_covariance_of_the_free_components(orc, name):
    """Two shell_N_12 above the wall (a = sep/2, eta = 1, kBT = 1, dt = 0.01, X = [[0, 0, 1.6], [2.4, 0, 1.5]], Q = default_rng(5)
    normalised), F = 0, slip 0, rtol 1e-10, max_iter 200; an ensemble of 256 replicas all at that configuration, reset before
    every step; replicas r and r + 128 get W and -W, W = default_rng(7).standard_normal(216) drawn pair by pair; 100 steps give
    S = 12 800 antithetic pairs.  e = (U(W) + U(-W))/2 carries the drift, o = (U(W) - U(-W))/2 the noise, per free slot, U read
    back from the move.  With Ntilde = ((K D_f)^T M^-1 K D_f)^-1 from the oracle's dense matrices, d = kBT sum_{k free}
    d Ntilde_{.k} / d q_k (central differences, h = 1e-5, through update_X_Q) and U_det the dense noise-free solve:
      (a) |mean(e) - U_det - d| <= 4 s.e. in every free slot, s.e. = std(e)/sqrt(S);
      (b) power, per mask: z of both held -- |d| >= 10 s.e. in x of each body and |d - d_allfree| >= 4 s.e. there (d_allfree: the
          divergence with nobody prescribed, at the same slots); rotation of body 1 driven with Omega = (0, 3, 0) -- |d_z| >= 10 s.e.
          for both bodies; translation of body 0 held -- |d_x - d_x^allfree| >= 4 s.e. on body 1;
      (c) diag(mean(o o^T)) dt/(2 kBT) within 4 sqrt(2/S) = 5 % of diag(Ntilde).
    The numpy restatement of the scheme alone meets these on the same inputs (worst (a) 1.14 / 2.45 / 1.73 s.e., variance ratios
    0.989-1.009 / 0.983-1.021 / 1.001-1.021, power 12.4 and 11.6, 6.4 and 7.6 / 31 and 60 / 6.8 s.e.); a step without the RFD term
    misses d_z by the power figure, ignoring the hold of body 0 gives 1.36 Ntilde_xx on body 1."""
    P, bi = _stat_case(name)
    t0 = time.perf_counter()
    r = _statistics(orc, P, bi)
    wall_s = time.perf_counter() - t0
    S, free, se, d, da = r["S"], r["free"], r["se"], r["d"], r["d_allfree"]
    fmt = lambda v: np.array2string(np.asarray(v), precision=3, suppress_small=False)
    print("statistics, %s: S = %d; deviations (s.e.) %s; d %s; d_allfree %s; s.e. %s; variance ratios %s; at most %d iterations; %.1f s"
          % (name, S, fmt(r["dev"]), fmt(d), fmt(da), fmt(se), fmt(r["ratio"]), r["its"], wall_s))
    assert S == 12800
    assert np.all(np.abs(r["dev"][free]) <= 4.0)                                                   # (a)
    if name == "z of both held":                                                                   # (b)
        for k in (0, 6):
            print("power in slot %d: |d| = %.1f s.e., |d - d_allfree| = %.1f s.e." % (k, abs(d[k]) / se[k], abs(d[k] - da[k]) / se[k]))
            assert abs(d[k]) >= 10.0 * se[k] and abs(d[k] - da[k]) >= 4.0 * se[k]
    elif name == "rotation of body 1 driven":
        for k in (2, 8):
            print("power in slot %d: |d_z| = %.1f s.e." % (k, abs(d[k]) / se[k]))
            assert abs(d[k]) >= 10.0 * se[k]
    else:
        print("power in slot 6: |d_x - d_x^allfree| = %.1f s.e." % (abs(d[6] - da[6]) / se[6]))
        assert abs(d[6] - da[6]) >= 4.0 * se[6]
    assert np.all(np.abs(r["ratio"][free] - 1.0) <= 4.0 * np.sqrt(2.0 / S))                        # (c)


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------

def test_example_ensemble_quasi2d_keeps_the_heights_and_diffuses_in_the_plane():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_quasi2d.py"), "--replicas", "16", "--bodies", "3",
                          "--steps", "5"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith("step ")]
    assert len(rows) == 5
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    print(out.stdout)
    assert np.all(np.isfinite(vals)) and np.all(vals[:, 2] > 0.0) and np.all(np.diff(vals[:, 2]) != 0.0)
    assert "heights unchanged bit for bit: True" in out.stdout
