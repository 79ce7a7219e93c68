"""The lock-step solves (rbl_gmres_saddle_multi, rbl_solve_mixed_multi, rbl_solve_mixed_dof_multi: gmres_multi_batch and the
"together" branch of apply_PC_multi_dev) at the shapes of tests/body_shapes.py, where tests/test_body_shapes_gpu.py took the
one-vector solvers: bodies of 3, 4 and 7 blobs (n = 3 N_blb < 32: k_block_solve_small<2/3> in one step), of 255 and 257 blobs
(k_block_solve_pipe<3> then <2>, ragged by three rows), of 513 blobs, and 300 trimers, whose 6 N_bod = 1800 body rows exceed
their N = 900 blobs in every batched tail and in the pitch of the multi-vector product.  What each case reaches is listed in
DESIGN.md section 5b.

The helpers and their bounds are those of tests/test_prescribed_multi_gpu.py (_columns, _column_parity, _solve_multi) and
tests/test_prescribed_dof_gpu.py (_dense_dof, _operator_residual): at rtol 1e-10 a lock-step column is within 1e-9 of the
sequential solve of that column and within one iteration of it, its true residual through the public operators is <= 1e-9, a
masked solution is within 1e-7 of numpy's, an unmasked one within 10 cond(A) rtol (body_shapes.COND_A), and the exactly-zero
column of every set returns exact zeros.  Every context has its workspaces poisoned."""
import numpy as np
import pytest

import body_shapes as bs
import test_prescribed_dof_gpu as td
import test_prescribed_gpu as t
import test_prescribed_multi_gpu as tm
from test_body_shapes_gpu import _dev, _nan, _poison_env, _ref, _stream

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def _body(c, wall, block):
    from rigid_body_light_amd import RigidBody
    with _poison_env():
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 0.01, wall_PC=wall, block_PC=block)
    assert rb.cb.get_option("poison_workspace") == 1
    return rb


def _residuals(rb, P, bi, sl, special, lam, U, F):
    worst = 0.0
    for col in range(bi.shape[0]):
        if col == special["zero"]:
            continue
        true_res, ferr = td._operator_residual(rb, P, bi[col], sl[col], lam[col], U[col], F[col])
        worst = max(worst, true_res)
        assert true_res <= 1e-9 and ferr <= 1e-12, (col, true_res, ferr)
    return worst


def _dense_masked(M, Kmat, P, bi, sl, special, lam, U, F):
    nb, worst = P.shape[0], 0.0
    for col in range(bi.shape[0]):
        if col == special["zero"]:
            continue
        B = bi[col].reshape(nb, 6)
        lam_d, U_d, F_d = td._dense_dof(M, Kmat, P, np.where(P, 0.0, B), np.where(P, B, 0.0), sl[col])
        d = max(t._rel(lam[col], lam_d), t._rel(U[col], U_d), t._rel(F[col], F_d))
        worst = max(worst, d)
        assert d <= 1e-7, (col, d)
    return worst


def _masked_case(name, wall, block, p, P, k, seed, dense):
    c, cfg, Qn, M, Kmat, Am = _ref(name, wall)
    rb = _body(c, wall, block)
    bi, sl, special = tm._columns(P, c["nblb"], k, seed=seed)
    label = "%s %s %s, %s mask, %d columns" % (name, "wall" if wall else "free", "block" if block else "diagonal",
                                                "whole-body" if p is not None else "component", k)
    lam, U, F, its, res = tm._column_parity(rb, p, P, bi, sl, special, label)
    assert np.isfinite(lam).all() and np.isfinite(U).all() and np.isfinite(F).all()
    worst_r = _residuals(rb, P, bi, sl, special, lam, U, F)
    worst_d = _dense_masked(M, Kmat, P, bi, sl, special, lam, U, F) if dense else float("nan")
    print("   worst true residual %.2e (1e-9), worst rel. diff to numpy %.2e (1e-7)" % (worst_r, worst_d))
    return rb, c, bi, sl, (lam, U, F, its, res)


def _saddle_columns(c, k, seed):
    """k right-hand sides [slip ; -F]: random, one scaled by 1e-6, one by 1e4 (k > 7), one with no slip, the last but one exactly zero"""
    n3, nb6 = 3 * c["nb"] * c["nblb"], 6 * c["nb"]
    rng = np.random.default_rng(seed)
    rhs = np.concatenate([0.1 * rng.standard_normal((k, n3)), rng.standard_normal((k, nb6))], axis=1)
    rhs[1] *= 1e-6
    if k > 7:
        rhs[7] *= 1e4
    rhs[0, :n3] = 0.0
    zero = k - 2
    rhs[zero] = 0.0
    return rhs, zero


def _unmasked_case(name, wall, block, k, seed):
    """solve_saddle_multi: column parity with solve_saddle, the true residual through apply_saddle, the dense solve"""
    c, cfg, Qn, M, Kmat, Am = _ref(name, wall)
    rb = _body(c, wall, block)
    rhs, zero = _saddle_columns(c, k, seed)
    x, its, res = rb.solve_saddle_multi(rhs, max_iter=200, rtol=RTOL)
    assert x.shape == rhs.shape and its.shape == res.shape == (k,) and np.isfinite(x).all()
    cond = bs.COND_A[(name, wall)]
    its_seq, w_seq, w_res, w_dense = [], 0.0, 0.0, 0.0
    for col in range(k):
        x1, it1, res1 = rb.solve_saddle(rhs[col], max_iter=200, rtol=RTOL)
        its_seq.append(it1)
        assert abs(int(its[col]) - it1) <= 1, (col, its[col], it1)
        if col == zero:
            assert its[col] <= 1 and not np.any(x[col]) and not np.any(x1), col
            continue
        assert 0 < its[col] < 200 and res[col] < RTOL and res1 < RTOL, (col, its[col], res[col])
        d = t._rel(x[col], x1)
        r = float(np.linalg.norm(rb.apply_saddle(x[col]) - rhs[col]) / np.linalg.norm(rhs[col]))
        e = t._rel(x[col], np.linalg.solve(Am, rhs[col]))
        w_seq, w_res, w_dense = max(w_seq, d), max(w_res, r), max(w_dense, e)
        assert d <= 1e-9 and r <= 1e-9 and e <= 10 * cond * RTOL, (col, d, r, e)
    print("%s %s %s, no mask, %d columns: lock-step iterations %s, sequential %s; worst rel. diff to the sequential solve %.2e (1e-9), true "
          "residual %.2e (1e-9), rel. diff to numpy %.2e = %.1e of the bound %.1e"
          % (name, "wall" if wall else "free", "block" if block else "diagonal", k, its.tolist(), its_seq, w_seq, w_res, w_dense,
             w_dense / (10 * cond * RTOL), 10 * cond * RTOL))
    return rb, c


def _mobility_columns(rb, c, ncol):
    """body_mobility_matrix(columns = range(ncol)) against the sequential solves of the same unit loads"""
    n3, nb6 = 3 * c["nb"] * c["nblb"], 6 * c["nb"]
    N, its = rb.body_mobility_matrix(max_iter=200, rtol=RTOL, columns=range(ncol))
    assert N.shape == (nb6, ncol) and its.shape == (ncol,) and np.isfinite(N).all()
    worst = 0.0
    for j in range(ncol):
        rhs = np.zeros(n3 + nb6)
        rhs[n3 + j] = 1.0
        x1, it1, res1 = rb.solve_saddle(rhs, max_iter=200, rtol=RTOL)
        assert res1 < RTOL and 0 < its[j] < 200 and abs(int(its[j]) - it1) <= 1, (j, its[j], it1)
        worst = max(worst, t._rel(N[:, j], x1[n3:]))
    print("   body_mobility_matrix, %d columns: iterations %s, worst rel. diff to the sequential columns %.2e (1e-9)" % (ncol, its.tolist(), worst))
    assert worst <= 1e-9


# ---- L1: 100 tetrahedra, n = 12 < IB: groups of 3 x 5 + 1; in free space the body-frame tables, column by column ---------------------
@pytest.mark.parametrize("masked", [True, False], ids=["component-mask", "no-mask"])
@pytest.mark.parametrize("wall", [True, False], ids=["wall", "free"])
def test_one_hundred_tetrahedra_sixteen_columns(wall, masked):
    if masked:
        _masked_case("G2", wall, True, None, td._mask("random", 100), 16, seed=61, dense=True)
    else:
        rb, c = _unmasked_case("G2", wall, True, 16, seed=62)
        if wall:
            _mobility_columns(rb, c, 16)


# ---- L2: 300 trimers, n = 9, 6 N_bod = 1800 > N = 900 ------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [True, False], ids=["block", "diagonal"])
def test_three_hundred_trimers_a_third_of_them_held_or_driven(block):
    nb = 300
    p = np.arange(nb) % 3 == 1
    P = np.repeat(p[:, None], 6, axis=1)
    rb, c, bi, sl, host = _masked_case("G1", True, block, p, P, 16, seed=63, dense=False)
    if not block:
        return
    # the device form into NaN outputs: the host form's bits, and no row of 16 x (2700 + 1800 + 1800) left unwritten
    import torch
    from rigid_body_light_amd._lib import DeviceContext, lib
    with _poison_env():
        ctx = DeviceContext(c["a"], c["eta"], True, cfg=c["cfg"], dt=0.01, stream_ptr=_stream())
    try:
        assert ctx.get_option("poison_workspace") == 1 and lib().rbl_set_blk_pc(ctx.h, 1) == 0
        ctx.set_config(c["X"], c["Q"])
        d_bi, d_sl = _dev(bi.reshape(-1)), _dev(sl.reshape(-1))
        d_lam, d_U, d_F = _nan(16 * 2700), _nan(16 * 1800), _nan(16 * 1800)
        its, res = ctx.solve_mixed_multi_dev(p, 16, d_bi.data_ptr(), d_sl.data_ptr(), 200, RTOL, d_lam.data_ptr(), d_U.data_ptr(), d_F.data_ptr())
        ctx.sync_check()
        torch.cuda.synchronize()
        assert np.array_equal(its, host[3]) and np.array_equal(res, host[4])
        for got, want in zip((d_lam, d_U, d_F), host[:3]):
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    finally:
        ctx.close()


# ---- L3: 43 bodies of 7 blobs, n = 21: groups of 3 + 2 ---------------------------------------------------------------------------------
def test_forty_three_seven_blob_bodies_five_columns():
    rb, c, bi, sl, host = _masked_case("G4", True, True, None, td._mask("random", 43), 5, seed=64, dense=True)
    _mobility_columns(rb, c, 12)


# ---- L4: n = 771 and 765: k_block_solve_pipe<3> then <2>, the last step of three rows -----------------------------------------------------
@pytest.mark.parametrize("name", ["G7", "G5"])
def test_bodies_one_blob_either_side_of_256_five_columns(name):
    nb = bs.CASES[name][1]
    p, P = tm._small_mask(nb, False)
    _masked_case(name, True, True, p, P, 5, seed=65, dense=True)


# ---- L5: one body of 513 blobs, n = 1539: 3 + 1 -------------------------------------------------------------------------------------------
def test_one_body_of_513_blobs_four_columns():
    _unmasked_case("G8", True, True, 4, seed=66)
