"""Prescribed kinematics for many right-hand sides in lock step (include/rbl.h section 7, the _multi entry points) on the GPU:
solve_mixed_multi / solve_mixed_dof_multi column by column against the sequential solve_mixed / solve_mixed_dof, against dense
numpy solutions on the oracle's matrices and through the public operators; the three preconditioner paths; fixed work; the
resistance matrix with lock_step=True; reproducibility, poisoned workspaces, the device form and the reduction of whole-row
component masks to whole-body masks.

Tolerances are the project's own for solve_saddle_multi and solve_mixed_dof: solves to rtol 1e-10 with the residual estimate below
1e-10, a lock-step column within 1e-9 (relative) of the sequential solve of the same column and within +-1 iteration of it (the
multi-vector product rounds differently from the one-vector product, nothing else differs), two solutions of one system within
1e-7, the true residual <= 1e-9, F_p = -K^T lambda to 1e-12.

The columns of a case (_columns): random loads / velocities and slip, one column scaled by 1e-6 and one by 1e4, one with no slip,
and one whose right-hand side is exactly zero -- every prescribed translation driven, every prescribed rotation held, no load on
the free components and slip = -K U_p, which for pure translations is exact in floating point.  Iterations are printed (run with
-s)."""
import numpy as np
import pytest

import test_poisoned_workspace_gpu as pw
import test_prescribed_dof_gpu as td
import test_prescribed_gpu as t

pytestmark = pytest.mark.gpu
WALL_BLOCK = t.WALL_BLOCK
NB, NBLB, K = 10, 12, 19                                   # 19 columns: a batch of 16 on the matrix cores, 3 on the one-vector product
TINY, HUGE, NOSLIP, ZERO = 3, 7, 5, 11                     # the special columns (all inside the first batch but for none; 17, 18: plain)


def _masks(nb=NB):
    """name -> (whole-body mask or None, component mask (nb, 6))"""
    three, everyone = t._sets(nb)["three"], t._sets(nb)["all"]
    return {"three": (three, np.repeat(three[:, None], 6, axis=1)), "all": (everyone, np.repeat(everyone[:, None], 6, axis=1)),
            "random": (None, td._mask("random", nb))}


def _small_mask(nb, whole):
    """for the larger bodies: bodies 1 and 4 prescribed, or a component mask with an all-free, a fully prescribed and a five-of-six body"""
    if whole:
        p = np.isin(np.arange(nb), [1, 4])
        return p, np.repeat(p[:, None], 6, axis=1)
    P = np.random.default_rng(41).random((nb, 6)) < 0.5
    P[0] = False
    P[1] = True
    if nb > 2:
        P[2] = True
        P[2, 4] = False
    else:
        P[0, 3:] = True                                    # two bodies: rotations of body 0, five of six of body 1
        P[1, 2] = False
    return None, P


def _columns(P, nblb, k, seed):
    """body_in (k, 6 nb) and slip (k, 3 N) for the component mask P (a whole-body mask as whole rows); see the module docstring"""
    nb = P.shape[0]
    rng = np.random.default_rng(seed)
    bi, sl = np.zeros((k, 6 * nb)), np.zeros((k, 3 * nb * nblb))
    for c in range(k):
        F, Up, slip = t._inputs(nb, nblb, seed=1000 * seed + c)
        bi[c], sl[c] = td._body_in(P, F, Up), slip
    special = {}
    if k > TINY:
        bi[TINY] *= 1e-6
        sl[TINY] *= 1e-6
    if k > HUGE:
        bi[HUGE] *= 1e4
        sl[HUGE] *= 1e4
    zero, noslip = (ZERO, NOSLIP) if k > ZERO else (k - 1, k - 2)
    sl[noslip] = 0.0
    T = rng.standard_normal((nb, 6))
    T[:, 3:] = 0.0
    Uz = np.where(P, T, 0.0)                               # prescribed translations driven, everything else 0
    bi[zero] = Uz.reshape(-1)
    sl[zero] = -np.repeat(Uz[:, None, :3], nblb, axis=1).reshape(-1)      # -K U_p: a translation moves every blob of the body with it
    special["zero"], special["noslip"] = zero, noslip
    return bi, sl, special


def _solve_multi(rb, p, P, bi, sl, **kw):
    return rb.solve_mixed_multi(p, bi, slip=sl, **kw) if p is not None else rb.solve_mixed_dof_multi(P, bi, slip=sl, **kw)


def _solve_one(rb, p, P, bi, sl, **kw):
    return rb.solve_mixed(p, bi, slip=sl, **kw) if p is not None else rb.solve_mixed_dof(P, bi, slip=sl, **kw)


def _column_parity(rb, p, P, bi, sl, special, label, max_iter=200):
    """the criteria of the issue's `column parity`, shared by every case: -> the lock-step results"""
    nb, k = P.shape[0], bi.shape[0]
    lam, U, F, its, res = _solve_multi(rb, p, P, bi, sl, max_iter=max_iter, rtol=1e-10)
    assert lam.shape == (k, sl.shape[1]) and U.shape == F.shape == (k, 6 * nb) and its.shape == res.shape == (k,)
    its_seq, worst = [], 0.0
    for c in range(k):
        s_c = None if c == special["noslip"] else sl[c]
        lam1, U1, F1, it1, res1 = _solve_one(rb, p, P, bi[c], s_c, max_iter=max_iter, rtol=1e-10)
        its_seq.append(it1)
        assert abs(int(its[c]) - it1) <= 1, (label, c, its[c], it1)
        assert 0 < its[c] < max_iter and res[c] < 1e-10 and res1 < 1e-10, (label, c, its[c], res[c])
        # echoed bitwise: the prescribed velocities and the free loads
        assert np.array_equal(U[c].reshape(nb, 6)[P], bi[c].reshape(nb, 6)[P]), (label, c)
        assert np.array_equal(F[c].reshape(nb, 6)[~P], bi[c].reshape(nb, 6)[~P]), (label, c)
        if c == special["zero"]:
            assert its[c] <= 1 and it1 <= 1, (label, its[c], it1)
            assert not np.any(lam[c]) and not np.any(F[c].reshape(nb, 6)[P]) and not np.any(U[c].reshape(nb, 6)[~P]), label
            assert not np.any(lam1)
            continue
        d = [t._rel(lam[c], lam1), t._rel(U[c], U1), t._rel(F[c], F1)]
        worst = max(worst, max(d))
        assert max(d) <= 1e-9, (label, c, d)
    print("%s: %d columns, lock-step iterations %s, sequential %s; worst rel. diff to the sequential solve %.2e"
          % (label, k, its.tolist(), its_seq, worst))
    assert len(set(its.tolist())) > 1, "every column took the same number of iterations: none rode along converged"
    return lam, U, F, its, res


# ---- 1. column parity with the sequential solve, dense parity, the true residual: 10 x 12 ---------------------------------------------
@pytest.mark.parametrize("which", ("three", "all", "random"))
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_column_parity_with_the_sequential_solve(wall, block, which):
    c, rb = t._body(NB, NBLB, wall, block)
    p, P = _masks()[which]
    bi, sl, special = _columns(P, NBLB, K, seed=51)
    _column_parity(rb, p, P, bi, sl, special, "column parity wall=%s block=%s mask=%s" % (wall, block, which))


@pytest.mark.parametrize("which", ("three", "all", "random"))
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_dense_parity_and_true_residual(orc, wall, block, which):
    c, rb = t._body(NB, NBLB, wall, block)
    M, Kmat = t._dense_matrices(orc, c, c["X"], c["Q"], wall)
    p, P = _masks()[which]
    bi, sl, special = _columns(P, NBLB, K, seed=52)
    lam, U, F, its, res = _solve_multi(rb, p, P, bi, sl, max_iter=200, rtol=1e-10)
    worst_d, worst_r, worst_f = 0.0, 0.0, 0.0
    for col in range(K):
        assert 0 < its[col] < 200 and res[col] < 1e-10
        if col == special["zero"]:
            assert not np.any(lam[col])
            continue
        B = bi[col].reshape(NB, 6)
        lam_d, U_d, F_d = td._dense_dof(M, Kmat, P, np.where(P, 0.0, B), np.where(P, B, 0.0), sl[col])
        d = max(t._rel(lam[col], lam_d), t._rel(U[col], U_d), t._rel(F[col], F_d))
        true_res, ferr = td._operator_residual(rb, P, bi[col], sl[col], lam[col], U[col], F[col])
        worst_d, worst_r, worst_f = max(worst_d, d), max(worst_r, true_res), max(worst_f, ferr)
        assert d <= 1e-7, (col, d)
        assert true_res <= 1e-9 and ferr <= 1e-12, (col, true_res, ferr)
    print("dense parity wall=%s block=%s mask=%s: iterations %s; worst rel. diff to numpy %.2e, true residual %.2e, F_p error %.2e"
          % (wall, block, which, its.tolist(), worst_d, worst_r, worst_f))


# ---- 2. the other preconditioner paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", (False, True))
@pytest.mark.parametrize("wall", (True, False))
def test_shared_factor_pass_and_body_frame_tables_6_x_162(wall, whole):
    """6 x shell_N_162 with the block preconditioner: above the wall per-configuration factors, ONE blk_solve over the 5 vectors
    (three share a pass, then two); in free space the body-frame tables (apply_PC_dev per column, one factor pass, the batched
    tail -- with a whole-body mask the tail reads neither orientations nor a masked factor)"""
    c, rb = t._body(6, 162, wall, True)
    p, P = _small_mask(6, whole)
    bi, sl, special = _columns(P, 162, 5, seed=53)
    lam, U, F, its, res = _column_parity(rb, p, P, bi, sl, special, "6 x 162 wall=%s block, %s mask" % (wall, "whole-body" if whole else "component"))
    for col in range(5):
        if col != special["zero"]:
            true_res, ferr = td._operator_residual(rb, P, bi[col], sl[col], lam[col], U[col], F[col])
            assert true_res <= 1e-9 and ferr <= 1e-12, (col, true_res, ferr)


def test_642_blobs_per_body_five_columns_component_mask():
    """N_blb > 256: the stride loops of the batched tails run three times with a ragged last pass"""
    c, rb = t._body(2, 642, True, True)
    p, P = _small_mask(2, False)
    bi, sl, special = _columns(P, 642, 5, seed=54)
    lam, U, F, its, res = _column_parity(rb, p, P, bi, sl, special, "2 x 642 wall block, component mask")
    for col in range(5):
        if col != special["zero"]:
            true_res, ferr = td._operator_residual(rb, P, bi[col], sl[col], lam[col], U[col], F[col])
            assert true_res <= 1e-9 and ferr <= 1e-12, (col, true_res, ferr)


# ---- 3. fixed work ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("three", "random"))
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_fixed_work(wall, block, which):
    """rtol = 0, max_iter = 9: no convergence test, every column does nine iterations and agrees with the sequential fixed-work solve.
    (The columns are the 19 of column parity without the exactly-zero right-hand side: with no test to stop it, a recurrence on a
    zero vector has nothing to normalise -- that column is column parity's business.)"""
    c, rb = t._body(NB, NBLB, wall, block)
    p, P = _masks()[which]
    bi, sl, special = _columns(P, NBLB, K, seed=55)
    keep = [col for col in range(K) if col != special["zero"]]
    bi, sl = np.ascontiguousarray(bi[keep]), np.ascontiguousarray(sl[keep])
    lam, U, F, its, res = _solve_multi(rb, p, P, bi, sl, max_iter=9, rtol=0.0)
    assert its.tolist() == [9] * len(keep)
    worst = 0.0
    for col in range(len(keep)):
        lam1, U1, F1, it1, res1 = _solve_one(rb, p, P, bi[col], sl[col], max_iter=9, rtol=0.0)
        assert it1 == 9
        d = max(t._rel(lam[col], lam1), t._rel(U[col], U1), t._rel(F[col], F1))
        worst = max(worst, d)
        assert d <= 1e-9, (col, d)
        assert abs(res[col] - res1) <= 1e-9 * max(res1, 1e-300) + 1e-12
    print("fixed work wall=%s block=%s mask=%s: 9 iterations a column, residual estimates %.1e..%.1e, worst rel. diff %.2e"
          % (wall, block, which, res.min(), res.max(), worst))


# ---- 4. the resistance matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_resistance_matrix_in_lock_step(wall, block):
    c, rb = t._body(NB, NBLB, wall, block)
    R0, its0 = rb.body_resistance_matrix(max_iter=200, rtol=1e-10)
    R, its = rb.body_resistance_matrix(max_iter=200, rtol=1e-10, lock_step=True)
    N, _ = rb.body_mobility_matrix(max_iter=200, rtol=1e-11)
    nR = np.linalg.norm(R)
    diff, sym, inv = np.linalg.norm(R - R0) / np.linalg.norm(R0), np.linalg.norm(R - R.T) / nR, np.linalg.norm(R @ N - np.eye(60))
    emin = np.linalg.eigvalsh(0.5 * (R + R.T)).min()
    print("resistance matrix in lock step wall=%s block=%s: iterations %d..%d (sequential %d..%d), rel. diff to the default %.2e, asymmetry %.2e, "
          "|R N - I|_F %.2e, smallest eigenvalue %.3e" % (wall, block, its.min(), its.max(), its0.min(), its0.max(), diff, sym, inv, emin))
    assert R.shape == (60, 60) and its.shape == (60,) and np.all(its > 0) and np.all(its < 200)
    assert diff <= 1e-7 and sym <= 1e-7 and emin > 0.0 and inv <= 1e-6
    Rc, itc = rb.body_resistance_matrix(max_iter=200, rtol=1e-10, columns=[2, 40], lock_step=True)
    assert Rc.shape == (60, 2) and itc.shape == (2,)
    assert t._rel(Rc[:, 0], R[:, 2]) <= 1e-9 and t._rel(Rc[:, 1], R[:, 40]) <= 1e-9      # (two columns: the one-vector product)
    # the default stays the sequential loop, bit for bit
    everyone = np.ones(NB, dtype=bool)
    for j in range(60):
        Uj = np.zeros(60)
        Uj[j] = 1.0
        _, _, Fj, itj, _ = rb.solve_mixed(everyone, Uj, max_iter=200, rtol=1e-10)
        assert np.array_equal(R0[:, j], -Fj) and its0[j] == itj, j


# ---- 5. hygiene ---------------------------------------------------------------------------------------------------------------------------
def test_reproducible_call_to_call():
    for wall, block in WALL_BLOCK:
        c, rb = t._body(NB, NBLB, wall, block)
        for which in ("three", "random"):
            p, P = _masks()[which]
            bi, sl, special = _columns(P, NBLB, K, seed=56)
            a = _solve_multi(rb, p, P, bi, sl, max_iter=200, rtol=1e-10)
            b = _solve_multi(rb, p, P, bi, sl, max_iter=200, rtol=1e-10)
            print("two calls wall=%s block=%s mask=%s: iterations %s" % (wall, block, which, a[3].tolist()))
            assert np.all(a[3] > 0) and np.all(a[3] < 200)
            for x, y in zip(a, b):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_poisoned_workspaces(wall, block):
    """test_poisoned_workspace_gpu.py's pattern: the same inputs through a fresh object with every workspace poisoned and through one
    without -- the same iteration counts, bitwise the same outputs.  17 columns (a batch of 16 and a batch of one, whose buffers
    the first batch used), solved to 1e-10 and with max_iter = 3, at which no column but the zero one has converged: the slots of
    a converged column, the scratch of the factor pass and the second batch must never show unwritten memory"""
    from rigid_body_light_amd import make_config
    c = make_config(NB, NBLB, wall)
    P = td._mask("random")
    p3 = t._sets(NB)["three"]
    bi, sl, special = _columns(P, NBLB, 17, seed=57)

    def fn(poison):
        rb = pw._body(poison, c["cfg"], c["X"], c["Q"], c["a"], wall, block)
        out = {}
        for tag, res in (("dof", rb.solve_mixed_dof_multi(P, bi, slip=sl, max_iter=200, rtol=1e-10)),
                         ("dof3", rb.solve_mixed_dof_multi(P, bi, slip=sl, max_iter=3, rtol=1e-10)),
                         ("body", rb.solve_mixed_multi(p3, bi, slip=sl, max_iter=200, rtol=1e-10)),
                         ("body3", rb.solve_mixed_multi(p3, bi, max_iter=3, rtol=1e-10))):
            for name, v in zip(("lam", "U", "F", "its", "res"), res):
                out[tag + "_" + name] = np.asarray(v)
        return out
    out = pw._twice(fn)
    print("poisoned workspaces wall=%s block=%s: iterations %s; with max_iter 3: %s" % (wall, block, out["dof_its"].tolist(), out["dof3_its"].tolist()))
    assert np.all(out["dof_its"] > 0) and np.all(out["dof_its"] < 200)
    short = np.delete(out["dof3_its"], special["zero"])
    assert np.all(short == 3) and np.all(np.delete(out["dof3_res"], special["zero"]) > 1e-10)      # none of them converged


def test_dev_forms_equal_the_host_forms():
    from rigid_body_light_amd._lib import DeviceContext, lib
    wall = True
    c, rb = t._body(NB, NBLB, wall, True)
    P = td._mask("random")
    p3 = t._sets(NB)["three"]
    bi, sl, special = _columns(P, NBLB, K, seed=58)
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=pw._stream())
    lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_config(c["X"], c["Q"])
    d_bi, d_slip = pw._dev(bi.reshape(-1)), pw._dev(sl.reshape(-1))
    for name, mask, host in (("solve_mixed_dof_multi_dev", P, rb.solve_mixed_dof_multi(P, bi, slip=sl, max_iter=200, rtol=1e-10)),
                             ("solve_mixed_multi_dev", p3, rb.solve_mixed_multi(p3, bi, slip=sl, max_iter=200, rtol=1e-10))):
        d_lam, d_U, d_F = pw._nan(K * 3 * NB * NBLB), pw._nan(K * 6 * NB), pw._nan(K * 6 * NB)
        its, res = getattr(ctx, name)(mask, K, d_bi.data_ptr(), d_slip.data_ptr(), 200, 1e-10, d_lam.data_ptr(), d_U.data_ptr(), d_F.data_ptr())
        ctx.sync_check()
        print("%s: iterations %s" % (name, its.tolist()))
        assert np.array_equal(its, host[3]) and np.array_equal(res, host[4])
        for got, want in zip((d_lam, d_U, d_F), host[:3]):
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    ctx.close()


@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_whole_rows_reduce_to_whole_body_masks(wall, block):
    """whole rows of the component mask: the same kernels on the same bit sets and the same factor values, so solve_mixed_multi's
    results bit for bit"""
    c, rb = t._body(NB, NBLB, wall, block)
    for name, p in t._sets(NB).items():                    # none, bodies 1 4 7, all
        P = np.repeat(p[:, None], 6, axis=1)
        bi, sl, special = _columns(P, NBLB, K, seed=59)
        want = rb.solve_mixed_multi(p, bi, slip=sl, max_iter=200, rtol=1e-10)
        got = rb.solve_mixed_dof_multi(P, bi, slip=sl, max_iter=200, rtol=1e-10)
        print("reduction wall=%s block=%s, whole bodies '%s': iterations %s" % (wall, block, name, got[3].tolist()))
        assert np.all(got[3] > 0) and np.all(got[3] < 200)
        for x, y in zip(got, want):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
