"""One Python binding (GPU): every method that `RigidBody` now reaches through its borrowed `DeviceContext` is compared with the
same method of an OWNING `DeviceContext` built from the same parameters, structure, configuration, wall and block flags.  Both
then reach one C function, and every product and reduction in the library is fixed-order and bitwise reproducible (DESIGN.md
section 2): the arrays must be equal bit for bit and the iteration counts equal.  A difference means the two disagree on an argument.

3 x shell_N_12, wall on and off, block_PC=True, kBT = 1 (the wrapper's fixed value)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
A, ETA, DT, NB, NBLB = 1.0, 1.0, 0.01, 3, 12
N3 = 3 * NB * NBLB


class _Pair:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["free", "wall"])
def pair(request, shell12):
    import torch
    from conftest import random_positions
    from rigid_body_light_amd import RigidBody
    from rigid_body_light_amd._lib import DeviceContext, lib
    wall = request.param
    p = _Pair()
    p.wall = wall
    p.X, p.Q = random_positions(NB, wall=wall, seed=410, min_dist=4.5)
    if wall:
        p.X[:, 2] += 1.4
    rng = np.random.default_rng(411)
    p.F, p.Up = rng.standard_normal((NB, 6)), 0.5 * rng.standard_normal((NB, 6))
    p.slip, p.W = 0.1 * rng.standard_normal(N3), rng.standard_normal(3 * N3)
    p.rb = RigidBody(shell12, p.X, p.Q, A, ETA, DT, wall_PC=wall, block_PC=True)
    p.ctx = DeviceContext(A, ETA, wall, cfg=shell12, dt=DT, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    p.ctx._chk(p.ctx.L.rbl_set_blk_pc(p.ctx.h, 1))
    p.ctx.set_config(p.X, p.Q)
    assert p.ctx.L is lib() and p.rb.ctx.h == p.rb.cb.handle() != p.ctx.h
    yield p
    p.ctx.close()


def _same(got, want):
    """tuples of arrays and numbers, equal bit for bit"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and np.array_equal(g.reshape(-1), w.reshape(-1))


def _body_in(p, prescribed_bodies):
    bi = np.array(p.F)
    bi[prescribed_bodies] = p.Up[prescribed_bodies]
    return bi


def test_solve_mixed(pair):
    p = pair
    bi = _body_in(p, [1])
    got = p.rb.solve_mixed([1], bi, slip=p.slip, max_iter=200, rtol=1e-10)
    want = p.ctx.solve_mixed(np.array([0, 1, 0], dtype=np.uint8), bi, 200, 1e-10, p.slip)
    _same(got, want)
    assert 0 < got[3] < 200 and got[4] < 1e-10


def test_solve_mixed_dof(pair):
    p = pair
    mask = np.zeros((NB, 6), dtype=bool)
    mask[0, 3:] = mask[2, 2] = True
    bi = np.where(mask, p.Up, p.F)
    got = p.rb.solve_mixed_dof(mask, bi, slip=p.slip, max_iter=200, rtol=1e-10)
    want = p.ctx.solve_mixed_dof(mask.astype(np.uint8), bi, 200, 1e-10, p.slip)
    _same(got, want)
    assert 0 < got[3] < 200 and got[4] < 1e-10


def test_solve_mixed_multi(pair):
    p = pair
    k = 3
    rng = np.random.default_rng(412)
    bi = np.stack([_body_in(p, [1]).reshape(-1)] * k) + 0.1 * rng.standard_normal((k, 6 * NB))
    slip = np.stack([p.slip] * k) * np.arange(1.0, k + 1)[:, None]
    got = p.rb.solve_mixed_multi([1], bi, slip=slip, max_iter=200, rtol=1e-10)
    want = p.ctx.solve_mixed_multi(np.array([0, 1, 0], dtype=np.uint8), bi, 200, 1e-10, slip)
    _same(got, want)
    assert got[0].shape == (k, N3) and np.array_equal(got[3], want[3]) and (got[3] > 0).all() and (got[3] < 200).all()


def test_RHS_and_Midpoint_mixed(pair):
    p = pair
    bi = _body_in(p, [1])
    got = p.rb.RHS_and_Midpoint_mixed([1], bi, slip=p.slip, W=p.W, method="cholesky")
    want = p.ctx.RHS_and_Midpoint_mixed(np.array([0, 1, 0], dtype=np.uint8), bi, slip=p.slip, W=p.W, method="cholesky")
    _same(got, want)
    _same(got, p.ctx.RHS_and_Midpoint_mixed(np.array([0, 1, 0], dtype=np.uint8), bi, slip=p.slip, W=p.W, method=0))
    assert np.linalg.norm(got[0] - p.slip) > 1e-3                        # the Brownian terms are in it


def test_interaction_forces_and_energy(pair):
    p = pair
    k, X0 = np.zeros((NB, 3)), np.array(p.X)
    k[2] = [1.0, 2.0, 0.5]
    X0[2] += [0.3, -0.2, 0.1]
    for o in (p.rb, p.ctx):
        o.set_bonds([[0, 1]], p.rb.blob_anchor(3), p.rb.blob_anchor(7), k=2.0, l0=1.0)
        o.set_traps(k, X0)
    assert p.rb.ctx.interactions_active() == p.ctx.interactions_active() == 64 + 8
    got, phys = p.rb.interaction_forces(), p.ctx.interaction_forces()[1]
    assert np.array_equal(got, -phys) and np.abs(got[:6]).max() > 1e-3 and np.abs(got[12:15]).max() > 1e-3    # reference convention
    assert p.rb.interaction_energy() == p.ctx.interaction_energy() > 0.0
    _same(p.rb.bond_state(), p.ctx.bond_state())
    for o in (p.rb, p.ctx):
        o.set_bonds(None, None, None, None, on=False)
        o.set_traps(k, X0, on=False)
    assert p.rb.ctx.interactions_active() == p.ctx.interactions_active() == 0


def test_solve_jointed(pair):
    p = pair
    rhs = np.array([[0.01, -0.02, 0.03]])
    for o in (p.rb, p.ctx):
        o.set_joints([[0, 1]], [0.0, 0.0, 1.5], [0.0, 0.0, -1.5])
    got = p.rb.solve_jointed(p.F, slip=p.slip, joint_rhs=rhs, max_iter=200, rtol=1e-10)
    want = p.ctx.solve_jointed(p.F, slip=p.slip, joint_rhs=rhs, max_iter=200, rtol=1e-10)
    _same(got, want)
    assert got[2].shape == (3,) and 0 < got[3] < 200 and got[4] < 1e-10
    _same(p.rb.joint_state(), p.ctx.joint_state())
    for o in (p.rb, p.ctx):
        o.set_joints(None, None, None, on=False)


def test_flow_slip_and_first_moments(pair):
    p = pair
    G = np.zeros((3, 3))
    G[0, 2] = 0.7                                                        # a shear the wall admits
    for o in (p.rb, p.ctx):
        o.set_background_flow(G=G)
    got, want = p.rb.flow_slip(), p.ctx.flow_slip()
    assert got.shape == (NB * NBLB, 3) and np.array_equal(got.reshape(-1), want) and np.abs(want).max() > 0.1
    lam = np.random.default_rng(413).standard_normal(N3)
    D, Dc = p.rb.first_moments(lam), p.ctx.first_moments(lam)
    assert D.shape == (NB, 3, 3) and np.array_equal(D, Dc) and np.abs(D).max() > 0.1
    for o in (p.rb, p.ctx):
        o.set_background_flow(on=False)


def test_velocity_field(pair):
    p = pair
    rng = np.random.default_rng(414)
    pts = p.X.mean(axis=0) + rng.uniform(-6.0, 6.0, (5, 3))
    if p.wall:
        pts[:, 2] = np.abs(pts[:, 2]) + 0.5
    lam = rng.standard_normal(N3)
    got, want = p.rb.velocity_field(pts, lam), p.ctx.velocity_field(pts, lam)
    assert got.shape == (5, 3) and np.array_equal(got.reshape(-1), want) and np.abs(want).min() > 0.0
    r = p.rb.get_blob_positions() + 0.01
    assert np.array_equal(p.rb.velocity_field(pts.reshape(-1), lam, positions=r), p.ctx.velocity_field(pts, lam, r))
