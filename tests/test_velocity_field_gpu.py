"""Fluid velocity at arbitrary points (include/rbl.h section 6) on the GPU: the CPU oracle with the points appended as
zero-force blobs, probes on blobs against apply_M's rows, the wall rule, every split shape, the full cfg 3 size, the physics
of a solved body (no slip at the blobs, the far-field Stokeslet), reproducibility, communicators and the example."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _body(nb, nblb, wall, seed=0):
    from rigid_body_light_amd import RigidBody, make_config
    c = make_config(nb, nblb, wall, seed=seed)
    rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=wall)
    return c, rb


def _points_near(r, a, n, dmin, dmax, wall, seed, zmin=None):
    """n random points whose nearest blob lies between dmin and dmax; with the wall above zmin (default 0.05 a)"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    R = r.reshape(-1, 3)
    tree = cKDTree(R)
    lo, hi = R.min(axis=0) - dmax, R.max(axis=0) + dmax
    if wall:
        lo[2] = zmin if zmin is not None else 0.05 * a
    out = []
    while sum(len(o) for o in out) < n:
        x = rng.uniform(lo, hi, (4 * n, 3))
        d, _ = tree.query(x)
        out.append(x[(d >= dmin) & (d <= dmax)])
    return np.concatenate(out)[:n]


def _oracle_rows(orc, lam, r, pts, a, eta, wall):
    N, P = lam.size // 3, pts.size // 3
    return orc.apply_M_rows(np.concatenate([lam, np.zeros(3 * P)]), np.concatenate([r.reshape(-1), pts.reshape(-1)]),
                            N, N + P, a, eta, wall, nthreads=8)


def _rel(u, v):
    return np.linalg.norm(u - v) / np.linalg.norm(v)


@pytest.mark.parametrize("wall", [False, True])
def test_oracle_parity_cfg1_random_points(orc, wall):
    c, rb = _body(10, 12, wall)
    r = rb.get_blob_positions().reshape(-1)
    lam = np.random.default_rng(1).standard_normal(r.size)
    a = c["a"]
    pts = _points_near(r, a, 1000, 0.3 * a, 50 * a, wall, seed=2)
    if wall:
        assert (pts[:, 2] < a).sum() >= 20                 # some points inside the damped layer
    u = rb.velocity_field(pts, lam, r)
    assert u.shape == pts.shape
    uo = _oracle_rows(orc, lam, r, pts, a, c["eta"], wall)
    assert _rel(u.reshape(-1), uo) <= 1e-12


@pytest.mark.parametrize("wall", [False, True])
def test_probes_on_blobs_return_apply_M_rows(wall):
    c, rb = _body(10, 12, wall)
    r = rb.get_blob_positions().reshape(-1, 3)
    lam = np.random.default_rng(4).standard_normal(r.size)
    idx = np.array([0, 5, 11, 12, 40, 77, 119, 118, 60])            # blobs of several bodies
    u = rb.velocity_field(r[idx], lam)                              # no RBL_ERR_OVERLAP: the self block
    U = rb.apply_M(lam, r.reshape(-1)).reshape(-1, 3)
    assert _rel(u, U[idx]) <= 1e-13
    for i, k in enumerate(idx):
        assert np.linalg.norm(u[i] - U[k]) <= 1e-13 * np.linalg.norm(U[k]) * 10


def test_points_at_or_below_the_wall_get_zero():
    c, rb = _body(10, 12, True)
    r = rb.get_blob_positions().reshape(-1)
    lam = np.random.default_rng(5).standard_normal(r.size)
    a = c["a"]
    good = _points_near(r, a, 300, 0.3 * a, 20 * a, True, seed=6)
    bad = good[:40].copy()
    bad[:, 2] = -np.abs(bad[:, 2])
    bad[:10, 2] = 0.0
    pts = np.concatenate([good[:150], bad, good[150:]])
    u = rb.velocity_field(pts, lam)
    ug = rb.velocity_field(good, lam)
    assert np.all(u[150:190] == 0.0)
    assert _rel(np.concatenate([u[:150], u[190:]]), ug) <= 1e-14


def _sources(N, wall, seed):
    from rigid_body_light_amd import make_config
    if N == 8100:
        from oracle import Oracle
        c = make_config(50, 162, wall)
        return Oracle().multi_body_pos(c["X"], c["Q"], c["cfg"] - c["cfg"].mean(axis=0)), c["a"]
    rng = np.random.default_rng(seed)
    a = 0.5
    r = np.empty((N, 3))
    n = 0
    while n < N:                                               # blobs at least 2a apart, above the wall
        x = rng.uniform([-3, -3, 0.6], [3, 3, 6], 3)
        if n == 0 or np.min(np.linalg.norm(r[:n] - x, axis=1)) > 2 * a:
            r[n] = x; n += 1
    return r.reshape(-1), a


def _ctx(a, wall):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    return DeviceContext(a, 1.0, wall, stream_ptr=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N", [1, 12, 8100])
@pytest.mark.parametrize("P", [1, 63, 65, 4097])
def test_ragged_and_split_shapes_against_the_oracle(orc, P, N):
    wall = (P + N) % 2 == 1
    r, a = _sources(N, wall, seed=P)
    lam = np.random.default_rng(7).standard_normal(r.size)
    pts = _points_near(r, a, P, 0.3 * a, 30 * a, wall, seed=P + 1)
    ctx = _ctx(a, wall)
    u = ctx.velocity_field(pts, lam, r)
    ctx.close()
    uo = _oracle_rows(orc, lam, r, pts, a, 1.0, wall)
    assert _rel(u, uo) <= 1e-12


def test_every_geometry_shape_against_the_oracle(orc):
    """both point counts per lane x (one chunk, several chunks): the sizes that select them, found through the _info entry point"""
    seen = set()
    for N in (12, 8100):
        for P in (100, 16384 + 37):
            wall = True
            r, a = _sources(N, wall, seed=N)
            ctx = _ctx(a, wall)
            ni, ch, wb = ctx.velocity_field_info(P, N)
            assert ni in (2, 4) and ch >= 1 and wb > 0
            seen.add((ni, ch > 1))
            lam = np.random.default_rng(8).standard_normal(r.size)
            pts = _points_near(r, a, P, 0.3 * a, 30 * a, wall, seed=N + P)
            u = ctx.velocity_field(pts, lam, r).reshape(-1, 3)
            ctx.close()
            rows = np.random.default_rng(9).choice(P, size=min(P, 300), replace=False)
            uo = _oracle_rows(orc, lam, r, pts[rows], a, 1.0, wall).reshape(-1, 3)
            assert _rel(u[rows], uo) <= 1e-12, (N, P, ni, ch)
    assert seen == {(2, False), (2, True), (4, False), (4, True)}, seen


def test_geometry_keeps_the_chip_busy_and_ignores_the_share():
    import torch
    ctx = _ctx(0.5, True)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for P, N in ((64, 128400), (4096, 128400), (65536, 128400), (4096, 8100)):
        ni, ch, wb = ctx.velocity_field_info(P, N)
        units = -(-P // (64 * ni)) * ch
        assert units >= 2 * n_cu, (P, N, ni, ch)
    ctx.close()


def test_full_size_cfg3_against_apply_M():
    c, rb = _body(200, 642, True)
    r = rb.get_blob_positions().reshape(-1)
    lam = np.random.default_rng(10).standard_normal(r.size)
    a = c["a"]
    pts = _points_near(r, a, 4096, 0.5 * a, 10 * a, True, seed=11, zmin=0.5 * a)
    u = rb.velocity_field(pts, lam)
    F = np.concatenate([lam, np.zeros(pts.size)])
    U = rb.apply_M(F, np.concatenate([r, pts.reshape(-1)]))[r.size:]
    assert _rel(u.reshape(-1), U) <= 1e-12


@pytest.mark.parametrize("wall", [False, True])
def test_solved_body_no_slip_at_its_blobs(wall):
    from rigid_body_light_amd import RigidBody, load_structure
    params, cfg = load_structure(162)
    a = params["sep"] / 2.0
    Rb = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()) + a
    rb = RigidBody(cfg, np.array([[0.0, 0.0, Rb + a]]), np.array([[1.0, 0.0, 0.0, 0.0]]), a, 1.0, 0.01, wall_PC=wall)
    n3 = 3 * rb.total_blobs
    F = np.array([0.3, -0.2, -1.0, 0.1, 0.5, -0.2])
    x, its, res = rb.solve_saddle(np.concatenate([np.zeros(n3), -F]), max_iter=200, rtol=1e-10)
    lam, U = x[:n3], x[n3:]
    u = rb.velocity_field(rb.get_blob_positions(), lam)
    KU = rb.K_dot(U)
    assert _rel(u.reshape(-1), KU.reshape(-1)) <= 1e-8


def test_far_field_is_the_stokeslet_of_the_total_force():
    from rigid_body_light_amd import RigidBody, load_structure
    params, cfg = load_structure(162)
    a = params["sep"] / 2.0
    rb = RigidBody(cfg, np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]]), a, 1.0, 0.01)
    n3 = 3 * rb.total_blobs
    F = np.array([0.3, -0.2, -1.0, 0.0, 0.0, 0.0])          # (a torque's rotlet would add O(T / (F r)) to the far field)
    x, _, _ = rb.solve_saddle(np.concatenate([np.zeros(n3), -F]), max_iter=200, rtol=1e-10)
    lam = x[:n3]
    f = lam.reshape(-1, 3).sum(axis=0)
    dirs = np.random.default_rng(12).standard_normal((8, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rr = 1e4 * a
    u = rb.velocity_field(rr * dirs, lam)
    for d, ud in zip(dirs, u):
        st = (f + d * (d @ f)) / (8 * np.pi * 1.0 * rr)
        assert np.linalg.norm(ud - st) <= 1e-3 * np.linalg.norm(st)


def test_reproducible_poison_dev_and_own_positions_bitwise():
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    from rigid_body_light_amd import make_config
    for wall in (False, True):
        c = make_config(50, 162, wall)
        lam = np.random.default_rng(13).standard_normal(3 * 50 * 162)
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        dev = torch.device("cuda:0")

        class _View:                                                   # the context's resident positions, no copy
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}
        p_ptr, n = ctx.positions_ptr()
        torch.cuda.synchronize()
        r = torch.as_tensor(_View(p_ptr, 3 * n), device=dev).clone()
        r_host = r.cpu().numpy()
        pts = _points_near(r_host, c["a"], 3001, 0.3 * c["a"], 20 * c["a"], wall, seed=14)
        u1 = ctx.velocity_field(pts, lam, r_host)
        u2 = ctx.velocity_field(pts, lam, r_host)
        u_own = ctx.velocity_field(pts, lam)                           # r_vecs = NULL: the context's own blobs
        assert np.array_equal(u1, u2) and np.array_equal(u1, u_own)
        d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
        d_lam = torch.from_numpy(lam).to(dev)
        d_u = torch.full((pts.size,), float("nan"), dtype=torch.float64, device=dev)
        ctx.velocity_field_dev(d_pts.data_ptr(), pts.shape[0], d_lam.data_ptr(), r.data_ptr(), n, d_u.data_ptr())
        ctx.sync_check()
        assert np.array_equal(d_u.cpu().numpy(), u1)
        ctx.velocity_field_dev(d_pts.data_ptr(), pts.shape[0], d_lam.data_ptr(), None, n, d_u.data_ptr())
        ctx.sync_check()
        assert np.array_equal(d_u.cpu().numpy(), u1)
        ctx.set_option("poison_workspace", 1)
        u_p = ctx.velocity_field(pts, lam, r_host)
        ctx.velocity_field_dev(d_pts.data_ptr(), pts.shape[0], d_lam.data_ptr(), r.data_ptr(), n, d_u.data_ptr())
        ctx.sync_check()
        assert np.array_equal(u_p, u1) and np.array_equal(d_u.cpu().numpy(), u1)
        ctx.close()


def test_no_damp_is_honoured(orc):
    """rbl_set_no_damp: the plain wall-corrected M, as apply_M applies it then (points in the damped layer z < a)"""
    import ctypes
    from rigid_body_light_amd._lib import lib
    c, rb = _body(10, 12, True)
    r = rb.get_blob_positions().reshape(-1)
    lam = np.random.default_rng(15).standard_normal(r.size)
    a = c["a"]
    pts = _points_near(r, a, 200, 0.3 * a, 3 * a, True, seed=16)
    pts[:, 2] = np.minimum(pts[:, 2], 0.9 * a)
    F = np.concatenate([lam, np.zeros(pts.size)])
    h = ctypes.c_void_p(rb.cb.handle())
    u_d = rb.velocity_field(pts, lam)
    lib().rbl_set_no_damp(h, 1)
    try:
        u_n = rb.velocity_field(pts, lam)
        U_n = rb.apply_M(F, np.concatenate([r, pts.reshape(-1)]))[r.size:]
    finally:
        lib().rbl_set_no_damp(h, 0)
    assert _rel(u_n.reshape(-1), U_n) <= 1e-12
    assert _rel(u_d, u_n) > 1e-3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_over_three_gloo_ranks_is_bitwise_the_single_rank_result():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "tools/check_velocity_field_comm.py"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout and "world 3" in p.stdout


def test_world1_rccl_communicator_is_bitwise_the_single_rank_result():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RBL_VF_NCCL="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "tools/check_velocity_field_comm.py"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout and "RCCL in librbl" in p.stdout


def test_flow_field_example(tmp_path):
    out = str(tmp_path / "ff.npz")
    p = subprocess.run([sys.executable, "examples/flow_field.py", "--nx", "32", "--nz", "16", "--out", out], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    z = np.load(out)
    a = float(z["a"])
    assert abs(z["z"][0] - 0.01 * a) <= 1e-12 * a and abs(d["wall_row_z"] - 0.01 * a) <= 1e-12 * a
    assert z["u"].shape == (16, 32, 3) and np.all(np.isfinite(z["u"]))
    assert d["max_speed"] > 0.0 and d["wall_row_max_speed"] < 1e-2 * d["max_speed"]
    assert d["blob_residual"] <= 1e-8
