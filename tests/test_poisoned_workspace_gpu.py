"""Unwritten device memory (RBL_OPT_POISON_WORKSPACE): every family of kernels runs the same seeded inputs through a fresh
context with its workspaces poisoned -- every allocation, and every scratch workspace at every reserve, filled with a pattern
that reads as NaN in fp64 and fp32 and as a large positive int32 -- and through one without.  Both must give the same status,
the same iteration counts and BITWISE the same outputs: the library's sums run in fixed orders (LDS ds_add_f64 with one lane
per address, work-queue units writing their own slabs, ordered reductions), so the only way the two runs can differ is a read
of a slot nobody wrote.  Output tensors handed to the _dev entry points are NaN beforehand, so a kernel that skips part of its
output (a ragged tail) fails too.  Systems are small except the one cfg-3 product."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, ETA = 0.3, 1.0
MODEL = dict(w=0.2, eps_wall=1.0, b_wall=0.1, eps_blob=1.0, b_blob=0.1)


@contextlib.contextmanager
def _poison_env(poison):
    keep = os.environ.get("RBL_POISON_WORKSPACE")
    os.environ["RBL_POISON_WORKSPACE"] = "1" if poison else "0"
    try:
        yield
    finally:
        if keep is None:
            os.environ.pop("RBL_POISON_WORKSPACE", None)
        else:
            os.environ["RBL_POISON_WORKSPACE"] = keep


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ctx(poison, wall, cfg=None, a=A, dt=0.0, opts=()):
    from rigid_body_light_amd._lib import DeviceContext
    with _poison_env(poison):
        ctx = DeviceContext(a, ETA, wall, cfg=cfg, dt=dt, stream_ptr=_stream())
    assert ctx.get_option("poison_workspace") == int(poison)
    for k, v in opts:
        ctx.set_option(k, v)
    return ctx


def _body(poison, cfg, X, Q, a, wall, block, dt=0.01, opts=()):
    from rigid_body_light_amd import RigidBody
    with _poison_env(poison):
        rb = RigidBody(cfg, X, Q, a, ETA, dt, wall_PC=wall, block_PC=block)
    assert rb.cb.get_option("poison_workspace") == int(poison)
    for k, v in opts:
        rb.cb.set_option(k, v)
    return rb


def _nan(shape):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=torch.float64, device="cuda:0")


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0")


def _cloud(N, wall, seed, a=A):
    """N blobs on a jittered cubic lattice (spacing 2.2 a), above the wall when there is one"""
    side = int(np.ceil(N ** (1.0 / 3.0) - 1e-9))
    idx = np.arange(N)
    r = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1) * (2.2 * a)
    r = r + np.random.default_rng(seed).uniform(-0.05 * a, 0.05 * a, r.shape)
    if wall:
        r[:, 2] += 1.5 * a
    return r


def _lattice_body(nblb, a=A):
    """a body of nblb blobs (any count, for awkward factor sizes): a lattice block, mean removed"""
    cfg = _cloud(nblb, False, 0, a)
    return cfg - cfg.mean(axis=0)


def _same(x, y, what):
    if isinstance(x, (int, float, str, bool, type(None))):
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (what, x, y)
        return
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
    assert x.tobytes() == y.tobytes(), (what, "differs bitwise in %d of %d entries" % (int(np.sum(x != y)), x.size))


def _run(fn, poison):
    try:
        return {"status": "ok", **fn(poison)}
    except RuntimeError as e:                     # (RblError): the library's status and message
        return {"status": str(e)}


def _twice(fn, must_succeed=True):
    """fn(poison) -> {name: output}: the clean run, then the poisoned one; same status, bitwise the same outputs"""
    clean = _run(fn, False)
    poisoned = _run(fn, True)
    if must_succeed:
        assert clean["status"] == "ok", clean["status"]
    assert clean.keys() == poisoned.keys(), (clean["status"], poisoned["status"])
    for k in clean:
        _same(clean[k], poisoned[k], k)
        if k != "status" and must_succeed:
            v = np.asarray(clean[k])
            assert v.dtype.kind != "f" or np.all(np.isfinite(v)), k
    return clean


# ---- products ---------------------------------------------------------------------------------------------------------------
def _product(N, wall, opts, nrhs=0, seed=1):
    def fn(poison):
        ctx = _ctx(poison, wall, opts=opts)
        r = _dev(_cloud(N, wall, seed).reshape(-1))
        rng = np.random.default_rng(seed)
        if nrhs:
            F = _dev(rng.standard_normal(3 * N * nrhs))
            out = _nan(3 * N * nrhs)
            ctx.apply_M_multi(F.data_ptr(), r.data_ptr(), N, nrhs, out.data_ptr())
        else:
            F = _dev(rng.standard_normal(3 * N))
            out = _nan(3 * N)
            ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, out.data_ptr())
        ctx.sync_check()
        ctx.close()
        return {"U": out.cpu().numpy()}
    return fn


# rows per lane, waves per workgroup, work queue, wave units: every shape kSymRows (rbl_kernels.hip) has a kernel for; one wave runs as
# wave-owned units (k_apply_M_symw) or, with sym_wave_units = 0, as one unit per workgroup (k_apply_M_sym<., 1 or 2, 1>)
SYM_SHAPES = [(1, 1, 1, 1), (2, 1, 1, 1), (1, 1, 1, 0), (2, 1, 1, 0), (2, 4, 1, 1), (2, 4, 0, 1), (4, 4, 1, 1), (4, 4, 0, 1)]


@pytest.mark.parametrize("N", [1, 63, 65, 257, 1500])
@pytest.mark.parametrize("rows,waves,queue,wave_units", SYM_SHAPES)
def test_symmetric_product(N, rows, waves, queue, wave_units):
    opts = (("matvec_kernel", 2), ("sym_rows_per_lane", rows), ("sym_waves", waves), ("sym_work_queue", queue),
            ("sym_wave_units", wave_units))
    _twice(_product(N, True, opts))


@pytest.mark.parametrize("N,wall", [(1, True), (63, False), (65, True), (257, False), (257, True)])
def test_default_ordered_relaxed_and_two_vector_products(N, wall):
    _twice(_product(N, wall, ()))
    _twice(_product(N, wall, (("matvec_kernel", 1),)))
    _twice(_product(N, wall, (("relaxed_always", 1),)))
    _twice(_product(N, wall, (), nrhs=2))


@pytest.mark.parametrize("nrhs", [1, 3, 4, 15, 16, 17, 19])
@pytest.mark.parametrize("N", [65, 257])
def test_mfma_multi_vector_product(nrhs, N):
    _twice(_product(N, True, (("matvec_kernel", 3),), nrhs=nrhs))


def test_cfg3_product_four_rows_per_lane():
    """the one large case: cfg 3 (200 bodies x 642 blobs), where four rows per lane and the work queue are the heuristic's choice"""
    from rigid_body_light_amd import make_config
    c = make_config(200, 642, True)

    def fn(poison):
        ctx = _ctx(poison, True, cfg=c["cfg"], a=c["a"])
        assert ctx.apply_M_sym_info(200 * 642, 1, 1)[0] == 4
        ctx.set_config(c["X"], c["Q"])
        N = 200 * 642
        r = _nan(3 * N)
        ctx.blob_positions(0, 200, r.data_ptr())
        F = _dev(np.random.default_rng(3).standard_normal(3 * N))
        out = _nan(3 * N)
        ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, out.data_ptr())
        ctx.sync_check()
        ctx.close()
        return {"U": out.cpu().numpy()}
    _twice(fn)


# ---- dense: build, Cholesky at odd n, M^1/2 W -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n", [(11, 33), (86, 257)])
def test_dense_build_and_cholesky(N, n):
    def fn(poison):
        ctx = _ctx(poison, True)
        r = _dev(_cloud(N, True, 5).reshape(-1))
        M = _nan((3 * N, 3 * N))
        ctx.build_M(r.data_ptr(), N, 1, M.data_ptr())
        L = M[:n, :n].contiguous()
        ctx.cholesky(L.data_ptr(), n, zero_upper=True)
        ctx.sync_check()
        ctx.close()
        return {"M": M.cpu().numpy(), "L": L.cpu().numpy()}
    _twice(fn)


def _roots_body(poison, wall, opts=()):
    from rigid_body_light_amd import make_config
    c = make_config(6, 42, wall)
    return _body(poison, c["cfg"], c["X"], c["Q"], c["a"], wall, True, opts=opts)


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("method,two_level", [("cholesky", 1), ("lanczos", 1), ("lanczos_pc", 0), ("lanczos_pc", 1)])
def test_square_roots(wall, method, two_level):
    """M^1/2 W: dense Cholesky, plain Lanczos, preconditioned Lanczos with the block-Jacobi and the two-level factor"""
    def fn(poison):
        rb = _roots_body(poison, wall, (("lanczos_two_level", two_level),))
        W = np.random.default_rng(7).standard_normal(3 * 6 * 42)
        out = {"y": np.asarray(rb.M_half_W(W, method=method)), "y_seeded": np.asarray(rb.M_half_W(None, seed=4, method=method))}
        if method != "cholesky":
            out["report"] = np.asarray(rb.cb.lanczos_report(), dtype=np.float64)
        return out
    _twice(fn)


# ---- block preconditioner -----------------------------------------------------------------------------------------------------
def _pc(nb, cfg, wall, opts, seed=9, a=A, spacing=None):
    from rigid_body_light_amd import make_config
    if cfg is None:
        c = make_config(nb, 42, wall)
        cfg, X, Q, a = c["cfg"], c["X"], c["Q"], c["a"]
    else:
        ext = np.ptp(cfg, axis=0).max() + 4 * a
        X = np.stack([np.arange(nb) * ext, np.zeros(nb), np.zeros(nb)], axis=1)
        if wall:
            X[:, 2] += -cfg[:, 2].min() + 1.5 * a
        Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    nblb = cfg.shape[0]

    def fn(poison):
        rb = _body(poison, cfg, X, Q, a, wall, True, opts=opts)
        rng = np.random.default_rng(seed)
        b = rng.standard_normal(3 * nb * nblb + 6 * nb)
        out = {"x": np.asarray(rb.apply_PC(b))}
        rb.set_config(X + 0.01 * rng.standard_normal(X.shape), Q)          # new configuration: factors rebuilt
        out["x2"] = np.asarray(rb.apply_PC(b))
        xs, its, res = rb.solve_saddle(b, max_iter=60, rtol=1e-9)
        out.update(xs=np.asarray(xs), its=int(its), res=float(res))
        return out
    return fn


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("opts", [(), (("block_explicit_small", 0),), (("bodyframe_factor", 0),), (("shared_gemm", 0),)],
                         ids=["default", "no_explicit", "per_config", "no_gemm"])
def test_block_pc_small_bodies(wall, opts):
    _twice(_pc(4, None, wall, opts))


def test_block_pc_body_frame_wall_approximation():
    _twice(_pc(4, None, True, (("bodyframe_wall_approx", 1),)))


@pytest.mark.parametrize("nblb", [171, 213, 427])
@pytest.mark.parametrize("opts", [(), (("block_explicit_large", 1),), (("block_explicit_large", 0), ("block_solve_pipe", 1)),
                                  (("block_explicit_large", 0), ("block_solve_pipe", 0)), (("block_explicit_large", 1), ("block_inverse_f32", 1)),
                                  (("block_tile_factor", 0),), (("block_tile_factor", 0), ("block_explicit_large", 1))],
                         ids=["default", "explicit", "pipe", "no_pipe", "f32", "panel", "panel_explicit"])
def test_block_pc_large_bodies(nblb, opts):
    """3 N_blb > 512: the dataflow tile factor at awkward sizes, explicit inverses, pipelined substitution, fp32 inverses.  427 blobs
    (n = 1281 = 10 x 128 + 1, odd): the tile kernel's inverse tasks read one row past the last row of L, which lies above the
    diagonal of L's next column -- not built when only the lower tiles are, i.e. NaN here -- so those columns of T must be zeroed"""
    _twice(_pc(3, _lattice_body(nblb), True, opts))


# ---- solvers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [(), (("gmres_one_kernel", 0),), (("gmres_one_kernel", 0), ("gmres_predict_checks", 0)),
                                  (("gmres_one_kernel", 0), ("gmres_overlap_check", 0)), (("gmres_one_kernel", 0), ("fused_krylov", 0))],
                         ids=["one_kernel", "general", "no_predict", "no_overlap", "unfused"])
@pytest.mark.parametrize("block", [False, True])
def test_gmres(opts, block):
    from rigid_body_light_amd import make_config
    c = make_config(8, 12, True)

    def fn(poison):
        rb = _body(poison, c["cfg"], c["X"], c["Q"], c["a"], True, block, opts=opts)
        rng = np.random.default_rng(13)
        out = {}
        for i, (mi, rt) in enumerate(((100, 1e-10), (7, 0.0), (100, 1e-10))):
            b = rng.standard_normal(3 * 8 * 12 + 48)
            x, its, res = rb.solve_saddle(b, max_iter=mi, rtol=rt)
            out.update({"x%d" % i: np.asarray(x), "its%d" % i: int(its), "res%d" % i: float(res)})
        return out
    _twice(fn)


@pytest.mark.parametrize("block", [False, True])
def test_lock_step_gmres(block):
    from rigid_body_light_amd import make_config
    c = make_config(6, 42, True)
    nsys = 3 * 6 * 42 + 36

    def fn(poison):
        rb = _body(poison, c["cfg"], c["X"], c["Q"], c["a"], True, block)
        rng = np.random.default_rng(17)
        rhs = rng.standard_normal((19, nsys))
        rhs[0] = 0.0
        rhs[1] = 0.0
        rhs[1, :nsys - 36] = rb.K_dot(rng.standard_normal(36)).reshape(-1)     # converges at iteration 1
        rhs[5] *= 1e-6
        x, its, res = rb.solve_saddle_multi(rhs, max_iter=100, rtol=1e-10)
        x17, its17, res17 = rb.solve_saddle_multi(rhs[:17], max_iter=100, rtol=1e-10)
        xf, itf, resf = rb.solve_saddle_multi(rhs[2:7], max_iter=9, rtol=0.0)
        return dict(x=x, its=its, res=res, x17=x17, its17=its17, res17=res17, xf=xf, itf=itf, resf=resf)
    out = _twice(fn)
    assert int(out["its"][1]) == 1 and int(out["its"][0]) <= 1 and not np.any(out["x"][0])


@pytest.mark.parametrize("warm", [0, 1, 2, 3])
@pytest.mark.parametrize("block", [False, True])
def test_deterministic_steps_with_warm_and_extrapolated_starts(warm, block):
    from rigid_body_light_amd import make_config
    c = make_config(6, 42, True)

    def fn(poison):
        rb = _body(poison, c["cfg"], c["X"], c["Q"], c["a"], True, block, opts=(("gmres_one_kernel", 0),))
        F = np.random.default_rng(19).standard_normal(36)
        out = {}
        for s in range(5):
            its, res = rb.step_deterministic(F, max_iter=60, rtol=1e-9, warm_start=warm)
            X, Q = rb.get_config()
            out.update({"its%d" % s: int(its), "res%d" % s: float(res), "X%d" % s: np.asarray(X), "Q%d" % s: np.asarray(Q)})
        return out
    _twice(fn)


# ---- whole steps, with and without the force model ----------------------------------------------------------------------------
@pytest.mark.parametrize("forces", [False, True])
@pytest.mark.parametrize("kind", ["deterministic", "brownian"])
@pytest.mark.parametrize("block", [False, True])
def test_steps(forces, kind, block):
    from rigid_body_light_amd import make_config
    c = make_config(8, 42, True)

    def fn(poison):
        rb = _body(poison, c["cfg"], c["X"], c["Q"], c["a"], True, block)
        if forces:
            rb.set_interactions(**MODEL)
        F = np.random.default_rng(23).standard_normal(48) * 0.1
        out = {}
        for s in range(3):
            if kind == "deterministic":
                its, res = rb.step_deterministic(F, max_iter=60, rtol=1e-9)
            else:
                its, res = rb.step_brownian(F, seed=31 + s, max_iter=60, rtol=1e-9)
            X, Q = rb.get_config()
            out.update({"its%d" % s: int(its), "res%d" % s: float(res), "X%d" % s: np.asarray(X), "Q%d" % s: np.asarray(Q)})
        if forces:
            out["ft"] = np.asarray(rb.interaction_forces())
        return out
    _twice(fn)


# ---- ensembles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 37])
@pytest.mark.parametrize("kind", ["deterministic", "brownian"])
def test_ensembles_with_forces(R, kind):
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    a = p["sep"] / 2.0
    nb = 3
    rng = np.random.default_rng(41)
    X = np.zeros((R, nb, 3))
    for r in range(R):
        X[r] = np.stack([np.arange(nb) * 4.0, np.zeros(nb), np.full(nb, 2.0)], axis=1) + rng.uniform(-0.3, 0.3, (nb, 3))
    Q = rng.standard_normal((R, nb, 4))
    Q /= np.linalg.norm(Q, axis=2, keepdims=True)
    F = rng.standard_normal((R, 6 * nb)) * 0.1

    def fn(poison):
        ctx = _ctx(poison, True, cfg=cfg, a=a, dt=0.01)
        ctx.ensemble_set_config(X, Q)
        ctx.set_interactions(**MODEL)
        out = {}
        for s in range(2):
            if kind == "deterministic":
                its, res = ctx.ensemble_step_deterministic(F, max_iter=60, rtol=1e-9)
            else:
                its, res = ctx.ensemble_step_brownian(F, seed=5 + s, max_iter=60, rtol=1e-9)
            Xs, Qs = ctx.ensemble_get_config()
            out.update({"its%d" % s: np.asarray(its), "res%d" % s: np.asarray(res), "X%d" % s: Xs, "Q%d" % s: Qs})
        fo = ctx.ensemble_interaction_forces()
        out["ft"], out["e"] = np.asarray(fo[0]), np.asarray(fo[1])
        ctx.close()
        return out
    _twice(fn)


# ---- one-rank communicator, staged all-gathers ---------------------------------------------------------------------------------
def test_world1_staged_allgather_poisoned():
    """d_commStage: the world-1 RCCL check (tools/check_nccl_world1.py, its own process: a communicator is per process), which
    runs both forms of the all-gather -- RBL_OPT_COMM_FORCE_STAGED on and off -- with every context poisoned.  Not bitwise
    against an unpoisoned run: the tool compares the sharded results with the un-sharded ones at its own tolerances, the same
    check tests/test_multirank_gpu.py makes without poisoning."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RBL_POISON_WORKSPACE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "tools/check_nccl_world1.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ALL OK" in p.stdout and "FAILED" not in p.stdout
