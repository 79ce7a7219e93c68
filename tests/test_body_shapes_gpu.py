"""Body kernels, the one-kernel solver and the ensembles at shapes other than 12 blobs per body, against the CPU oracle
(tests/body_shapes.py: the shapes, the dense reference, the condition numbers that tests/test_body_shapes_cpu.py measures).

Every context here is created with its workspaces poisoned (RBL_OPT_POISON_WORKSPACE) and every output tensor starts as NaN: a
row nobody writes fails instead of passing by luck.  References are the oracle's dense matrices: built once per configuration,
shared, read-only.

The bounds on solutions are 10 cond(A) rtol with cond(A) from body_shapes.COND_A (the residual of a solve is asserted on the
ORACLE's matrix, not on the GPU's operator: an operator wrong by delta leaves a residual of about delta).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import body_shapes as bs

pytestmark = pytest.mark.gpu
DT, KBT = 0.01, 0.02
F_BODY = [0.3, 0.0, -1.0, 0.0, 0.2, 0.0]


# ---------------------------------------------------------------------------------------------------------------- helpers
@contextlib.contextmanager
def _poison_env():
    keep = os.environ.get("RBL_POISON_WORKSPACE")
    os.environ["RBL_POISON_WORKSPACE"] = "1"
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


def _ctx(c, wall, block=False, opts=(), config=True):
    from rigid_body_light_amd._lib import DeviceContext, lib
    with _poison_env():
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=DT, kBT=KBT, stream_ptr=_stream())
    assert ctx.get_option("poison_workspace") == 1
    for k, v in opts:
        ctx.set_option(k, v)
    if block:
        assert lib().rbl_set_blk_pc(ctx.h, 1) == 0
    if config:
        ctx.set_config(c["X"], c["Q"])
    return ctx


def _dev(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda:0")


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")


def _rel(x, y):
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import Oracle
    return Oracle()


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _ref(name, wall, seed=0):
    """-> (case, cfg (mean removed), Qn, M, K, A) of a named configuration: built once, shared, read-only"""
    from oracle import oracle as onp
    c = bs.case(name, wall, seed)
    M, K, Am, _ = bs.dense(_oracle(), c["cfg"], c["X"], c["Q"], c["a"], c["eta"], wall)
    cfg, Qn = onp.remove_mean(c["cfg"]), onp.normalize_quats(c["Q"])
    _frozen(M, K, Am, cfg, Qn, c["X"], c["Q"], c["cfg"])
    return c, cfg, Qn, M, K, Am


def _rhs(c, seed=31):
    """a right-hand side of the shape the solver tests of test_gpu_parity.py use"""
    n3 = 3 * c["nb"] * c["nblb"]
    rng = np.random.default_rng(seed)
    return np.concatenate([0.3 * rng.standard_normal(n3), np.tile([0.1, 0, -1.0, 0.2, 0, 0.05], c["nb"])])


@functools.lru_cache(maxsize=None)
def _dense_solution(name, wall):
    c, _, _, _, _, Am = _ref(name, wall)
    b = _rhs(c)
    xs = np.linalg.solve(Am, b)
    return _frozen(b, xs)


def _solve(c, wall, b, block, opts, max_iter, rtol):
    ctx = _ctx(c, wall, block, opts)
    db, x = _dev(b), _nan(b.size)
    its, res = ctx.gmres_saddle(db.data_ptr(), max_iter, rtol, x.data_ptr())
    ctx.sync_check()
    ctx.close()
    return x.cpu().numpy(), its, res


def _assert_solves(tag, x, its, Am, b, xs, cond, rtol):
    """the two assertions of every solve: the residual on the oracle's matrix, and the distance to the dense solution"""
    r = float(np.linalg.norm(Am @ x - b) / np.linalg.norm(b))
    e = _rel(x, xs)
    print("%s: %3d iterations  |A x - b| / |b| %.2e (bound %.0e)  |x - x*| / |x*| %.2e (bound %.1e)" % (tag, its, r, 10 * rtol, e, 10 * cond * rtol))
    assert np.isfinite(x).all(), tag
    assert r <= 10 * rtol, tag
    assert e <= 10 * cond * rtol, tag
    return r, e


# ---------------------------------------------------------------------------------------------------------------- (a) operators
def _block_variants(name, wall):
    """option sets of the block preconditioner: in free space the body-frame factor on and off (k_pc_bodyframe and
    k_pc_block_tail are different kernels), and at G4-G7 the explicit small-body inverses both ways"""
    v = [()]
    if not wall:
        v.append((("bodyframe_factor", 0),))
    if name in ("G4", "G5", "G6", "G7"):
        v.append((("block_explicit_small", 0),))
        if not wall:
            v.append((("bodyframe_factor", 0), ("block_explicit_small", 0)))
    return v


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name", bs.G_CASES + bs.S_CASES + ["E1"])
def test_operators_vs_oracle(name, wall):
    """K U, K^T lambda, the diagonal and the block preconditioner (every option set of _block_variants) and the saddle product
    against K @ U, K.T @ lam, oracle.apply_PC and the dense saddle matrix, G1-G9 and S1-S5, free space and wall -- and E1, 49
    tetrahedra: fewer than 64 bodies with 3 N_blb even, the one shape here at which k_bf_gemv loads its table in pairs.

    Bounds (the project's existing ones, test_device_body_operators_vs_host_and_oracle): K U atol 1e-13; K^T lambda atol 1e-12
    times |lambda|_inf N_blb R_b -- the existing 1e-12 was set for a sum over 12 blobs at unit lever arm, here the sum has N_blb
    terms of size up to |lambda|_inf R_b --; preconditioners and saddle product 1e-12 relative.

    Measured worst over the 30 cases (one MI355X): K U 3.6e-15 absolute (G5); K^T lambda 9.9e-14 absolute against a bound of
    5.8e-9 there (G6), and 1.7e-4 of its bound at worst (S3: 8.9e-16 of 5.2e-12); diagonal preconditioner 1.2e-15 (S5, wall);
    block preconditioner 2.8e-15 over all 57 option sets (G8, free space, bodyframe_factor = 0); saddle product 4.2e-16 (G7)."""
    from oracle import oracle as onp
    c, cfg, Qn, M, K, Am = _ref(name, wall)
    nb, nblb = c["nb"], c["nblb"]
    n3, nb6 = 3 * nb * nblb, 6 * nb
    rng = np.random.default_rng(61)
    U, lam, x = rng.standard_normal(nb6), rng.standard_normal(n3), rng.standard_normal(n3 + nb6)
    dU, dl, dx = _dev(U), _dev(lam), _dev(x)
    ctx = _ctx(c, wall)
    o1, o2, o3, o4 = _nan(n3), _nan(nb6), _nan(n3 + nb6), _nan(n3 + nb6)
    ctx.K_x_U(dU.data_ptr(), o1.data_ptr())
    ctx.KT_x_Lam(dl.data_ptr(), o2.data_ptr())
    ctx.apply_PC(dx.data_ptr(), o3.data_ptr())
    ctx.apply_saddle(dx.data_ptr(), o4.data_ptr())
    ctx.sync_check()
    ctx.close()
    kt_atol = 1e-12 * np.abs(lam).max() * nblb * bs.radius(c["cfg"])
    e_ku = float(np.abs(o1.cpu().numpy() - K @ U).max())
    e_kt = float(np.abs(o2.cpu().numpy() - K.T @ lam).max())
    e_pc = _rel(o3.cpu().numpy(), onp.apply_PC(_oracle(), x, c["X"], Qn, cfg, c["a"], c["eta"], wall, False))
    e_sd = _rel(o4.cpu().numpy(), Am @ x)
    print("%s %s: K U %.2e (1e-13)  K^T lam %.2e (%.2e)  diagonal PC %.2e  saddle %.2e (1e-12)" % (name, wall, e_ku, e_kt, kt_atol, e_pc, e_sd))
    assert e_ku <= 1e-13 and e_kt <= kt_atol and e_pc <= 1e-12 and e_sd <= 1e-12
    ref_blk = onp.apply_PC(_oracle(), x, c["X"], Qn, cfg, c["a"], c["eta"], wall, True)
    for opts in _block_variants(name, wall):
        ctx = _ctx(c, wall, block=True, opts=opts)
        o5, o6 = _nan(n3 + nb6), _nan(n3 + nb6)
        ctx.apply_PC(dx.data_ptr(), o5.data_ptr())
        ctx.apply_saddle(dx.data_ptr(), o6.data_ptr())
        ctx.sync_check()
        ctx.close()
        e_blk, e_sd = _rel(o5.cpu().numpy(), ref_blk), _rel(o6.cpu().numpy(), Am @ x)
        print("%s %s: block PC %s %.2e  saddle %.2e (1e-12)" % (name, wall, dict(opts), e_blk, e_sd))
        assert e_blk <= 1e-12 and e_sd <= 1e-12, opts


# ---------------------------------------------------------------------------------------------------------------- (b) general solver
RTOL_B = 1e-10


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name", bs.G_CASES)
def test_general_solver_vs_dense_solve(name, wall):
    """gmres_saddle of the general (multi-launch) solver, rtol 1e-10, max_iter 200, with the block preconditioner under fused_krylov
    in {0, 1} x matvec_kernel in {0, 1} and with the diagonal preconditioner once; G1-G9.  G1-G3 with fused_krylov = 0 or
    matvec_kernel = 1 reach k_saddle_tail with more body rows (6 N_bod) than its grid has threads (256 ceil(N / 256)): before
    its loop over the body rows strode, rows 1024 .. 1799 (G1), 512 .. 599 (G2) and 512 .. 539 (G3) of every Arnoldi vector were
    never written, and these cases failed here with x = NaN.

    Asserted: |A x - b| / |b| <= 10 rtol on the oracle's A; |x - A^-1 b| / |A^-1 b| <= 10 cond(A) rtol; the iteration counts of
    the four block-preconditioner variants agree within 1.

    Measured worst over the 18 cases, 90 solves (one MI355X): residual 9.8e-11 (G2, wall; bound 1e-9); solution error 2.5e-10 (G2,
    diagonal preconditioner; bound 2.4e-7), 1.2e-3 of its bound at worst (G1, wall); the four block-preconditioner variants took the
    same number of iterations in every case (11 .. 23; G8, one body: 1).  With k_saddle_tail as it was, G1-G3 stop at the first
    variant (fused_krylov = 0) with `RblError: gmres: non-finite Hessenberg solve [rbl status 10]`."""
    c, cfg, Qn, M, K, Am = _ref(name, wall)
    b, xs = _dense_solution(name, wall)
    cond = bs.COND_A[(name, wall)]
    counts = []
    for fused in (0, 1):
        for mk in (0, 1):
            opts = (("gmres_one_kernel", 0), ("fused_krylov", fused), ("matvec_kernel", mk))
            x, its, res = _solve(c, wall, b, True, opts, 200, RTOL_B)
            _assert_solves("%s %s block fused=%d matvec_kernel=%d" % (name, wall, fused, mk), x, its, Am, b, xs, cond, RTOL_B)
            counts.append(its)
    assert max(counts) - min(counts) <= 1, counts
    x, its, res = _solve(c, wall, b, False, (("gmres_one_kernel", 0),), 200, RTOL_B)
    _assert_solves("%s %s diagonal" % (name, wall), x, its, Am, b, xs, cond, RTOL_B)


# ---------------------------------------------------------------------------------------------------------------- (c) one-kernel solver
def _fits(name, max_iter, mixed=False):
    return bs.small_fits(bs.shape(bs.CASES[name][0]).shape[0], bs.CASES[name][1], max_iter, mixed)


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name,max_iter", [(n, 255) for n in bs.S_CASES + bs.E_CASES + ["G9", "G7"]] + [("S3", 100)])
def test_one_kernel_solver_at_its_limits(name, wall, max_iter):
    """gmres_one_kernel = 1 requested at S1-S5 (the documented limits), at E1-E4 (the largest shapes of those families that the
    kernel's LDS takes) and at G9 and G7 (65 bodies; 514 blobs): the two assertions of the general-solver test against the dense
    solve, and the solution equals the general solver's to 1e-8.

    Which solver ran is read from the answer: where rbl_gmres_small_fits (restated as body_shapes.small_fits, pinned against the
    library on the CPU) says no, the call falls back to the general solver and must give the general solver's answer bit for bit,
    iteration count included; where it says yes the answers differ in rounding (the one kernel sums in other orders).  So this
    test also states the finding: S1 (64 x 4), S2 (1 x 256) and S4 (36 x 7) satisfy N <= 256, N_bod <= 64 and max_iter <= 255 and
    still do NOT run in the one kernel, at any iteration limit; S3 does at max_iter = 100 and does not at 255.

    Measured worst (one MI355X): residual 9.6e-11 (S2; bound 1e-9); solution error 2.4e-10, 1.4e-3 of its bound (E4); one kernel
    against general solver 1.0e-12 (E1, free space; bound 1e-8), and never 0 where the one kernel ran."""
    c, cfg, Qn, M, K, Am = _ref(name, wall)
    b, xs = _dense_solution(name, wall)
    cond = bs.COND_A[(name, wall)]
    xg, ig, rg = _solve(c, wall, b, False, (("gmres_one_kernel", 0),), max_iter, RTOL_B)
    xo, io, ro = _solve(c, wall, b, False, (("gmres_one_kernel", 1),), max_iter, RTOL_B)
    _assert_solves("%s %s m=%d general" % (name, wall, max_iter), xg, ig, Am, b, xs, cond, RTOL_B)
    _assert_solves("%s %s m=%d one-kernel requested" % (name, wall, max_iter), xo, io, Am, b, xs, cond, RTOL_B)
    d = _rel(xo, xg)
    same = np.array_equal(xo, xg) and io == ig
    print("%s %s m=%d: fits %s  bitwise the general solver's %s  |x_one - x_gen| / |x_gen| %.2e (1e-8)" % (name, wall, max_iter, _fits(name, max_iter), same, d))
    assert d <= 1e-8
    assert same == (not _fits(name, max_iter))


def test_more_than_255_iterations_are_refused_by_both_solvers():
    """max_iter = 256 at S1: the one-kernel solver does not take it (rbl_gmres_small_fits: max_iter <= 255), the call goes on to
    the general solver -- whose Arnoldi kernels hold 256 basis vectors and which refuses it as an argument error, before any launch
    of the iteration.  There is no answer to compare: both settings of the option end in the same refusal."""
    from rigid_body_light_amd._lib import RblError
    c = _ref("S1", True)[0]
    b = _dev(_rhs(c))
    for one in (0, 1):
        ctx = _ctx(c, True, opts=(("gmres_one_kernel", one),))
        x = _nan(b.numel())
        with pytest.raises(RblError, match="at most 255 iterations"):
            ctx.gmres_saddle(b.data_ptr(), 256, RTOL_B, x.data_ptr())
        its, res = ctx.gmres_saddle(b.data_ptr(), 255, RTOL_B, x.data_ptr())     # the context is still good
        ctx.sync_check()
        ctx.close()
        assert 0 < its < 255 and res < RTOL_B


def _mixed_inputs(nb, nblb, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nb, 6)), rng.standard_normal((nb, 6)), 0.1 * rng.standard_normal(3 * nb * nblb)


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name", ["S1", "S3", "E4"])
def test_masked_solve_vs_dense(name, wall):
    """solve_mixed with every other body held or driven, against _dense_mixed of tests/test_prescribed_gpu.py with what that test
    asserts (1e-7 on lambda, U and F at rtol 1e-10; prescribed velocities and free loads echoed exactly).

    Measured worst (one MI355X): lambda 2.8e-10 (S3, wall), U 4.0e-11, F 7.4e-11; 40 .. 52 iterations."""
    from test_prescribed_gpu import _body_in, _dense_mixed
    c, cfg, Qn, M, K, Am = _ref(name, wall)
    nb, nblb = c["nb"], c["nblb"]
    p = np.arange(nb) % 2 == 1
    F, Up, slip = _mixed_inputs(nb, nblb, 11)
    ctx = _ctx(c, wall)
    lam, U, Fo, its, res = ctx.solve_mixed(p.astype(np.uint8), _body_in(p, F, Up), max_iter=200, rtol=1e-10, slip=slip)
    ctx.close()
    lam_d, U_d, F_d = _dense_mixed(M, K, p, F, Up, slip)
    print("%s %s masked: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e F %.2e (1e-7)"
          % (name, wall, its, res, _rel(lam, lam_d), _rel(U, U_d), _rel(Fo, F_d)))
    assert 0 < its < 200 and res < 1e-10
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(Fo, F_d) <= 1e-7
    assert np.array_equal(U.reshape(nb, 6)[p], Up[p]) and np.array_equal(Fo.reshape(nb, 6)[~p], F[~p])


# ---------------------------------------------------------------------------------------------------------------- (d) ensembles
RTOL_E = 1e-12


def _replicas(ens, wall):
    name = bs.ensemble_case(ens)
    R, m = bs.ENSEMBLES[ens]
    refs = [_ref(name, wall, bs.replica_seed(r)) for r in range(R)]
    X = np.stack([rf[0]["X"] for rf in refs])
    Q = np.stack([rf[0]["Q"] for rf in refs])
    return name, R, m, refs, X, Q


def _oracle_step(c, cfg, Qn, wall, F, slip, W, split_rand, Am=None):
    """the step assembled from the oracle's dense matrices (test_brownian_step_vs_dense_numpy's chain): oracle.RHS_and_Midpoint,
    dense solve at the midpoint, oracle.evolve from q^n.  W = None: the deterministic step (solve at q^n).  -> X, Q"""
    from oracle import oracle as onp
    n3 = 3 * c["nb"] * c["nblb"]
    if W is None:
        rhs = np.concatenate([slip, -F])
    else:
        rhs, Xh, Qh = onp.RHS_and_Midpoint(_oracle(), slip, F, W[:n3], W[n3:2 * n3], W[2 * n3:], c["X"], Qn, cfg, c["a"], c["eta"], wall,
                                           DT, KBT, split_rand)
        Am = bs.dense(_oracle(), cfg, Xh, Qh, c["a"], c["eta"], wall)[2]
    U = np.linalg.solve(Am, rhs)[n3:]
    return onp.evolve(c["X"], Qn, U, DT)


def _assert_displacement(tag, Xg, Qg, Xr, Qr, X0, Q0, cond, rtol):
    """q^{n+1} - q^n against the reference's: 10 cond(A) rtol relative, plus 1e-12 absolute on the quaternions"""
    bound = 10 * cond * rtol
    dXg, dXr = Xg.reshape(-1) - X0.reshape(-1), Xr.reshape(-1) - X0.reshape(-1)
    dQg, dQr = Qg.reshape(-1) - Q0.reshape(-1), Qr.reshape(-1) - Q0.reshape(-1)
    ex = float(np.linalg.norm(dXg - dXr) / np.linalg.norm(dXr))
    eq = float(np.linalg.norm(dQg - dQr))
    assert np.isfinite(Xg).all() and np.isfinite(Qg).all(), tag
    assert np.linalg.norm(dXr) > 1e-5, tag                                        # the bodies did move
    ok = ex <= bound and eq <= bound * np.linalg.norm(dQr) + 1e-12
    return ex / bound, eq / (bound * np.linalg.norm(dQr) + 1e-12), ok


def _ensemble_inputs(R, nb, nblb, seed):
    rng = np.random.default_rng(seed)
    n3 = 3 * nb * nblb
    F = np.tile(F_BODY, (R, nb)) + 0.1 * rng.standard_normal((R, 6 * nb))
    return F, 0.1 * rng.standard_normal((R, n3)), rng.standard_normal((R, 3 * n3))


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("ens", list(bs.ENSEMBLES))
def test_ensemble_steps_vs_oracle_chain(ens, wall):
    """One ensemble_step_deterministic and one ensemble_step_brownian (injected noise W, split_rand both ways) of replicas with
    DISTINCT configurations, solved to rtol 1e-12, against the oracle chain replica by replica -- not against the single-context
    step.  q^{n+1} - q^n agrees with the reference's to 10 cond(A) rtol relative, plus 1e-12 absolute on the quaternions.

    S1 (5 replicas), S2 (3) and S4 (3) sit at the documented limits; the library refuses them (RBL_ERR_SIZE from the host-side check of
    rbl_ensemble_set_config, nothing launched, no ensemble left behind): they do not fit the one-kernel solver's LDS, whatever the
    documented limits say.  That refusal is what is asserted for them; the comparison runs on S3 (2 replicas, and 5: R N_bod = 320
    crosses the 256-thread per-body kernels), S5 (300 replicas) and E1-E4, the largest shapes of those families that fit.

    Measured worst (one MI355X), as a fraction of the bound: deterministic 1.8e-3 (positions; S3, wall), 8.1e-4 (quaternions);
    Brownian 1.1e-3 (positions; S3, wall), 4.1e-4 (quaternions).  The tightest bound is S5's, 6.3e-10."""
    from rigid_body_light_amd._lib import RblError
    name, R, m, refs, X, Q = _replicas(ens, wall)
    c = refs[0][0]
    nb, nblb = c["nb"], c["nblb"]
    ctx = _ctx(c, wall, config=False)
    if not _fits(name, 1):
        with pytest.raises(RblError, match="one-kernel solver") as e:
            ctx.ensemble_set_config(X, Q)
        assert "[rbl status 4]" in str(e.value) and ctx.ensemble_info() == (0, 0)
        ctx.close()
        return
    cond = bs.COND_A[(name, wall)]
    F, slip, W = _ensemble_inputs(R, nb, nblb, 17)
    worst = {}
    for kind in ("deterministic", "brownian split", "brownian"):
        ctx.ensemble_set_config(X, Q)
        if kind == "deterministic":
            its, res = ctx.ensemble_step_deterministic(F, max_iter=m, rtol=RTOL_E, slip=slip)
        else:
            its, res = ctx.ensemble_step_brownian(F, W=W, split_rand=kind == "brownian split", max_iter=m, rtol=RTOL_E, slip=slip)
        Xg, Qg = ctx.ensemble_get_config()
        wx = wq = 0.0
        good = True
        for r in range(R):
            cr, cfg, Qn, M, K, Am = refs[r]
            Xr, Qr = _oracle_step(cr, cfg, Qn, wall, F[r], slip[r], None if kind == "deterministic" else W[r], kind == "brownian split", Am)
            fx, fq, ok = _assert_displacement("%s replica %d" % (kind, r), Xg[r], Qg[r], Xr, Qr, cr["X"], Qn, cond, RTOL_E)
            wx, wq, good = max(wx, fx), max(wq, fq), good and ok
        worst[kind] = (wx, wq)
        print("%s %s %s: R = %d, iterations %d .. %d, residual estimate <= %.1e; displacement error / bound: X %.2e  Q %.2e (bound %.1e)"
              % (ens, wall, kind, R, its.min(), its.max(), res.max(), wx, wq, 10 * cond * RTOL_E))
        assert good, (kind, wx, wq)
    ctx.close()


@pytest.mark.parametrize("shape_name,nb", [("trimer", 65), ("fib257", 1), ("tetra", 64), ("fib256", 1)])
def test_ensembles_beyond_the_solver_are_refused_and_leave_no_state(shape_name, nb):
    """65 trimers and one body of 257 blobs are beyond the documented limits, 64 tetrahedra and one body of 256 blobs beyond the LDS
    bound: all RBL_ERR_SIZE from rbl_ensemble_set_config's first checks -- rbl_gmres_small_fits on the host, before rbl_dev_init,
    any allocation or any launch -- and the context holds no ensemble afterwards, also when it held one before."""
    from rigid_body_light_amd._lib import RblError
    cfg = bs.shape(shape_name)
    c = {"cfg": cfg, "a": bs.A, "eta": bs.ETA}
    ctx = _ctx(c, True, config=False)
    X, Q = bs.lattice(nb, cfg, True)
    with pytest.raises(RblError, match="one-kernel solver") as e:
        ctx.ensemble_set_config(X[None], Q[None])
    assert "[rbl status 4]" in str(e.value)
    assert ctx.ensemble_info() == (0, 0)
    with pytest.raises(RblError):
        ctx.ensemble_get_config()
    # an ensemble that was there before the refused call is still there, untouched
    X1, Q1 = bs.lattice(1, cfg, True, seed=4)
    if bs.small_fits(cfg.shape[0], 1, 1):
        ctx.ensemble_set_config(X1[None], Q1[None])
        with pytest.raises(RblError):
            ctx.ensemble_set_config(X[None], Q[None])
        assert ctx.ensemble_info() == (1, 1)
        assert np.array_equal(ctx.ensemble_get_config()[0], X1[None])
    ctx.close()


def test_iteration_limits_at_which_64_trimers_do_not_fit_are_refused_per_step():
    """S3 fits the one-kernel solver at max_iter <= 38 and 65 .. 189 only: the ensemble is accepted, a step at the default
    max_iter = 50 is RBL_ERR_SIZE (host-side, ens_check_solver), the configuration stays, and the step at max_iter = 100 runs"""
    from rigid_body_light_amd._lib import RblError
    name, R, m, refs, X, Q = _replicas("S3", True)
    c = refs[0][0]
    ctx = _ctx(c, True, config=False)
    ctx.ensemble_set_config(X, Q)
    F = np.tile(F_BODY, c["nb"])
    for bad in (50, 255):
        with pytest.raises(RblError, match="beyond the one-kernel solver"):
            ctx.ensemble_step_deterministic(F, max_iter=bad, rtol=1e-8)
        assert np.array_equal(ctx.ensemble_get_config()[0], X)
    its, res = ctx.ensemble_step_deterministic(F, max_iter=100, rtol=1e-8)
    assert (its < 100).all() and (res < 1e-8).all()
    assert not np.array_equal(ctx.ensemble_get_config()[0], X)
    ctx.close()


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("ens", ["S3x5", "E4"])
def test_ensemble_masked_solve_vs_dense(ens, wall):
    """ensemble solve_mixed with a DIFFERENT mask per replica against _dense_mixed, replica by replica, with what
    tests/test_prescribed_gpu.py asserts of a masked solve (1e-7 at rtol 1e-10, echoes exact).  The shape meant for this is 5
    replicas of S1, which no ensemble takes; S3x5 is 5 replicas of 64 trimers, E4 (51 tetrahedra, max_iter = 100) the shape just
    inside the masked solver's own limit: 52 tetrahedra fit neither form at max_iter = 100, and the mask costs 6 N_bod doubles
    of LDS that put 49 tetrahedra outside the masked form at max_iter = 255 where the unmasked one takes them.

    Measured worst (one MI355X): lambda 3.9e-10 (E4, free space, 42 of 51 bodies prescribed), U 5.0e-11, F 6.2e-11; at most 54
    iterations."""
    from test_prescribed_gpu import _body_in, _dense_mixed
    name, R, m, refs, X, Q = _replicas(ens, wall)
    c = refs[0][0]
    nb, nblb = c["nb"], c["nblb"]
    assert _fits(name, m, mixed=True)
    if ens == "E4":
        assert not bs.small_fits(nblb, nb + 1, m, True) and not _fits("E1", 255, mixed=True) and _fits("E1", 255)
    rng = np.random.default_rng(23)
    masks = rng.random((R, nb)) < np.linspace(0.2, 0.8, R)[:, None]
    masks[0] = np.arange(nb) % 2 == 1                      # replica 0: every other body
    ins = [_mixed_inputs(nb, nblb, 40 + r) for r in range(R)]
    body_in = np.stack([_body_in(masks[r], ins[r][0], ins[r][1]) for r in range(R)])
    slip = np.stack([ins[r][2] for r in range(R)])
    ctx = _ctx(c, wall, config=False)
    ctx.ensemble_set_config(X, Q)
    lam, U, Fo, its, res = ctx.ensemble_solve_mixed(masks.astype(np.uint8), body_in, max_iter=m, rtol=1e-10, slip=slip)
    ctx.close()
    assert (its > 0).all() and (its < m).all() and (res < 1e-10).all()
    for r in range(R):
        p = masks[r]
        F, Up, sl = ins[r]
        lam_d, U_d, F_d = _dense_mixed(refs[r][3], refs[r][4], p, F, Up, sl)
        print("%s %s replica %d (%d of %d prescribed): %d iterations, rel. diff lambda %.2e U %.2e F %.2e (1e-7)"
              % (ens, wall, r, p.sum(), nb, its[r], _rel(lam[r], lam_d), _rel(U[r], U_d), _rel(Fo[r], F_d)))
        assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7 and _rel(Fo[r], F_d) <= 1e-7
        assert np.array_equal(U[r].reshape(nb, 6)[p], Up[p]) and np.array_equal(Fo[r].reshape(nb, 6)[~p], F[~p])


def test_a_run_above_the_wall_is_three_one_step_calls_bitwise():
    """run(n_steps = 3, on_error = "reject") above the wall on 5 replicas of 64 trimers (S1 was meant, which no ensemble
    takes) against three one-step calls, bitwise: test_a_run_is_the_loop_bitwise's claim where the replicas hold 320 bodies, so
    that the per-body kernels (k_ens_midpoint, k_ens_evolve) need a second workgroup of 256 threads, and where k_ens_verdict's
    workgroup checks the 192 blobs of a replica against the wall."""
    from rigid_body_light_amd import Ensemble
    name, R, m, refs, X, Q = _replicas("S3x5", True)
    c = refs[0][0]
    F, slip, _ = _ensemble_inputs(R, c["nb"], c["nblb"], 19)
    kw = dict(max_iter=m, rtol=1e-8)

    def make():
        with _poison_env():
            e = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=DT, kBT=KBT, wall=True)
        assert e.ctx.get_option("poison_workspace") == 1
        return e

    ens = make()
    its, res = [], []
    for n in range(3):
        it, rs = ens.step_brownian(F, seed=40 + n, slip=slip, **kw)
        its.append(it); res.append(rs)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = make()
    out = ens.run(3, F=F, brownian=True, seed=40, on_error="reject", slip=slip, **kw)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)
    assert np.isfinite(Xr).all() and not np.array_equal(Xr, X)
    assert np.array_equal(out.iters_sum, np.sum(its, axis=0)) and np.array_equal(out.resid_max, np.max(res, axis=0))
    assert np.array_equal(out.accepted, np.full(R, 3)) and not out.rejected.any() and not out.first_status.any()
    assert (out.steps_done, out.stopped_at) == (3, -1)


# ---------------------------------------------------------------------------------------------------------------- (e) single-context steps
@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name,block", [("G2", False), ("G2", True), ("G7", True), ("S1", False)])
def test_single_context_steps_vs_oracle_chain(name, block, wall):
    """step_deterministic and step_brownian (method 0: the dense Cholesky root; injected noise, split_rand both ways) of one
    context against the same oracle chain with the same bound as the ensembles: rtol 1e-12, displacement to 10 cond(A) rtol
    relative plus 1e-12 absolute on the quaternions.  G2 (100 tetrahedra: k_saddle_tail's case) with both preconditioners, G7
    (two bodies of 257 blobs) with the block preconditioner, S1 with the diagonal one.

    Measured worst (one MI355X), as a fraction of the bound: deterministic 8.2e-4 (positions; S1, wall), 4.5e-4 (quaternions);
    Brownian 2.6e-4 (positions), 1.1e-4 (quaternions)."""
    c, cfg, Qn, M, K, Am = _ref(name, wall)
    nb, nblb = c["nb"], c["nblb"]
    cond = bs.COND_A[(name, wall)]
    F, slip, W = (v[0] for v in _ensemble_inputs(1, nb, nblb, 29))
    for kind in ("deterministic", "brownian split", "brownian"):
        ctx = _ctx(c, wall, block)
        if kind == "deterministic":
            its, res = ctx.step_deterministic(F, max_iter=200, rtol=RTOL_E, slip=slip)
        else:
            its, res = ctx.step_brownian(F, max_iter=200, rtol=RTOL_E, slip=slip, W=W, method=0, split_rand=kind == "brownian split")
        Xg, Qg = ctx.get_config(nb)
        ctx.close()
        Xr, Qr = _oracle_step(c, cfg, Qn, wall, F, slip, None if kind == "deterministic" else W, kind == "brownian split", Am)
        fx, fq, ok = _assert_displacement(kind, Xg, Qg, Xr, Qr, c["X"], Qn, cond, RTOL_E)
        print("%s %s block=%s %s: %d iterations, residual estimate %.1e; displacement error / bound: X %.2e  Q %.2e (bound %.1e)"
              % (name, wall, block, kind, its, res, fx, fq, 10 * cond * RTOL_E))
        assert ok, (kind, fx, fq)
