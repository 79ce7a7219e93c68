"""Imposed flow, body-frame slip and first moments (include/rbl.h section 8) on the GPU: the term and the moments against their
numpy restatement (tests/flow_reference.py) to rounding bounds, where the term enters every step family (bit for bit against the
same step with the term passed as `slip`), off is off, the physics of a force-free shell in a linear flow and of held shells in
shear over the wall against dense numpy solves, the recorded moments, poisoned workspaces and the example.

Two shapes: 10 x shell_N_12 (a body smaller than a wave, ten bodies on a grid that does not divide evenly) and 2 x shell_N_642
with random quaternions (a per-body loop strides more than once over its workgroup).  Tolerances: rounding bounds for the O(N)
kernels; 1e-7 between two solutions of one system (solves to rtol 1e-10), as tests/test_prescribed_gpu.py."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flow_reference as FR  # noqa: E402

WALL_BLOCK = [(False, False), (False, True), (True, False), (True, True)]
SHAPES = [(10, 12), (2, 642)]
ONE_FAMILIES = ["deterministic", "brownian", "mixed", "mixed_dof", "brownian_mixed"]
ENS_FAMILIES = ["deterministic", "brownian", "mixed", "brownian_mixed"]


def _body(nb, nblb, wall, block, dt=0.001, seed=0):
    from rigid_body_light_amd import RigidBody, make_config
    c = make_config(nb, nblb, wall, seed=seed)
    return c, RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], dt, wall_PC=wall, block_PC=block)


def _flow(wall, seed=5):
    """(u0, G): anything in free space, u = (G02 z, G12 z, 0) above the wall"""
    rng = np.random.default_rng(seed)
    if wall:
        G = np.zeros((3, 3))
        G[0, 2], G[1, 2] = 0.8, -0.3
        return np.zeros(3), G
    return rng.standard_normal(3), rng.standard_normal((3, 3))


def _pattern(nb, nblb, seed=6):
    """(slip_body (nblb, 3), scale (nb,) in [0, 1] with a passive body)"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.2, 1.0, nb)
    scale[nb // 2] = 0.0
    return 0.3 * rng.standard_normal((nblb, 3)), scale


def _set_model(obj, wall, nb, nblb, part="both", on=True):
    u0, G = _flow(wall)
    sb, sc = _pattern(nb, nblb)
    kw = {}
    if part in ("flow", "both"):
        obj.set_background_flow(u0, G, on=on)
        kw.update(u0=u0, G=G)
    if part in ("slip", "both"):
        obj.set_body_slip(sb, sc, on=on)
        kw.update(slip_body=sb, scale=sc)
    return kw


def _rel(x, y):
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    return np.linalg.norm(x - y) / np.linalg.norm(y)


def _ens_configs(R, nb, wall):
    from rigid_body_light_amd import make_config
    cs = [make_config(nb, 12, wall, seed=20 + 3 * r) for r in range(R)]
    return cs[0], np.stack([c["X"] for c in cs]), np.stack([c["Q"] for c in cs])


def _ensemble(R, nb, wall, dt=0.001):
    from rigid_body_light_amd import Ensemble
    c, X, Q = _ens_configs(R, nb, wall)
    return c, X, Q, Ensemble(c["cfg"], X, Q, c["a"], c["eta"], dt, kBT=1.0, wall=wall)


# ---- 1. the term ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["flow", "slip", "both"])
@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("nb,nblb", SHAPES)
def test_flow_slip_against_numpy(orc, nb, nblb, wall, part):
    c, rb = _body(nb, nblb, wall, False)
    assert not np.any(rb.flow_slip())                                     # both parts off: zeros
    kw = _set_model(rb, wall, nb, nblb, part)
    ref, bound = FR.flow_term(orc, c["X"], c["Q"], c["cfg"], **kw)
    got = rb.flow_slip()
    assert got.shape == (nb * nblb, 3)
    err = np.abs(got.reshape(-1) - ref)
    print("flow_slip %dx%d wall=%s %s: max err / bound %.3f, |t| max %.3g" % (nb, nblb, wall, part, np.max(err / np.maximum(bound, 1e-300)), np.abs(ref).max()))
    assert np.all(err <= bound)
    assert np.abs(ref).max() > 0.1
    if part != "flow":
        k = nb // 2                                                       # the passive body carries the flow alone
        own = FR.flow_term(orc, c["X"], c["Q"], c["cfg"], u0=kw.get("u0"), G=kw.get("G"))[0] if part == "both" else np.zeros(3 * nb * nblb)
        assert np.all(np.abs(got.reshape(nb, -1)[k] - own.reshape(nb, -1)[k]) <= bound.reshape(nb, -1)[k])
    assert rb.flow_slip().tobytes() == got.tobytes()                      # bitwise repeatable
    m = rb.flow_model()
    assert m["flow_on"] == (part != "slip") and m["body_slip_on"] == (part != "flow")


@pytest.mark.parametrize("wall", [False, True])
def test_ensemble_flow_slip_replica_by_replica(orc, wall):
    R, nb, nblb = 3, 10, 12
    c, X, Q, ens = _ensemble(R, nb, wall)
    assert not np.any(ens.flow_slip())
    kw = _set_model(ens, wall, nb, nblb)
    got = ens.flow_slip()
    assert got.shape == (R, 3 * nb * nblb)
    from rigid_body_light_amd import RigidBody
    for r in range(R):
        ref, bound = FR.flow_term(orc, X[r], Q[r], c["cfg"], **kw)
        assert np.all(np.abs(got[r] - ref) <= bound), r
        rb = RigidBody(c["cfg"], X[r], Q[r], c["a"], c["eta"], 0.001, wall_PC=wall)
        _set_model(rb, wall, nb, nblb)
        assert rb.flow_slip().tobytes() == got[r].tobytes(), r            # the same kernel on the same positions
    assert ens.flow_slip().tobytes() == got.tobytes()
    ens.close()


# ---- 2. first moments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,nblb", SHAPES)
def test_first_moments_against_einsum(orc, nb, nblb):
    c, rb = _body(nb, nblb, True, False)
    lam = np.random.default_rng(7).standard_normal(3 * nb * nblb)
    D = rb.first_moments(lam)
    ref, bound = FR.first_moments(orc, c["X"], c["Q"], c["cfg"], lam)
    assert D.shape == (nb, 3, 3)
    print("first_moments %dx%d: max err / bound %.3g" % (nb, nblb, np.max(np.abs(D - ref) / bound)))
    assert np.all(np.abs(D - ref) <= bound)
    # the antisymmetric part is the torque of K^T lambda, the row sums' partner
    T = rb.KT_dot(lam).reshape(nb, 6)[:, 3:]
    tb = np.stack([bound[:, 1, 2] + bound[:, 2, 1], bound[:, 2, 0] + bound[:, 0, 2], bound[:, 0, 1] + bound[:, 1, 0]], axis=-1)
    assert np.all(np.abs(FR.torque(D) - T) <= tb)
    assert rb.first_moments(lam).tobytes() == D.tobytes()
    S = rb.stresslets(lam)
    assert np.allclose(S, FR.stresslet(ref), rtol=0, atol=float(bound.max()) * 2)


# ---- 3. where it enters, bit for bit ---------------------------------------------------------------------------------------------
def _one_step(rb, family, nb, nblb, slip, seed=9):
    """one step of `family` from the object's state with seeded inputs -> iteration count"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal(6 * nb)
    W = rng.standard_normal(9 * nb * nblb)
    p = np.isin(np.arange(nb), [1, 4, 7])
    p6 = np.zeros((nb, 6), dtype=bool)
    p6[1, 3:] = True
    p6[4, :3] = True
    p6[7, 2] = True
    kw = dict(slip=slip, max_iter=150, rtol=1e-10)
    if family == "deterministic":
        return rb.step_deterministic(F, **kw)[0]
    if family == "brownian":
        return rb.step_brownian(F, W=W, **kw)[0]
    if family == "mixed":
        return rb.step_mixed(p, F, **kw)[1]
    if family == "mixed_dof":
        return rb.step_mixed_dof(p6, F, **kw)[1]
    return rb.step_brownian_mixed(p, F, W=W, **kw)[1]


@pytest.mark.parametrize("family", ONE_FAMILIES)
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_step_with_the_model_is_the_step_with_the_term_as_slip(wall, block, family):
    nb, nblb = 10, 12
    host = 0.05 * np.random.default_rng(10).standard_normal(3 * nb * nblb)
    for with_host in (False, True):
        _, a = _body(nb, nblb, wall, block)
        _set_model(a, wall, nb, nblb)
        t = a.flow_slip().reshape(-1)
        assert np.abs(t).max() > 0.1
        its_a = _one_step(a, family, nb, nblb, host if with_host else None)
        _, b = _body(nb, nblb, wall, block)
        _set_model(b, wall, nb, nblb, on=False)                           # set and switched off: the caller passes the term
        its_b = _one_step(b, family, nb, nblb, host + t if with_host else t)      # slip + t, in that order
        (Xa, Qa), (Xb, Qb) = a.get_config(), b.get_config()
        assert its_a == its_b and 0 < its_a < 150
        assert Xa.tobytes() == Xb.tobytes() and Qa.tobytes() == Qb.tobytes(), (family, with_host)
        _, z = _body(nb, nblb, wall, block)                               # and the term did something
        _one_step(z, family, nb, nblb, host if with_host else None)
        assert np.abs(z.get_config()[0] - Xa).max() > 1e-6


def _ens_step(ens, family, slip, seed=9):
    R, nb = ens.R, ens.N_bodies
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, 6 * nb))
    W = rng.standard_normal((R, 9 * nb * ens.blobs_per_body))
    p = np.zeros((R, nb), dtype=bool)
    p[:, 1] = True
    p[1, 4] = True
    kw = dict(slip=slip, max_iter=150, rtol=1e-10)
    if family == "deterministic":
        return ens.step_deterministic(F, **kw)[0]
    if family == "brownian":
        return ens.step_brownian(F, W=W, **kw)[0]
    if family == "mixed":
        return ens.step_mixed(p, F, **kw)[1]
    return ens.step_brownian_mixed(p, F, W=W, **kw)[1]


@pytest.mark.parametrize("family", ENS_FAMILIES)
@pytest.mark.parametrize("wall", [False, True])
def test_ensemble_step_with_the_model_is_the_step_with_the_term_as_slip(wall, family):
    R, nb, nblb = 3, 10, 12
    host = 0.05 * np.random.default_rng(10).standard_normal((R, 3 * nb * nblb))
    for with_host in (False, True):
        _, _, _, a = _ensemble(R, nb, wall)
        _set_model(a, wall, nb, nblb)
        t = a.flow_slip()
        its_a = _ens_step(a, family, host if with_host else None)
        _, _, _, b = _ensemble(R, nb, wall)
        _set_model(b, wall, nb, nblb, on=False)
        its_b = _ens_step(b, family, host + t if with_host else t)
        (Xa, Qa), (Xb, Qb) = a.get_config(), b.get_config()
        assert np.array_equal(its_a, its_b) and np.all(its_a > 0) and np.all(its_a < 150)
        assert Xa.tobytes() == Xb.tobytes() and Qa.tobytes() == Qb.tobytes(), (family, with_host)
        _, _, _, z = _ensemble(R, nb, wall)
        _ens_step(z, family, host if with_host else None)
        assert np.abs(z.get_config()[0] - Xa).max() > 1e-6
        for e in (a, b, z):
            e.close()


def _stepper_ctx(c, wall, nb, nblb, on):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=0.001, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    _set_model(ctx, wall, nb, nblb, on=on)
    return ctx


@pytest.mark.parametrize("wall", [False, True])
def test_deterministic_stepper_with_the_model_is_the_solve_with_the_term_as_slip(wall):
    """krylov.py's DeterministicStepper, the Python-driven family of section 8: step() with the model on against solve(slip = t) +
    evolve on a context with the model switched off, bitwise on the configuration and the iteration count; and against
    rbl_step_deterministic with the model on: the same iteration count, the configuration to 1e-12"""
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd.krylov import DeterministicStepper
    nb, nblb = 10, 12
    c = make_config(nb, nblb, wall)
    dev = torch.device("cuda:0")
    F = np.random.default_rng(3).standard_normal(6 * nb)
    a = _stepper_ctx(c, wall, nb, nblb, True)
    t = a.flow_slip()
    sa = DeterministicStepper(a, nb, nblb, dev)
    assert sa.slip_at_qn().cpu().numpy().tobytes() == t.tobytes()
    its_a, _ = sa.step(F, iters=150, rtol=1e-10)
    b = _stepper_ctx(c, wall, nb, nblb, False)
    sb = DeterministicStepper(b, nb, nblb, dev)
    assert sb.slip_at_qn() is None                                          # off: the step is what it was
    lam, U, its_b, _ = sb.solve(F, iters=150, rtol=1e-10, slip=torch.from_numpy(t).to(dev))
    b.evolve(U.cpu().numpy())
    cc = _stepper_ctx(c, wall, nb, nblb, True)
    its_c, _ = cc.step_deterministic(F, max_iter=150, rtol=1e-10)
    (Xa, Qa), (Xb, Qb), (Xc, Qc) = a.get_config(nb), b.get_config(nb), cc.get_config(nb)
    assert its_a == its_b == its_c and 0 < its_a < 150
    assert Xa.tobytes() == Xb.tobytes() and Qa.tobytes() == Qb.tobytes()
    assert np.abs(Xa - Xc).max() <= 1e-12 and np.abs(Qa - Qc).max() <= 1e-12   # (the C step forms -F by another kernel)
    z = _stepper_ctx(c, wall, nb, nblb, False)                              # and the term did something
    DeterministicStepper(z, nb, nblb, dev).step(F, iters=150, rtol=1e-10)
    assert np.abs(z.get_config(nb)[0] - Xa).max() > 1e-6
    for ctx in (a, b, cc, z):
        ctx.close()


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("wall", [False, True])
def test_brownian_stepper_with_the_model_is_the_step_with_the_term_as_slip(wall, method):
    """krylov.py's BrownianStepper (ShardedBrownianStepper goes through the same step): model on and slip=None against model off
    and slip = flow_slip(), bitwise on configuration and iteration count; with a host slip present to 1e-12 (slip + t, that order)"""
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd.krylov import BrownianStepper
    nb, nblb = 10, 12
    c = make_config(nb, nblb, wall)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(4)
    F, W = rng.standard_normal(6 * nb), rng.standard_normal(9 * nb * nblb)
    host = 0.05 * rng.standard_normal(3 * nb * nblb)
    kw = dict(W=W, method=method, iters=150, rtol=1e-10)
    for with_host in (False, True):
        a = _stepper_ctx(c, wall, nb, nblb, True)
        t = a.flow_slip()
        sa = BrownianStepper(a, nb, nblb, dev)
        if with_host:
            assert np.abs(sa.slip_at_qn(host).cpu().numpy() - (host + t)).max() <= 1e-15
        its_a, _ = sa.step(F, slip=host if with_host else None, **kw)
        b = _stepper_ctx(c, wall, nb, nblb, False)
        its_b, _ = BrownianStepper(b, nb, nblb, dev).step(F, slip=host + t if with_host else t, **kw)
        (Xa, Qa), (Xb, Qb) = a.get_config(nb), b.get_config(nb)
        assert its_a == its_b and 0 < its_a < 150
        if with_host:
            assert np.abs(Xa - Xb).max() <= 1e-12 and np.abs(Qa - Qb).max() <= 1e-12
        else:
            assert Xa.tobytes() == Xb.tobytes() and Qa.tobytes() == Qb.tobytes()
        z = _stepper_ctx(c, wall, nb, nblb, False)
        BrownianStepper(z, nb, nblb, dev).step(F, slip=host if with_host else None, **kw)
        assert np.abs(z.get_config(nb)[0] - Xa).max() > 1e-6
        for ctx in (a, b, z):
            ctx.close()


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ONE_FAMILIES)
def test_off_is_off_and_recording_changes_nothing(family):
    nb, nblb, wall, block = 10, 12, True, True
    host = 0.05 * np.random.default_rng(10).standard_normal(3 * nb * nblb)
    runs = []
    for state in ("never", "off", "record"):
        _, rb = _body(nb, nblb, wall, block)
        if state == "off":
            _set_model(rb, False, nb, nblb, on=False)                     # even a flow the wall would refuse: it is off
        if state == "record":
            rb.record_moments()
        its = [_one_step(rb, family, nb, nblb, host, seed=30 + n) for n in range(2)]
        runs.append((its, rb.get_config()))
        if state == "record":
            assert np.all(np.isfinite(rb.step_moments()))
        else:
            with pytest.raises(RuntimeError):
                rb.step_moments()
    for its, (X, Q) in runs[1:]:
        assert its == runs[0][0]
        assert X.tobytes() == runs[0][1][0].tobytes() and Q.tobytes() == runs[0][1][1].tobytes()


@pytest.mark.parametrize("family", ENS_FAMILIES)
def test_ensemble_off_is_off_and_recording_changes_nothing(family):
    R, nb, nblb, wall = 3, 10, 12, True
    runs = []
    for state in ("never", "off", "record"):
        _, _, _, ens = _ensemble(R, nb, wall)
        if state == "off":
            _set_model(ens, False, nb, nblb, on=False)
        if state == "record":
            ens.record_moments()
        its = [_ens_step(ens, family, None, seed=30 + n) for n in range(2)]
        runs.append((its, ens.get_config()))
        if state == "record":
            assert ens.step_moments().shape == (R, nb, 3, 3) and np.all(np.isfinite(ens.step_moments()))
        else:
            with pytest.raises(RuntimeError):
                ens.step_moments()
        ens.close()
    for its, (X, Q) in runs[1:]:
        assert all(np.array_equal(i, j) for i, j in zip(its, runs[0][0]))
        assert X.tobytes() == runs[0][1][0].tobytes() and Q.tobytes() == runs[0][1][1].tobytes()


# ---- 5. physics, free space -------------------------------------------------------------------------------------------------------
def _dense_matrices(orc, c, X, Q, wall):
    """M (B M B with the wall, as apply_M applies it) and K of a configuration, built as tests/test_prescribed_gpu.py builds them"""
    from oracle import oracle as O
    cfg = c["cfg"] - c["cfg"].mean(axis=0)
    Qn = O.normalize_quats(np.asarray(Q, dtype=np.float64).reshape(-1, 4))
    r = orc.multi_body_pos(X, Qn, cfg)
    K = O.K_matrix(X, Qn, cfg)
    M = orc.rotne_prager_tensor(r, c["a"], c["eta"], wall)
    if wall:
        B = orc.damp(r, c["a"])
        M = B[:, None] * M * B[None, :]
    return M, K


def _one_c(S, E):
    """S = c E: the ratios over the components that carry E, their mean and relative spread"""
    m = np.abs(E) > 0.05 * np.abs(E).max()
    c = S[m] / E[m]
    return c.mean(), (c.max() - c.min()) / abs(c.mean())


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("nblb", [12, 42])
def test_force_free_shell_follows_a_linear_flow(orc, nblb, block):
    from oracle import oracle as O
    from rigid_body_light_amd import RigidBody, load_structure
    params, cfg = load_structure(nblb)
    a, eta, dt = params["sep"] / 2.0, 1.0, 0.01
    rng = np.random.default_rng(40 + nblb)
    X = rng.uniform(-2.0, 2.0, (1, 3))
    Q = rng.standard_normal((1, 4))
    Q /= np.linalg.norm(Q)
    G = rng.standard_normal((3, 3))
    G -= np.trace(G) / 3.0 * np.eye(3)
    u0 = rng.standard_normal(3)
    rb = RigidBody(cfg, X, Q, a, eta, dt, wall_PC=False, block_PC=block)
    rb.set_background_flow(u0, G)
    t = rb.flow_slip().reshape(-1)
    lam, U, F, its, res = rb.solve_mixed([], np.zeros(6), slip=t, max_iter=200, rtol=1e-10)
    U_exp = u0 + G @ X[0]
    Om_exp = 0.5 * np.array([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
    nU = np.linalg.norm(U_exp)
    E = 0.5 * (G + G.T)
    S = rb.stresslets(lam)[0]
    c, spread = _one_c(S, E)
    c_faxen = (20.0 / 3.0) * np.pi * eta * params["Rh"] ** 3
    print("shell_N_%d block=%s: %d iterations; |U - (u0 + G X)| / |U| %.2e, |Omega - curl/2| / |U| %.2e; S = c E with c = %.6g, spread %.2e; "
          "c / ((20/3) pi eta r_h^3) = %.4f" % (nblb, block, its, np.linalg.norm(U[:3] - U_exp) / nU, np.linalg.norm(U[3:] - Om_exp) / nU, c, spread,
                                               abs(c) / c_faxen))
    assert 0 < its < 200
    assert np.linalg.norm(U[:3] - U_exp) <= 1e-7 * nU and np.linalg.norm(U[3:] - Om_exp) <= 1e-7 * nU
    assert spread <= 1e-6
    assert np.abs(S - c * E).max() <= 1e-6 * np.abs(S).max()
    # the dense numpy saddle solve on the oracle's matrices
    cc = {"cfg": cfg, "a": a, "eta": eta}
    M, K = _dense_matrices(orc, cc, X, Q, False)
    n3 = 3 * nblb
    x = np.linalg.solve(np.block([[M, -K], [K.T, np.zeros((6, 6))]]), np.concatenate([FR.flow_term(orc, X, Q, cfg, u0=u0, G=G)[0], np.zeros(6)]))
    D_d = FR.first_moments(orc, X, Q, cfg, x[:n3])[0]
    c_d, spread_d = _one_c(FR.stresslet(D_d)[0], E)
    print("    dense: |U - exact| / |U| %.2e, spread %.2e" % (np.linalg.norm(x[n3:n3 + 3] - U_exp) / nU, spread_d))
    assert _rel(lam, x[:n3]) <= 1e-7 and _rel(U, x[n3:]) <= 1e-7 and abs(c - c_d) <= 1e-7 * abs(c_d)
    # one time step: the shell is carried and turned by the flow
    X0, Q0 = rb.get_config()
    its2, _ = rb.step_deterministic(np.zeros(6), max_iter=200, rtol=1e-10)
    X1, Q1 = rb.get_config()
    U_step = (X1[0] - X0[0]) / dt
    q = O.quat_mul(Q1[0], Q0[0] * np.array([1.0, -1.0, -1.0, -1.0]))     # the step's rotation
    v = q[1:] * np.sign(q[0])
    Om_step = 2.0 * np.arctan2(np.linalg.norm(v), abs(q[0])) * v / np.linalg.norm(v) / dt
    print("    step: %d iterations, |U_step - exact| / |U| %.2e, |Omega_step - exact| / |U| %.2e"
          % (its2, np.linalg.norm(U_step - U_exp) / nU, np.linalg.norm(Om_step - Om_exp) / nU))
    assert np.linalg.norm(U_step - U_exp) <= 1e-7 * nU and np.linalg.norm(Om_step - Om_exp) <= 1e-7 * nU


# ---- 6. physics, wall -------------------------------------------------------------------------------------------------------------
def _dense_mixed(M, K, p, F, Up, slip):
    """numpy.linalg.solve on the constrained matrix [M -K_f; K_f^T 0] -> (lambda, U (all bodies), F (all bodies)), as
    tests/test_prescribed_gpu.py"""
    n3 = M.shape[0]
    colf = np.repeat(~p, 6)
    Kf, Kp = K[:, colf], K[:, ~colf]
    nf6 = Kf.shape[1]
    A = np.block([[M, -Kf], [Kf.T, np.zeros((nf6, nf6))]])
    x = np.linalg.solve(A, np.concatenate([slip + Kp @ Up[p].reshape(-1), -F[~p].reshape(-1)]))
    lam = x[:n3]
    U = np.array(Up, dtype=np.float64)
    U[~p] = x[n3:].reshape(-1, 6)
    Fo = np.array(F, dtype=np.float64)
    Fo[p] = -(Kp.T @ lam).reshape(-1, 6)
    return lam, U.reshape(-1), Fo.reshape(-1)


@pytest.mark.parametrize("block", [False, True])
def test_shells_in_shear_over_the_wall_against_the_dense_solve(orc, block):
    nb, nblb, wall, gdot = 10, 12, True, 0.7
    c, rb = _body(nb, nblb, wall, block)
    G = np.zeros((3, 3))
    G[0, 2] = gdot
    rb.set_background_flow(G=G)
    p = np.isin(np.arange(nb), [1, 4, 7])
    F = 0.2 * np.random.default_rng(50).standard_normal((nb, 6))
    Up = np.zeros((nb, 6))                                                # held
    lam, U, Fo, its, res = rb.solve_mixed(p, np.where(p[:, None], Up, F).reshape(-1), slip=rb.flow_slip().reshape(-1), max_iter=200, rtol=1e-10)
    M, K = _dense_matrices(orc, c, c["X"], c["Q"], wall)
    r = rb.get_blob_positions()
    minus_uinf = np.stack([-gdot * r[:, 2], np.zeros(len(r)), np.zeros(len(r))], axis=1).reshape(-1)
    lam_d, U_d, F_d = _dense_mixed(M, K, p, F, Up, minus_uinf)
    print("shear over the wall block=%s: %d iterations, rel. diff lambda %.2e U %.2e F %.2e; held body load %s"
          % (block, its, _rel(lam, lam_d), _rel(U, U_d), _rel(Fo, F_d), Fo.reshape(nb, 6)[1, :3]))
    assert 0 < its < 200
    assert _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(Fo, F_d) <= 1e-7
    assert U.reshape(nb, 6)[0, 0] > 0.0                                    # a free shell is carried along +x


def test_flows_that_do_not_vanish_on_the_wall_raise():
    nb, nblb = 10, 12
    _, rb = _body(nb, nblb, True, False)
    X0 = rb.get_config()[0].copy()
    bad = [(np.array([0.1, 0.0, 0.0]), np.zeros((3, 3)))]
    for i, j in ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (2, 2)):
        G = np.zeros((3, 3))
        G[i, j] = 0.5
        bad.append((np.zeros(3), G))
    for u0, G in bad:
        rb.set_background_flow(u0, G)
        with pytest.raises(RuntimeError, match="z = 0"):
            rb.flow_slip()
        with pytest.raises(RuntimeError, match="z = 0"):
            rb.step_deterministic(np.zeros(6 * nb))
        with pytest.raises(RuntimeError, match="z = 0"):
            rb.step_brownian_mixed([1], np.zeros(6 * nb))
    assert np.array_equal(rb.get_config()[0], X0)                          # nothing moved
    _, _, _, ens = _ensemble(3, nb, True)
    ens.set_background_flow(*bad[0])
    with pytest.raises(RuntimeError, match="z = 0"):
        ens.flow_slip()
    with pytest.raises(RuntimeError, match="z = 0"):
        ens.step_deterministic(np.zeros(6 * nb))
    ens.set_background_flow(on=False)
    ens.set_body_slip(np.zeros((nblb, 3)), np.ones(nb))
    ens.ctx.set_body_slip(np.zeros((nblb, 3)), np.ones(nb + 1))           # n_scale of another body count: refused at the use
    with pytest.raises(RuntimeError, match="n_scale"):
        ens.step_brownian(np.zeros(6 * nb))
    ens.close()


# ---- 7. recorded moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall,block", WALL_BLOCK)
def test_recorded_moments_of_the_deterministic_and_the_brownian_step(wall, block):
    nb, nblb = 10, 12
    n3 = 3 * nb * nblb
    rng = np.random.default_rng(60)
    F = rng.standard_normal(6 * nb)
    host = 0.05 * rng.standard_normal(n3)
    W = rng.standard_normal(3 * n3)
    _, rb = _body(nb, nblb, wall, block)
    _set_model(rb, wall, nb, nblb)
    rb.record_moments()
    # deterministic: the lambda of solve_saddle on the same right-hand side at q^n
    slip = host + rb.flow_slip().reshape(-1)
    x, its, _ = rb.solve_saddle(np.concatenate([slip, -F]), max_iter=200, rtol=1e-10)
    D_ref = rb.first_moments(x[:n3])
    rb.step_deterministic(F, slip=host, max_iter=200, rtol=1e-10)
    D = rb.step_moments()
    print("recorded, deterministic wall=%s block=%s: rel. diff %.2e" % (wall, block, _rel(D, D_ref)))
    assert _rel(D, D_ref) <= 1e-7
    # Brownian: RHS_and_Midpoint + solve_saddle replayed by hand, moments with the lever arms of the midpoint configuration
    Xn, Qn = rb.get_config()
    slip = host + rb.flow_slip().reshape(-1)
    rhs, Xh, Qh = rb.RHS_and_Midpoint(slip, F, W=W, method="lanczos_pc")
    rb.set_config(Xh.reshape(Xn.shape), Qh.reshape(Qn.shape))
    x, its, _ = rb.solve_saddle(rhs, max_iter=200, rtol=1e-10)
    D_ref = rb.first_moments(x[:n3])
    rb.set_config(Xn, Qn)
    rb.step_brownian(F, slip=host, W=W, method="lanczos_pc", max_iter=200, rtol=1e-10)
    D = rb.step_moments()
    print("recorded, Brownian wall=%s block=%s: rel. diff %.2e" % (wall, block, _rel(D, D_ref)))
    assert _rel(D, D_ref) <= 1e-7
    rb.record_moments()                                                    # set again: what was recorded is gone
    with pytest.raises(RuntimeError):
        rb.step_moments()


def test_a_step_that_fails_leaves_no_record():
    """only a step that recorded leaves a readable set: after a step whose solve fails (two bodies on top of each other:
    RBL_ERR_OVERLAP) step_moments is RBL_ERR_STATE, not the previous step's moments"""
    nb, nblb = 10, 12
    for family in ONE_FAMILIES:
        c, rb = _body(nb, nblb, True, False)
        rb.record_moments()
        _one_step(rb, family, nb, nblb, None)
        assert np.all(np.isfinite(rb.step_moments()))
        X, Q = rb.get_config()
        X = X.copy()
        X[3] = X[2]
        Q = Q.copy()
        Q[3] = Q[2]
        rb.set_config(X, Q)
        with pytest.raises(RuntimeError):
            _one_step(rb, family, nb, nblb, None)
        with pytest.raises(RuntimeError, match="record"):
            rb.step_moments()


@pytest.mark.parametrize("wall", [False, True])
def test_ensemble_record_equals_the_one_system_record(wall):
    from rigid_body_light_amd import RigidBody
    R, nb, nblb = 3, 10, 12
    rng = np.random.default_rng(61)
    F = rng.standard_normal((R, 6 * nb))
    W = rng.standard_normal((R, 9 * nb * nblb))
    p = np.isin(np.arange(nb), [2, 5])

    def single(r):
        rb = RigidBody(c["cfg"], X[r], Q[r], c["a"], c["eta"], 0.001, wall_PC=wall, block_PC=False)
        _set_model(rb, wall, nb, nblb)
        rb.record_moments()
        return rb

    kw = dict(max_iter=200, rtol=1e-10)
    steps = {"deterministic": (lambda e: e.step_deterministic(F, **kw), lambda s, r: s.step_deterministic(F[r], **kw)),
             "brownian": (lambda e: e.step_brownian(F, W=W, **kw), lambda s, r: s.step_brownian(F[r], W=W[r], method="cholesky", **kw)),
             "mixed": (lambda e: e.step_mixed(p, F, **kw), lambda s, r: s.step_mixed(p, F[r], **kw)),
             "brownian_mixed": (lambda e: e.step_brownian_mixed(p, F, W=W, **kw),
                                lambda s, r: s.step_brownian_mixed(p, F[r], W=W[r], method="cholesky", **kw))}
    for name, (ens_step, one_step) in steps.items():
        c, X, Q, ens = _ensemble(R, nb, wall)
        _set_model(ens, wall, nb, nblb)
        ens.record_moments()
        ens_step(ens)
        De = ens.step_moments()
        for r in range(R):
            s = single(r)
            one_step(s, r)
            d = _rel(De[r], s.step_moments())
            print("ensemble record, %s wall=%s replica %d: rel. diff %.2e" % (name, wall, r, d))
            assert d <= 1e-7
        ens.close()
    # seeded noise: with the dense root and the same seed replica 0 draws what the one-system step draws
    c, X, Q, ens = _ensemble(R, nb, wall)
    _set_model(ens, wall, nb, nblb)
    ens.record_moments()
    ens.step_brownian(F, seed=77, **kw)
    s = single(0)
    s.step_brownian(F[0], seed=77, method="cholesky", **kw)
    assert _rel(ens.step_moments()[0], s.step_moments()) <= 1e-7
    ens.close()


# ---- 8. poisoned workspaces --------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("wall", [False, True])
def test_new_buffers_are_written_before_they_are_read(wall):
    """the method of tests/test_poisoned_workspace_gpu.py: the same seeded calls through a context whose workspaces are filled with
    NaN patterns at every allocation and reserve, and through a clean one: bitwise the same outputs, all finite"""
    from rigid_body_light_amd import Ensemble, RigidBody, make_config
    nb, nblb, R = 10, 12, 3
    c = make_config(nb, nblb, wall)
    ce, Xe, Qe = _ens_configs(R, nb, wall)
    rng = np.random.default_rng(70)
    F, lam = rng.standard_normal(6 * nb), rng.standard_normal(3 * nb * nblb)
    W = rng.standard_normal(9 * nb * nblb)
    p = np.isin(np.arange(nb), [1, 4, 7])

    def run(poison):
        out = {}
        with _poison_env(poison):
            rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], 0.001, wall_PC=wall, block_PC=True)
            ens = Ensemble(ce["cfg"], Xe, Qe, ce["a"], ce["eta"], 0.001, kBT=1.0, wall=wall)
        assert rb.cb.get_option("poison_workspace") == int(poison) and ens.ctx.get_option("poison_workspace") == int(poison)
        out["moments_first"] = rb.first_moments(lam)                      # before anything else has touched the context
        out["zeros"] = rb.flow_slip()
        for obj in (rb, ens):
            _set_model(obj, wall, nb, nblb)
            obj.record_moments()
        out["term"] = rb.flow_slip()
        out["its_det"] = rb.step_deterministic(F, max_iter=150, rtol=1e-10)[0]
        out["D_det"] = rb.step_moments()
        out["its_bd"] = rb.step_brownian(F, W=W, max_iter=150, rtol=1e-10)[0]
        out["D_bd"] = rb.step_moments()
        out["its_mx"] = rb.step_mixed(p, F, max_iter=150, rtol=1e-10)[1]
        out["D_mx"] = rb.step_moments()
        out["its_bmx"] = rb.step_brownian_mixed(p, F, W=W, max_iter=150, rtol=1e-10)[1]
        out["D_bmx"] = rb.step_moments()
        out["X"], out["Q"] = rb.get_config()
        out["ens_term"] = ens.flow_slip()
        out["ens_its_det"] = ens.step_deterministic(F, max_iter=150, rtol=1e-10)[0]
        out["ens_D_det"] = ens.step_moments()
        out["ens_its_bd"] = ens.step_brownian(F, seed=3, max_iter=150, rtol=1e-10)[0]
        out["ens_D_bd"] = ens.step_moments()
        out["ens_its_bmx"] = ens.step_brownian_mixed(p, F, seed=4, max_iter=150, rtol=1e-10)[1]
        out["ens_D_bmx"] = ens.step_moments()
        out["ens_X"], out["ens_Q"] = ens.get_config()
        ens.close()
        return out

    clean, poisoned = run(False), run(True)
    assert clean.keys() == poisoned.keys()
    for k in clean:
        x, y = np.asarray(clean[k]), np.asarray(poisoned[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (k, "differs bitwise in %d of %d entries" % (int(np.sum(x != y)), x.size))
        assert np.all(np.isfinite(x)), k


# ---- 9. the example -----------------------------------------------------------------------------------------------------------------
def test_example_runs_in_its_shrunken_form():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "shear_flow.py"), "--quick"], cwd=ROOT, capture_output=True, text=True,
                       timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "S / E" in r.stdout and "ensemble" in r.stdout
