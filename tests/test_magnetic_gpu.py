"""The dipole terms of include/rbl.h section 4 on the GPU: permanent moments fixed in the bodies, the torque of a uniform field
B(t) and the dipole pairs between body centres against the numpy all-pairs oracle (tests/magnetic_oracle.py), generalised forces
against the library's own energy, ensembles against single contexts bitwise, the terms inside the steps, a run with a rotating
field against the loop that advances the field time by hand, synchronous rotation and step-out, Langevin statistics, the example."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import magnetic_oracle as mo  # noqa: E402
import table_oracle  # noqa: E402

R_SHELL = 0.79207921                                       # largest blob distance from the centre of shell_N_12


# ------------------------------------------------------------------------------------------------------------ shapes
def _quats(n, seed):
    Q = np.random.default_rng(seed).standard_normal((n, 4))
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _shell12():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return cfg, p["sep"] / 2.0


def _cloud(nb, seed=3):
    """nb shell_N_12 on a jittered grid above the wall (the dipole terms see the centres only; no other term is on, so the shells
    may interpenetrate)"""
    cfg, a = _shell12()
    rng = np.random.default_rng(seed)
    side = int(np.ceil(nb ** (1.0 / 3.0)))
    idx = np.arange(nb)
    X = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1) * 1.1 + rng.uniform(-0.35, 0.35, (nb, 3))
    X[:, 2] += R_SHELL + a + 0.5
    return {"cfg": cfg, "X": X, "Q": _quats(nb, seed + 1), "a": a, "eta": 1.0, "dt": 0.01}


def _square(gap=0.4, seed=6):
    """four shells on a square above the wall, surfaces `gap` apart (the steps: the shells do not touch)"""
    cfg, a = _shell12()
    d = 2.0 * R_SHELL + gap
    X = np.array([[0.0, 0.0, 0.0], [d, 0.05, 0.1], [0.05, d, -0.1], [d + 0.1, d - 0.05, 0.05]]) + [0.0, 0.0, R_SHELL + a + 0.3]
    return {"cfg": cfg, "X": X, "Q": _quats(4, seed), "a": a, "eta": 1.0, "dt": 0.01}


def _ctx(c, wall=True, kBT=1.0, dt=None):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"] if dt is None else dt, kBT=kBT,
                        stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    return ctx


def _radii(X, margin=1e-3):
    """r_core and r_cut in the gaps of the sorted pair distances (a tenth and six tenths of the way through them): pairs in all
    three regimes, none within `margin` of either radius.  margin = 1e-3 wherever the distances leave such gaps; the 132 355
    distances of the 515-body case lie 1e-4 apart on average, so there it is 1e-7: the device and numpy round a distance of
    order 10 to 2e-15, eight orders below, so both sides still put every pair into the same regime"""
    d = np.sort(mo.pair_distances(X))
    assert d.size >= 3

    def gap(k):
        while d[k] - d[k - 1] < 4 * margin:                # the next gap wide enough
            k += 1
        return k

    k1 = gap(max(int(0.1 * d.size), 1))
    k2 = gap(max(int(0.6 * d.size), k1 + 1))
    r_core, r_cut = 0.5 * (d[k1] + d[k1 - 1]), 0.5 * (d[k2] + d[k2 - 1])
    assert (d < r_core).any() and ((d > r_core) & (d < r_cut)).any() and (d > r_cut).any()
    assert np.abs(d - r_core).min() > margin and np.abs(d - r_cut).min() > margin
    return r_core, r_cut


FIELD = dict(B0=[0.3, -0.2, 0.5], B1=[1.0, 0.0, 0.4], B2=[0.0, 0.8, -0.1])


def _moments(nb, layout, seed=12):
    m = np.random.default_rng(seed).standard_normal((nb, 3))
    return m[0] if layout == "shared" else m


def _compare(ctx, c, m_body, c_dd, r_core, r_cut, B, label):
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    FTo, Eo, Eabs = mo.dipoles(c["X"], c["Q"], m_body, c_dd=c_dd, r_core=r_core, r_cut=r_cut, B=B, with_scale=True)
    FTo = FTo.reshape(-1)
    dF, dE = np.abs(FT - FTo).max() / np.abs(FTo).max(), abs(E - Eo) / Eabs
    print("  %-40s |FT|max %.3e E %.6e   dFT/|FT|max %.2e  dE/sum|terms| %.2e" % (label, np.abs(FTo).max(), Eo, dF, dE))
    assert not f.any()                                     # f_blob does not contain the body-level terms
    assert dF <= 1e-12
    assert dE <= 1e-12                                     # a sum of terms of both signs: relative to the sum of their magnitudes
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(FT, FT2) and ctx.interaction_energy() == E       # two calls: bitwise
    return FT, E


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("layout", ["shared", "per_body"])
@pytest.mark.parametrize("nb", [1, 2, 3, 65, 130, 515])
def test_forces_torques_and_energy_agree_with_the_all_pairs_oracle(nb, layout):
    """no partner, one partner, more partners than a wave has lanes (65) and than two passes cover (130), and a window of more
    than 512 bodies, which the four-wave instantiation of the kernel takes (515: three partners in its third pass); static
    field and omega t = 7.3; finite and infinite cutoff.  fp64 on both sides: 1e-12 of the largest entry."""
    c = _cloud(nb)
    m_body = _moments(nb, layout)
    ctx = _ctx(c)
    c_dd = 1.7
    if nb >= 3:
        cases = [_radii(c["X"], 1e-3 if nb <= 130 else 1e-7)]
    elif nb == 2:                                          # the one pair in each regime in turn
        d = mo.pair_distances(c["X"])[0]
        cases = [(1.5 * d, 2.0 * d), (0.5 * d, 2.0 * d), (0.25 * d, 0.5 * d)]
    else:
        cases = [(0.5, 2.0)]
    print("N_bod %d, moments %s" % (nb, layout))
    for r_core, r_cut in cases:
        for omega, t in ((0.0, 0.0), (2.0, 3.65)):
            B = mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], omega, t)
            ctx.set_magnetic_field(omega=omega, **FIELD)
            ctx.set_field_time(t)
            for cut in (r_cut, np.inf):
                ctx.set_dipoles(m_body, c_dd=c_dd, r_core=r_core, r_cut=cut)
                assert ctx.interactions_active() == 48
                _compare(ctx, c, m_body, c_dd, r_core, cut, B, "core %.3f cut %.3f omega t %.2f" % (r_core, cut, omega * t))
    # each term alone
    r_core, r_cut = cases[0]
    ctx.set_magnetic_field(None, None, None, on=False)
    if nb > 1:
        ctx.set_dipoles(m_body, c_dd=c_dd, r_core=r_core, r_cut=np.inf)
        assert ctx.interactions_active() == 16
        _compare(ctx, c, m_body, c_dd, r_core, np.inf, None, "pairs alone")
    ctx.set_magnetic_field(omega=2.0, **FIELD)
    ctx.set_dipoles(m_body)
    assert ctx.interactions_active() == 32
    _compare(ctx, c, m_body, 0.0, 1.0, np.inf, mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], 2.0, 3.65), "field alone")
    ctx.close()


def test_the_sums_add_with_the_builtin_terms_a_pair_table_and_traps():
    c = _square(gap=0.15)
    nb, nblb, a = 4, 12, c["a"]
    ctx = _ctx(c)
    import torch
    r = torch.empty(3 * nb * nblb, dtype=torch.float64, device="cuda:0")
    ctx.blob_positions(0, nb, r.data_ptr())
    ctx.sync_check()
    r = r.cpu().numpy().reshape(-1, 3)
    builtin = dict(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=2 * a + 1.0)
    x = np.linspace(0.6, 1.8, 65)
    pair = (np.exp(-x) - np.exp(-1.8), -np.exp(-x), 0.6, 1.8)
    traps = (np.tile([1.5, 0.0, 0.7], (nb, 1)), c["X"] + 0.2)
    ctx.set_interactions(**builtin)
    ctx.set_pair_table(*pair)
    ctx.set_traps(*traps)
    f0, FT0 = ctx.interaction_forces()
    fo, FTo, Eo, _ = table_oracle.interactions(r, c["X"], nblb, a, True, builtin=builtin, pair=pair, traps=traps)
    assert np.abs(FT0 - FTo).max() <= 1e-12 * np.abs(FTo).max()
    m_body = _moments(nb, "per_body")
    r_core, r_cut = _radii(c["X"])
    ctx.set_dipoles(m_body, c_dd=1.7, r_core=r_core, r_cut=r_cut)
    ctx.set_magnetic_field(omega=2.0, **FIELD)
    ctx.set_field_time(3.65)
    assert ctx.interactions_active() == 1 + 2 + 8 + 16 + 32
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    FTm, Em, Eabs = mo.dipoles(c["X"], c["Q"], m_body, c_dd=1.7, r_core=r_core, r_cut=r_cut,
                               B=mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], 2.0, 3.65), with_scale=True)
    tot = FTo + FTm.reshape(-1)
    assert np.abs(FTm).max() > 1e-2 * np.abs(FTo).max()      # the new terms are not lost beside the old ones
    print("all terms: dFT/|FT|max %.2e, dE %.2e" % (np.abs(FT - tot).max() / np.abs(tot).max(), abs(E - Eo - Em) / (abs(Eo) + Eabs)))
    assert np.array_equal(f, f0)                               # the blob forces are untouched
    assert np.abs(FT - tot).max() <= 1e-12 * np.abs(tot).max()
    assert abs(E - (Eo + Em)) <= 1e-12 * (abs(Eo) + Eabs)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 4
def test_generalised_forces_are_minus_the_energy_gradient_through_the_library():
    """every body displaced and rotated (dq(delta) Q) by +-h through set_config, every new term on.  h = 1e-6: truncation
    ~ h^2 |FT|, rounding ~ eps sum|terms| / h = 2e-10 sum|terms|; with sum|terms| <= 100 |FT|max (asserted) both stay below
    1e-7 |FT|max, the oracle's own bound in tests/test_magnetic_cpu.py"""
    c = _cloud(3, seed=9)
    m_body = _moments(3, "per_body")
    r_core, r_cut = _radii(c["X"])
    ctx = _ctx(c)
    ctx.set_dipoles(m_body, c_dd=1.7, r_core=r_core, r_cut=r_cut)
    ctx.set_magnetic_field(omega=2.0, **FIELD)
    ctx.set_field_time(3.65)
    assert ctx.interactions_active() == 48
    _, FT = ctx.interaction_forces()
    X0, Q0 = ctx.get_config(3)
    X0, Q0 = np.reshape(X0, (3, 3)).copy(), np.reshape(Q0, (3, 4)).copy()
    Eabs = mo.dipoles(X0, Q0, m_body, c_dd=1.7, r_core=r_core, r_cut=r_cut,
                      B=mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], 2.0, 3.65), with_scale=True)[2]
    assert Eabs <= 100 * np.abs(FT).max()
    h = 1e-6
    g = np.zeros((3, 6))
    for i in range(3):
        for k in range(6):
            E = []
            for s in (1.0, -1.0):
                X, Q = X0.copy(), Q0.copy()
                if k < 3:
                    X[i, k] += s * h
                else:
                    delta = np.zeros(3)
                    delta[k - 3] = s * h
                    Q[i] = mo.rotate(Q0[i], delta)
                ctx.set_config(X, Q)
                E.append(ctx.interaction_energy())
            g[i, k] = (E[0] - E[1]) / (2 * h)
    ctx.close()
    err = np.abs(FT + g.reshape(-1)).max() / np.abs(FT).max()
    print("generalised forces: |FT|max %.3e, worst relative difference %.2e" % (np.abs(FT).max(), err))
    assert err <= 1e-7


# ------------------------------------------------------------------------------------------------------------ 5
def _replicas(R=3, twins=False):
    c = _square()
    rng = np.random.default_rng(21)
    X = c["X"][None] + rng.uniform(-0.08, 0.08, (R, 4, 3))
    Q = np.stack([_quats(4, 30 + r) for r in range(R)])
    if twins:                                              # replicas 0 and 1 at identical coordinates
        X[1], Q[1] = X[0], Q[0]
    return c, X, Q


def _ens(c, X, Q, kBT=1.0, wall=True, dt=None):
    from rigid_body_light_amd import Ensemble
    return Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"] if dt is None else dt, kBT=kBT, wall=wall)


DIP = dict(c_dd=1.7, r_core=1.9, r_cut=2.75)              # among the square's sides (1.83 .. 2.08) and among its diagonals (2.65 .. 2.88)


@pytest.mark.parametrize("times", ["shared", "per_replica"])
@pytest.mark.parametrize("layout", ["shared", "per_body", "per_replica"])
def test_every_replica_is_bitwise_the_single_context(layout, times):
    R = 3
    c, X, Q = _replicas(R, twins=True)
    d = np.concatenate([mo.pair_distances(X[r]) for r in range(R)])
    assert (d > DIP["r_core"]).any() and (d < DIP["r_cut"]).any()
    rng = np.random.default_rng(5)
    m = {"shared": rng.standard_normal(3), "per_body": rng.standard_normal((4, 3)), "per_replica": rng.standard_normal((R, 4, 3))}[layout]
    if layout == "per_replica":
        m[1] = m[0]                                        # the twins carry the same moments
    t = 3.65 if times == "shared" else np.array([3.65, 3.65, -11.2])
    ens = _ens(c, X, Q)
    ens.set_dipoles(m, **DIP)
    ens.set_magnetic_field(omega=2.0, **FIELD)
    ens.set_field_time(t)
    FTe, Ee = ens.interaction_forces(), ens.interaction_energy()
    assert np.array_equal(ens.field_time(), np.atleast_1d(t))
    ens.close()
    assert np.array_equal(FTe[0], FTe[1]) and Ee[0] == Ee[1]           # twins at identical coordinates do not feel each other
    for rep in range(R):
        s = _ctx(dict(c, X=X[rep], Q=Q[rep]))
        s.set_dipoles(m[rep] if layout == "per_replica" else m, **DIP)
        s.set_magnetic_field(omega=2.0, **FIELD)
        tr = t if times == "shared" else t[rep]
        s.set_field_time(tr)
        _, FT = s.interaction_forces()
        E = s.interaction_energy()
        s.close()
        assert np.abs(FT).max() > 0.1
        assert np.array_equal(FTe[rep], -FT) and Ee[rep] == E           # reference convention: -K^T f_phys
        FTo, Eo = mo.dipoles(X[rep], Q[rep], m[rep] if layout == "per_replica" else m,
                             B=mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], 2.0, tr), **DIP)
        assert np.abs(FT - FTo.reshape(-1)).max() <= 1e-12 * np.abs(FTo).max()   # ... so the two cannot be wrong together


def test_an_ensemble_refuses_moments_or_times_of_another_length():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = _replicas(3)
    ens = _ens(c, X, Q)
    ens.set_dipoles(np.ones(3), **DIP)
    ens.set_magnetic_field(omega=2.0, **FIELD)
    ens.interaction_forces()
    ens.ctx.set_dipoles(np.ones((2, 3)), **DIP)               # neither 1, N_bod = 4 nor R N_bod = 12 entries
    with pytest.raises(RblError, match="status 7"):            # RBL_ERR_STATE
        ens.interaction_forces()
    with pytest.raises(RblError, match="status 7"):
        ens.step_deterministic(np.zeros(24))
    ens.set_dipoles(np.ones(3), **DIP)
    ens.ctx.set_field_time([0.1, 0.2])                         # neither 1 nor R = 3 entries
    with pytest.raises(RblError, match="status 7"):
        ens.interaction_forces()
    with pytest.raises(RblError, match="status 7"):
        ens.step_deterministic(np.zeros(24))
    assert np.array_equal(ens.get_config()[0], X)              # nothing moved
    ens.set_field_time(0.1)
    ens.step_deterministic(np.zeros(24))
    ens.close()


# ------------------------------------------------------------------------------------------------------------ 6
def _switch_on(obj, m_body, t=3.65):
    obj.set_dipoles(m_body, **DIP)
    obj.set_magnetic_field(omega=2.0, **FIELD)
    obj.set_field_time(t)


def test_a_deterministic_step_adds_the_new_terms_at_qn():
    c = _square()
    m_body = 2.0 * _moments(4, "per_body")
    ctx = _ctx(c)
    _switch_on(ctx, m_body)
    assert ctx.interactions_active() == 48
    _, FT = ctx.interaction_forces()
    assert np.abs(FT).max() > 0.1
    ctx.step_deterministic(np.zeros(24), max_iter=80, rtol=1e-12)
    Xa, Qa = ctx.get_config(4)
    assert ctx.field_time()[0] == 3.65                         # no step advances the clock
    ctx.close()
    ref = _ctx(c)                                              # the terms off, the caller passing -FT (reference convention)
    ref.step_deterministic(-FT, max_iter=80, rtol=1e-12)
    Xb, Qb = ref.get_config(4)
    ref.close()
    assert np.abs(np.reshape(Qa, (4, 4)) - c["Q"]).max() > 1e-5
    assert np.abs(Xa - Xb).max() <= 1e-12 and np.abs(Qa - Qb).max() <= 1e-12


def test_only_the_free_slots_of_a_mask_feel_the_new_terms():
    from rigid_body_light_amd import RigidBody
    c = _square()
    m_body = 2.0 * _moments(4, "per_body")
    mask = np.array([True, False, False, False])
    out = []
    for with_model in (True, False):
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True)
        body_in = np.zeros(24)
        Xs, Qs = (np.array(v) for v in rb.get_config())
        if with_model:
            _switch_on(rb, m_body)
            assert rb.dipoles()["on"] and rb.magnetic_field()["on"] and rb.field_time() == 3.65
            loads = rb.interaction_forces()                    # reference convention, -K^T f_phys
            assert np.abs(loads[:6]).max() > 0.1 and np.abs(loads[6:]).max() > 0.1
        else:
            body_in[6:] = loads[6:]
        rb.step_mixed(mask, body_in, max_iter=100, rtol=1e-12)
        out.append(rb.get_config())
    X0, Q0 = out[0]
    assert np.array_equal(X0[0], Xs[0]) and np.array_equal(Q0[0], Qs[0])              # the held body stays, torque or not
    assert np.abs(Q0[1:] - Qs[1:]).max() > 1e-5
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-12 and np.abs(out[0][1] - out[1][1]).max() <= 1e-12


@pytest.mark.parametrize("kind", ["deterministic", "brownian"])
def test_switched_off_the_new_terms_leave_no_trace(kind):
    c = _square()
    out = []
    for had in (True, False):
        ctx = _ctx(c, kBT=0.1)
        if had:                                                # on, evaluated, off again
            _switch_on(ctx, _moments(4, "per_body"))
            assert np.abs(ctx.interaction_forces()[1]).max() > 0.0
            ctx.set_dipoles(None, on=False)
            ctx.set_magnetic_field(None, None, None, on=False)
            assert not ctx.interactions_on()
        F = np.tile([0.0, 0.0, 0.3, 0.0, 0.0, 0.0], 4)
        if kind == "deterministic":
            ctx.step_deterministic(F, max_iter=50, rtol=1e-10)
        else:
            ctx.step_brownian(F, max_iter=50, rtol=1e-10, seed=3, method=2)
        out.append(ctx.get_config(4))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------------------ 7
T0, OMEGA = 0.37, 30.0                                       # omega dt = 0.3 per step, |omega t| <= 13


def _driven(c, X, Q, omega=OMEGA, t0=T0):
    ens = _ens(c, X, Q)
    ens.set_dipoles(3.0 * _moments(4, "per_body"), **DIP)
    ens.set_magnetic_field(B1=[2.0, 0.0, 0.0], B2=[0.0, 0.0, 2.0], omega=omega)
    ens.set_field_time(t0)
    return ens


@pytest.mark.parametrize("family", ["deterministic", "brownian"])
def test_a_run_with_a_rotating_field_is_the_loop_bitwise(family):
    R, steps = 3, 5
    c, X, Q = _replicas(R)
    F = 0.2 * np.random.default_rng(11).standard_normal((R, 24))
    kw = dict(max_iter=50, rtol=1e-8)
    ens = _driven(c, X, Q)
    for n in range(steps):
        ens.set_field_time(T0 + c["dt"] * n)
        if family == "brownian":
            ens.step_brownian(F, seed=40 + n, **kw)
        else:
            ens.step_deterministic(F, **kw)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = _driven(c, X, Q)
    out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, stride=5, **kw)
    Xr, Qr = ens.get_config()
    assert np.array_equal(ens.field_time(), [T0])              # the run leaves the context's field time as it was
    ens.close()
    assert np.array_equal(out.accepted, np.full(R, steps))
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)
    assert np.array_equal(out.X[0], Xl) and np.array_equal(out.Q[0], Ql)
    still = _driven(c, X, Q, omega=0.0)                        # ... and not the run in a field that stands still
    still.run(steps, F=F, brownian=family == "brownian", seed=40, **kw)
    assert not np.array_equal(still.get_config()[1], Qr)
    still.close()


@pytest.mark.parametrize("family", ["deterministic", "brownian"])
def test_under_reject_the_field_waits_for_a_rejected_replica(family):
    """replica 2 starts with a body below the wall: every one of its steps is refused (an ordinary refusal), its counter stays 0
    and its configuration unchanged; the others equal the loop beside a harmless replica 2 (the noise depends on the replica's
    index and the step only)"""
    R, steps = 3, 5
    c, X, Q = _replicas(R)
    Xbad = X.copy()
    Xbad[2, 0, 2] = -0.5
    F = 0.2 * np.random.default_rng(11).standard_normal((R, 24))
    kw = dict(max_iter=50, rtol=1e-8)
    ens = _driven(c, X, Q)
    for n in range(steps):
        ens.set_field_time(T0 + c["dt"] * n)
        if family == "brownian":
            ens.step_brownian(F, seed=40 + n, **kw)
        else:
            ens.step_deterministic(F, **kw)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = _driven(c, Xbad, Q)
    Xa, Qa = ens.get_config()
    out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, on_error="reject", **kw)
    Xe, Qe = ens.get_config()
    ens.close()
    assert out.accepted.tolist() == [steps, steps, 0] and out.rejected.tolist() == [0, 0, steps]
    assert np.array_equal(Xe[2], Xa[2]) and np.array_equal(Qe[2], Qa[2])
    assert np.array_equal(Xe[:2], Xl[:2]) and np.array_equal(Qe[:2], Ql[:2])


def test_a_run_with_a_clock_per_replica_is_the_loop_bitwise():
    R, steps = 3, 4
    c, X, Q = _replicas(R)
    t0 = np.array([0.37, -0.2, 1.05])
    F = np.zeros((R, 24))
    ens = _driven(c, X, Q)
    for n in range(steps):
        ens.set_field_time(t0 + c["dt"] * n)
        ens.step_deterministic(F)
    Xl, Ql = ens.get_config()
    ens.set_config(X, Q)
    ens.set_field_time(t0)
    ens.run(steps, F=F, brownian=False)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)


# ------------------------------------------------------------------------------------------------------------ 8
@functools.lru_cache(maxsize=None)
def _free_shell_mu_rr():
    """rotational mobility about y of one shell_N_12 in free space, from body_mobility_matrix"""
    from rigid_body_light_amd import RigidBody
    cfg, a = _shell12()
    rb = RigidBody(cfg, np.array([[0.0, 0.0, 50.0]]), np.array([[1.0, 0.0, 0.0, 0.0]]), a, 1.0, 0.01, wall_PC=False)
    N, _ = rb.body_mobility_matrix(rtol=1e-12)
    return float(N[4, 4])


def _winding(ratio):
    """turns of the moment about y over 8 periods of a field of strength |B| = 1 rotating in the (x, z) plane at omega = ratio *
    omega_c, |m| = 1, kBT = 0; omega dt = 0.02"""
    cfg, a = _shell12()
    mu = _free_shell_mu_rr()
    omega = ratio * mu                                         # omega_c = |m| |B| mu_rr
    dt = 0.02 / omega
    steps = int(np.ceil(8 * 2 * np.pi / 0.02))
    m_body = np.array([1.0, 0.0, 0.0])
    X, Q = np.array([[[0.0, 0.0, 50.0]]]), np.array([[[1.0, 0.0, 0.0, 0.0]]])
    ens = _ens({"cfg": cfg, "a": a, "eta": 1.0, "dt": dt}, X, Q, kBT=0.0, wall=False)
    ens.set_dipoles(m_body)
    ens.set_magnetic_field(B1=[1.0, 0.0, 0.0], B2=[0.0, 0.0, 1.0], omega=omega)
    out = ens.run(steps, F=np.zeros(6), brownian=False, stride=6, rtol=1e-10)
    ens.close()
    assert np.array_equal(out.accepted, [steps])
    m = np.stack([mo.rot(q) @ m_body for q in out.Q[:, 0, 0]])
    assert np.abs(m[:, 1]).max() < 1e-6                         # the moment stays perpendicular to the axis
    ang = np.unwrap(np.concatenate([[0.0], np.arctan2(m[:, 2], m[:, 0])]))   # 0.12 rad of field per frame: no aliasing
    return int(np.round(ang[-1] / (2 * np.pi)))


def test_synchronous_rotation_below_the_critical_frequency_and_step_out_above():
    assert _winding(0.5) == 8
    assert _winding(2.0) < 8


# ------------------------------------------------------------------------------------------------------------ 9
def test_langevin_orientation_statistics_in_a_static_field():
    """R = 256 single shell_N_12 in free space at z = 50 (far above z = a, see test_equipartition_in_a_harmonic_trap), kBT = 1,
    static field along z with xi = |m| |B| / kBT = 2, dt from |m| |B| mu_rr dt = 0.02.  500 steps of burn-in (ten relaxation
    times 1 / (2 kBT mu_rr) = 50 steps), then 1500 steps with a frame every 50.  <cos theta> against coth xi - 1 / xi = 0.5373
    within 4 SE + |m| |B| mu_rr dt: SE from the spread of the per-replica means (SE <= 0.02 asserted), the allowance twice the
    forward-Euler bias of the linearised restoring torque.  A torque of the wrong sign lands near -0.54."""
    cfg, a = _shell12()
    R, xi, kBT = 256, 2.0, 1.0
    mu = _free_shell_mu_rr()
    dt = 0.02 / (xi * kBT * mu)
    X = np.tile([0.3, -0.4, 50.0], (R, 1, 1))
    Q = _quats(R, 17).reshape(R, 1, 4)
    m_body = np.array([0.0, 0.6, 0.8])
    ens = _ens({"cfg": cfg, "a": a, "eta": 1.0, "dt": dt}, X, Q, kBT=kBT, wall=False)
    ens.set_dipoles(m_body)
    ens.set_magnetic_field(B0=[0.0, 0.0, xi * kBT])
    ens.run(500, F=np.zeros(6), seed=1000, max_iter=50, rtol=1e-8)
    out = ens.run(1500, F=np.zeros(6), seed=5000, stride=50, max_iter=50, rtol=1e-8)
    ens.close()
    assert out.Q.shape == (30, R, 1, 4) and np.array_equal(out.accepted, np.full(R, 1500))
    q = out.Q[:, :, 0, :]
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    cos = 2 * (y * z + w * x) * m_body[1] + (1 - 2 * (x * x + y * y)) * m_body[2]      # third row of R(Q) times m_body, |m| = 1
    per_rep = cos.mean(axis=0)
    v, se = per_rep.mean(), per_rep.std(ddof=1) / np.sqrt(R)
    want = 1.0 / np.tanh(xi) - 1.0 / xi
    print("<cos theta> %.4f, Langevin %.4f, SE %.4f, allowance %.4f" % (v, want, se, 4 * se + 0.02))
    assert se <= 0.02
    assert abs(v - want) <= 4 * se + xi * kBT * mu * dt


# ------------------------------------------------------------------------------------------------------------ 10
def test_example_magnetic_rollers_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "magnetic_rollers.py"), "--replicas", "16", "--steps", "40"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "rolling velocity" in out.stdout and "omega" in out.stdout
