"""Bonds and tethers of include/rbl.h section 4 on the GPU: forces, torques, energy and bond state against the numpy oracle
(tests/bond_oracle.py) for every count of bond ends on one body at which the kernel takes another path, the sum with every other
term of the model, generalised forces against the library's own energy, ensembles against single contexts bitwise, the term
inside the steps and the runs, a relaxing dumbbell, equipartition of a tethered bead, the example."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import body_shapes  # noqa: E402
import bond_oracle as bo  # noqa: E402
import magnetic_oracle as mo  # noqa: E402
import table_oracle  # noqa: E402

R_SHELL = 0.79207921                                       # largest blob distance from the centre of shell_N_12


# ------------------------------------------------------------------------------------------------------------ shapes
def _quats(n, seed):
    Q = np.random.default_rng(seed).standard_normal((n, 4))
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _structure(name):
    if name == "shell12":
        from rigid_body_light_amd import load_structure
        p, cfg = load_structure(12)
        return cfg, p["sep"] / 2.0
    return body_shapes.shape(name), body_shapes.A


def _ctx(c, wall=True, kBT=1.0, dt=None):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"] if dt is None else dt, kBT=kBT,
                        stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    return ctx


def bond_tab(lo=1.2, hi=2.4, n=65):
    """T(d) = 4 + d^2 / 2 + sin(3 d) / 10 on lo .. hi: positive and increasing over every length the tests use, its tangents
    included, so that no energy or tension is the small difference of large terms; not a cubic, so the interpolant is not exact"""
    x = np.linspace(lo, hi, n)
    return (4.0 + 0.5 * x * x + 0.1 * np.sin(3.0 * x), x + 0.3 * np.cos(3.0 * x), lo, hi)


def _cloud(structure, nb, seed=3):
    """nb bodies on a jittered grid above the wall (only the bonds are on, so the bodies may interpenetrate).  Bodies 0 and 1 have
    identity orientations and centres made of short binary fractions: anchors can name one point in the same doubles"""
    cfg, a = _structure(structure)
    rng = np.random.default_rng(seed)
    side = int(np.ceil(nb ** (1.0 / 3.0)))
    idx = np.arange(nb)
    X = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1) * 1.1 + rng.uniform(-0.35, 0.35, (nb, 3))
    X[:, 2] += 3.0
    Q = _quats(nb, seed + 1)
    X[0], Q[0] = [0.5, 0.25, 3.0], [1.0, 0.0, 0.0, 0.0]
    if nb > 1:
        X[1], Q[1] = [1.5, 0.75, 3.25], [1.0, 0.0, 0.0, 0.0]
    return {"cfg": cfg, "X": X, "Q": Q, "a": a, "eta": 1.0, "dt": 0.01}


def _hub(c, nbb, ends, seed=7):
    """bonds that put `ends` bond ends on body 0, the hub, of the first nbb bodies of c: one bond to each of the other nbb - 1
    bodies (every other one stored with the larger index first), then tethers of the hub: a random one, one of length exactly 0
    (tabulated), and with nbb > 1 a body-body bond of length exactly 0 (harmonic, l0 > 0: a tension and still no force), then
    random tethers.  Kinds alternate, the first bond is tabulated.  -> body, anchor, kind, k, l0"""
    rng = np.random.default_rng(seed + 100 * nbb + ends)
    body, anchor, kind = [], [], []

    def add(i, j, sA, sB, kd=None):
        body.append([i, j]); anchor.append(list(sA) + list(sB)); kind.append((len(kind) + 1) % 2 if kd is None else kd)

    for j in range(1, nbb):
        if len(body) == ends:
            break
        sA, sB = 0.3 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)
        if j % 2:
            add(j, 0, sB, sA)
        else:
            add(0, j, sA, sB)
    if len(body) < ends:
        add(0, -1, 0.3 * rng.standard_normal(3), c["X"][0] + rng.uniform(-2.0, 2.0, 3))
    if len(body) < ends:                                       # X_0 + s_A = P, every coordinate a short binary fraction
        add(0, -1, [0.25, 0.5, 0.125], [0.75, 0.75, 3.125], kd=1)
    if len(body) < ends and nbb > 1:                           # X_0 + s_A = X_1 + s_B = (1, 0.5, 3.125)
        add(0, 1, [0.5, 0.25, 0.125], [-0.5, -0.25, -0.125], kd=0)
    while len(body) < ends:
        add(0, -1, 0.3 * rng.standard_normal(3), c["X"][0] + rng.uniform(-2.0, 2.0, 3))
    n = len(body)
    assert sum(1 for b in body if 0 in b) == ends
    return (np.array(body), np.array(anchor), np.array(kind), rng.uniform(0.5, 2.5, n), rng.uniform(0.05, 0.25, n))


def _lengths(c, body, anchor):
    return np.array([np.linalg.norm(np.subtract(*bo.end_points(c["X"], c["Q"], body, anchor, b)[2:])) for b in range(len(body))])


def _tables(c, body, anchor, kind):
    """the grids to evaluate with: the fixed one when the tabulated bonds reach below it, into it and beyond it (asserted, none
    within 1e-6 of either end: both sides round a length to 1e-15); for fewer than three tabulated bonds three grids that put the
    first of them into each regime in turn"""
    d = _lengths(c, body, anchor)[kind == 1]
    if d.size < 3:
        d0 = d[0] if d.size else 1.0
        return [bond_tab(1.5 * d0, 2.0 * d0), bond_tab(0.5 * d0, 2.0 * d0), bond_tab(0.25 * d0, 0.5 * d0)]
    t = bond_tab()
    assert (d < t[2]).any() and ((d > t[2]) & (d < t[3])).any() and (d > t[3]).any()
    assert min(np.abs(d - t[2]).min(), np.abs(d - t[3]).min()) > 1e-6
    return [t]


def _rel(got, want):
    """largest relative difference, entry by entry; where the oracle has an exact zero the library must have one too"""
    got, want = np.asarray(got), np.asarray(want)
    zero = want == 0.0
    assert np.array_equal(got[zero], want[zero])
    return float((np.abs(got - want)[~zero] / np.abs(want)[~zero]).max()) if (~zero).any() else 0.0


def _compare(ctx, c, body, anchor, kind, k, l0, table, label):
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    FTo, Eo, state, Eabs = bo.bonds(c["X"], c["Q"], body, anchor, k, l0, kind=kind, table=table, with_scale=True)
    FTo = FTo.reshape(-1)
    dF, dE = np.abs(FT - FTo).max() / np.abs(FTo).max(), abs(E - Eo) / Eabs
    got = ctx.bond_state()
    dS = [_rel(got[q], state[q]) for q in range(3)]
    print("  %-34s |FT|max %.3e E %.6e   dFT/|FT|max %.2e  dE/sum|terms| %.2e  state %.1e %.1e %.1e"
          % (label, np.abs(FTo).max(), Eo, dF, dE, dS[0], dS[1], dS[2]))
    assert not f.any()                                     # f_blob does not contain the body-level terms
    assert dF <= 1e-12
    assert dE <= 1e-12
    assert max(dS) <= 1e-13                                # each a single chain of fp64 operations
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(FT, FT2) and ctx.interaction_energy() == E       # two calls: bitwise
    got2 = ctx.bond_state()
    assert all(np.array_equal(got[q], got2[q]) for q in range(3))
    return FT


# ------------------------------------------------------------------------------------------------------------ 1
# nb: [(bodies that carry bonds, ends on the hub)]
HUB_CASES = {1: [(1, 1), (1, 63), (1, 64), (1, 65), (1, 130)], 2: [(2, 1), (2, 65), (1, 63)], 3: [(3, 64), (3, 130), (2, 65)],
             66: [(66, 65), (66, 130)]}


@pytest.mark.parametrize("structure", ["shell12", "bipyramid"])
@pytest.mark.parametrize("nb", [1, 2, 3, 66])
def test_forces_torques_energy_and_state_agree_with_the_oracle(nb, structure):
    """ends on one body: 0 (a body no bond names: nbb < nb), 1 (one lane), 63, 64 (a full wave), 65 (the first lane of the second
    pass) and 130 (a tail in the third pass); bonds stored with the larger index first, both kinds, tabulated bonds below, inside
    and beyond the grid, two bonds of length exactly 0.  fp64 on both sides: 1e-12 of the largest entry / of the sum of |terms|"""
    c = _cloud(structure, nb)
    ctx = _ctx(c)
    print("N_bod %d, %s (N_blb %d)" % (nb, structure, len(c["cfg"])))
    for nbb, ends in HUB_CASES[nb]:
        body, anchor, kind, k, l0 = _hub(c, nbb, ends)
        if (body[:, 1] >= 0).sum() > 1:
            assert (body[:, 0] > body[:, 1]).any() and (body[body[:, 1] >= 0][:, 0] < body[body[:, 1] >= 0][:, 1]).any()
        if ends > nbb:                                     # the two bonds of length exactly 0 are there, one of them tabulated
            d = _lengths(c, body, anchor)
            assert (d[kind == 1] == 0.0).any() and (nbb == 1 or (d[kind == 0] == 0.0).any())
        ctx.set_bonds(body, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
        for table in _tables(c, body, anchor, kind):
            ctx.set_bond_table(*table)
            assert ctx.interactions_active() == 64
            FT = _compare(ctx, c, body, anchor, kind, k, l0, table, "%d bonded, %d ends, grid %.2f..%.2f" % (nbb, ends, table[2], table[3]))
            if nbb < nb:                                   # no bond names the last body: nothing at all is added to it
                assert np.array_equal(FT[6 * nbb:], np.zeros(6 * (nb - nbb)))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 2
def _square(gap=0.4, seed=6):
    """four shells on a square above the wall, surfaces `gap` apart (the steps: the shells do not touch)"""
    cfg, a = _structure("shell12")
    d = 2.0 * R_SHELL + gap
    X = np.array([[0.0, 0.0, 0.0], [d, 0.05, 0.1], [0.05, d, -0.1], [d + 0.1, d - 0.05, 0.05]]) + [0.0, 0.0, R_SHELL + a + 0.3]
    return {"cfg": cfg, "X": X, "Q": _quats(4, seed), "a": a, "eta": 1.0, "dt": 0.01}


def _ring(c, scale=1.0):
    """five bonds on the square: three sides blob to blob (one stored with the larger index first), a tabulated diagonal between
    the centres and a tether of body 3's blob 5 to a point above it.  The sides' lengths fall inside the fixed grid's reach or
    beyond it, the diagonal beyond it"""
    from rigid_body_light_amd._lib import blob_anchor
    s = [blob_anchor(c["cfg"], q) for q in range(12)]
    body = np.array([[0, 1], [3, 1], [2, 3], [0, 3], [3, -1]])
    anchor = np.array([np.concatenate(v) for v in ((s[0], s[7]), (s[2], s[4]), (s[9], s[1]), (np.zeros(3), np.zeros(3)),
                                                   (s[5], c["X"][3] + [0.2, -0.3, 1.4]))])
    kind = np.array([0, 1, 0, 1, 0])
    k = scale * np.array([3.0, 1.5, 2.0, 0.8, 2.5])
    l0 = np.array([0.6, 0.0, 0.3, 0.0, 0.4])
    return body, anchor, kind, k, l0


def _set_ring(obj, c, scale=1.0):
    body, anchor, kind, k, l0 = _ring(c, scale)
    obj.set_bond_table(*bond_tab())
    obj.set_bonds(body, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
    return body, anchor, kind, k, l0


FIELD = dict(B0=[0.3, -0.2, 0.5], B1=[1.0, 0.0, 0.4], B2=[0.0, 0.8, -0.1])


def test_the_sums_add_with_every_other_term_of_the_model():
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
    m_body = np.random.default_rng(12).standard_normal((nb, 3))
    dip = dict(c_dd=1.7, r_core=1.9, r_cut=2.75)
    ctx.set_interactions(**builtin)
    ctx.set_pair_table(*pair)
    ctx.set_traps(*traps)
    ctx.set_dipoles(m_body, **dip)
    ctx.set_magnetic_field(omega=2.0, **FIELD)
    ctx.set_field_time(3.65)
    assert ctx.interactions_active() == 1 + 2 + 8 + 16 + 32
    f0, FT0 = ctx.interaction_forces()
    fo, FTo, Eo, _ = table_oracle.interactions(r, c["X"], nblb, a, True, builtin=builtin, pair=pair, traps=traps)
    FTm, Em, Eabs_m = mo.dipoles(c["X"], c["Q"], m_body, B=mo.field(FIELD["B0"], FIELD["B1"], FIELD["B2"], 2.0, 3.65), with_scale=True, **dip)
    rest = FTo + FTm.reshape(-1)
    assert np.abs(FT0 - rest).max() <= 1e-12 * np.abs(rest).max()
    body, anchor, kind, k, l0 = _set_ring(ctx, c)
    assert ctx.interactions_active() == 1 + 2 + 8 + 16 + 32 + 64
    assert np.array_equal(ctx.blob_anchor(7), anchor[0, 3:])
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    FTb, Eb, _, Eabs_b = bo.bonds(c["X"], c["Q"], body, anchor, k, l0, kind=kind, table=bond_tab(), with_scale=True)
    tot = rest + FTb.reshape(-1)
    assert np.abs(FTb).max() > 1e-2 * np.abs(rest).max()       # the bonds are not lost beside the other terms
    print("all terms: dFT/|FT|max %.2e, dE %.2e" % (np.abs(FT - tot).max() / np.abs(tot).max(),
                                                    abs(E - Eo - Em - Eb) / (abs(Eo) + Eabs_m + Eabs_b)))
    assert np.array_equal(f, f0)                               # the blob forces are untouched
    assert np.abs(FT - tot).max() <= 1e-12 * np.abs(tot).max()
    assert abs(E - (Eo + Em + Eb)) <= 1e-12 * (abs(Eo) + Eabs_m + Eabs_b)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 3
def test_generalised_forces_are_minus_the_energy_gradient_through_the_library():
    """every body displaced and rotated (dq(delta) Q) by +-h through set_config, only the bonds on.  h = 1e-6: truncation
    ~ h^2 |FT|, rounding ~ eps sum|terms| / h = 2e-10 sum|terms|; with sum|terms| <= 100 |FT|max (asserted) both stay below
    1e-7 |FT|max, the oracle's own bound in tests/test_bonds_cpu.py"""
    c = _square()
    ctx = _ctx(c)
    body, anchor, kind, k, l0 = _set_ring(ctx, c)
    d = _lengths(c, body, anchor)[kind == 1]
    lo, hi = bond_tab()[2:]
    assert ((d > lo) & (d < hi)).any() and (d > hi).any()       # a tabulated bond inside the grid and one on the upper tangent
    assert ctx.interactions_active() == 64
    _, FT = ctx.interaction_forces()
    X0, Q0 = ctx.get_config(4)
    X0, Q0 = np.reshape(X0, (4, 3)).copy(), np.reshape(Q0, (4, 4)).copy()
    Eabs = bo.bonds(X0, Q0, body, anchor, k, l0, kind=kind, table=bond_tab(), with_scale=True)[3]
    assert Eabs <= 100 * np.abs(FT).max()
    h = 1e-6
    g = np.zeros((4, 6))
    for i in range(4):
        for q in range(6):
            E = []
            for s in (1.0, -1.0):
                X, Q = X0.copy(), Q0.copy()
                if q < 3:
                    X[i, q] += s * h
                else:
                    delta = np.zeros(3)
                    delta[q - 3] = s * h
                    Q[i] = mo.rotate(Q0[i], delta)
                ctx.set_config(X, Q)
                E.append(ctx.interaction_energy())
            g[i, q] = (E[0] - E[1]) / (2 * h)
    ctx.close()
    err = np.abs(FT + g.reshape(-1)).max() / np.abs(FT).max()
    print("generalised forces: |FT|max %.3e, worst relative difference %.2e" % (np.abs(FT).max(), err))
    assert err <= 1e-7


# ------------------------------------------------------------------------------------------------------------ 4
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


@pytest.mark.parametrize("sets", ["one", "per_replica"])
def test_every_replica_is_bitwise_the_single_context(sets):
    R = 3
    c, X, Q = _replicas(R, twins=True)
    body, anchor, kind, k, l0 = _ring(c)
    if sets == "per_replica":                              # a stiffness and rest-length sweep; the twins share their values
        k = k[None] * np.array([1.0, 1.0, 1.7])[:, None]
        l0 = l0[None] + np.array([0.0, 0.0, 0.1])[:, None]
    ens = _ens(c, X, Q)
    ens.set_bond_table(*bond_tab())
    ens.set_bonds(body, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
    assert ens.ctx.interactions_active() == 64
    FTe, Ee, Se = ens.interaction_forces(), ens.interaction_energy(), ens.bond_state()
    assert all(s.shape == (R, 5) for s in Se)
    ens.close()
    assert np.array_equal(FTe[0], FTe[1]) and Ee[0] == Ee[1]   # twins at identical coordinates do not feel each other
    for rep in range(R):
        kr, lr = (k[rep], l0[rep]) if sets == "per_replica" else (k, l0)
        s = _ctx(dict(c, X=X[rep], Q=Q[rep]))
        s.set_bond_table(*bond_tab())
        s.set_bonds(body, anchor[:, :3], anchor[:, 3:], kr, lr, kind=kind)
        _, FT = s.interaction_forces()
        E = s.interaction_energy()
        S = s.bond_state()
        s.close()
        assert np.abs(FT).max() > 0.1
        assert np.array_equal(FTe[rep], -FT) and Ee[rep] == E           # reference convention: -K^T f_phys
        assert all(np.array_equal(Se[q][rep], S[q]) for q in range(3))
        FTo = bo.bonds(X[rep], Q[rep], body, anchor, kr, lr, kind=kind, table=bond_tab())[0]
        assert np.abs(FT - FTo.reshape(-1)).max() <= 1e-12 * np.abs(FTo).max()   # ... so the two cannot be wrong together


def test_an_ensemble_refuses_another_set_count_and_a_body_index_beyond_the_system():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = _replicas(3)
    body, anchor, kind, k, l0 = _ring(c)
    ens = _ens(c, X, Q)
    _set_ring(ens, c)
    ens.interaction_forces()
    ens.ctx.set_bonds(body, anchor[:, :3], anchor[:, 3:], np.tile(k, (2, 1)), l0, kind=kind)   # neither 1 nor R = 3 sets
    for call in (ens.interaction_forces, ens.bond_state, lambda: ens.step_deterministic(np.zeros(24))):
        with pytest.raises(RblError, match="status 7"):        # RBL_ERR_STATE
            call()
    far = body.copy()
    far[2] = [2, 4]                                            # N_bod = 4
    ens.set_bonds(far, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
    for call in (ens.interaction_forces, ens.bond_state, lambda: ens.step_deterministic(np.zeros(24))):
        with pytest.raises(RblError, match=r"bond 2 .*status 7"):
            call()
    assert np.array_equal(ens.get_config()[0], X)              # nothing moved
    ens.set_bond_table(None, None, 0.0, 0.0, on=False)         # a tabulated bond and no table that is on
    ens.set_bonds(body, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
    with pytest.raises(RblError, match=r"bond 1 .*status 7"):
        ens.interaction_forces()
    _set_ring(ens, c)
    ens.step_deterministic(np.zeros(24))
    ens.close()
    s = _ctx(c)                                                # the single context names the bond too
    s.set_bond_table(*bond_tab())
    s.set_bonds(far, anchor[:, :3], anchor[:, 3:], k, l0, kind=kind)
    for call in (s.interaction_forces, s.bond_state, lambda: s.step_deterministic(np.zeros(24), max_iter=50, rtol=1e-8)):
        with pytest.raises(RblError, match=r"bond 2 .*status 7"):
            call()
    s.close()


# ------------------------------------------------------------------------------------------------------------ 5
def test_a_deterministic_step_adds_the_bonds_at_qn():
    c = _square()
    ctx = _ctx(c)
    _set_ring(ctx, c)
    assert ctx.interactions_active() == 64
    _, FT = ctx.interaction_forces()
    assert np.abs(FT).max() > 0.1
    ctx.step_deterministic(np.zeros(24), max_iter=80, rtol=1e-12)
    Xa, Qa = ctx.get_config(4)
    ctx.close()
    ref = _ctx(c)                                              # the term off, the caller passing -FT (reference convention)
    ref.step_deterministic(-FT, max_iter=80, rtol=1e-12)
    Xb, Qb = ref.get_config(4)
    ref.close()
    assert np.abs(np.reshape(Xa, (4, 3)) - c["X"]).max() > 1e-5
    assert np.abs(Xa - Xb).max() <= 1e-12 and np.abs(Qa - Qb).max() <= 1e-12


def test_only_the_free_slots_of_a_mask_feel_the_bonds():
    from rigid_body_light_amd import RigidBody
    c = _square()
    mask = np.array([True, False, False, False])
    out = []
    for with_model in (True, False):
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True)
        body_in = np.zeros(24)
        Xs, Qs = (np.array(v) for v in rb.get_config())
        if with_model:
            body, anchor, kind, k, l0 = _set_ring(rb, c)
            assert rb.ctx.interactions_active() == 64
            assert np.array_equal(rb.blob_anchor(4), anchor[1, 3:])
            loads = rb.interaction_forces()                    # reference convention, -K^T f_phys
            assert np.abs(loads[:6]).max() > 0.1 and np.abs(loads[6:]).max() > 0.1
            state = rb.bond_state()
            want = bo.bonds(c["X"], c["Q"], body, anchor, k, l0, kind=kind, table=bond_tab())[2]
            assert all(np.allclose(state[q], want[q], rtol=1e-13, atol=0.0) for q in range(3))
        else:
            body_in[6:] = loads[6:]
        rb.step_mixed(mask, body_in, max_iter=100, rtol=1e-12)
        out.append(rb.get_config())
    X0, Q0 = out[0]
    assert np.array_equal(X0[0], Xs[0]) and np.array_equal(Q0[0], Qs[0])              # the held body stays, bonded or not
    assert np.abs(X0[1:] - Xs[1:]).max() > 1e-5
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-12 and np.abs(out[0][1] - out[1][1]).max() <= 1e-12


@pytest.mark.parametrize("family", ["deterministic", "brownian"])
def test_switched_off_the_bonds_leave_no_trace(family):
    c = _square()
    out = []
    for had in (True, False):
        ctx = _ctx(c, kBT=0.1)
        if had:                                                # on, evaluated, off again
            _set_ring(ctx, c)
            assert np.abs(ctx.interaction_forces()[1]).max() > 0.0
            ctx.set_bonds(None, None, None, None, on=False)
            assert not ctx.interactions_on() and ctx.bonds()["body"].shape == (5, 2)
        F = np.tile([0.0, 0.0, 0.3, 0.0, 0.0, 0.0], 4)
        if family == "deterministic":
            ctx.step_deterministic(F, max_iter=50, rtol=1e-10)
        else:
            ctx.step_brownian(F, max_iter=50, rtol=1e-10, seed=3, method=2)
        out.append(ctx.get_config(4))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("family", ["deterministic", "brownian"])
def test_a_run_with_bonds_is_the_loop_bitwise(family):
    R, steps = 3, 5
    c, X, Q = _replicas(R)
    F = 0.2 * np.random.default_rng(11).standard_normal((R, 24))
    kw = dict(max_iter=50, rtol=1e-8)
    ens = _ens(c, X, Q)
    _set_ring(ens, c, scale=4.0)
    for n in range(steps):
        if family == "brownian":
            ens.step_brownian(F, seed=40 + n, **kw)
        else:
            ens.step_deterministic(F, **kw)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = _ens(c, X, Q)
    _set_ring(ens, c, scale=4.0)
    out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, stride=5, **kw)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(out.accepted, np.full(R, steps))
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)
    assert np.array_equal(out.X[0], Xl) and np.array_equal(out.Q[0], Ql)
    free = _ens(c, X, Q)                                       # ... and not the run of unbonded bodies
    free.run(steps, F=F, brownian=family == "brownian", seed=40, **kw)
    assert not np.array_equal(free.get_config()[0], Xr)
    free.close()


# ------------------------------------------------------------------------------------------------------------ 6
def test_a_stretched_dumbbell_relaxes_monotonically_about_a_midpoint_that_stays():
    """two shell_N_12 with identity orientations in free space, one harmonic bond between the centres stretched to 1.5 l0; l0 = 3
    keeps the shells apart.  k dt = 1: about a tenth of the extension goes per step (two beads, mu = 0.06 each), so 20 steps
    leave an eighth of it.  The configuration is symmetric under inversion about the midpoint (the shell is an icosahedron), so
    the two displacements are opposite: |dX_1 + dX_2| <= 1e-7 |dX_1|, three orders above the solver's 1e-10"""
    cfg, a = _structure("shell12")
    l0 = 3.0
    X = np.array([[0.0, 0.0, 50.0], [1.5 * l0, 0.0, 50.0]])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    ctx = _ctx({"cfg": cfg, "X": X, "Q": Q, "a": a, "eta": 1.0, "dt": 1.0}, wall=False, kBT=0.0)
    ctx.set_bonds([[0, 1]], np.zeros(3), np.zeros(3), 1.0, l0)
    d_prev, X_prev = ctx.bond_state()[0][0], X
    assert d_prev == 1.5 * l0
    for n in range(20):
        ctx.step_deterministic(np.zeros(12), max_iter=100, rtol=1e-10)
        Xn = np.reshape(ctx.get_config(2)[0], (2, 3)).copy()
        d = ctx.bond_state()[0][0]
        dX = Xn - X_prev
        assert l0 < d < d_prev, (n, d, d_prev)
        assert np.linalg.norm(dX[0] + dX[1]) <= 1e-7 * np.linalg.norm(dX[0]), (n, dX)
        d_prev, X_prev = d, Xn
    print("extension after 20 steps: %.4f of the initial one" % ((d_prev - l0) / (0.5 * l0)))
    assert np.linalg.norm(X_prev.sum(axis=0) - X.sum(axis=0)) <= 1e-7 * np.linalg.norm(X_prev[0] - X[0])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 7
@functools.lru_cache(maxsize=None)
def _free_shell_mu_tt():
    """translational mobility 1 / (6 pi eta R_h) of one shell_N_12 in free space, from body_mobility_matrix"""
    from rigid_body_light_amd import RigidBody
    cfg, a = _structure("shell12")
    rb = RigidBody(cfg, np.array([[0.0, 0.0, 50.0]]), np.array([[1.0, 0.0, 0.0, 0.0]]), a, 1.0, 0.01, wall_PC=False)
    N, _ = rb.body_mobility_matrix(rtol=1e-12)
    return float(N[0, 0])


def tethered_bead_ratio(dt_factor=0.5, R=256, seed=1000):
    """k <|p_A - P|^2> / (3 kBT) of one shell_N_12 in free space whose surface anchor (blob 0) is tethered to a lab point by a
    harmonic bond with l0 = 0, and its standard error from the R replica means.  dt = dt_factor * 0.02 / (k mu), mu = 1 / (6 pi
    eta R_h); 5 relaxation times 1 / (k mu) of burn-in from zero extension, 12 sampled with a frame every 0.4"""
    from rigid_body_light_amd._lib import blob_anchor
    cfg, a = _structure("shell12")
    k, kBT = 2.0, 1.0
    mu = _free_shell_mu_tt()
    dt = dt_factor * 0.02 / (k * mu)
    per_tau = int(round(50 / dt_factor))
    s = blob_anchor(cfg, 0)
    assert abs(np.linalg.norm(s) - R_SHELL) < 1e-6             # off the centre, on the surface
    Q = _quats(R, 17).reshape(R, 1, 4)
    X = np.tile([0.3, -0.4, 50.0], (R, 1, 1))
    P = np.array([0.3, -0.4, 50.0]) + mo.rot(Q[0, 0]) @ s
    X = X + (P - np.stack([X[r, 0] + mo.rot(Q[r, 0]) @ s for r in range(R)]))[:, None, :]      # every replica starts at zero extension
    ens = _ens({"cfg": cfg, "a": a, "eta": 1.0, "dt": dt}, X, Q, kBT=kBT, wall=False)
    assert np.array_equal(ens.blob_anchor(0), s)
    ens.set_bonds([[0, -1]], s, P, k, 0.0)
    assert np.abs(ens.bond_state()[0]).max() < 1e-13
    ens.run(5 * per_tau, F=np.zeros(6), seed=seed, max_iter=50, rtol=1e-8)
    steps, stride = 12 * per_tau, (2 * per_tau) // 5
    out = ens.run(steps, F=np.zeros(6), seed=seed + 5000, stride=stride, max_iter=50, rtol=1e-8)
    length_now = ens.bond_state()[0][:, 0]
    ens.close()
    assert np.array_equal(out.accepted, np.full(R, steps)) and out.X.shape == (steps // stride, R, 1, 3)
    pA = np.stack([[out.X[f, r, 0] + mo.rot(out.Q[f, r, 0]) @ s for r in range(R)] for f in range(out.X.shape[0])])
    r2 = ((pA - P) ** 2).sum(axis=2)                           # (frames, R)
    assert np.allclose(np.sqrt(r2[-1]), length_now, rtol=1e-12, atol=0.0)        # the last frame is where bond_state looks
    per_rep = k * r2.mean(axis=0) / (3.0 * kBT)
    return float(per_rep.mean()), float(per_rep.std(ddof=1) / np.sqrt(R)), dt


def test_equipartition_of_a_bead_tethered_by_its_surface():
    """For l0 = 0 the Boltzmann distribution of p_A - P is Gaussian with variance kBT / k per component whatever the orientation,
    so k <|p_A - P|^2> / (3 kBT) = 1.  The standard error must be <= 2 % (the test cannot pass by being noisy) and the ratio
    within 4 standard errors of 1.
    dt: at k mu dt = 0.02 the ratio measured 1.0187 +- 0.0135 and at half of it 1.0025 +- 0.0141 (tools/bench_bonds.py,
    profiles/bonds.jsonl): the two differ by more than one standard error -- the force is taken at q^n, so the variance carries a
    bias of the order of k mu_point dt / 2, and the surface point's mobility, rotation included, is about 1.5 mu -- hence the
    test runs at the halved step, k mu dt = 0.01 (dt_factor = 0.5), with twice the steps for the same relaxation times."""
    ratio, se, dt = tethered_bead_ratio()
    print("k <|p_A - P|^2> / (3 kBT) = %.4f, SE %.4f (dt %.4f)" % (ratio, se, dt))
    assert se <= 0.02
    assert abs(ratio - 1.0) <= 4.0 * se


# ------------------------------------------------------------------------------------------------------------ 8
def test_example_tethered_chain_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tethered_chain.py"), "--replicas", "16", "--steps", "40"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "end-to-end distance" in out.stdout and "largest bond extension" in out.stdout
