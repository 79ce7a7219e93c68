"""Blob types with a pair table per type pair (include/rbl.h section 4) on the GPU: agreement with the numpy all-pairs restatement
(tests/typed_oracle.py) at every path of the typed pair kernel, the type layouts, reproducibility and balance, forces against the
energy, orientation dependence through a Janus patch, the term inside the steps, the ensembles and their runs, the periodic cell,
and the switch leaving no trace."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import body_shapes  # noqa: E402
import table_oracle  # noqa: E402
import typed_oracle  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ scenes
def _quats(n, seed):
    Q = np.random.default_rng(seed).standard_normal((n, 4))
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _structure(nblb):
    """(cfg, a): the shells of the package, a Fibonacci sphere of touching blobs where there is no file (130)"""
    from rigid_body_light_amd import load_structure
    if nblb in (12, 42, 642):
        p, cfg = load_structure(nblb)
        return cfg, p["sep"] / 2.0
    return body_shapes.fib(nblb, 0.5), 0.5


def _packed3(nblb, nb=3, spread=1.6):
    """nb shells on a triangle packed as test_interaction_tables_gpu packs its eight: centres 1.6 R apart, so the shells
    interpenetrate (blobs of different bodies closer than 2a), and at z = R + a / 2, so the lowest blobs lie below h = a"""
    cfg, a = _structure(nblb)
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    X = np.array([[0.0, 0.0, 0.0], [1.0, 0.04, 0.0], [0.45, 0.9, 0.0]])[:nb] * spread * R
    X[:, 2] = R + 0.5 * a
    X[:, :2] += np.random.default_rng(5).uniform(-0.05, 0.05, (nb, 2))
    return {"cfg": cfg, "X": X, "Q": _quats(nb, 6 + nblb), "a": a, "eta": 1.0, "dt": 0.01, "R": R}


def _apart3(nblb=12, gap=0.4):
    """test_interaction_tables_gpu's triangle of three shells whose surfaces are `gap` apart, well above the wall"""
    cfg, a = _structure(nblb)
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    d = 2.0 * R + gap
    X = np.array([[0.0, 0.0, 0.0], [d, 0.05, 0.1], [0.5 * d, 0.87 * d, -0.1]]) + [0.0, 0.0, R + a + 0.3]
    return {"cfg": cfg, "X": X, "Q": _quats(3, 6), "a": a, "eta": 1.0, "dt": 0.01, "R": R}


def _ctx(c, wall, kBT=1.0):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], kBT=kBT, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    return ctx


def _positions(ctx, nb, nblb):
    import torch
    r = torch.empty(3 * nb * nblb, dtype=torch.float64, device="cuda:0")
    ctx.blob_positions(0, nb, r.data_ptr())
    ctx.sync_check()
    return r.cpu().numpy().reshape(-1, 3)


def _scene_positions(c, wall=True):
    ctx = _ctx(c, wall)
    r = _positions(ctx, c["X"].shape[0], c["cfg"].shape[0])
    ctx.close()
    return r


# ------------------------------------------------------------------------------------------------------------ the model
def _lj_table(lo, hi, n, eps=1.5):
    """test_interaction_tables_gpu's Lennard-Jones-like law with its minimum inside (lo, hi), shifted to U(hi) = 0"""
    sig = (lo + 0.25 * (hi - lo)) / 2.0 ** (1.0 / 6.0)
    x = np.linspace(lo, hi, n)
    s6 = (sig / x) ** 6
    sh = (sig / hi) ** 6
    return 4 * eps * (s6 * s6 - s6) - 4 * eps * (sh * sh - sh), -24 * eps * (2 * s6 * s6 - s6) / x, lo, hi


def _soft_table(lo, hi, n, eps=2.0):
    b = 0.3 * (hi - lo)
    x = np.linspace(lo, hi, n)
    return eps * (np.exp(-(x - lo) / b) - np.exp(-(hi - lo) / b)), -eps / b * np.exp(-(x - lo) / b), lo, hi


def _well_table(hi, n, eps):
    """a purely attractive well, U = -eps (1 - r / hi)^2 on [0, hi]: zero with zero slope at the cutoff"""
    x = np.linspace(0.0, hi, n)
    return -eps * (1.0 - x / hi) ** 2, 2.0 * eps * (1.0 - x / hi) / hi, 0.0, hi


def _builtin(r_cut, w=0.3):
    return dict(w=w, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=r_cut)


RC_BUILTIN, RC_PAIR = 3.0, 4.0       # cutoffs of the built-in term and of the untyped table, in units of a
# type pair -> (r_cut / a, grid points, eps): (0, 0) reaches beyond both cutoffs above, (0, 1) ends below both; (1, 1) and every
# pair not listed has no table
TYPE_TABLES = {(0, 0): (5.2, 1025, 0.8), (0, 1): (2.6, 17, 1.2), (1, 2): (3.5, 257, 0.6), (2, 2): (4.5, 2, 0.9), (2, 0): (2.3, 65, 1.1),
               (7, 7): (4.8, 129, 0.7), (3, 6): (3.2, 33, 1.3), (0, 7): (5.0, 9, 0.5), (5, 4): (2.8, 513, 1.0), (6, 1): (4.1, 3, 0.4)}


R_MIN_TYPED, R_MIN_PAIR = 1.5, 1.6   # the grids start inside the overlaps: pairs closer than that see the tangent at r_min


def _tables(n_types, a):
    return {(s, t): _lj_table(R_MIN_TYPED * a, rc * a, n, eps) for (s, t), (rc, n, eps) in TYPE_TABLES.items() if max(s, t) < n_types}


def _types(n_types, n, seed=12):
    t = np.random.default_rng(seed + n_types).integers(0, n_types, n)
    t[:n_types] = np.arange(n_types)                       # every type occurs
    return t.astype(np.int32)


def _full_model(c, r, n_types):
    """every term on -> keyword arguments of typed_oracle.interactions without the types (d: the pair distances)"""
    nb, nblb, a = c["X"].shape[0], c["cfg"].shape[0], c["a"]
    d = typed_oracle.pair_distances(r, nblb)
    z = r[:, 2]
    k = np.tile([[1.5, 0.0, 0.7]], (nb, 1)) * (1.0 + np.arange(nb))[:, None]
    return dict(tables=_tables(n_types, a), builtin=_builtin(RC_BUILTIN * a), pair=_lj_table(R_MIN_PAIR * a, RC_PAIR * a, 257),
                height=_soft_table(z.min() + 0.2 * (z.max() - z.min()), z.min() + 0.7 * (z.max() - z.min()), 65),
                traps=(k, c["X"] + np.random.default_rng(3).uniform(-0.3, 0.3, c["X"].shape))), d


def _apply(obj, types=None, n_types=None, tables=None, builtin=None, pair=None, height=None, traps=None):
    """switch the model of a DeviceContext, a RigidBody or an Ensemble to exactly these terms"""
    if builtin is not None:
        obj.set_interactions(**builtin)
    if pair is not None:
        obj.set_pair_table(*pair)
    if height is not None:
        obj.set_height_table(*height)
    if traps is not None:
        obj.set_traps(*traps)
    obj.clear_type_tables()
    for (s, t), tab in (tables or {}).items():
        obj.set_type_table(s, t, *tab)
    if types is not None:
        obj.set_blob_types(types, n_types=n_types)


def _rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / np.abs(np.asarray(y)).max()


def _against_oracle(ctx, r, c, wall, types_flat, model, label=""):
    """forces, body forces / torques and energy to 1e-12 of the largest magnitude, the ordered pair count exactly"""
    nblb = c["cfg"].shape[0]
    assert typed_oracle.clear_of_cutoffs(r, nblb, typed_oracle.cutoffs(model["builtin"], model["pair"], model["tables"]))
    fo, FTo, Eo, npo, nty = typed_oracle.interactions(r, c["X"], nblb, c["a"], wall, types=types_flat, **model)
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    pp = ctx.interaction_stats()[1]
    print("  %s wall %d: |f|max %.3e |FT|max %.3e E %.6e  df %.1e dFT %.1e dE %.1e  pairs %d (typed %d)" % (
        label, wall, np.abs(fo).max(), np.abs(FTo).max(), Eo, _rel(f, fo), _rel(FT, FTo), abs(E - Eo) / abs(Eo), pp, nty))
    assert _rel(f, fo) <= 1e-12 and _rel(FT, FTo) <= 1e-12 and abs(E - Eo) <= 1e-12 * abs(Eo)
    assert pp == npo
    return fo, nty


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_types", [1, 2, 3, 8])
@pytest.mark.parametrize("nblb", [12, 42, 130, 642])
def test_every_term_on_agrees_with_the_all_pairs_oracle(nblb, n_types):
    """a part-filled wave, one wave, a 256-lane workgroup, three tiles with two LDS chunks (the type slot crosses the chunk
    boundary); the built-in term, the untyped table, the height table and the traps on beside the type tables"""
    c = _packed3(nblb)
    a = c["a"]
    types = _types(n_types, nblb)
    for wall in (True, False):
        ctx = _ctx(c, wall)
        r = _positions(ctx, 3, nblb)
        model, d = _full_model(c, r, n_types)
        assert (d < R_MIN_TYPED * a).any() and (r[:, 2] < a).any()             # overlaps r < 2a, down to the tangent branch; blobs below h = a
        rc = {k: t[3] for k, t in model["tables"].items()}
        assert rc[(0, 0)] > max(RC_BUILTIN, RC_PAIR) * a and (d > RC_PAIR * a).any() and ((d > RC_PAIR * a) & (d < rc[(0, 0)])).any()
        if n_types >= 2:
            assert rc[(0, 1)] < min(RC_BUILTIN, RC_PAIR) * a and (d < rc[(0, 1)]).any() and (1, 1) not in model["tables"]
        _apply(ctx, types=types, n_types=n_types, **model)
        assert ctx.interactions_active() == 128 + 15
        fo, nty = _against_oracle(ctx, r, c, wall, np.tile(types, 3), model, "%dx%d types %d" % (3, nblb, n_types))
        assert nty > 0
        # the type tables matter: the same model without them is another force
        f0 = typed_oracle.interactions(r, c["X"], nblb, a, wall, **dict(model, tables=None))[0] if wall and nblb <= 130 else None
        assert f0 is None or _rel(f0, fo) > 1e-6
        ctx.close()


def test_the_typed_cutoff_alone_decides_the_cull():
    """two shell_N_12 further apart than the built-in cutoff and the untyped table's reach: only T_00 sees the pair, so the
    neighbour list has to be built with the typed cutoff"""
    c = _apart3(12, 1.2)
    c["X"], c["Q"] = c["X"][:2], c["Q"][:2]
    a = c["a"]
    ctx = _ctx(c, True)
    r = _positions(ctx, 2, 12)
    d = typed_oracle.pair_distances(r, 12)
    hi = d.min() + 0.5 * (d.max() - d.min())
    model = dict(tables={(0, 0): _lj_table(0.9 * d.min(), hi, 17)}, builtin=_builtin(2 * a), pair=_lj_table(0.5 * a, 0.95 * d.min(), 9),
                 height=None, traps=None)
    assert np.linalg.norm(c["X"][0] - c["X"][1]) > 2 * c["R"] + 2 * a + 0.1 and d.min() > max(2 * a, model["pair"][3])
    _apply(ctx, types=np.zeros(12, dtype=int), n_types=1, **model)
    for cull in (1, 0):
        ctx.set_option("interaction_cull", cull)
        _, nty = _against_oracle(ctx, r, c, True, np.zeros(24, dtype=int), model, "typed reach, cull %d" % cull)
        assert nty == 2 * int((d <= hi).sum()) > 0 and tuple(ctx.interaction_stats()) == (2, nty)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 2
def test_types_per_body_and_the_shared_layout_tiled():
    c = _packed3(42)
    ctx = _ctx(c, True)
    r = _positions(ctx, 3, 42)
    model, _ = _full_model(c, r, 3)
    per_body = np.stack([_types(3, 42, seed=s) for s in (1, 2, 3)])
    per_body[2] = 1                                                              # a body of one type
    assert not np.array_equal(per_body[0], per_body[1])
    _apply(ctx, types=per_body, n_types=3, **model)
    assert ctx.blob_types()["types"].shape == (126,)
    _against_oracle(ctx, r, c, True, per_body.reshape(-1), model, "per-body types")
    shared = per_body[0]
    ctx.set_blob_types(shared, n_types=3)
    f1, FT1 = ctx.interaction_forces()
    E1, st1 = ctx.interaction_energy(), ctx.interaction_stats()
    ctx.set_blob_types(np.tile(shared, (3, 1)), n_types=3)
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(f1, f2) and np.array_equal(FT1, FT2) and ctx.interaction_energy() == E1 and ctx.interaction_stats() == st1
    ctx.close()


@pytest.mark.parametrize("nblb", [42, 642])
def test_one_type_with_T00_is_the_untyped_pair_table(nblb):
    c = _packed3(nblb)
    a = c["a"]
    ctx = _ctx(c, True)
    r = _positions(ctx, 3, nblb)
    d = typed_oracle.pair_distances(r, nblb)
    X = _lj_table(R_MIN_PAIR * a, RC_PAIR * a, 257)
    assert (d < R_MIN_PAIR * a).any()
    ctx.set_interactions(**_builtin(RC_BUILTIN * a))
    ctx.set_pair_table(*X)
    f_u, FT_u = ctx.interaction_forces()
    E_u, st_u = ctx.interaction_energy(), ctx.interaction_stats()
    assert ctx.interactions_active() == 3
    ctx.set_pair_table(None, None, 0.0, 0.0, on=False)
    ctx.set_type_table(0, 0, *X)
    ctx.set_blob_types(np.zeros(nblb, dtype=int), n_types=1)
    assert ctx.interactions_active() == 129
    f_t, FT_t = ctx.interaction_forces()
    E_t = ctx.interaction_energy()
    print("T_00 = X against the untyped X at N_blb %d: df %.1e of the largest force, dE %.1e; bitwise: forces %s, energy %s" % (
        nblb, _rel(f_t, f_u), abs(E_t - E_u) / abs(E_u), np.array_equal(f_t, f_u), E_t == E_u))
    assert np.abs(f_t - f_u).max() <= 1e-13 * np.abs(f_u).max() and np.abs(FT_t - FT_u).max() <= 1e-13 * np.abs(FT_u).max()
    assert abs(E_t - E_u) <= 1e-13 * abs(E_u) and ctx.interaction_stats() == st_u
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("nblb", [12, 642])
def test_two_evaluations_and_the_cull_switch_are_bitwise(nblb):
    c = _packed3(nblb)
    ctx = _ctx(c, True)
    r = _positions(ctx, 3, nblb)
    model, d = _full_model(c, r, 3)
    _apply(ctx, types=_types(3, nblb), n_types=3, **model)
    f1, FT1 = ctx.interaction_forces()
    E1, (bp1, pp1) = ctx.interaction_energy(), ctx.interaction_stats()
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(f1, f2) and np.array_equal(FT1, FT2) and ctx.interaction_energy() == E1
    ctx.set_option("interaction_cull", 0)
    f0, FT0 = ctx.interaction_forces()
    E0, (bp0, pp0) = ctx.interaction_energy(), ctx.interaction_stats()
    assert bp0 == 6 and pp0 == pp1 > 0
    assert np.array_equal(f0, f1) and np.array_equal(FT0, FT1) and E0 == E1
    ctx.close()


def test_two_bodies_without_weight_or_wall_exchange_opposite_forces_and_torques():
    c = _packed3(42, nb=2)
    ctx = _ctx(c, False)
    r = _positions(ctx, 2, 42)
    model, _ = _full_model(c, r, 3)
    model.update(builtin=_builtin(RC_BUILTIN * c["a"], w=0.0), height=None, traps=None)
    per_body = np.stack([_types(3, 42, seed=4), _types(3, 42, seed=9)])
    _apply(ctx, types=per_body, n_types=3, **model)
    _against_oracle(ctx, r, c, False, per_body.reshape(-1), model, "two bodies")
    f, FT = ctx.interaction_forces()
    FT = FT.reshape(2, 6)
    torque_about_origin = FT[:, 3:] + np.cross(c["X"], FT[:, :3])
    print("sum of forces %s, of torques about the origin %s; largest %.3e, %.3e" % (
        FT[:, :3].sum(axis=0), torque_about_origin.sum(axis=0), np.abs(FT[:, :3]).max(), np.abs(torque_about_origin).max()))
    assert np.abs(FT[:, :3]).max() > 1.0
    assert np.abs(FT[:, :3].sum(axis=0)).max() <= 1e-12 * np.abs(FT[:, :3]).max()
    assert np.abs(torque_about_origin.sum(axis=0)).max() <= 1e-12 * np.abs(torque_about_origin).max()
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).max()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 4
def test_generalised_forces_are_minus_the_energy_gradient_with_every_term_on():
    """central differences through rbl_update_X_Q over all 6 N_bod body coordinates, as test_interaction_tables_gpu's"""
    c = _packed3(42)
    nb = 3
    ctx = _ctx(c, True)
    r = _positions(ctx, nb, 42)
    model, _ = _full_model(c, r, 3)
    model["tables"] = {k: _lj_table(t[2], t[3], 513, eps=0.5) for k, t in model["tables"].items()}   # fine grids: a smooth energy
    model["pair"] = _lj_table(model["pair"][2], model["pair"][3], 513)
    _apply(ctx, types=np.stack([_types(3, 42, seed=s) for s in (1, 2, 3)]), n_types=3, **model)
    assert ctx.interactions_active() == 143
    _, FT = ctx.interaction_forces()
    X0, Q0 = ctx.get_config(nb)
    eps = 1e-6
    g = np.zeros(6 * nb)
    for k in range(6 * nb):
        E = []
        for s in (1.0, -1.0):
            U = np.zeros(6 * nb)
            U[k] = s * eps
            ctx.set_config(X0, Q0)
            Xs, Qs = ctx.update_X_Q(U, nb)
            ctx.set_config(Xs, Qs)
            E.append(ctx.interaction_energy())
        g[k] = (E[0] - E[1]) / (2 * eps)
    ctx.close()
    assert np.abs(FT).max() > 1.0
    assert np.abs(FT + g).max() <= 1e-6 * np.abs(FT).max(), np.abs(FT + g).max() / np.abs(FT).max()


# ------------------------------------------------------------------------------------------------------------ 5
def _janus_pair(turned):
    """two shell_N_42 along x, nearest blob centres 2.5 a apart; the cap (type 1) is the hemisphere about the body's z axis.
    Body 0's cap faces body 1; body 1's cap faces body 0, or -- turned by pi about z^ -- away from it"""
    cfg, a = _structure(42)
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    s = np.sqrt(0.5)
    to_plus_x, to_minus_x = [s, 0.0, s, 0.0], [s, 0.0, -s, 0.0]                  # rotations by +-pi/2 about y^: z^ -> +-x^
    X = np.array([[0.0, 0.0, 3.0 * R], [2.0 * R + 2.5 * a, 0.0, 3.0 * R]])
    return {"cfg": cfg, "X": X, "Q": np.array([to_plus_x, to_plus_x if turned else to_minus_x]), "a": a, "eta": 1.0, "dt": 0.01, "R": R}


def test_a_janus_pair_attracts_cap_to_cap_and_only_repels_when_one_is_turned():
    from rigid_body_light_amd import patch_types
    cfg, a = _structure(42)
    types = patch_types(cfg, [0.0, 0.0, 1.0])
    hi = 4.0 * a
    builtin = dict(w=0.0, eps_wall=0.0, b_wall=0.1, eps_blob=2.0, b_blob=0.1 * a, r_cut=2 * a + 2.0 * a)
    out = {}
    for turned in (False, True):
        c = _janus_pair(turned)
        ctx = _ctx(c, False)
        r = _positions(ctx, 2, 42)
        cap = r[np.tile(types, 2) == 1]
        # the caps point where they are meant to
        assert cap[:types.sum(), 0].mean() > c["X"][0, 0] + 0.3 * c["R"]
        side = cap[types.sum():, 0].mean() - c["X"][1, 0]
        assert side > 0.3 * c["R"] if turned else side < -0.3 * c["R"]
        ctx.set_interactions(**builtin)
        _, FT_steric = ctx.interaction_forces()
        model = dict(tables={(1, 1): _well_table(hi, 129, 5.0)}, builtin=builtin, pair=None, height=None, traps=None)
        _apply(ctx, types=types, n_types=2, tables=model["tables"])
        assert ctx.interactions_active() == 129
        _, nty = _against_oracle(ctx, r, c, False, np.tile(types, 2), model, "janus turned %d" % turned)
        f, FT = ctx.interaction_forces()
        ctx.set_type_table(1, 1, *_well_table(hi, 129, 500.0))                   # a hundred times deeper
        f_deep, FT_deep = ctx.interaction_forces()
        out[turned] = (nty, FT.reshape(2, 6), FT_steric.reshape(2, 6), np.array_equal(f, f_deep) and np.array_equal(FT, FT_deep))
        ctx.close()
    nty, FT, FT_steric, same = out[False]                                        # caps facing each other
    print("facing: %d typed pairs, F_x on body 0 %+.4e (steric alone %+.4e)" % (nty, FT[0, 0], FT_steric[0, 0]))
    assert nty > 0 and not same
    assert FT_steric[0, 0] < 0.0 < FT[0, 0] and FT[1, 0] < 0.0                   # alone the shells repel; with the caps they attract
    nty, FT, FT_steric, same = out[True]                                         # body 1 turned by pi
    print("turned: %d typed pairs, F_x on body 0 %+.4e (steric alone %+.4e)" % (nty, FT[0, 0], FT_steric[0, 0]))
    assert nty == 0                                                              # no type-1 pair inside the cutoff ...
    assert same                                                                  # ... so the table's depth does not reach the result
    assert FT[0, 0] < 0.0 < FT[1, 0] and _rel(FT, FT_steric) <= 1e-13            # only the steric repulsion remains


# ------------------------------------------------------------------------------------------------------------ 6
def _step_terms(c, r, nblb, scale=0.002):
    """type tables gentle enough for a time step (the cores are steep at r_min)"""
    d = typed_oracle.pair_distances(r, nblb)
    span = d.max() - d.min()
    return {(0, 0): _lj_table(d.min() + 0.1 * span, d.min() + 0.6 * span, 257, eps=scale),
            (0, 1): _lj_table(d.min() + 0.05 * span, d.min() + 0.4 * span, 65, eps=2 * scale)}


def test_a_deterministic_step_adds_the_typed_term_at_qn():
    c = _apart3(12, 0.4)
    ctx = _ctx(c, True)
    tables = _step_terms(c, _positions(ctx, 3, 12), 12, scale=0.02)
    _apply(ctx, types=_types(2, 12), n_types=2, tables=tables)
    assert ctx.interactions_active() == 128 and not ctx.interaction_params()["on"] and ctx.interactions_on()
    _, FT = ctx.interaction_forces()
    assert np.abs(FT).max() > 0.05
    ctx.step_deterministic(np.zeros(18), max_iter=80, rtol=1e-12)
    Xa, Qa = ctx.get_config(3)
    ctx.close()
    ref = _ctx(c, True)                                     # no model, the caller passing -FT (reference convention)
    ref.step_deterministic(-FT, max_iter=80, rtol=1e-12)
    Xb, Qb = ref.get_config(3)
    ref.close()
    assert np.abs(np.reshape(Xa, (3, 3)) - c["X"]).max() > 1e-5
    assert np.abs(Xa - Xb).max() <= 1e-12 and np.abs(Qa - Qb).max() <= 1e-12


def test_the_free_slots_of_a_mask_feel_the_typed_term_and_the_prescribed_do_not():
    from rigid_body_light_amd import RigidBody
    c = _apart3(12, 0.4)
    tables = _step_terms(c, _scene_positions(c), 12, scale=0.02)
    mask = np.array([True, False, False])
    out = []
    for with_model in (True, False):
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True)
        body_in = np.zeros(18)
        if with_model:
            _apply(rb, types=_types(2, 12), n_types=2, tables=tables)
            loads = rb.interaction_forces()              # reference convention, -K^T f_phys
            assert np.abs(loads[:6]).max() > 0.05 and np.abs(loads[6:]).max() > 0.05
        else:
            body_in[6:] = loads[6:]                      # the model's loads on the free bodies only
        rb.step_mixed(mask, body_in, max_iter=100, rtol=1e-12)
        out.append(rb.get_config())
    assert np.array_equal(out[0][0][0], c["X"][0])           # the held body stays although the model loads it
    assert np.abs(out[0][0][1:] - c["X"][1:]).max() > 1e-5
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-12 and np.abs(out[0][1] - out[1][1]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 7
def _replicas(R):
    c = _apart3(12, 0.4)
    rng = np.random.default_rng(21)
    X = c["X"][None] + rng.uniform(-0.08, 0.08, (R, 3, 3))
    Q = np.stack([_quats(3, 30 + r) for r in range(R)])
    return c, X, Q


ENS_TYPES = np.stack([_types(2, 12, seed=s) for s in (5, 6, 7)])                 # per body, shared by the replicas


@functools.lru_cache(maxsize=None)
def _ens_tables():
    return {(0, 0): _lj_table(1.0, 2.2, 257, eps=0.02), (1, 0): _lj_table(0.9, 1.7, 65, eps=0.03)}


def _ens(c, X, Q, kBT=1.0, types=ENS_TYPES):
    from rigid_body_light_amd import Ensemble
    e = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=kBT, wall=True)
    _apply(e, types=types, n_types=2, tables=_ens_tables())
    return e


@pytest.mark.parametrize("layout", ["per_body", "shared"])
def test_ensemble_forces_are_each_replicas_single_context_forces(layout):
    R = 3
    c, X, Q = _replicas(R)
    types = ENS_TYPES if layout == "per_body" else ENS_TYPES[0]
    ens = _ens(c, X, Q, types=types)
    assert ens.ctx.interactions_active() == 128
    FTe, Ee = ens.interaction_forces(), ens.interaction_energy()
    ens.close()
    assert FTe.shape == (R, 18) and Ee.shape == (R,)
    flat = np.broadcast_to(types, (3, 12)).reshape(-1)
    for rep in range(R):
        cr = dict(c, X=X[rep], Q=Q[rep])
        s = _ctx(cr, True)
        _apply(s, types=types, n_types=2, tables=_ens_tables())
        _, FT = s.interaction_forces()
        E = s.interaction_energy()
        model = dict(tables=_ens_tables(), builtin=None, pair=None, height=None, traps=None)
        _, nty = _against_oracle(s, _positions(s, 3, 12), cr, True, flat, model, "replica %d" % rep)   # so that the two cannot be wrong together
        s.close()
        assert nty > 0
        assert np.abs(FTe[rep] + FT).max() <= 1e-12 * np.abs(FT).max()         # reference convention: -K^T f_phys
        assert abs(Ee[rep] - E) <= 1e-12 * abs(E)
        one = _ens(c, X[rep:rep + 1], Q[rep:rep + 1], types=types)             # replica r of R is bitwise the R = 1 call
        assert np.array_equal(one.interaction_forces()[0], FTe[rep]) and one.interaction_energy()[0] == Ee[rep]
        one.close()


@pytest.mark.parametrize("family", ["brownian", "deterministic"])
def test_an_ensemble_run_with_the_typed_term_is_the_loop_bitwise(family):
    R, steps = 3, 5
    c, X, Q = _replicas(R)
    F = 0.2 * np.random.default_rng(11).standard_normal((R, 18))
    kw = dict(max_iter=50, rtol=1e-8)
    ens = _ens(c, X, Q)
    for n in range(steps):
        if family == "brownian":
            ens.step_brownian(F, seed=40 + n, **kw)
        else:
            ens.step_deterministic(F, **kw)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = _ens(c, X, Q)
    out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, stride=5, **kw)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(out.accepted, np.full(R, steps))
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)
    assert np.array_equal(out.X[0], Xl) and np.array_equal(out.Q[0], Ql)
    from rigid_body_light_amd import Ensemble                                   # ... and not the run of an ensemble without the term
    bare = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=True)
    bare.run(steps, F=F, brownian=family == "brownian", seed=40, **kw)
    assert np.abs(bare.get_config()[0] - Xr).max() > 1e-7
    bare.close()


def test_an_ensemble_refuses_types_of_another_length_and_stays_usable():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = _replicas(3)
    ens = _ens(c, X, Q)
    good = ens.interaction_forces()
    ens.ctx.set_blob_types(np.zeros(24, dtype=np.int32), n_types=2)               # neither N_blb = 12 nor N_bod N_blb = 36 entries
    with pytest.raises(RblError, match=r"blob types hold neither.*status 7"):     # RBL_ERR_STATE
        ens.interaction_forces()
    with pytest.raises(RblError, match="status 7"):
        ens.step_deterministic(np.zeros(18))
    assert np.array_equal(ens.get_config()[0], X)                                 # nothing moved
    ens.set_blob_types(ENS_TYPES, n_types=2)
    assert np.array_equal(ens.interaction_forces(), good)
    ens.step_deterministic(np.zeros(18))
    assert np.abs(ens.get_config()[0] - X).max() > 0.0
    ens.close()


# ------------------------------------------------------------------------------------------------------------ 8
def _across(n_rep=1):
    """two shell_N_12 above the wall whose only contact is through the x boundary of the cell: body 1 sits a gap short of one
    cell length from body 0.  The type table reaches furthest, so its cutoff sets the smallest admissible cell"""
    cfg, a = _structure(12)
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    rc_typed = 4.5 * a
    need = 2.0 * R + rc_typed
    L = (2.0 * need + 1.0, 2.0 * need + 2.5)
    X = np.array([[0.2, 0.3, R + 2 * a], [0.2 + L[0] - (2.0 * R + 0.8 * a), 0.5, R + 2.3 * a]])
    c = {"cfg": cfg, "X": X, "Q": _quats(2, 3), "a": a, "eta": 1.0, "dt": 0.01, "R": R}
    model = dict(tables={(0, 1): _lj_table(1.2 * a, rc_typed, 129), (1, 1): _lj_table(1.0 * a, 3.0 * a, 33, eps=0.7)},
                 builtin=_builtin(2.5 * a), pair=_lj_table(1.1 * a, 3.5 * a, 65), height=None, traps=None)
    return c, L, need, model, _types(2, 12, seed=2)


def _check_across(r, c, L, model, types):
    """the oracle's side: nothing inside a cutoff directly, something through the boundary, for the type tables too"""
    assert typed_oracle.clear_of_cutoffs(r, 12, typed_oracle.cutoffs(model["builtin"], model["pair"], model["tables"]), L=L)
    direct = typed_oracle.interactions(r, c["X"], 12, c["a"], True, types=np.tile(types, 2), **model)
    per = typed_oracle.interactions(r, c["X"], 12, c["a"], True, types=np.tile(types, 2), L=L, **model)
    assert direct[3] == 0 and per[3] > 0 and per[4] > 0
    return per


def test_a_typed_pair_through_the_boundary_and_a_cell_too_small_for_the_typed_cutoff():
    c, L, need, model, types = _across()
    ctx = _ctx(c, True)
    r = _positions(ctx, 2, 12)
    fo, FTo, Eo, npo, nty = _check_across(r, c, L, model, types)
    _apply(ctx, types=types, n_types=2, **model)
    ctx.set_periodic(L[0], L[1], images=(1, 1))
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    print("through the boundary: df %.1e dFT %.1e dE %.1e, %d pairs (%d typed)" % (_rel(f, fo), _rel(FT, FTo), abs(E - Eo) / abs(Eo), npo, nty))
    assert _rel(f, fo) <= 1e-12 and _rel(FT, FTo) <= 1e-12 and abs(E - Eo) <= 1e-12 * abs(Eo)
    assert ctx.interaction_stats()[1] == npo
    # a cell that would do for the built-in term and the untyped table, and not for the type table
    need_untyped = 2.0 * c["R"] + model["pair"][3]
    small = 2.0 * (0.5 * (need + need_untyped))
    assert 2.0 * need_untyped < small < 2.0 * need
    ctx.set_periodic(small, L[1], images=(1, 1))
    with pytest.raises(RuntimeError, match=r"periodic cell too small: Lx = .*needs 2 R_body \+ r_cut = %s.*<= L / 2" % ("%.6f" % need)[:-1]):
        ctx.interaction_forces()
    ctx.set_type_table(0, 1, None, None, 0.0, 0.0, on=False)                     # without the long table the small cell is served
    ctx.interaction_forces()
    ctx.set_type_table(0, 1, *model["tables"][(0, 1)])
    with pytest.raises(RuntimeError, match="periodic cell too small"):
        ctx.interaction_forces()
    ctx.set_periodic(L[0], L[1], images=(1, 1))                                  # the next valid cell
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(f2, f) and np.array_equal(FT2, FT)
    ctx.close()


@pytest.mark.parametrize("cells", ["one", "per_replica"])
def test_an_ensemble_in_a_cell_sees_the_typed_pair_through_the_boundary(cells):
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import RblError
    c, L, need, model, types = _across()
    R = 2
    Ls = [L, (L[0] + 1.0, L[1] + 1.5)] if cells == "per_replica" else [L, L]
    X = np.stack([c["X"], c["X"] + [0.1, -0.1, 0.05]])
    X[1, 1, 0] += Ls[1][0] - L[0]
    Q = np.stack([c["Q"], _quats(2, 8)])
    ens = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=True)
    _apply(ens, types=types, n_types=2, **model)
    if cells == "one":
        ens.set_cell(L[0], L[1])
    else:
        ens.set_cells([l[0] for l in Ls], [l[1] for l in Ls])
    FTe, Ee = ens.interaction_forces(), ens.interaction_energy()
    for rep in range(R):
        cr = dict(c, X=X[rep], Q=Q[rep])
        fo, FTo, Eo, npo, nty = _check_across(_scene_positions(cr), cr, Ls[rep], model, types)
        print("replica %d in %s: dFT %.1e dE %.1e (%d typed pairs)" % (rep, Ls[rep], _rel(-FTe[rep], FTo), abs(Ee[rep] - Eo) / abs(Eo), nty))
        assert _rel(-FTe[rep], FTo) <= 1e-12 and abs(Ee[rep] - Eo) <= 1e-12 * abs(Eo)
    small = need + 0.5 * (2.0 * c["R"] + model["pair"][3])                       # between twice the untyped need and twice the typed one
    if cells == "one":
        ens.set_cell(small, L[1])
    else:
        ens.set_cells([Ls[0][0], small], [l[1] for l in Ls])
    with pytest.raises(RblError, match=r"%speriodic cell too small: Lx = .*needs 2 R_body \+ r_cut = %s" % (
            "replica 1: " if cells == "per_replica" else "", ("%.6f" % need)[:-1])):
        ens.interaction_forces()
    if cells == "one":
        ens.set_cell(L[0], L[1])
    else:
        ens.set_cells([l[0] for l in Ls], [l[1] for l in Ls])
    assert np.array_equal(ens.interaction_forces(), FTe)                         # the next valid cell is served
    ens.close()


# ------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("how", ["types_off", "tables_off"])
def test_switched_off_the_types_leave_no_trace(how):
    c = _apart3(12, 0.4)
    a = c["a"]
    tables = _step_terms(c, _scene_positions(c), 12, scale=0.02)
    out = []
    for had in (True, False):
        res = []
        for kind in ("forces", "deterministic", "brownian"):
            ctx = _ctx(c, True, kBT=0.1)
            ctx.set_interactions(**_builtin(2 * a + 1.0))
            if had:
                _apply(ctx, types=_types(2, 12), n_types=2, tables=tables)
                assert ctx.interactions_active() == 129
                f_on = ctx.interaction_forces()[0]                               # on, evaluated ...
                if how == "types_off":
                    ctx.set_blob_types(_types(2, 12), n_types=2, on=False)       # ... the types stored switched off
                else:
                    for (s, t), tab in tables.items():
                        ctx.set_type_table(s, t, *tab, on=False)                 # ... the types on, every table off
                    assert ctx.blob_types()["on"]
                assert ctx.interactions_active() == 1
            if kind == "forces":
                f, FT = ctx.interaction_forces()
                res += [f, FT, np.array(ctx.interaction_energy()), np.array(ctx.interaction_stats())]
                assert not had or np.abs(f - f_on).max() > 1e-6                  # the term did change the forces while it was on
            else:
                F = np.tile([0.0, 0.0, 0.3, 0.0, 0.0, 0.0], 3)
                if kind == "deterministic":
                    ctx.step_deterministic(F, max_iter=50, rtol=1e-10)
                else:
                    ctx.step_brownian(F, max_iter=50, rtol=1e-10, seed=3, method=2)
                res += list(ctx.get_config(3))
            ctx.close()
        out.append(res)
    assert len(out[0]) == len(out[1]) == 8
    for x, y in zip(*out):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 10
def test_example_janus_shells_runs():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "janus_shells.py"), "--replicas", "8", "--steps", "40"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "interactions_active 129" in out.stdout and "interactions_active   1" in out.stdout and "bound fraction:" in out.stdout
