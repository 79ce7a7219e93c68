"""The tabulated pair and height potentials and the harmonic traps of include/rbl.h section 4 on the GPU: agreement with the numpy
all-pairs restatement (tests/table_oracle.py) on the smallest shapes that reach every path of the pair kernel, exactness of the
cull under the larger cutoff, the built-in steric law recovered through a table within the Hermite error bounds, generalised
forces against the energy, the terms inside the steps and the ensembles, equipartition in a trap, and the example."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import table_oracle  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ shapes
def _quats(n, seed):
    Q = np.random.default_rng(seed).standard_normal((n, 4))
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


def _three(n_blobs, gap):
    """three shells on a triangle above the wall, surfaces `gap` apart: every body within a cutoff of the other two"""
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(n_blobs)
    a = p["sep"] / 2.0
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    d = 2.0 * R + gap
    X = np.array([[0.0, 0.0, 0.0], [d, 0.05, 0.1], [0.5 * d, 0.87 * d, -0.1]]) + [0.0, 0.0, R + a + 0.3]
    return {"cfg": cfg, "X": X, "Q": _quats(3, 6), "a": a, "eta": 1.0, "dt": 0.01}


def _packed():
    """test_interactions_gpu's packed case: 8 shell_N_42 whose shells interpenetrate, lowest blobs below h = a (above the wall)"""
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(42)
    a = p["sep"] / 2.0
    R = np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()
    idx = np.arange(8)
    X = np.stack([idx % 4, idx // 4, np.zeros(8)], axis=1) * 1.6 * R
    X[:, 2] = R + 0.5 * a
    X += np.random.default_rng(5).uniform(-0.05, 0.05, X.shape) * np.array([1, 1, 0])
    return {"cfg": cfg, "X": X, "Q": _quats(8, 6), "a": a, "eta": 1.0, "dt": 0.01}


SHAPES = {
    "3x12": lambda: _three(12, 0.4),          # 36 blobs, one tile of 64 lanes
    "packed_8x42": _packed,                   # overlapping blobs, blobs below h = a
    "3x642": lambda: _three(642, 0.15),       # N_blb > 512: two chunks; > 128: three tiles of 256 lanes
}


def _ctx(c, wall, kBT=1.0, dt=None):
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"] if dt is None else dt, kBT=kBT,
                        stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    return ctx


def _positions(ctx, nb, nblb):
    import torch
    r = torch.empty(3 * nb * nblb, dtype=torch.float64, device="cuda:0")
    ctx.blob_positions(0, nb, r.data_ptr())
    ctx.sync_check()
    return r.cpu().numpy().reshape(-1, 3)


def _between_bodies(r, nblb):
    """distances between blobs of different bodies"""
    nb = r.shape[0] // nblb
    return np.concatenate([np.linalg.norm(r[i * nblb:(i + 1) * nblb, None] - r[None, j * nblb:(j + 1) * nblb], axis=2).ravel()
                           for i in range(nb) for j in range(i + 1, nb)])


def _lj_table(lo, hi, n, eps=1.5):
    """a Lennard-Jones-like law with its minimum inside (lo, hi), shifted to U(hi) = 0 -> (U, dU, lo, hi)"""
    sig = (lo + 0.25 * (hi - lo)) / 2.0 ** (1.0 / 6.0)
    x = np.linspace(lo, hi, n)

    def U(r):
        s6 = (sig / r) ** 6
        return 4 * eps * (s6 * s6 - s6)

    s6 = (sig / x) ** 6
    return U(x) - U(hi), -24 * eps * (2 * s6 * s6 - s6) / x, lo, hi


def _soft_table(lo, hi, n, eps=2.0):
    """a screened repulsion in the height, shifted to U(hi) = 0 -> (U, dU, lo, hi)"""
    b = 0.3 * (hi - lo)
    x = np.linspace(lo, hi, n)
    return eps * (np.exp(-(x - lo) / b) - np.exp(-(hi - lo) / b)), -eps / b * np.exp(-(x - lo) / b), lo, hi


def _builtin(a, r_cut):
    return dict(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=r_cut)


def _apply(ctx, builtin=None, pair=None, height=None, traps=None):
    """switch the context's model to exactly these terms (a context whose built-in term was never set keeps r_cut = 0)"""
    if builtin is not None:
        ctx.set_interactions(**builtin)
    elif ctx.interaction_params()["on"]:
        ctx.set_interactions(**{k: v for k, v in ctx.interaction_params().items() if k not in ("on", "a")}, on=False)
    if pair is not None:
        ctx.set_pair_table(*pair)
    else:
        ctx.set_pair_table(None, None, 0.0, 0.0, on=False)
    if height is not None:
        ctx.set_height_table(*height)
    else:
        ctx.set_height_table(None, None, 0.0, 0.0, on=False)
    if traps is not None:
        ctx.set_traps(*traps)
    else:
        ctx.set_traps(None, None, on=False)


def _check(ctx, r, c, nblb, wall, **terms):
    """forces, body forces / torques and energy against the oracle, to 1e-12 of the largest magnitude -> (ordered pairs, oracle's)"""
    _apply(ctx, **terms)
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    fo, FTo, Eo, npo = table_oracle.interactions(r, c["X"], nblb, c["a"], wall, **terms)
    pp = ctx.interaction_stats()[1]
    print("  %-28s |f|max %.3e |FT|max %.3e E %.6e  df %.1e dFT %.1e dE %.1e  pairs %d" % (
        "+".join(sorted(terms)), np.abs(fo).max(), np.abs(FTo).max(), Eo, np.abs(f - fo).max(), np.abs(FT - FTo).max(), abs(E - Eo), pp))
    assert np.abs(f - fo).max() <= 1e-12 * np.abs(fo).max()
    assert np.abs(FT - FTo).max() <= 1e-12 * np.abs(FTo).max()
    assert abs(E - Eo) <= 1e-12 * abs(Eo)
    assert pp == npo
    return pp


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", [2, 17, 65537])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_term_agrees_with_the_all_pairs_oracle(shape, n):
    c = SHAPES[shape]()
    nb, nblb, a = c["X"].shape[0], c["cfg"].shape[0], c["a"]
    ctx = _ctx(c, True)
    r = _positions(ctx, nb, nblb)
    d = _between_bodies(r, nblb)
    # r_min above the smallest distance between blobs of different bodies (the tangent branch), r_cut below the largest (the skip)
    r_min, r_cut = d.min() + 0.1 * (d.max() - d.min()), d.min() + 0.45 * (d.max() - d.min())
    assert d.min() < r_min < r_cut < d.max()
    assert (d < r_min).any() and ((d > r_min) & (d < r_cut)).any() and (d > r_cut).any()
    z = r[:, 2]
    h_min, h_cut = z.min() + 0.2 * (z.max() - z.min()), z.min() + 0.7 * (z.max() - z.min())
    assert (z < h_min).any() and ((z > h_min) & (z < h_cut)).any() and (z > h_cut).any()
    if shape == "packed_8x42":
        assert d.min() < 2 * a and z.min() < a
    pair, height = _lj_table(r_min, r_cut, n), _soft_table(h_min, h_cut, n)
    print("%s n=%d: r_min %.4f r_cut %.4f of [%.4f, %.4f], h_min %.4f h_cut %.4f" % (shape, n, r_min, r_cut, d.min(), d.max(), h_min, h_cut))
    pp_t = _check(ctx, r, c, nblb, True, pair=pair)                                          # the table alone: ia_r_cut is still 0
    assert pp_t == 2 * int((d <= r_cut).sum())
    rc_small, rc_large = max(2 * a, 0.6 * r_cut), 1.3 * r_cut
    assert 2 * a <= rc_small < r_cut < rc_large < d.max() and (d < rc_small).any()
    assert _check(ctx, r, c, nblb, True, pair=pair, builtin=_builtin(a, rc_small)) == pp_t    # the table's cutoff the larger one
    assert _check(ctx, r, c, nblb, True, pair=pair, builtin=_builtin(a, rc_large)) > pp_t     # ... then the smaller one
    _check(ctx, r, c, nblb, True, height=height, builtin=_builtin(a, rc_small))               # beside the wall repulsion
    k = np.tile([[1.5, 0.0, 0.7]], (nb, 1)) * (1.0 + np.arange(nb))[:, None]                  # no trap along y
    k[nb - 1] = [0.0, 2.0, 0.0]
    traps = (k, c["X"] + np.random.default_rng(3).uniform(-0.3, 0.3, c["X"].shape))
    _check(ctx, r, c, nblb, True, traps=traps)
    _check(ctx, r, c, nblb, True, traps=traps, pair=pair, height=height, builtin=_builtin(a, rc_small))
    ctx.close()
    free = _ctx(c, False)                                                                      # the height table without the wall
    rf = _positions(free, nb, nblb)
    _check(free, rf, c, nblb, False, height=height)
    _check(free, rf, c, nblb, False, height=height, builtin=_builtin(a, rc_small))
    free.close()


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape", ["3x12", "packed_8x42"])
def test_cull_under_the_larger_cutoff_is_exact_and_results_are_bitwise_reproducible(shape):
    c = SHAPES[shape]()
    nb, nblb, a = c["X"].shape[0], c["cfg"].shape[0], c["a"]
    ctx = _ctx(c, True)
    d = _between_bodies(_positions(ctx, nb, nblb), nblb)
    r_cut = d.min() + 0.45 * (d.max() - d.min())
    builtin = _builtin(a, max(2 * a, 0.5 * r_cut))
    assert builtin["r_cut"] < r_cut                                     # the table's cutoff is the larger one
    assert (d > builtin["r_cut"]).any() and ((d > builtin["r_cut"]) & (d < r_cut)).any()
    _apply(ctx, builtin=builtin, pair=_lj_table(d.min() + 0.1 * (d.max() - d.min()), r_cut, 17))
    f1, FT1 = ctx.interaction_forces()
    E1 = ctx.interaction_energy()
    bp1, pp1 = ctx.interaction_stats()
    f2, FT2 = ctx.interaction_forces()
    assert np.array_equal(f1, f2) and np.array_equal(FT1, FT2)
    ctx.set_option("interaction_cull", 0)
    f0, FT0 = ctx.interaction_forces()
    E0 = ctx.interaction_energy()
    bp0, pp0 = ctx.interaction_stats()
    assert bp0 == nb * (nb - 1) and pp0 == pp1 == 2 * int((d <= r_cut).sum())
    assert np.array_equal(f0, f1) and np.array_equal(FT0, FT1) and E0 == E1
    ctx.close()


def test_cull_keeps_the_pairs_only_the_table_reaches():
    """two shell_N_12 whose surfaces are further apart than the built-in cutoff and closer than the table's: a neighbour list
    built with the built-in cutoff would drop the pair"""
    c = _three(12, 1.2)
    c["X"], c["Q"] = c["X"][:2], c["Q"][:2]
    a = c["a"]
    ctx = _ctx(c, True)
    r = _positions(ctx, 2, 12)
    d = _between_bodies(r, 12)
    R = np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max()
    builtin = _builtin(a, 2 * a)
    r_cut = d.min() + 0.5 * (d.max() - d.min())
    assert np.linalg.norm(c["X"][0] - c["X"][1]) > 2 * R + builtin["r_cut"] + 0.1 and d.min() > builtin["r_cut"]
    pair = _lj_table(0.9 * d.min(), r_cut, 17)
    for cull in (1, 0):
        ctx.set_option("interaction_cull", cull)
        assert _check(ctx, r, c, 12, True, builtin=builtin, pair=pair) == 2 * int((d <= r_cut).sum()) > 0
        assert ctx.interaction_stats()[0] == 2
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 3
def test_the_builtin_steric_law_through_a_table_stays_within_the_hermite_bounds():
    """U(r) = eps (2a / r) exp(-(r - 2a) / b) tabulated on [2a, r_cut] against the built-in term.  With A = eps 2a exp(2a / b) and
    c = 1 / b, U = A exp(-c r) / r and U'''' = A exp(-c r) (c^4 / r + 4 c^3 / r^2 + 12 c^2 / r^3 + 24 c / r^4 + 24 / r^5), largest
    at r = 2a.  Cubic Hermite on a grid of spacing h: |U - H| <= h^4 / 384 max|U''''|, |U' - H'| <= sqrt(3) / 216 h^3 max|U''''|.
    Below 2a both are the same tangent."""
    c = _packed()
    nb, nblb, a = 8, 42, c["a"]
    eps, b, n = 2.0, 0.1, 129
    r_cut = 2 * a + 10 * b
    ctx = _ctx(c, True)
    r = _positions(ctx, nb, nblb)
    ctx.set_interactions(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=eps, b_blob=b, r_cut=r_cut)
    f_ref, FT_ref = ctx.interaction_forces()
    E_ref = ctx.interaction_energy()
    pp_ref = ctx.interaction_stats()[1]
    x = np.linspace(2 * a, r_cut, n)
    U = eps * (2 * a / x) * np.exp(-(x - 2 * a) / b)
    ctx.set_interactions(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=0.0, b_blob=b, r_cut=r_cut)
    ctx.set_pair_table(U, -U * (1.0 / x + 1.0 / b), 2 * a, r_cut)
    f, FT = ctx.interaction_forces()
    E = ctx.interaction_energy()
    pp = ctx.interaction_stats()[1]
    assert pp == pp_ref > 0
    h, cc, r0 = (r_cut - 2 * a) / (n - 1), 1.0 / b, 2 * a
    U4 = eps * (cc ** 4 + 4 * cc ** 3 / r0 + 12 * cc ** 2 / r0 ** 2 + 24 * cc / r0 ** 3 + 24 / r0 ** 4)       # U''''(2a)
    bound_U, bound_F = h ** 4 / 384 * U4, np.sqrt(3) / 216 * h ** 3 * U4
    # pairs per blob inside r_cut: the force on a blob sums that many pair forces, each off by at most bound_F per component
    body = np.arange(nb * nblb) // nblb
    dist = np.linalg.norm(r[:, None, :] - r[None, :, :], axis=2)
    inside = (dist <= r_cut) & (body[:, None] != body[None, :])
    assert (dist[inside] < 2 * a).any() and (dist[inside] > 2 * a).any() and inside.sum() == pp
    per_blob = inside.sum(axis=1)
    round_f, round_E = 1e-12 * np.abs(f_ref).max(), 1e-12 * abs(E_ref)
    df, dE = np.abs(f - f_ref).max(axis=1), abs(E - E_ref)
    print("dE %.3e (bound %.3e), max df %.3e (bound %.3e at that blob), U'''' %.3e, h %.3e" % (
        dE, 0.5 * pp * bound_U, df.max(), per_blob[df.argmax()] * bound_F, U4, h))
    assert dE <= 0.5 * pp * bound_U + round_E                       # every ordered pair carries half its energy
    assert (df <= per_blob * bound_F + round_f).all()
    assert dE > 10 * round_E and df.max() > 10 * round_f             # the comparison is not one of a law with itself
    # overlapping blobs alone: a blob all of whose partners are below 2a sees the same tangent in both constructions
    only_inner = (per_blob > 0) & (np.where(inside, dist, 0.0).max(axis=1) < 2 * a)
    if only_inner.any():
        assert (df[only_inner] <= round_f).all()
    ctx.close()


def test_below_two_a_the_table_and_the_builtin_tangent_coincide():
    """two shell_N_12 pushed into each other until every pair inside the cutoff is an overlap (r < 2a): agreement to rounding"""
    c = _three(12, 0.0)
    c["X"], c["Q"] = c["X"][:2].copy(), c["Q"][:2]
    a = c["a"]
    c["X"][1] = c["X"][0] + [0.35 * a, 0.1 * a, 0.05 * a]
    eps, b = 2.0, 0.1
    r_cut = 2 * a * (1 + 1e-9)
    ctx = _ctx(c, True)
    r = _positions(ctx, 2, 12)
    d = _between_bodies(r, 12)
    assert (d < 2 * a).any() and not ((d >= 2 * a) & (d <= r_cut)).any()
    ctx.set_interactions(eps_blob=eps, b_blob=b, r_cut=r_cut)
    f_ref, FT_ref = ctx.interaction_forces()
    E_ref = ctx.interaction_energy()
    x = np.linspace(2 * a, r_cut, 2)
    U = eps * (2 * a / x) * np.exp(-(x - 2 * a) / b)
    ctx.set_interactions(eps_blob=0.0, b_blob=b, r_cut=r_cut)
    ctx.set_pair_table(U, -U * (1.0 / x + 1.0 / b), 2 * a, r_cut)
    f, FT = ctx.interaction_forces()
    assert np.abs(f_ref).max() > 1.0
    assert np.abs(f - f_ref).max() <= 1e-12 * np.abs(f_ref).max() and np.abs(FT - FT_ref).max() <= 1e-12 * np.abs(FT_ref).max()
    assert abs(ctx.interaction_energy() - E_ref) <= 1e-12 * abs(E_ref)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 4
def test_generalised_forces_are_minus_the_energy_gradient_with_all_four_terms_on():
    """test_interactions_gpu's central differences through rbl_update_X_Q, every one of the 6 N_bod components"""
    c = _packed()
    sel = [0, 1, 4, 5]
    c["X"], c["Q"] = c["X"][sel], c["Q"][sel]
    nb, a = len(sel), c["a"]
    ctx = _ctx(c, True)
    r = _positions(ctx, nb, 42)
    d, z = _between_bodies(r, 42), r[:, 2]
    pair = _lj_table(d.min() + 0.1 * (d.max() - d.min()), d.min() + 0.6 * (d.max() - d.min()), 513)
    height = _soft_table(z.min() + 0.2 * (z.max() - z.min()), z.min() + 0.7 * (z.max() - z.min()), 513)
    traps = (np.array([[1.0, 0.0, 2.0], [0.5, 1.5, 0.0], [0.0, 0.0, 0.0], [3.0, 3.0, 3.0]]), c["X"] + 0.2)
    _apply(ctx, builtin=_builtin(a, 2 * a + 1.0), pair=pair, height=height, traps=traps)
    assert ctx.interactions_active() == 15
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
    ctx.set_config(X0, Q0)
    assert np.abs(FT).max() > 1.0
    assert np.abs(FT + g).max() <= 1e-6 * np.abs(FT).max(), np.abs(FT + g).max() / np.abs(FT).max()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 5
def _new_terms(c, r, nblb):
    d, z = _between_bodies(r, nblb), r[:, 2]
    nb = c["X"].shape[0]
    # eps: the table's core is steep at r_min; a step must not throw the bodies across the box
    return dict(pair=_lj_table(d.min() + 0.1 * (d.max() - d.min()), d.min() + 0.6 * (d.max() - d.min()), 257, eps=0.002),
                height=_soft_table(z.min() + 0.2 * (z.max() - z.min()), z.min() + 0.7 * (z.max() - z.min()), 257),
                traps=(np.tile([0.8, 0.0, 1.2], (nb, 1)), c["X"] + [0.3, 0.1, -0.2]))


def test_a_deterministic_step_adds_the_new_terms_at_qn():
    c = _three(12, 0.4)
    ctx = _ctx(c, True)
    terms = _new_terms(c, _positions(ctx, 3, 12), 12)
    _apply(ctx, **terms)
    assert not ctx.interaction_params()["on"] and ctx.interactions_on()
    _, FT = ctx.interaction_forces()
    assert np.abs(FT).max() > 0.1
    ctx.step_deterministic(np.zeros(18), max_iter=80, rtol=1e-12)
    Xa, Qa = ctx.get_config(3)
    ctx.close()
    ref = _ctx(c, True)                                     # the terms off, the caller passing -FT (reference convention)
    ref.step_deterministic(-FT, max_iter=80, rtol=1e-12)
    Xb, Qb = ref.get_config(3)
    ref.close()
    assert np.abs(np.reshape(Xa, (3, 3)) - c["X"]).max() > 1e-5
    assert np.abs(Xa - Xb).max() <= 1e-12 and np.abs(Qa - Qb).max() <= 1e-12


def test_the_free_slots_of_a_mask_feel_the_new_terms():
    """RigidBody.step_mixed with body 0 held: the model loads the free bodies only (rbl_mixed.hip, mx_upload) -- the same step as
    one without the model whose caller passes the model's loads in the free slots"""
    from rigid_body_light_amd import RigidBody
    c = _three(12, 0.4)
    probe = _ctx(c, True)
    terms = _new_terms(c, _positions(probe, 3, 12), 12)
    probe.close()
    mask = np.array([True, False, False])
    out = []
    for with_model in (True, False):
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=True)
        body_in = np.zeros(18)
        if with_model:
            rb.set_pair_table(*terms["pair"])
            rb.set_height_table(*terms["height"])
            rb.set_traps(*terms["traps"])
            loads = rb.interaction_forces()              # reference convention, -K^T f_phys
            assert np.abs(loads).max() > 0.1
        else:
            body_in[6:] = loads[6:]
        rb.step_mixed(mask, body_in, max_iter=100, rtol=1e-12)
        out.append(rb.get_config())
    assert np.array_equal(out[0][0][0], c["X"][0])           # the held body stays
    assert np.abs(out[0][0][1:] - c["X"][1:]).max() > 1e-5
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-12 and np.abs(out[0][1] - out[1][1]).max() <= 1e-12


def test_a_body_displaced_from_its_trap_centre_moves_towards_it():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    c = {"cfg": cfg, "X": np.array([[0.1, -0.2, 3.0]]), "Q": np.array([[0.9, 0.1, 0.3, -0.2]]), "a": p["sep"] / 2.0, "eta": 1.0, "dt": 0.05}
    X0 = c["X"] + [0.4, 0.0, -0.3]
    ctx = _ctx(c, False)
    ctx.set_traps(np.array([[2.0, 2.0, 2.0]]), X0)
    assert ctx.interactions_on() and ctx.interactions_active() == 8
    ctx.step_deterministic(np.zeros(6), max_iter=50, rtol=1e-12)
    X = ctx.get_config(1)[0].reshape(1, 3)
    ctx.close()
    move = X - c["X"]
    assert move[0, 0] > 1e-4 and move[0, 2] < -1e-4 and abs(move[0, 1]) < 1e-3 * abs(move[0, 0])
    assert np.linalg.norm(X - X0) < np.linalg.norm(c["X"] - X0)


@pytest.mark.parametrize("kind", ["deterministic", "brownian"])
def test_switched_off_the_new_terms_leave_no_trace(kind):
    c = _three(12, 0.4)
    out = []
    for had in (True, False):
        ctx = _ctx(c, True, kBT=0.1)
        if had:                                              # on, evaluated, off again
            terms = _new_terms(c, _positions(ctx, 3, 12), 12)
            _apply(ctx, **terms)
            assert np.abs(ctx.interaction_forces()[1]).max() > 0.0
            ctx.set_pair_table(*terms["pair"], on=False)
            ctx.set_height_table(*terms["height"], on=False)
            ctx.set_traps(*terms["traps"], on=False)
            assert not ctx.interactions_on()
        F = np.tile([0.0, 0.0, 0.3, 0.0, 0.0, 0.0], 3)
        if kind == "deterministic":
            ctx.step_deterministic(F, max_iter=50, rtol=1e-10)
        else:
            ctx.step_brownian(F, max_iter=50, rtol=1e-10, seed=3, method=2)
        out.append(ctx.get_config(3))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------------------ 6
def _replicas(R):
    """R replicas of the three-shell triangle, each with its own jitter and orientations"""
    c = _three(12, 0.4)
    rng = np.random.default_rng(21)
    X = c["X"][None] + rng.uniform(-0.08, 0.08, (R, 3, 3))
    Q = np.stack([_quats(3, 30 + r) for r in range(R)])
    return c, X, Q


@functools.lru_cache(maxsize=None)
def _ens_pair_table():
    return _lj_table(1.0, 2.2, 257, eps=0.02)


def _ens(c, X, Q, traps, kBT=1.0):
    from rigid_body_light_amd import Ensemble
    e = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=kBT, wall=True)
    e.set_pair_table(*_ens_pair_table())
    e.set_traps(*traps)
    return e


def _trap_layouts(X):
    R = X.shape[0]
    k = np.array([[1.0, 0.0, 2.0], [0.5, 1.5, 0.0], [2.0, 2.0, 2.0]])
    shared = (k, X[0] + 0.2)
    per_replica = (k[None] * (1.0 + np.arange(R))[:, None, None], X + np.random.default_rng(2).uniform(-0.3, 0.3, X.shape))
    return {"shared": shared, "per_replica": per_replica}


@pytest.mark.parametrize("layout", ["shared", "per_replica"])
def test_ensemble_forces_are_the_single_context_forces_of_each_replica(layout):
    R = 3
    c, X, Q = _replicas(R)
    traps = _trap_layouts(X)[layout]
    ens = _ens(c, X, Q, traps)
    FTe, Ee = ens.interaction_forces(), ens.interaction_energy()
    ens.close()
    assert FTe.shape == (R, 18) and Ee.shape == (R,)
    for rep in range(R):
        s = _ctx(dict(c, X=X[rep], Q=Q[rep]), True)
        s.set_pair_table(*_ens_pair_table())
        k, X0 = traps if layout == "shared" else (traps[0][rep], traps[1][rep])
        s.set_traps(k, X0)
        _, FT = s.interaction_forces()
        E = s.interaction_energy()
        assert s.interaction_stats()[1] > 0
        # the oracle too, so that the two cannot be wrong together
        _, FTo, Eo, _ = table_oracle.interactions(_positions(s, 3, 12), X[rep], 12, c["a"], True, pair=_ens_pair_table(), traps=(k, X0))
        s.close()
        assert np.abs(FTe[rep] + FT).max() <= 1e-12 * max(1.0, np.abs(FT).max())      # reference convention: -K^T f_phys
        assert abs(Ee[rep] - E) <= 1e-12 * max(1.0, abs(E))
        assert np.abs(FT - FTo).max() <= 1e-12 * np.abs(FTo).max() and abs(E - Eo) <= 1e-12 * abs(Eo)


def test_an_ensemble_refuses_traps_of_another_length():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = _replicas(3)
    ens = _ens(c, X, Q, _trap_layouts(X)["shared"])
    ens.ctx.set_traps(np.ones((2, 3)), np.zeros((2, 3)))      # neither N_bod = 3 nor R N_bod = 9 entries
    with pytest.raises(RblError, match="status 7"):            # RBL_ERR_STATE
        ens.interaction_forces()
    with pytest.raises(RblError, match="status 7"):
        ens.step_deterministic(np.zeros(18))
    Xa, Qa = ens.get_config()
    assert np.array_equal(Xa, X)                               # nothing moved
    ens.close()


@pytest.mark.parametrize("layout", ["shared", "per_replica"])
@pytest.mark.parametrize("family", ["brownian", "deterministic"])
def test_an_ensemble_run_with_the_new_terms_is_the_loop_bitwise(family, layout):
    R, steps = 3, 5
    c, X, Q = _replicas(R)
    traps = _trap_layouts(X)[layout]
    F = 0.2 * np.random.default_rng(11).standard_normal((R, 18))
    kw = dict(max_iter=50, rtol=1e-8)
    ens = _ens(c, X, Q, traps)
    for n in range(steps):
        if family == "brownian":
            ens.step_brownian(F, seed=40 + n, **kw)
        else:
            ens.step_deterministic(F, **kw)
    Xl, Ql = ens.get_config()
    ens.close()
    ens = _ens(c, X, Q, traps)
    out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, stride=5, **kw)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(out.accepted, np.full(R, steps))
    assert np.array_equal(Xr, Xl) and np.array_equal(Qr, Ql)
    assert np.array_equal(out.X[0], Xl) and np.array_equal(out.Q[0], Ql)
    # ... and not the run of an ensemble without them
    from rigid_body_light_amd import Ensemble
    bare = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=True)
    bare.run(steps, F=F, brownian=family == "brownian", seed=40, **kw)
    assert np.abs(bare.get_config()[0] - Xr).max() > 1e-6
    bare.close()


# ------------------------------------------------------------------------------------------------------------ 7
def test_equipartition_in_a_harmonic_trap():
    """R = 256 replicas of one shell_N_12 in free space at kBT = 1 in an isotropic trap of stiffness k; mu = 1 / (6 pi eta R_h) with
    R_h from the structure file, dt from k mu dt = 0.02.  500 steps of burn-in from the trap centre, then 1500 steps in one run with
    a frame every 50.  v = k <(X - X0)^2> / kBT per axis; its standard error from the spread of the per-replica means (the replicas
    are independent).  |v - 1| <= 4 SE + k mu dt: the allowance is twice the forward-Euler bias k mu dt / 2 of an
    Ornstein-Uhlenbeck process (the force is taken at q^n).  SE <= 0.02, so the test cannot pass by being noisy.
    The trap sits at z = 50, a hundred thermal excursions (sqrt(kBT / k) = 0.5) above z = a: the Brownian root follows the
    reference's M_half_W (c_rigid_obj.cpp:667-669), which scales the noise of a blob below z = a by z / a with or without the
    wall, so a free-space run has to stay above that height to sample at kBT (with the centre at z = 0.5 the same run gave
    v = 0.51, and a run without any trap half the free diffusion coefficient)."""
    from rigid_body_light_amd import Ensemble, load_structure
    p, cfg = load_structure(12)
    a, eta, kBT, k, R = p["sep"] / 2.0, 1.0, 1.0, 4.0, 256
    mu = 1.0 / (6 * np.pi * eta * p["Rh"])
    dt = 0.02 / (k * mu)
    X0 = np.array([0.3, -0.4, 50.0])
    X = np.tile(X0, (R, 1, 1))
    Q = _quats(R, 17).reshape(R, 1, 4)
    ens = Ensemble(cfg, X, Q, a=a, eta=eta, dt=dt, kBT=kBT, wall=False)
    ens.set_traps(np.full((1, 3), k), X0.reshape(1, 3))
    ens.run(500, F=np.zeros(6), seed=1000, max_iter=50, rtol=1e-8)
    out = ens.run(1500, F=np.zeros(6), seed=5000, stride=50, max_iter=50, rtol=1e-8)
    ens.close()
    assert out.X.shape == (30, R, 1, 3) and np.array_equal(out.accepted, np.full(R, 1500))
    per_rep = k * ((out.X[:, :, 0, :] - X0) ** 2).mean(axis=0) / kBT           # (R, 3): one sample per replica and axis
    v, se = per_rep.mean(axis=0), per_rep.std(axis=0, ddof=1) / np.sqrt(R)
    print("k <dx^2> / kBT per axis %s, SE %s, allowance %s" % (v, se, 4 * se + k * mu * dt))
    assert (se <= 0.02).all()
    assert (np.abs(v - 1.0) <= 4 * se + k * mu * dt).all()


# ------------------------------------------------------------------------------------------------------------ 8
def test_example_tabulated_potentials_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tabulated_potentials.py"), "--replicas", "16", "--steps", "40"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "trap" in out.stdout and "pair energy" in out.stdout
