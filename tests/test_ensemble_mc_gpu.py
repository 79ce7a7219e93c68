"""Metropolis sampling of the force model on the GPU (include/rbl.h section 5, rbl_ensemble_mc; Ensemble.metropolis): every traced
trial's energy change and verdict against the numpy oracle (tests/mc_oracle.py), the shapes at which the kernel takes another path,
periodic cells, the bitwise contracts, the stationary distribution against a quadrature, and the wall."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_shapes  # noqa: E402
import mc_oracle  # noqa: E402

TOL = 1e-12                  # tests/test_interactions_gpu.py's bound on the energy against the same kind of oracle


def _shell():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return p["sep"] / 2.0, np.asarray(cfg, dtype=np.float64).reshape(-1, 3)


def _quats(shape, seed):
    Q = np.random.default_rng(seed).standard_normal(shape + (4,))
    return Q / np.linalg.norm(Q, axis=-1, keepdims=True)


def _ens(cfg, a, X, Q, wall=True, kBT=1.0):
    from rigid_body_light_amd import Ensemble
    return Ensemble(cfg, X, Q, a=a, eta=1.0, dt=0.01, kBT=kBT, wall=wall)


def _tab(f, df, lo, hi, n):
    x = np.linspace(lo, hi, n)
    return f(x), df(x), lo, hi


def _builtin(a, w=0.5, r_cut=None):
    return dict(w=w, eps_wall=4.0, b_wall=0.1, eps_blob=3.0, b_blob=0.2, r_cut=3.0 * a if r_cut is None else r_cut)


def _check(ens, models, cfg, X0, Q0, res, kBT, n_dE=None, full=True):
    """the checks of a traced chain, replica by replica (models[r]: the oracle's model of replica r) -> the largest |dE - oracle| /
    scale, and the verdicts that occurred"""
    Xe, Qe = ens.get_config()
    E_end = ens.interaction_energy()
    worst, seen = 0.0, set()
    for r in range(X0.shape[0]):
        tr = res.trace[r]
        n = int((tr[:, 0] >= 0).sum())
        assert n == min(res.tried[r], tr.shape[0])
        dEo, scale, below, Xr, Qr = mc_oracle.replay(models[r], cfg, X0[r], Q0[r], tr[:n])
        v = tr[:n, 9].astype(int)
        seen |= set(v.tolist())
        assert np.array_equal(v == 2, below), "a trial is rejected at the wall iff the proposal puts a blob below z = 0"
        ev = v != 2
        m = min(n, n_dE or n)
        dev = np.abs(tr[:m, 7] - dEo[:m])[ev[:m]] / scale[:m][ev[:m]]
        if dev.size:
            worst = max(worst, dev.max())
        assert (dev <= TOL).all(), (r, dev.max())
        kT = np.broadcast_to(kBT, (X0.shape[0],))[r]
        dE, u6 = tr[:n, 7][ev], tr[:n, 8][ev]
        with np.errstate(over="ignore"):
            p = np.exp(-dE / kT)
        assert not ((dE > 0.0) & (np.abs(u6 - p) < 1e-12)).any(), "a verdict too close to call: choose another seed"
        assert np.array_equal(v[ev] == 1, (dE <= 0.0) | (u6 < p))
        assert (v == 1).sum() <= res.accepted[r] and (v == 2).sum() <= res.wall_rejected[r]
        if full:
            assert n == res.tried[r] and (v == 1).sum() == res.accepted[r] and (v == 2).sum() == res.wall_rejected[r]
            assert np.abs(Xr - Xe[r]).max() <= 1e-12 and np.abs(Qr - Qe[r]).max() <= 1e-12
            bound = TOL * np.nanmax(scale) * max(1, int(res.accepted[r]))
            assert abs(res.energy_end[r] - E_end[r]) <= bound, (r, res.energy_end[r], E_end[r], bound)
    print("largest |dE - oracle| / scale: %.3g" % worst)
    return worst, seen


# ---- 1. trace against the oracle -------------------------------------------------------------------------------------------------
def _case_a(R=3, seed=1):
    a, cfg = _shell()
    Rb = body_shapes.radius(cfg - cfg.mean(axis=0))
    rng = np.random.default_rng(seed)
    X = np.array([[0.0, 0.0, 0.0], [2.0 * Rb + 0.6, 0.0, 0.0], [Rb + 0.3, 2.0 * Rb + 0.3, 0.3]]) + [0.0, 0.0, Rb + 0.15]
    X = X[None] + rng.uniform(-0.05, 0.05, (R, 3, 3))
    Q = _quats((R, 3), seed + 1)
    builtin = _builtin(a)
    pair = _tab(lambda r: -0.8 * np.exp(-(r - 2 * a) ** 2), lambda r: 1.6 * (r - 2 * a) * np.exp(-(r - 2 * a) ** 2), 0.1, 4.0 * a, 129)
    height = _tab(lambda z: 0.3 * (z - 1.0) ** 2, lambda z: 0.6 * (z - 1.0), 0.2, 3.0, 65)
    k = np.tile([0.5, 0.0, 3.0], (R, 3, 1)) * (1.0 + 0.5 * np.arange(R))[:, None, None]
    X0t = X + rng.uniform(-0.2, 0.2, X.shape) - [0.0, 0.0, 0.1]
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(**builtin)
    ens.set_pair_table(*pair)
    ens.set_height_table(*height)
    ens.set_traps(k, X0t)
    models = [dict(a=a, wall=True, builtin=builtin, pair=pair, height=height, traps=(k[r], X0t[r])) for r in range(R)]
    return ens, models, cfg, X, Q


def _case_b(R=3, seed=4):
    from rigid_body_light_amd import patch_types
    a, cfg = _shell()
    c0 = cfg - cfg.mean(axis=0)
    Rb = body_shapes.radius(c0)
    rng = np.random.default_rng(seed)
    d = 2.0 * Rb + 0.5
    X = np.array([[0.0, 0.0, 0.0], [d, 0.0, 0.2], [d, d, 0.0], [0.0, d, 0.3]]) + [0.0, 0.0, Rb + 1.0]
    X = X[None] + rng.uniform(-0.05, 0.05, (R, 4, 3))
    Q = _quats((R, 4), seed + 1)
    builtin = _builtin(a, w=0.2)
    types = np.asarray(patch_types(cfg, [0.0, 0.0, 1.0])).astype(int)
    tables = {(0, 0): _tab(lambda r: 0.6 / (r + 0.3), lambda r: -0.6 / (r + 0.3) ** 2, 0.0, 3.5 * a, 65),
              (0, 1): _tab(lambda r: -1.2 * np.exp(-r), lambda r: 1.2 * np.exp(-r), 0.2, 4.5 * a, 65)}
    body = np.array([[0, 1], [1, 2], [2, 3], [3, -1]])
    anchor_a = np.array([c0[0], c0[3], c0[7], c0[5]])
    anchor_b = np.array([c0[6], c0[1], c0[2], [0.0, d, 0.5]])
    kind = np.array([0, 1, 0, 0])
    kk = np.array([2.0, 1.5, 1.0, 0.8])[None] * (1.0 + np.arange(R))[:, None]
    l0 = np.tile([1.0, 0.0, 1.5, 0.5], (R, 1)) + 0.1 * np.arange(R)[:, None]
    btab = _tab(lambda x: 0.5 * (x - 1.0) ** 2 + 0.1 * x, lambda x: (x - 1.0) + 0.1, 0.4, 2.0, 33)
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(**builtin)
    ens.set_blob_types(types, n_types=2)
    for (s, t), tab in tables.items():
        ens.set_type_table(s, t, *tab)
    ens.set_bond_table(*btab)
    ens.set_bonds(body, anchor_a, anchor_b, kk, l0, kind=kind)
    ktr = np.tile([0.3, 0.4, 0.0], (R, 4, 1)) * (1.0 + np.arange(R))[:, None, None]   # traps beside the typed tables and the bond table
    X0t = X + rng.uniform(-0.3, 0.3, X.shape)
    ens.set_traps(ktr, X0t)
    models = [dict(a=a, wall=True, builtin=builtin, types=np.tile(types, 4), tables=tables, traps=(ktr[r], X0t[r]),
                   bonds=dict(body=body, anchor=np.concatenate([anchor_a, anchor_b], axis=1), k=kk[r], l0=l0[r], kind=kind, table=btab))
              for r in range(R)]
    return ens, models, cfg, X, Q


@pytest.mark.parametrize("case", ["a", "b"])
def test_every_traced_trial_against_the_oracle(case):
    ens, models, cfg, X, Q = _case_a() if case == "a" else _case_b()
    nb = X.shape[1]
    E0 = ens.interaction_energy()
    res = ens.metropolis(40, 0.3, 0.4, seed=11, trace=40 * nb)
    assert np.array_equal(res.energy_start, E0) and (res.tried == 40 * nb).all()
    _, seen = _check(ens, models, cfg, X, Q, res, 1.0)
    if case == "a":
        assert seen == {0, 1, 2}, seen
    else:
        assert {0, 1} <= seen
    ens.close()


# ---- 2. shapes -------------------------------------------------------------------------------------------------------------------
def _most(nblb):
    """the most bodies of nblb blobs an ensemble accepts (rbl_ensemble_set_config: the one-kernel solver's size rule)"""
    return max(nb for nb in range(1, 65) if body_shapes.small_fits(nblb, nb, 1))


@pytest.mark.parametrize("name,nb", [("shell", 1), ("trimer", 5), ("shell", 0), ("tetra", 0), ("fib130", 1), ("fib100", 2)])
def test_shapes(name, nb):
    """one body alone (no pairs); 5 trimers; as many shells and as many tetrahedra as an ensemble holds (nb = 0: 19 x 12 = 228 blobs
    with a ragged last lane group, 53 x 4 = 212 blobs: more replicas' worth than that is refused by rbl_ensemble_set_config, so 21 shells,
    64 tetrahedra and two bodies of 130 blobs cannot be set); a moved body of more than two waves' worth of lanes; two bodies of more
    than a wave's worth each"""
    a = body_shapes.A
    if nb == 0:
        nb = _most(12 if name == "shell" else 4)
        assert nb * (12 if name == "shell" else 4) >= 200
    cfg = _shell()[1] * (a / _shell()[0]) if name == "shell" else body_shapes.shape(name)
    X, Q = body_shapes.lattice(nb, cfg - cfg.mean(axis=0), True, seed=3)
    R = 2
    X = X[None] + np.random.default_rng(5).uniform(-0.02, 0.02, (R,) + X.shape)
    Q = np.stack([Q, _quats((nb,), 9)])
    builtin = _builtin(a, r_cut=4.0 * a)
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(**builtin)
    sweeps = -(-64 // nb)
    res = ens.metropolis(sweeps, 0.3, 0.4, seed=3, trace=sweeps * nb)
    _check(ens, [dict(a=a, wall=True, builtin=builtin)] * R, cfg, X, Q, res, 1.0, n_dE=64)
    assert res.accepted.min() > 0
    ens.close()


# ---- 3. cells --------------------------------------------------------------------------------------------------------------------
def _across(R):
    a, cfg = _shell()
    Rb = body_shapes.radius(cfg - cfg.mean(axis=0))
    builtin = _builtin(a, r_cut=4.0 * a)
    L = 2.0 * (2.0 * Rb + builtin["r_cut"]) + 1.0
    X = np.tile(np.array([[0.4, 1.0, Rb + 1.0], [L - 2.0 * Rb - 0.5, 1.2, Rb + 1.2]]), (R, 1, 1))   # in range only through the boundary
    X += np.random.default_rng(2).uniform(-0.03, 0.03, X.shape)
    return a, cfg, builtin, L, X, _quats((R, 2), 6)


def test_a_shared_cell_takes_the_minimum_image():
    a, cfg, builtin, L, X, Q = _across(2)
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(**builtin)
    ens.set_cell(L, 0.0)
    m = dict(a=a, wall=True, builtin=builtin, L=(L, 0.0))
    assert mc_oracle.energy_terms(m, cfg, X[0], Q[0])["pairs"] > 1e-3
    assert mc_oracle.energy_terms(dict(m, L=None), cfg, X[0], Q[0])["pairs"] == 0.0
    res = ens.metropolis(20, 0.2, 0.3, seed=2, trace=40)
    _check(ens, [m] * 2, cfg, X, Q, res, 1.0)
    ens.close()


def test_a_cell_per_replica():
    a, cfg, builtin, L, X, Q = _across(3)
    Lx, Ly = np.array([L, L + 1.5, L]), np.array([0.0, L + 2.0, L + 1.0])
    X[1, 1, 0] += 1.5
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(**builtin)
    ens.set_cells(Lx, Ly)
    models = [dict(a=a, wall=True, builtin=builtin, L=(Lx[r], Ly[r])) for r in range(3)]
    for r in range(3):
        assert mc_oracle.energy_terms(models[r], cfg, X[r], Q[r])["pairs"] > 1e-3
    res = ens.metropolis(20, 0.2, 0.3, seed=5, trace=40)
    _check(ens, models, cfg, X, Q, res, 1.0)
    ens.close()


# ---- 4. bitwise contracts --------------------------------------------------------------------------------------------------------
KBT4 = np.array([1.0, 0.7, 1.5, 2.0])


def _rich(replicas):
    """case (b)'s model and a cell per replica, with replica-indexed traps, bond sets and cells, for the named replicas of R = 4"""
    a, cfg = _shell()
    c0 = cfg - cfg.mean(axis=0)
    Rb = body_shapes.radius(c0)
    rng = np.random.default_rng(8)
    d = 2.0 * Rb + 0.5
    X = np.array([[0.0, 0.0, 0.0], [d, 0.0, 0.2], [d, d, 0.0]]) + [0.0, 0.0, Rb + 0.8]
    X = X[None] + rng.uniform(-0.05, 0.05, (4, 3, 3))
    Q = _quats((4, 3), 10)
    builtin = _builtin(a)
    Lx = 2.0 * (2.0 * Rb + builtin["r_cut"]) + 1.0 + np.arange(4.0)
    Ly = Lx[::-1].copy()
    k = np.tile([0.5, 0.2, 1.0], (4, 3, 1)) * (1.0 + np.arange(4))[:, None, None]
    X0t = X + rng.uniform(-0.2, 0.2, X.shape)
    kk = np.array([2.0, 1.0])[None] * (1.0 + np.arange(4))[:, None]
    l0 = np.tile([1.0, 1.5], (4, 1))
    sel = list(replicas)
    ens = _ens(cfg, a, X[sel], Q[sel])
    ens.set_interactions(**builtin)
    ens.set_traps(k[sel], X0t[sel])
    ens.set_bonds([[0, 1], [1, 2]], [c0[0], c0[3]], [c0[6], c0[1]], kk[sel], l0[sel])
    ens.set_cells(Lx[sel], Ly[sel])
    return ens, X[sel], Q[sel]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_reproducible_and_split_chains_and_launches():
    ens, X, Q = _rich(range(4))
    args = dict(step_x=0.3, step_theta=0.4, seed=21, kBT=KBT4)
    ref = ens.metropolis(12, stride=4, **args)
    cfg_ref = ens.get_config()
    ens.set_config(X, Q)
    again = ens.metropolis(12, stride=4, **args)
    assert _same(ens.get_config(), cfg_ref)
    for f in ("tried", "accepted", "wall_rejected", "energy_start", "energy_end", "X", "Q", "E"):
        assert np.array_equal(getattr(ref, f), getattr(again, f)), f
    assert ref.accepted.min() > 0 and (ref.accepted < ref.tried).all()
    # n1 + n2 sweeps; the frames are the configurations of the shorter chains
    ens.set_config(X, Q)
    r1 = ens.metropolis(4, **args)
    assert _same(ens.get_config(), (ref.X[0], ref.Q[0]))
    r2 = ens.metropolis(8, sweep_start=4, **args)
    assert _same(ens.get_config(), cfg_ref) and _same(ens.get_config(), (ref.X[2], ref.Q[2]))
    assert np.array_equal(r1.accepted + r2.accepted, ref.accepted) and np.array_equal(r1.tried + r2.tried, ref.tried)
    assert np.abs(r2.energy_end - ref.energy_end).max() <= 1e-10 and np.array_equal(ref.E[2], ref.energy_end)
    # one sweep per launch
    ens.set_config(X, Q)
    ens.ctx.set_option("mc_sweeps_per_launch", 1)
    one = ens.metropolis(12, stride=4, **args)
    assert _same(ens.get_config(), cfg_ref)
    for f in ("accepted", "wall_rejected", "energy_end", "X", "Q", "E"):
        assert np.array_equal(getattr(ref, f), getattr(one, f)), f
    ens.close()
    # replica r of R = 4 is the R = 1 ensemble of that replica with replica_base = r
    for r in (0, 3):
        e1, _, _ = _rich([r])
        one = e1.metropolis(12, replica_base=r, step_x=0.3, step_theta=0.4, seed=21, kBT=KBT4[r])
        assert _same(e1.get_config(), (cfg_ref[0][r:r + 1], cfg_ref[1][r:r + 1]))
        assert one.accepted[0] == ref.accepted[r] and one.energy_end[0] == ref.energy_end[r]
        e1.close()


def test_frozen_bodies_and_the_step_that_follows():
    ens, Xin, Qin = _rich(range(4))
    X, Q = ens.get_config()                               # (the quaternions as the library normalised them)
    frozen = np.zeros((4, 3), dtype=bool)
    frozen[:, 1] = True
    frozen[2] = True
    E0 = ens.interaction_energy()
    res = ens.metropolis(10, 0.3, 0.4, seed=2, frozen=frozen, kBT=KBT4)
    Xn, Qn = ens.get_config()
    assert np.array_equal(Xn[:, 1], X[:, 1]) and np.array_equal(Qn[:, 1], Q[:, 1])
    assert np.array_equal(Xn[2], X[2]) and np.array_equal(Qn[2], Q[2]) and res.tried[2] == 0 and res.energy_end[2] == E0[2]
    assert np.array_equal(res.tried, [20, 20, 0, 20]) and (Xn[0, 0] != X[0, 0]).any()
    ens.step_brownian(np.zeros(18), seed=5)
    Xa, Qa = ens.get_config()
    ens.close()
    # the step continues as from set_config of the same numbers.  set_config normalises the quaternions again, which moves the last
    # bit of some: the replicas it leaves bit for bit as they were (replicas are independent) must step to the same bits, the others
    # to the same configuration up to that bit's consequence
    fresh, _, _ = _rich(range(4))
    fresh.set_config(Xn, Qn)
    Xs, Qs = fresh.get_config()
    fresh.step_brownian(np.zeros(18), seed=5)
    Xf, Qf = fresh.get_config()
    fresh.close()
    exact = [r for r in range(4) if np.array_equal(Xs[r], Xn[r]) and np.array_equal(Qs[r], Qn[r])]
    assert exact, "no replica whose quaternions the second normalisation leaves alone: choose another seed"
    for r in exact:
        assert np.array_equal(Xf[r], Xa[r]) and np.array_equal(Qf[r], Qa[r]), r
    assert np.abs(Xf - Xa).max() <= 1e-9 and np.abs(Qf - Qa).max() <= 1e-9 and np.abs(Xa - Xn).max() > 1e-4


# ---- 5. distribution -------------------------------------------------------------------------------------------------------------
def _quadrature(c0, a, kT, n, w=0.5, eps=4.0, bw=0.1):
    """<h>, <h^2>, <n.c_0>, <(n.c_0)^2> of one body above the wall under weight and wall repulsion, exp(-U / kT) with every blob at
    z >= 0: the blob heights h + n.c_k depend on the orientation through the lab z axis seen from the body, n, uniform on the sphere
    -- Gauss-Legendre in cos(beta) times a uniform grid in the azimuth --, the height by the trapezoid rule on a fine grid"""
    mu, wmu = np.polynomial.legendre.leggauss(n)
    gam = 2.0 * np.pi * (np.arange(2 * n) + 0.5) / (2 * n)
    s = np.sqrt(1.0 - mu * mu)
    nv = np.stack([np.outer(s, np.cos(gam)), np.outer(s, np.sin(gam)), np.outer(mu, np.ones_like(gam))], axis=-1).reshape(-1, 3)
    wq = np.repeat(wmu, 2 * n)
    off = nv @ c0.T                                       # (orientations, blobs)
    t = np.linspace(0.0, 8.0, 4001)                       # height above the lowest admissible one
    h = -off.min(axis=1)[:, None] + t[None, :]
    z = h[:, :, None] + off[:, None, :]
    U = (w * z + np.where(z >= a, eps * np.exp(-(np.maximum(z, a) - a) / bw), eps + eps / bw * (a - z))).sum(axis=2)
    p = np.exp(-(U - U.min()) / kT) * wq[:, None]
    tw = np.full(t.size, t[1] - t[0])
    tw[[0, -1]] *= 0.5
    p = p * tw[None, :]
    Z = p.sum()
    o = off[:, 0][:, None]
    return np.array([(p * h).sum(), (p * h * h).sum(), (p * o).sum(), (p * o * o).sum()]) / Z


def _reference(c0, a, kT, se):
    fine, coarse = _quadrature(c0, a, kT, 48), _quadrature(c0, a, kT, 32)
    assert (np.abs(fine - coarse) < 0.25 * se).all(), (fine, coarse, se)     # the reference's own error, from two orientation sets
    return fine


def _sample(cfg, a, kBT, seed):
    R = 256
    X = np.tile([[0.0, 0.0, 2.5]], (R, 1, 1))
    ens = _ens(cfg, a, X, _quats((R, 1), seed))
    ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1)
    ens.metropolis(500, 0.4, 0.6, seed=seed, kBT=kBT)
    res = ens.metropolis(1500, 0.4, 0.6, seed=seed, kBT=kBT, sweep_start=500, stride=1)
    ens.close()
    c0 = cfg - cfg.mean(axis=0)
    h = res.X[:, :, 0, 2]                                 # (frames, R)
    q = res.Q[:, :, 0, :]
    row = np.stack([2 * (q[..., 1] * q[..., 3] - q[..., 0] * q[..., 2]), 2 * (q[..., 2] * q[..., 3] + q[..., 0] * q[..., 1]),
                    1 - 2 * (q[..., 1] ** 2 + q[..., 2] ** 2)], axis=-1)
    o = row @ c0[0]
    return np.stack([h.mean(axis=0), (h * h).mean(axis=0), o.mean(axis=0), (o * o).mean(axis=0)], axis=1)   # (R, 4) time averages


def _moments_ok(S, ref, which):
    """mean and variance (from the first two moments, its standard error by the delta method) of the 256 time averages"""
    n = S.shape[0]
    for k in which:
        se = S[:, k].std(ddof=1) / np.sqrt(n)
        print("moment %d: %.5f against %.5f, standard error %.2g" % (k, S[:, k].mean(), ref[k], se))
        assert abs(S[:, k].mean() - ref[k]) <= 4.0 * se, (k, S[:, k].mean(), ref[k], se)
    if 0 in which and 1 in which:
        mu = S[:, 0].mean()
        v = S[:, 1] - 2.0 * mu * S[:, 0]
        var, se = S[:, 1].mean() - mu * mu, v.std(ddof=1) / np.sqrt(n)
        assert abs(var - (ref[1] - ref[0] ** 2)) <= 4.0 * se, (var, ref[1] - ref[0] ** 2, se)


def _se(S):
    return S.std(axis=0, ddof=1) / np.sqrt(S.shape[0])


def test_distribution_of_a_shell_above_the_wall():
    a, cfg = _shell()
    S = _sample(cfg, a, None, 31)
    _moments_ok(S, _reference(cfg - cfg.mean(axis=0), a, 1.0, _se(S)), (0, 1))


def test_distribution_of_a_trimer_exercises_the_rotation_proposal():
    cfg, a = body_shapes.trimer(), body_shapes.A
    S = _sample(cfg, a, None, 32)
    _moments_ok(S, _reference(cfg - cfg.mean(axis=0), a, 1.0, _se(S)), (0, 1, 2, 3))


def test_two_temperatures_in_one_call():
    a, cfg = _shell()
    kBT = np.where(np.arange(256) < 128, 1.0, 2.0)
    S = _sample(cfg, a, kBT, 33)
    c0 = cfg - cfg.mean(axis=0)
    _moments_ok(S[:128], _reference(c0, a, 1.0, _se(S[:128])), (0, 1))
    _moments_ok(S[128:], _reference(c0, a, 2.0, _se(S[128:])), (0, 1))


# ---- 6. wall ---------------------------------------------------------------------------------------------------------------------
def test_a_start_below_the_wall_raises_and_moves_nothing():
    from rigid_body_light_amd._lib import RblError
    a, cfg = _shell()
    X = np.tile([[0.0, 0.0, 2.5]], (3, 1, 1))
    X[1, 0, 2] = 0.2                                      # a blob of replica 1 below z = 0
    Q = _quats((3, 1), 3)
    ens = _ens(cfg, a, X, Q)
    ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1)
    with pytest.raises(RblError, match="replica 1"):
        ens.metropolis(5, 0.3, 0.3)
    Xn, Qn = ens.get_config()
    assert np.array_equal(Xn, X) and np.array_equal(Qn, Q / np.linalg.norm(Q, axis=-1, keepdims=True))
    ens.close()


def test_no_frame_has_a_blob_below_the_wall():
    a, cfg = _shell()
    X = np.tile([[0.0, 0.0, 1.5]], (4, 1, 1))
    ens = _ens(cfg, a, X, _quats((4, 1), 4))
    ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1)
    res = ens.metropolis(60, 2.0, 0.5, seed=9, stride=1)
    assert (res.wall_rejected > 0).all() and (res.accepted > 0).all()
    assert np.array_equal(res.tried, [60] * 4)
    for f in range(0, 60, 7):
        for r in range(4):
            assert mc_oracle.positions(cfg, res.X[f, r], res.Q[f, r])[:, :, 2].min() >= -1e-13
    ens.close()
