"""The ensemble's flow field and the observers of its runs on the GPU (include/rbl.h section 5: rbl_ensemble_velocity_field,
rbl_ensemble_run_observed; Ensemble.velocity_field, Ensemble.run / run_jointed with probes, probe_body, moments).

The field is held against tests/ensemble_probe_oracle.py (the CPU oracle, no library code) to 1e-12 relative in the 2-norm, the
bound of the existing field and product tests, and against section 6's single-context field to 1e-13; lattice translations to
1e-13.  Everything a run records is compared BITWISE with the same quantities obtained one call at a time.

Shapes (tests/body_shapes.py): S5 (one trimer), S3 (64 trimers), and -- rbl_ensemble_set_config refuses S4 and S2, which do not
fit the one-kernel solver's LDS (held by tests/test_body_shapes_gpu.py; test_the_largest_shapes_are_still_refused below) -- the
largest members of their families that an ensemble can hold: E3 (30 x fib7, 210 blobs) and E2 (one body of 238 blobs).
The cell is tests/test_ensemble_periodic_gpu.py's: 10 x shell_N_12 in periodic_cases.layer10()."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import body_shapes as bs  # noqa: E402
import ensemble_probe_oracle as epo  # noqa: E402
import joint_kinds_oracle as jk  # noqa: E402
import joint_oracle as jo  # noqa: E402
import periodic_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ens(cfg, a, X, Q, eta=1.0, dt=0.01, kBT=0.0, wall=True):
    from rigid_body_light_amd import Ensemble
    return Ensemble(cfg, np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64), a, eta, dt, kBT=kBT, wall=wall)


def _positions(orc, cfg, X, Q):
    from oracle import oracle as O
    return orc.multi_body_pos(X, O.normalize_quats(Q), O.remove_mean(cfg)).reshape(-1, 3)


def _field(ens, pts, lam, body=None):
    """Ensemble.velocity_field through the C ABI with the output poisoned beforehand: every entry must be written"""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    P = pts.shape[-2]
    u = np.full((ens.R, P, 3), np.nan)
    rc = ens.ctx.L.rbl_ensemble_velocity_field(ens.ctx.h, pts.ctypes.data, P, 1 if pts.ndim == 2 else pts.shape[0], -1 if body is None else body,
                                               lam.ctypes.data, u.ctypes.data)
    assert rc == 0, ens.ctx.L.rbl_last_error(ens.ctx.h)
    assert np.isfinite(u).all()
    return u


def _shape_case(name, R, wall):
    cs = [bs.case(name, wall, seed=bs.replica_seed(r)) for r in range(R)]
    return cs[0], np.stack([c["X"] for c in cs]), np.stack([c["Q"] for c in cs])


def _points(r, a, P, wall, seed, blobs_of=()):
    """P points around the blobs r: random ones from 0.3 a to 8 a from the nearest blob (with the wall from z = 0.05 a: some
    inside the damped layer), then, where P leaves room, one at z = 0, one below it, and points ON the blobs blobs_of"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    tree = cKDTree(r)
    lo, hi = r.min(axis=0) - 8 * a, r.max(axis=0) + 8 * a
    if wall:
        lo[2] = 0.05 * a
    out = np.zeros((0, 3))
    while out.shape[0] < P:
        x = rng.uniform(lo, hi, (4 * P + 16, 3))
        d, _ = tree.query(x)
        out = np.concatenate([out, x[(d >= 0.3 * a) & (d <= 8 * a)]])[:P]
    special = [r[k] for k in blobs_of]
    if wall:
        special += [np.array([out[0, 0], out[0, 1], 0.0]), np.array([out[0, 0] + 0.1, out[0, 1], -0.7 * a])]
    for i, x in enumerate(special[:max(P - 1, 0)]):
        out[P - 1 - i] = x
    return out


# ------------------------------------------------------------------------------------------------ 1: the one-shot field, open and wall
FIELD_P = [1, 63, 64, 65, 128, 129, 256, 257]                # the wave, 64 NI and 64 NI + 1 for NI = 1, 2, 4 (the tiles of 64 NI lanes)


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("name", ["S5", "S3", "E3", "E2"])
def test_field_against_the_oracle_open_and_wall(orc, name, wall):
    c, X, Q = _shape_case(name, 3, wall)
    a, eta, n3 = c["a"], c["eta"], 3 * c["nb"] * c["nblb"]
    ens = _ens(c["cfg"], a, X, Q, eta=eta, wall=wall)
    one = _ens(c["cfg"], a, X[1:2], Q[1:2], eta=eta, wall=wall)
    r = [_positions(orc, c["cfg"], X[k], Q[k]) for k in range(3)]
    N = r[0].shape[0]
    on = [0, N // 3, N - 1] if c["nb"] == 1 else [0, c["nblb"], N - 1]                 # blobs of several bodies
    worst = 0.0
    for i, P in enumerate(FIELD_P):
        lam = np.random.default_rng(100 + P).standard_normal((3, n3))
        shared = i % 2 == 0
        if shared:                                                                      # one set: around (and on) replica 0's blobs
            pts = _points(r[0], a, P, wall, seed=P, blobs_of=on)
        else:
            pts = np.stack([_points(r[k], a, P, wall, seed=P + k, blobs_of=on) for k in range(3)])
        u = _field(ens, pts, lam)
        assert _bits(u, _field(ens, pts, lam))                                          # run twice
        assert _bits(u, ens.velocity_field(pts, lam))                                   # the Python method is the same call
        u1 = _field(one, pts if shared else pts[1:2], lam[1:2])
        assert _bits(u1[0], u[1]), (P, "replica 1 of 3 is not the R = 1 call")
        for k in range(3):
            pk = pts if shared else pts[k]
            if shared and k:                                                            # replica 0's blobs are not replica k's: keep the
                pk = pk[:max(P - len(on) - (2 if wall else 0), 1)]                      # random points only (others may lie inside k's blobs)
            ref = epo.field_open(orc, r[k], lam[k], pk, a, eta, wall)
            worst = max(worst, _rel(u[k, :pk.shape[0]], ref))
            assert _rel(u[k, :pk.shape[0]], ref) <= TOL, (name, wall, P, k)
            if wall and P >= 8 and (not shared or k == 0):
                assert np.all(u[k, P - len(on) - 2:P - len(on)] == 0.0)                 # z = 0 and below: exactly zero
    print("%s wall=%s: worst rel. error %.2e" % (name, wall, worst))
    ens.close(); one.close()


def test_the_largest_shapes_are_still_refused():
    """why S4 and S2 are not among the cases above: no ensemble can hold them (an existing refusal, unchanged)"""
    from rigid_body_light_amd._lib import RblError
    for name in ("S4", "S2"):
        c, X, Q = _shape_case(name, 1, True)
        with pytest.raises(RblError, match="one-kernel solver"):
            _ens(c["cfg"], c["a"], X, Q)


def _threshold(ens, ni):
    """the smallest point count at which rbl_ensemble_probe_info returns `ni` points per lane, or None"""
    lo, hi = 1, 1 << 24
    if ens.probe_info(hi)[0] < ni:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ens.probe_info(mid)[0] >= ni else (mid + 1, hi)
    return lo


@pytest.mark.parametrize("wall", [False, True])
def test_every_launch_geometry(orc, wall):
    """every NI the geometry can return on this device (found through rbl_ensemble_probe_info), at a whole number of its 64 NI
    tiles and one point more: bitwise the same field evaluated in pieces small enough for NI = 1 -- a point's sum does not depend on
    the geometry --, and a sample of it, the last tile included, against the oracle"""
    c, X, Q = _shape_case("S5", 3, wall)
    a, eta = c["a"], c["eta"]
    ens = _ens(c["cfg"], a, X, Q, eta=eta, wall=wall)
    r = [_positions(orc, c["cfg"], X[k], Q[k]) for k in range(3)]
    lam = np.random.default_rng(5).standard_normal((3, 9))
    assert ens.probe_info(1) == (1, 1, 1) and ens.probe_info(64) == (1, 1, 1) and ens.probe_info(65) == (1, 2, 1)
    assert ens.probe_info(256) == (1, 4, 1) and ens.probe_info(257) == (1, 4, 2) and ens.probe_info(0)[2] == 0
    seen = {1}
    for ni in (2, 4):
        p0 = _threshold(ens, ni)
        if p0 is None:
            continue
        for P in (-(-p0 // (64 * ni)) * 64 * ni, -(-p0 // (64 * ni)) * 64 * ni + 1):
            got, waves, tiles = ens.probe_info(P)
            assert got == ni and waves == 4 and tiles == -(-P // (256 * ni))
            seen.add(got)
            pts = _points(r[0], a, P, wall, seed=ni)
            u = _field(ens, pts, lam)
            piece = 4096
            assert ens.probe_info(piece)[0] == 1
            parts = np.concatenate([_field(ens, pts[i:i + piece], lam) for i in range(0, P, piece)], axis=1)
            assert _bits(u, parts), (ni, P)
            idx = np.concatenate([np.random.default_rng(P).choice(P - 200, 300, replace=False), np.arange(P - 200, P)])
            for k in range(3):
                assert _rel(u[k, idx], epo.field_open(orc, r[k], lam[k], pts[idx], a, eta, wall)) <= TOL, (ni, P, k)
    print("points per lane reached on this device:", sorted(seen))
    assert seen == {1, 2, 4}
    ens.close()


@pytest.mark.parametrize("wall", [False, True])
def test_points_fixed_in_a_body(orc, wall):
    """offsets fixed in body 0 and in the last body of every replica; the lattice's bodies carry random orientations"""
    c, X, Q = _shape_case("S3", 3, wall)
    a, eta, nb = c["a"], c["eta"], c["nb"]
    ens = _ens(c["cfg"], a, X, Q, eta=eta, wall=wall)
    one = _ens(c["cfg"], a, X[2:3], Q[2:3], eta=eta, wall=wall)
    lam = np.random.default_rng(8).standard_normal((3, 3 * nb * c["nblb"]))
    rng = np.random.default_rng(9)
    s = rng.uniform(-6 * a, 6 * a, (130, 3))
    s = s[np.linalg.norm(s, axis=1) > bs.radius(c["cfg"]) + 1.3 * a][:100]               # clear of the body's own blobs
    sets = np.stack([s, 0.9 * s, 1.1 * s])
    for body in (0, nb - 1):
        for pts in (s, sets):
            u = _field(ens, pts, lam, body)
            assert _bits(u, _field(ens, pts, lam, body))
            assert _bits(u[2], _field(one, pts if pts.ndim == 2 else pts[2:3], lam[2:3], body)[0])
            for k in range(3):
                x = epo.place(pts if pts.ndim == 2 else pts[k], X[k], Q[k], body)
                ref = epo.field_open(orc, _positions(orc, c["cfg"], X[k], Q[k]), lam[k], x, a, eta, wall)
                assert _rel(u[k], ref) <= TOL, (body, k)
                lab = _field(ens, x, lam)[k]                                             # the same points given as lab points
                assert _rel(u[k], lab) <= 1e-13
    ens.close(); one.close()


def test_field_against_section_6(orc):
    """replica r's field is the single context's velocity_field at replica r's blobs"""
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    for wall in (False, True):
        c, X, Q = _shape_case("E3", 3, wall)
        a = c["a"]
        ens = _ens(c["cfg"], a, X, Q, wall=wall)
        lam = np.random.default_rng(21).standard_normal((3, 3 * c["nb"] * c["nblb"]))
        ctx = DeviceContext(a, 1.0, wall, stream_ptr=torch.cuda.current_stream().cuda_stream)
        r0 = _positions(orc, c["cfg"], X[0], Q[0])
        pts = _points(r0, a, 500, wall, seed=22)
        u = _field(ens, pts, lam)
        for k in range(3):
            rk = _positions(orc, c["cfg"], X[k], Q[k])
            keep = np.min(np.linalg.norm(pts[:, None, :] - rk[None, :, :], axis=2), axis=1) > 0.3 * a
            assert keep.sum() > 300
            v = ctx.velocity_field(pts[keep], lam[k], rk).reshape(-1, 3)
            assert _rel(u[k][keep], v) <= 1e-13, (wall, k)
        ctx.close(); ens.close()


def test_the_r_dependent_refusals_and_the_flags():
    """the halves of the refusals that need an ensemble (tests/test_ensemble_observed_cpu.py has the others), and the two flags"""
    from rigid_body_light_amd._lib import RblError
    c, X, Q = _shape_case("S5", 3, True)
    ens = _ens(c["cfg"], c["a"], X, Q)
    L, h = ens.ctx.L, ens.ctx.h
    x, lam, u = np.ones((2, 4, 3)), np.zeros((3, 9)), np.zeros((3, 4, 3))
    assert L.rbl_ensemble_velocity_field(h, x.ctypes.data, 4, 2, -1, lam.ctypes.data, u.ctypes.data) == 11 and b"point_sets" in L.rbl_last_error(h)
    assert L.rbl_ensemble_velocity_field(h, x.ctypes.data, 4, 1, 1, lam.ctypes.data, u.ctypes.data) == 11 and b"probe_body" in L.rbl_last_error(h)
    x[0, 3, 2] = np.inf
    assert L.rbl_ensemble_velocity_field(h, x.ctypes.data, 4, 1, -1, lam.ctypes.data, u.ctypes.data) == 11 and b"set 0, point 3" in L.rbl_last_error(h)
    F = np.zeros(6)
    for kw, word in ((dict(probes=np.ones((2, 4, 3))), "point_sets"), (dict(probes=np.ones((4, 3)), probe_body=1), "probe_body")):
        with pytest.raises(RblError, match=word):                         # through the binding, past the Python layer's own checks
            ens.ctx.ensemble_run_observed(2, F_body=F, brownian=False, **kw)
    X0, _ = ens.get_config()
    lam = np.ones((3, 9))
    lam[1, 4] = np.inf
    with pytest.raises(RblError, match=r"replica 1.*status 10"):            # RBL_ERR_NONFINITE, latched in the replica's word
        ens.velocity_field(np.array([[0.3, 0.2, 4.0]]), lam)
    Xb = X.copy()
    Xb[2, 0, 2] = -0.5
    ens.set_config(Xb, Q)
    with pytest.raises(RblError, match=r"replica 2.*status 2"):            # a blob below the wall
        ens.velocity_field(np.array([[0.3, 0.2, 4.0]]), np.ones((3, 9)))
    ens.close()


# ------------------------------------------------------------------------------------------------ 2: the cell
@functools.lru_cache(maxsize=None)
def _cell_case():
    """tests/test_ensemble_periodic_gpu.py's D: layer10() itself and two copies with the bodies displaced by up to 0.05"""
    c = pc.layer10()
    rng = np.random.default_rng(51)
    X = np.stack([c["X"], c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape), c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape)])
    return c, X, np.stack([c["Q"]] * 3)


def _cell_points(r, a, L, seed, n_random):
    """n_random points in and around the cell (some in the damped layer, one at z = 0, one below), a point ON blob 17, a point on
    blob 100 moved by a lattice vector"""
    rng = np.random.default_rng(seed)
    Lx, Ly = L[0], (L[1] if L[1] > 0.0 else 10.0)
    out = []
    while len(out) < n_random:
        x = rng.uniform([-0.5 * Lx, -0.5 * Ly, 0.05 * a], [1.5 * Lx, 1.5 * Ly, 6.0])
        d = x[None, :] - r
        d[:, 0] -= L[0] * np.rint(d[:, 0] / L[0])
        if L[1] > 0.0:
            d[:, 1] -= L[1] * np.rint(d[:, 1] / L[1])
        if np.min(np.linalg.norm(d, axis=1)) > 0.3 * a:
            out.append(x)
    out[0][2] = 0.6 * a                                                                  # inside the damped layer
    out += [np.array([1.0, 2.0, 0.0]), np.array([2.0, 1.0, -0.4]), r[17].copy(), r[100] + np.array([-L[0], 2 * L[1], 0.0])]
    return np.array(out)


@pytest.mark.parametrize("images,open_y", [((1, 1), False), ((2, 1), False), ((1, 1), True), ((16, 1), False)])
def test_field_in_the_cell(orc, images, open_y):
    c, X, Q = _cell_case()
    a = c["a"]
    L = (c["L"][0], 0.0 if open_y else c["L"][1])
    ens = _ens(c["cfg"], a, X, Q)
    one = _ens(c["cfg"], a, X[1:2], Q[1:2])
    lam = np.random.default_rng(61).standard_normal((3, 360))
    r = [_positions(orc, c["cfg"], X[k], Q[k]) for k in range(3)]
    n_random = 4 if images[0] == 16 else 10
    pts = _cell_points(r[0], a, L, 62, n_random)
    open_u = _field(ens, pts, lam)
    ens.set_cell(L[0], L[1], images=images)
    one.set_cell(L[0], L[1], images=images)
    u = _field(ens, pts, lam)
    assert _bits(u, _field(ens, pts, lam))
    assert _bits(u[1], _field(one, pts, lam[1:2])[0])                                     # replica 1 of 3 is the R = 1 call
    n_im = (images[0], 0 if open_y else images[1])
    ref = epo.field_cell(orc, r[0], lam[0], pts, a, 1.0, L, n_im)
    assert _rel(u[0], ref) <= TOL, (images, open_y, _rel(u[0], ref))
    assert np.all(u[0, n_random:n_random + 2] == 0.0)                                     # z = 0 and below
    assert _rel(open_u[0, :n_random], u[0, :n_random]) > 1e-3                             # the cell matters here
    for k in (1, 2):                                                                       # the other replicas, on the random points
        ref = epo.field_cell(orc, r[k], lam[k], pts[:n_random], a, 1.0, L, n_im)
        assert _rel(u[k, :n_random], ref) <= TOL, (images, open_y, k)
    shift = np.array([2 * L[0], -L[1], 0.0])                                              # a lattice vector
    assert _rel(_field(ens, pts + shift, lam), u) <= 1e-13
    sets = np.stack([pts, pts + shift, pts - shift])                                      # per-replica sets
    assert _rel(_field(ens, sets, lam), u) <= 1e-13
    ens.set_cell(L[0], L[1], images=images, on=False)
    assert _bits(_field(ens, pts, lam), open_u)                                           # cell off: the open launch, bitwise
    ens.close(); one.close()


def test_every_launch_geometry_in_the_cell(orc):
    """the cell's instantiations with two and four points per lane: tests/test_ensemble_periodic_gpu.py's case A (4 tetrahedra,
    16 blobs, in a cell of two lattice spacings) at (1, 1) images, three replicas, at the point counts where
    rbl_ensemble_probe_info returns NI = 2 and NI = 4 -- bitwise the same points evaluated in pieces at NI = 1, and 16 sampled
    points, the last tile's among them, against the restatement"""
    cases = [pc.layers("tetra", 4, 2, 2, seed=s) for s in range(3)]
    c = cases[0]
    a, L = c["a"], c["L"]
    X, Q = np.stack([k["X"] for k in cases]), np.stack([k["Q"] for k in cases])
    ens = _ens(c["cfg"], a, X, Q)
    ens.set_cell(L[0], L[1], images=(1, 1))
    r = [_positions(orc, c["cfg"], X[k], Q[k]) for k in range(3)]
    lam = np.random.default_rng(71).standard_normal((3, 48))
    seen = set()
    for ni in (2, 4):
        p0 = _threshold(ens, ni)
        if p0 is None:
            continue
        P = -(-p0 // (64 * ni)) * 64 * ni + 1                                              # whole tiles and one point more
        assert ens.probe_info(P)[0] == ni and ens.probe_info(4096)[0] == 1
        seen.add(ni)
        pts = np.random.default_rng(70 + ni).uniform([-0.5 * L[0], -0.5 * L[1], 0.05 * a], [1.5 * L[0], 1.5 * L[1], 6.0], (P, 3))
        u = _field(ens, pts, lam)
        parts = np.concatenate([_field(ens, pts[i:i + 4096], lam) for i in range(0, P, 4096)], axis=1)
        assert _bits(u, parts), ni
        idx = np.concatenate([np.random.default_rng(ni).choice(P - 8, 8, replace=False), np.arange(P - 8, P)])
        for k in range(3):
            assert _rel(u[k, idx], epo.field_cell(orc, r[k], lam[k], pts[idx], a, 1.0, L, (1, 1))) <= TOL, (ni, k)
    assert seen == {2, 4}
    ens.close()


def test_the_device_form_is_the_host_form_bitwise():
    """rbl_ensemble_velocity_field_dev on device arrays: lab points shared and per replica, points fixed in a body, open and in
    the cell"""
    import torch
    c, X, Q = _cell_case()
    a, L = c["a"], c["L"]
    ens = _ens(c["cfg"], a, X, Q)
    rng = np.random.default_rng(81)
    lam = rng.standard_normal((3, 360))
    d_lam = torch.tensor(lam, device="cuda")
    for cell in (False, True):
        ens.set_cell(L[0], L[1], images=(1, 1), on=cell)
        for pts, body in ((rng.uniform([0.0, 0.0, 0.1], [L[0], L[1], 5.0], (130, 3)), None),
                          (rng.uniform([0.0, 0.0, 0.1], [L[0], L[1], 5.0], (3, 65, 3)), None),
                          (rng.uniform(-4.0, 4.0, (70, 3)), 9)):
            d_pts = torch.tensor(pts, device="cuda")
            P = pts.shape[-2]
            d_u = torch.full((3, P, 3), float("nan"), dtype=torch.float64, device="cuda")
            ens.ctx.ensemble_velocity_field_dev(d_pts.data_ptr(), P, 1 if pts.ndim == 2 else 3, d_lam.data_ptr(), d_u.data_ptr(), body=body)
            torch.cuda.synchronize()
            assert _bits(d_u.cpu().numpy(), ens.velocity_field(pts, lam, body=body)), (cell, pts.shape, body)
    ens.close()


def test_a_point_half_a_cell_from_a_blob(orc):
    """A tie of the nearest-image reduction, made exact as tests/test_periodic_shapes_gpu.py makes it: a body of three blobs with
    coordinates on a grid of 2^-30 whose mean is exactly zero, unrotated, its centre on the grid, a = 1/2 (so the scaling by 1 / a is
    exact), L = (8, 7.5): the blob positions are exact sums and the two points lie exactly L / 2 = 4 from blob 0 in x, one on either
    side.  Either image of that blob is a nearest one, and at nx = 1 the truncated sums of the two differ; the
    device must give one of the two, to the bound of every other cell case"""
    a, L = 0.5, (8.0, 7.5)
    cfg = np.array([[1.0, 0.0, 0.0], [-0.5, 0.875, 0.0], [-0.5, -0.875, 0.0]])           # centres >= 2a apart
    X = np.array([[[1.25 + 2.0 ** -30, 2.5, 2.0 - 2.0 ** -29]]])
    Q = np.array([[[1.0, 0.0, 0.0, 0.0]]])
    r = _positions(orc, cfg, X[0], Q[0])
    assert np.array_equal(r, cfg + X[0, 0]) and np.array_equal(cfg.mean(axis=0), np.zeros(3))
    ens = _ens(cfg, a, X, Q)
    ens.set_cell(L[0], L[1], images=(1, 1))
    lam = np.zeros((1, 9))
    lam[0, :3] = [1.0, -0.5, 0.7]                                                         # blob 0 alone carries a force
    pts = np.stack([r[0] + np.array([4.0, 0.25, 0.5]), r[0] + np.array([-4.0, -0.375, 0.75])])
    assert np.array_equal(pts[:, 0] - r[0, 0], [4.0, -4.0])                               # exactly half a cell
    u = _field(ens, pts, lam)[0]
    ens.close()
    for i, side in enumerate((1.0, -1.0)):
        r2 = r.copy()
        r2[0, 0] += side * L[0]                                                           # the same blob a whole cell over, exactly
        keep = epo.field_cell(orc, r, lam[0], pts[i:i + 1], a, 1.0, L, (1, 1))[0]
        flip = epo.field_cell(orc, r2, lam[0], pts[i:i + 1], a, 1.0, L, (1, 1))[0]
        assert _rel(keep, flip) > 1e-6                                                    # the two choices do differ
        errs = (_rel(u[i], keep), _rel(u[i], flip))
        print("tie at %+g: rel. difference to the oracle's choice %.2e, to the other nearest image %.2e" % (side * 4.0, errs[0], errs[1]))
        assert min(errs) <= TOL, (i, errs)


# ------------------------------------------------------------------------------------------------ 3: runs, deterministic, no force model
def _shell12():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return cfg, p["sep"] / 2.0


def _run_case(cell):
    """3 replicas of 3 x shell_N_12 above the wall (open), or tests/test_ensemble_periodic_gpu.py's D in its cell"""
    if cell:
        c, X, Q = _cell_case()
        return c["cfg"], c["a"], X, Q, c["L"]
    from conftest import random_positions
    cfg, a = _shell12()
    X, Q = np.zeros((3, 3, 3)), np.zeros((3, 3, 4))
    for r in range(3):
        x, q = random_positions(3, wall=True, seed=100 + r, min_dist=4.0)
        x[:, 2] += 1.5
        X[r], Q[r] = x, q
    return cfg, a, X, Q, None


KW = dict(max_iter=200, rtol=1e-9)


@pytest.mark.parametrize("cell,body", [(False, None), (False, 0), (True, None)])
def test_a_deterministic_observed_run_is_the_loop_bitwise(orc, cell, body):
    """run(7, stride=1, probes, moments) against: the same run without observers (X, Q, counters, frames); the loop
    solve -> velocity_field -> step (frame_u, u_sum); the loop of step_deterministic with record_moments (D_sum, frame_D).
    In the cell solve_jointed is refused, so there the run is the masked one with nobody prescribed and lambda solve_mixed's."""
    cfg, a, X, Q, L = _run_case(cell)
    nb = X.shape[1]
    rng = np.random.default_rng(31)
    F = 0.5 * rng.standard_normal((3, 6 * nb))
    if body is None:
        r0 = _positions(orc, cfg, X[0], Q[0])
        pts = _points(r0, a, 70, True, seed=32) if not cell else _cell_points(r0, a, L, 33, 12)
    else:
        pts = rng.uniform(-5.0, 5.0, (70, 3))
        pts = pts[np.linalg.norm(pts, axis=1) > 1.0 + 1.5 * a]
    free = np.zeros(nb, dtype=bool)

    def make():
        e = _ens(cfg, a, X, Q)
        if cell:
            e.set_cell(L[0], L[1], images=(1, 1))
        return e

    def run(e, **obs):
        if cell:
            return e.run(7, prescribed=free, body_in=F, brownian=False, stride=1, **KW, **obs)
        return e.run(7, F=F, brownian=False, stride=1, **KW, **obs)

    ens = make()
    plain = run(ens)
    Xp, Qp = ens.get_config()
    ens.close()
    ens = make()
    res = run(ens, probes=pts, probe_body=body, moments=True)
    Xo, Qo = ens.get_config()
    from rigid_body_light_amd._lib import RblError
    with pytest.raises(RblError, match="status 7"):                        # observers are arguments: nothing was recorded as state
        ens.step_moments()
    ens.close()
    assert _bits(Xo, Xp) and _bits(Qo, Qp)
    for name in ("X", "Q", "accepted_at", "accepted", "rejected", "iters_sum", "resid_max", "first_status"):
        assert _bits(getattr(res, name), getattr(plain, name)), name
    assert res.accepted.tolist() == [7, 7, 7] and plain.u_sum is None and plain.D_sum is None
    assert res.frame_u.shape == (7, 3, pts.shape[0], 3) and res.frame_D.shape == (7, 3, nb, 3, 3)
    # the loop: lambda of the solve at q^n, the field of it, the moments the step records, then the step
    ens = make()
    ens.record_moments(True)
    usum, Dsum = np.zeros_like(res.u_sum), np.zeros_like(res.D_sum)
    for n in range(7):
        lam = ens.solve_mixed(free, F, **KW)[0] if cell else ens.solve_jointed(F, **KW)[0]
        u = ens.velocity_field(pts, lam, body=body)
        assert _bits(res.frame_u[n], u), n
        if cell:
            ens.step_mixed(free, F, **KW)
        else:
            ens.step_deterministic(F, **KW)
        D = ens.step_moments()
        assert _bits(res.frame_D[n], D), n
        usum += u
        Dsum += D
    assert _bits(res.u_sum, usum) and _bits(res.D_sum, Dsum)
    assert _bits(res.u_mean, usum / 7.0) and _bits(res.D_mean, Dsum / 7.0)
    assert _rel(res.stresslet_mean, epo.stresslet(Dsum / 7.0)) <= 1e-15
    ens.close()
    # ... and the field itself against the restatement: step 0 is evaluated at q^0
    ens = make()
    lam0 = ens.solve_mixed(free, F, **KW)[0] if cell else ens.solve_jointed(F, **KW)[0]
    ens.close()
    for k in range(3):
        rk = _positions(orc, cfg, X[k], Q[k])
        xk = epo.place(pts, X[k], Q[k], body)
        if cell:
            sel = np.arange(pts.shape[0]) if k == 0 else np.arange(12)    # (the points on blobs are on replica 0's blobs)
            ref = epo.field_cell(orc, rk, lam0[k], xk[sel], a, 1.0, L, (1, 1))
        else:
            sel = np.flatnonzero(np.min(np.linalg.norm(xk[:, None, :] - rk[None, :, :], axis=2), axis=1) > 0.2 * a)
            ref = epo.field_open(orc, rk, lam0[k], xk[sel], a, 1.0, True)
        assert _rel(res.frame_u[0, k][sel], ref) <= TOL, k


def test_an_observed_run_with_nothing_to_observe_is_the_plain_run():
    cfg, a, X, Q, _ = _run_case(False)
    F = 0.3 * np.random.default_rng(41).standard_normal((3, 18))
    out = []
    for how in ("run", "observed"):
        ens = _ens(cfg, a, X, Q, kBT=1.0)
        if how == "run":
            res = ens.run(5, F=F, seed=3, stride=2, **KW)
        else:
            res, rc = ens.ctx.ensemble_run_observed(5, F_body=F, seed=3, stride=2, **KW)
            assert rc == 0 and res.u_sum is None and res.D_sum is None
        out.append((res, ens.get_config()))
        ens.close()
    assert all(_bits(p, q) for p, q in zip(out[0][1], out[1][1]))
    for name in ("X", "Q", "accepted", "iters_sum", "resid_max"):
        assert _bits(getattr(out[0][0], name), getattr(out[1][0], name)), name


# ------------------------------------------------------------------------------------------------ 4: runs, Brownian
def test_brownian_observers_do_not_perturb_and_sum_in_step_order(orc):
    cfg, a, X, Q, _ = _run_case(False)
    F = 0.3 * np.random.default_rng(42).standard_normal((3, 18))
    pts = _points(_positions(orc, cfg, X[0], Q[0]), a, 65, True, seed=43)
    ens = _ens(cfg, a, X, Q, kBT=1.0)
    plain = ens.run(6, F=F, seed=11, stride=1, **KW)
    end = ens.get_config()
    ens.close()
    ens = _ens(cfg, a, X, Q, kBT=1.0)
    res = ens.run(6, F=F, seed=11, stride=1, probes=pts, moments=True, **KW)
    assert all(_bits(p, q) for p, q in zip(end, ens.get_config()))
    ens.close()
    for name in ("X", "Q", "accepted_at", "accepted", "rejected", "iters_sum", "resid_max"):
        assert _bits(getattr(res, name), getattr(plain, name)), name
    usum, Dsum = np.zeros_like(res.u_sum), np.zeros_like(res.D_sum)
    for n in range(6):
        usum += res.frame_u[n]
        Dsum += res.frame_D[n]
    assert _bits(res.u_sum, usum) and _bits(res.D_sum, Dsum)
    assert np.abs(res.frame_u[1] - res.frame_u[0]).max() > 0.0                          # instantaneous values: they fluctuate
    # a 1-step run's D is step_moments() after step_brownian from the same start and seed: the midpoint configuration
    ens = _ens(cfg, a, X, Q, kBT=1.0)
    one = ens.run(1, F=F, seed=11, moments=True, probes=pts, **KW)
    ens.close()
    ens = _ens(cfg, a, X, Q, kBT=1.0)
    ens.record_moments(True)
    ens.step_brownian(F, seed=11, **KW)
    assert _bits(one.D_sum, ens.step_moments())
    ens.close()
    assert _bits(one.D_sum, res.frame_D[0]) and _bits(one.u_sum, res.frame_u[0])


def _landing_case():
    """tests/test_ensemble_run_gpu.py: test_a_new_configuration_is_validated_before_it_commits, two replicas of one shell and a
    time step of 40: replica 1 is pushed towards the wall (U = -N F_body: F_z > 0 pushes down) from 3.0 above it (LANDING_GAP), far enough for a
    first step to land above z = 0 and near enough for a later one to land below; replica 0 drifts sideways, high up"""
    cfg, a = _shell12()
    X0 = np.zeros((2, 1, 3)); Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (2, 1, 1))
    X0[0, 0] = [0.0, 0.0, 9.0]
    X0[1, 0, 2] = -cfg[:, 2].min() + LANDING_GAP
    F = np.zeros((2, 6))
    F[0], F[1] = [0.05, 0, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0]
    pts = np.array([[3.0, 0.5, 2.0], [-2.0, 1.0, 6.0], [0.5, -3.0, 0.3]])
    return cfg, a, X0, Q0, F, pts


LANDING_GAP = 3.0
LANDING = dict(seed=5, stride=1, max_iter=100, rtol=1e-9)


def test_reject_skips_the_step_and_the_frame_repeats_the_last_accepted_value():
    cfg, a, X0, Q0, F, pts = _landing_case()
    ens = _ens(cfg, a, X0, Q0, dt=40.0, kBT=1e-4)
    res = ens.run(5, F=F, on_error="reject", probes=pts, moments=True, **LANDING)
    ens.close()
    print("accepted", res.accepted.tolist(), "rejected", res.rejected.tolist(), "accepted_at", res.accepted_at.T.tolist())
    acc = res.accepted_at[:, 1]
    assert res.accepted[0] == 5 and 1 <= res.accepted[1] < 5, "the construction: replica 1 accepts a step, then lands below the wall"
    ens = _ens(cfg, a, X0[:1], Q0[:1], dt=40.0, kBT=1e-4)
    alone = ens.run(5, F=F[:1], on_error="reject", probes=pts, moments=True, **LANDING)
    ens.close()
    for name in ("u_sum", "D_sum"):                                                       # the other replica is unaffected
        assert _bits(getattr(res, name)[0], getattr(alone, name)[0]), name
    assert _bits(res.frame_u[:, 0], alone.frame_u[:, 0]) and _bits(res.frame_D[:, 0], alone.frame_D[:, 0])
    usum, Dsum, prev = np.zeros((3, 3)), np.zeros((1, 3, 3)), 0
    for n in range(5):
        if acc[n] > prev:                                                                 # accepted in step n: its value is added
            usum += res.frame_u[n, 1]
            Dsum += res.frame_D[n, 1]
        else:                                                                             # rejected: the frame repeats the last accepted value
            assert n > 0 and _bits(res.frame_u[n, 1], res.frame_u[n - 1, 1]) and _bits(res.frame_D[n, 1], res.frame_D[n - 1, 1]), n
        prev = acc[n]
    assert _bits(res.u_sum[1], usum) and _bits(res.D_sum[1], Dsum)
    assert _bits(res.u_mean[1], usum / res.accepted[1])


def test_stop_adds_nothing_from_the_stopping_step_on():
    from rigid_body_light_amd._lib import RblError
    cfg, a, X0, Q0, F, pts = _landing_case()
    ens = _ens(cfg, a, X0, Q0, dt=40.0, kBT=1e-4)
    with pytest.raises(RblError, match="status 2"):
        ens.run(5, F=F, on_error="stop", check_every=0, probes=pts, moments=True, **LANDING)
    res = ens.last_run
    ens.close()
    s = res.stopped_at
    assert 1 <= s < 5 and res.accepted.tolist() == [s, s]
    usum = np.zeros_like(res.u_sum)
    for n in range(s):
        usum += res.frame_u[n]
    assert _bits(res.u_sum, usum)
    for n in range(s, 5):
        assert _bits(res.frame_u[n], res.frame_u[s - 1]) and _bits(res.frame_D[n], res.frame_D[s - 1]), n


def test_a_replica_that_accepts_nothing_has_zero_means():
    cfg, a, X0, Q0, F, pts = _landing_case()
    X0 = X0.copy()
    X0[1, 0, 2] = -0.5                                                                    # below the wall from the start
    ens = _ens(cfg, a, X0, Q0, dt=0.01, kBT=1.0)
    res = ens.run(3, F=F, on_error="reject", stride=1, probes=pts, moments=True, max_iter=100)
    ens.close()
    assert res.accepted.tolist() == [3, 0]
    ens = _ens(cfg, a, X0, Q0, dt=0.01, kBT=1.0)
    plain = ens.run(3, F=F, on_error="reject", stride=1, max_iter=100)
    ens.close()
    # the failing replica's solve leaves a lambda that is not finite: the probe kernel's own flags must not reach a word that is
    # set already, so the error records are the unobserved run's
    assert res.first_flags[1] != 0
    for name in ("first_flags", "first_status", "rejected", "accepted", "X", "Q", "accepted_at"):
        assert _bits(getattr(res, name), getattr(plain, name)), name
    assert not res.u_sum[1].any() and not res.u_mean[1].any() and not res.frame_u[:, 1].any() and not res.D_mean[1].any()
    assert np.isfinite(res.u_mean).all() and np.isfinite(res.stresslet_mean).all() and res.u_mean[0].any()


# ------------------------------------------------------------------------------------------------ 5: run_jointed with observers
def test_a_jointed_observed_run(orc):
    """tests/joint_kinds_oracle.py's case_steps (three bodies: a motor, a hinge, a pivot), three replicas a little apart"""
    cfg, a = _shell12()
    X0, Q0, jr = jk.case_steps()

    def turned(angle, axis, shift):
        q = jk.qrot(angle, jo._unit(axis))
        return np.asarray(X0) @ jo.rot(q).T + shift, np.array([jk.qmul(q, p) for p in jo.unit(Q0)])

    reps = [(X0, jo.unit(Q0)), turned(0.01, [0.2, 1.0, -0.3], [0.01, -0.005, 0.02]), turned(-0.015, [1.0, 0.1, 0.4], [-0.008, 0.012, 0.015])]
    X, Q = np.array([p[0] for p in reps]), np.array([p[1] for p in reps])
    rng = np.random.default_rng(2024)
    F = rng.standard_normal((3, 18))
    rates = np.zeros((2, 5))
    rates[0, 1], rates[1, 1] = 0.7, -0.4
    kw = dict(schedule=([2, 3], rates), stride=2, max_iter=100, rtol=1e-10)
    wall = False
    pts = _points(_positions(orc, cfg, X[0], Q[0]), a, 40, wall, seed=77)
    out = []
    for obs in (dict(), dict(probes=pts, moments=True), dict(probes=0.8 * pts - pts.mean(axis=0), probe_body=1)):
        ens = _ens(cfg, a, X, Q, wall=wall)
        ens.set_joint_kinds(**jr)
        res = ens.run_jointed(6, F, **kw, **obs)
        out.append((res, ens.get_config()))
        ens.close()
    plain = out[0][0]
    for res, cfg_end in out[1:]:
        assert all(_bits(p, q) for p, q in zip(cfg_end, out[0][1]))
        for name in ("X", "Q", "accepted", "iters_sum", "resid_max", "theta", "cycle_pos", "phi_sum", "frame_theta", "frame_phi", "frame_gap"):
            assert _bits(getattr(res, name), getattr(plain, name)), name
    res = out[1][0]
    assert res.frame_u.shape == (3, 3, 40, 3) and res.frame_D.shape == (3, 3, 3, 3, 3) and np.abs(res.u_sum).max() > 0.0
    # the field against the restatement with the lambda of solve_jointed at the recorded configuration.  With gamma = 0 and
    # no motor turning the step's joint rows are zero, which is solve_jointed's system with joint_rhs = None; the configuration of
    # step 2 is reached by an unobserved run of two steps, bitwise (above)
    kw = dict(gamma=0.0, max_iter=100, rtol=1e-10)
    ens = _ens(cfg, a, X, Q, wall=wall)
    ens.set_joint_kinds(**jr)
    res = ens.run_jointed(3, F, stride=1, probes=pts, **kw)
    ens.close()
    ens = _ens(cfg, a, X, Q, wall=wall)
    ens.set_joint_kinds(**jr)
    for n in (0, 2):
        if n:
            ens.run_jointed(n, F, **kw)
        Xn, Qn = ens.get_config()
        lam = ens.solve_jointed(F, max_iter=100, rtol=1e-10)[0]
        same = _bits(res.frame_u[n], ens.velocity_field(pts, lam))
        print("step %d: frame_u bitwise the field of solve_jointed's lambda: %s" % (n, same))
        for k in range(3):
            ref = epo.field_open(orc, _positions(orc, cfg, Xn[k], Qn[k]), lam[k], pts, a, 1.0, wall)
            assert _rel(res.frame_u[n, k], ref) <= TOL, (n, k)
    ens.close()


# ------------------------------------------------------------------------------------------------ 6: the example
def test_the_example_runs_at_its_smallest_setting():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_swimmer_flow.py"), "--replicas", "2", "--cycles", "1", "--steps-per-stroke", "4",
                        "--grid", "5"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["example"] == "ensemble_swimmer_flow" and d["probes"] == 25 and np.isfinite(d["decay_exponent"])
