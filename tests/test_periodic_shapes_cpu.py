"""The periodic cell away from 12-blob bodies, without a GPU: the vectorised minimum-image oracles of tests/periodic_oracle.py
against the double loops that define them, and the soundness of every case that tests/test_periodic_shapes_gpu.py,
tests/test_periodic_forces_gpu.py and tests/test_pair_regimes_periodic_gpu.py run on the device -- so that no GPU case is vacuous:

  - every force case meets the documented uniqueness condition 2 R_body + r_cut <= L / 2 on both axes (dipoles: r_cut <= L / 2),
  - its oracle counts pairs inside the cutoff of BOTH kinds, minimum image direct and minimum image through a boundary,
  - no pair lies within 1e-9 of a cutoff or a core radius (fp64 on both sides rounds a distance of order 10 to 2e-15: both put
    every pair on the same side, and the pair counts can be compared as integers),
  - the row sets of the product cases hold the first and the last row of every 256-blob tile, and
  - every star of the per-pair probe has a target whose nearest image is not the direct displacement."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_probe as pp  # noqa: E402
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402


def _maxrel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / np.abs(np.asarray(y)).max()


def _loop_inputs():
    """(name, r, X, n_blb, a, L) of the two configurations the loops are cheap enough for"""
    from test_periodic_gpu import FORCE_CELL, _across
    c = _across()
    ten = pc.layer10()
    return [("across", pc.blob_positions(c["cfg"], c["X"], c["Q"]), c["X"], 12, c["a"], FORCE_CELL),
            ("layer10", ten["r"], ten["X"], 12, ten["a"], ten["L"])]


@pytest.mark.parametrize("which", ["steric", "table", "both"])
def test_vectorised_pair_terms_equal_the_loop(which):
    for name, r, _, n_blb, a, L in _loop_inputs():
        steric = (1.5, 0.1, 2.0 * a + 2.0) if which != "table" else None
        table = pc.PAIR_TABLE if which != "steric" else None
        f0, E0 = po.pair_forces(r, n_blb, a, L, steric=steric, table=table)
        f1, E1, nd, nt = po.pair_forces_v(r, n_blb, a, L, steric=steric, table=table, rows=50)      # (rows: a ragged last block)
        print("%s, %s: forces %.1e, energy %.1e; %d direct and %d pairs through a boundary" % (name, which, _maxrel(f1, f0), abs(E1 - E0) / abs(E0), nd, nt))
        assert np.abs(f0).max() > 1e-3 and _maxrel(f1, f0) <= 1e-14 and abs(E1 - E0) <= 1e-14 * abs(E0)
        assert nt > 0 and (nd > 0) == (name == "layer10")             # the three bodies of "across" meet through the boundaries only
        # the counts against a loop of their own
        cut = max(steric[2] if steric else 0.0, table[3] if table else 0.0)
        loop = [0, 0]
        for i in range(len(r)):
            for j in range(len(r)):
                if i // n_blb != j // n_blb and np.linalg.norm(po.nearest(r[i] - r[j], L)) <= cut:
                    loop[int(not np.array_equal(po.nearest(r[i] - r[j], L), r[i] - r[j]))] += 1
        assert (nd, nt) == tuple(loop)


@pytest.mark.parametrize("r_core", [1.0, 3.4])
def test_vectorised_dipoles_equal_the_loop(r_core):
    for name, _, X, _, _, L in _loop_inputs():
        m = np.random.default_rng(5).standard_normal(X.shape)
        FT0, E0 = po.dipole_pairs(X, m, 0.8, r_core, 5.0, L)
        FT1, E1, nd, nt = po.dipole_pairs_v(X, m, 0.8, r_core, 5.0, L)
        print("%s, r_core %.1f: FT %.1e, energy %.1e; %d direct and %d pairs through a boundary" % (name, r_core, _maxrel(FT1, FT0), abs(E1 - E0) / abs(E0), nd, nt))
        assert np.abs(FT0).max() > 1e-3 and _maxrel(FT1, FT0) <= 1e-14 and abs(E1 - E0) <= 1e-14 * abs(E0)
        assert nt > 0 and (nd > 0) == (name == "layer10")


def test_one_body_terms_are_the_open_oracles_with_the_pair_terms_off():
    """the same terms from the compiled all-pairs oracle (tests/interaction_oracle.py) with eps_blob = 0, and from the table oracle
    called the plain way with every body: one-body terms do not care how the blobs are grouped"""
    import interaction_oracle as io
    import table_oracle as to
    c = pc.force_case("12xshell_height")
    b = c["builtin"]
    f, FT, E = po.one_body_terms(c["r"], c["X"], 12, c["a"], True, builtin=b)
    f0, FT0, E0 = io.interactions(c["r"], c["X"], 12, c["a"], True, b["w"], b["eps_wall"], b["b_wall"], 0.0, 1.0, 2.0 * c["a"])
    assert _maxrel(f, f0) <= 1e-14 and _maxrel(FT, FT0) <= 1e-13 and abs(E - E0) <= 1e-14 * abs(E0)
    f, FT, E = po.one_body_terms(c["r"], c["X"], 12, c["a"], True, builtin=b, height=c["height"], traps=c["traps"])
    full = dict(b, eps_blob=0.0, b_blob=1.0, r_cut=-1.0)
    f0, FT0, E0, n = to.interactions(c["r"], c["X"], 12, c["a"], True, builtin=full, height=c["height"], traps=c["traps"])
    assert n == 0 and np.array_equal(f, f0) and _maxrel(FT, FT0) <= 1e-14 and abs(E - E0) <= 1e-14 * abs(E0)
    assert np.abs(f0[:, 2] + b["w"]).max() > 1e-3                      # the wall and the height table do act on these blobs
    z = c["r"][:, 2]
    assert (z > c["height"][3]).any() and (z < c["height"][3]).any()   # blobs on both sides of h_cut


def _distances(r, n_blb, L):
    """minimum-image distances of the ordered pairs of blobs of different bodies, one flat array"""
    body = np.arange(len(r)) // n_blb
    out = []
    for i0 in range(0, len(r), 128):
        d = po.nearest(r[i0:i0 + 128, None, :] - r[None, :, :], L)
        out.append(np.sqrt((d * d).sum(axis=2))[body[i0:i0 + 128, None] != body[None, :]])
    return np.concatenate(out)


@pytest.mark.parametrize("name", list(pc.FORCE_CASES))
def test_every_force_case_is_sound(name):
    c = pc.force_case(name)
    nb, nblb, L = c["X"].shape[0], c["nblb"], c["L"]
    cut = pc.pair_cutoff(c)
    need = 2.0 * c["R"] + cut
    print("%s: %d x %d blobs, cell %.3f x %.3f, 2 R_body + r_cut = %.3f" % (name, nb, nblb, L[0], L[1], need))
    assert need <= 0.5 * min(L)                                       # the uniqueness condition, both axes
    assert c["r"][:, 2].min() > c["a"]                                 # every blob clear of the wall
    m = po.force_model(c["r"], c["X"], nblb, c["a"], L, builtin=c["builtin"], steric=c["steric"], table=c["table"], height=c["height"],
                       traps=c["traps"])
    print("    %d direct pairs and %d through a boundary inside the cutoff" % (m["direct"], m["through"]))
    if name in pc.TWO_BODIES:
        # one pair of bodies has ONE image inside the cutoff (that is the condition above), and the fold of a blob pair inside the
        # cutoff is the fold of the centres: blob displacements differ from the centres' by less than 2 R_body, so a raw component
        # of one pair beyond L / 2 and of another within r_cut would need 2 R_body + r_cut > L / 2.  Two bodies: one kind only
        assert m["through"] > 0 and m["direct"] == 0
    else:
        assert m["through"] > 0 and m["direct"] > 0
    d = _distances(c["r"], nblb, L)
    for radius in [x for x in (c["steric"][2] if c["steric"] else None, c["table"][3] if c["table"] else None,
                               c["table"][2] if c["table"] else None, 2.0 * c["a"]) if x is not None]:
        assert np.abs(d - radius).min() > 1e-9, radius
    assert int((d <= cut).sum()) == m["direct"] + m["through"]
    # what the case is there to reach (constants of rbl_forces.hip, read from the source)
    src = open(os.path.join(ROOT, "rigid_body_light_amd", "csrc", "rbl_forces.hip")).read()
    chunk = int(re.search(r"constexpr int IA_CHUNK = (\d+);", src).group(1))
    bt = int(re.search(r"constexpr int IA_BT = (\d+);", src).group(1))
    assert re.search(r"const int bt = S\.N_blb > 128 \? IA_BT :", src)
    reach = {"65xtetra": nb == 64 + 1, "130xtetra": 2 * 64 < nb <= 3 * 64, "3xfib130": 128 < nblb <= bt, "3xfib257": nblb == bt + 1,
             "2xfib513": nblb == chunk + 1}
    assert reach.get(name, True)


@pytest.mark.parametrize("nb", list(pc.DIPOLE_CASES))
def test_every_dipole_case_is_sound(nb):
    c = pc.dipole_case(nb)
    L, rc = c["L"], pc.DIPOLE["r_cut"]
    assert rc <= 0.5 * min(L)
    X = c["X"]
    d = np.linalg.norm(po.nearest(X[:, None, :] - X[None, :, :], L), axis=2)[~np.eye(nb, dtype=bool)]
    for core in c["cores"]:
        _, _, nd, nt = po.dipole_pairs_v(X, c["m_lab"], pc.DIPOLE["c_dd"], core, rc, L)
        print("%d trimers, cell %.2f x %.2f, r_core %.3f: %d direct pairs, %d through a boundary, %d in the core" % (nb, L[0], L[1], core, nd, nt, (d < core).sum()))
        assert nd > 0 and nt > 0 and nd + nt == int((d <= rc).sum())
        assert np.abs(d - core).min() > 1e-9 and np.abs(d - rc).min() > 1e-9
    assert not (d < c["cores"][0]).any() and (d < c["cores"][1]).any() and (d > c["cores"][1]).any()


# ---------------------------------------------------------------------------------------------------- the product's cases
TB = 256


def _tile():
    src = open(os.path.join(ROOT, "rigid_body_light_amd", "csrc", "rbl_kernels.hip")).read()
    m = re.search(r"^constexpr int TB = (\d+);", src, re.M)
    assert m, "rbl_kernels.hip no longer declares the ordered kernels' tile TB"
    return int(m.group(1))


def _chunks(N, jsplit, tb):
    """rbl_launch_apply_M_per's column chunks restated: tiles per chunk"""
    jtiles = (N + tb - 1) // tb
    jchunk = (jtiles + jsplit - 1) // jsplit * tb
    return [(min(j0 + jchunk, N) - j0 + tb - 1) // tb for j0 in range(0, N, jchunk)]


@pytest.mark.parametrize("name", list(pc.PRODUCT_CASES))
def test_every_product_case_reaches_its_tile_edges(name):
    import body_shapes as bs
    tb = _tile()
    assert tb == TB
    c = pc.product_case(name)
    N, rows = len(c["r"]), c["rows"]
    want = {"64xtetra": 256, "1xfib257": 257}.get(name, 765)
    assert N == want and len(rows) <= 16 and rows == sorted(set(rows))
    for t0 in range(0, N, tb):                                        # the first and the last row of every tile
        assert t0 in rows and min(t0 + tb, N) - 1 in rows
    for t0 in range(tb, N, tb):                                       # ... and of the bodies on either side of a tile boundary
        for body in {(t0 - 1) // c["nblb"], t0 // c["nblb"]}:
            assert body * c["nblb"] in rows and (body + 1) * c["nblb"] - 1 in rows
    assert all(l == 0.0 or l > 4.0 * c["a"] for l in c["L"]) and bs.min_distance(c["r"]) >= 2.0 * c["a"] - 1e-12
    assert c["r"][:, 2].min() > c["a"]
    if name == "64xtetra":
        assert N % tb == 0
    if name == "1xfib257":
        assert min(c["L"]) > 2.0 * c["R"] + 2.0 * c["a"] + 1.0
    if want == 765:
        assert _chunks(N, 2, tb) == [2, 1] and _chunks(N, 3, tb) == [1, 1, 1] and _chunks(N, 5, tb) == [1, 1, 1] and N - 2 * tb == 253
        for b, e in pc.RANGES_765:
            inside = [i for i in sorted(set(pc.ROWS_765 + pc.ROWS_765_RANGE)) if b <= i < e]
            for t0 in range(b, e, tb):                                # the first and the last row of every ROW tile of the range
                assert t0 in inside and min(t0 + tb, e) - 1 in inside
        assert [min(256, 700 - t0) for t0 in range(100, 700, tb)] == [256, 256, 88]


# ---------------------------------------------------------------------------------------------------- the per-pair probe
CELL = (37.3, 41.9)                                                   # in radii; commensurate with nothing in the star


@pytest.mark.parametrize("a", pp.RADII)
def test_every_star_has_targets_whose_nearest_image_is_not_the_direct_one(a):
    for off in pp.PLACEMENTS:
        for hi, h in enumerate(pp.HEIGHTS):
            for w, where in enumerate(pp.WHERE):
                st = pp.star(a, h, off, where, (w + hi) % 3 - 1)
                d = (st["r"] - st["r"][st["src"]])[st["target"]]
                for L in ((CELL[0] * a, CELL[1] * a), (CELL[0] * a, 0.0), (0.0, CELL[1] * a)):
                    folded = po._folds(d, L)
                    near = np.linalg.norm(po.nearest(d, L), axis=1) / a
                    assert folded.sum() >= 10                         # (the r^ = 30 and 1000 targets off the z axis)
                    assert (near[folded] < 20.0).any() and near.min() > 1e-9   # far targets fold onto near separations
