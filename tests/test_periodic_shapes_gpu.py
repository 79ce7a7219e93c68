"""The periodic product k_apply_M_per<PX, PY> at the edges of its 256-blob tiles, against tests/periodic_oracle.py: rows(), sampled
at the first and the last row of every tile and of the bodies beside a tile boundary (tests/test_periodic_shapes_cpu.py checks the
row sets), every case at ordered_jsplit 0, 1, 2, 3 and 5 (more than there are tiles), relative L2 <= 1e-12 as in
tests/test_periodic_gpu.py, and bitwise equal when repeated.  The cases are tests/periodic_cases.py: PRODUCT_CASES:

    64 x tetra, (1, 1)       256   no ragged tile at all (njj == TB everywhere)
    1 x fib(257), (1, 1)     257   a column tile of one blob, a row tile with one valid row
    3 x fib(255), (1, 1)     765   three tiles, the last of 253; j-split 2: chunks of two tiles and of one
    the same, (2, 0), (0, 2) 765   <true, false> and <false, true> beyond one tile
    2 x shell_N_12           24    16 images on one axis and 1 on the other, both ways: the cap, and nx != ny

and the device entry point with row ranges whose row tiles align with no column tile, and two bodies exactly half a cell apart."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ETA = 1.0
JSPLITS = (0, 1, 2, 3, 5)
_REF = {}                     # (case, rows) -> the oracle's rows: computed once, shared, never written to


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _body(c):
    from rigid_body_light_amd import RigidBody
    return RigidBody(c["cfg"], c["X"], c["Q"], c["a"], ETA, 0.01, wall_PC=True)


def _rows(orc, name, c, which):
    key = (name, tuple(which))
    if key not in _REF:
        _REF[key] = po.rows(orc, c["r"], list(which), c["a"], ETA, c["L"], c["images"])
        _REF[key].setflags(write=False)
    return _REF[key]


def _idx(which):
    return np.concatenate([np.arange(3 * i, 3 * i + 3) for i in which])


@pytest.mark.parametrize("name", list(pc.PRODUCT_CASES))
def test_product_at_the_tile_edges(orc, name):
    c = pc.product_case(name)
    rb = _body(c)
    rb.set_periodic(c["L"][0], c["L"][1], images=c["images"])
    r = rb.get_blob_positions().reshape(-1)
    assert np.abs(r - c["r"].reshape(-1)).max() <= 1e-13
    F = np.random.default_rng(21).standard_normal(r.size)
    ref = _rows(orc, name, c, c["rows"]) @ F
    idx = _idx(c["rows"])
    for js in JSPLITS:
        rb.cb.set_option("ordered_jsplit", js)
        U = rb.apply_M(F, r)
        print("%s, images %s, j-split %d: rel. error of %d sampled rows %.2e" % (name, c["images"], js, len(c["rows"]), _rel(U[idx], ref)))
        assert np.isfinite(U).all() and _rel(U[idx], ref) <= 1e-12
        assert np.array_equal(rb.apply_M(F, r), U)                    # one summation order
    rb.cb.set_option("ordered_jsplit", 0)


def test_row_ranges_that_align_with_no_column_tile(orc):
    """the 765-blob case through the device entry point: (100, 700) gives row tiles at 100, 356 and 612, the last of 88 rows;
    (255, 257) straddles a tile boundary; (764, 765) is one row.  The output is pre-filled: the words behind the range stay"""
    import torch
    name = "3xfib255"
    c = pc.product_case(name)
    rb = _body(c)
    rb.set_periodic(c["L"][0], c["L"][1], images=c["images"])
    N = 765
    which = sorted(pc.ROWS_765 + pc.ROWS_765_RANGE)
    assert len(set(which)) == len(which)
    R =np.concatenate([_rows(orc, name, c, pc.ROWS_765), _rows(orc, name, c, pc.ROWS_765_RANGE)])
    order = np.argsort(pc.ROWS_765 + pc.ROWS_765_RANGE)
    F = np.random.default_rng(22).standard_normal(3 * N)
    ref = (R @ F).reshape(-1, 3)[order]                               # row k of ref: blob which[k]
    dev = torch.device("cuda:0")
    dF, dr = torch.from_numpy(F).to(dev), torch.from_numpy(c["r"].reshape(-1).copy()).to(dev)
    for js in (0, 2):
        rb.cb.set_option("ordered_jsplit", js)
        for b, e in pc.RANGES_765:
            out = torch.full((3 * N,), -7.0, dtype=torch.float64, device=dev)
            rb.ctx.apply_M(dF.data_ptr(), dr.data_ptr(), N, b, e, out.data_ptr())
            rb.ctx.sync_check()
            got = out.cpu().numpy()
            inside = [k for k, i in enumerate(which) if b <= i < e]
            g = got[:3 * (e - b)].reshape(-1, 3)[[which[k] - b for k in inside]]
            print("rows [%d, %d), j-split %d: %d sampled rows, rel. error %.2e" % (b, e, js, len(inside), _rel(g, ref[inside])))
            assert len(inside) >= 1 and _rel(g, ref[inside]) <= 1e-12
            assert np.isfinite(got[:3 * (e - b)]).all() and np.all(got[3 * (e - b):] == -7.0)
    rb.cb.set_option("ordered_jsplit", 0)


@pytest.mark.parametrize("images", [(16, 1), (1, 16)])
def test_image_cap_and_unequal_image_counts(orc, images):
    """2 x shell_N_12 against the dense M_per: 300 blocks x 99 images.  The oracle's sum over 33 x 3 images in a 6.7 x 4.0 cell
    differs from its sum over 3 x 33 by far more than the tolerance (asserted), so counts that are swapped cannot pass"""
    from rigid_body_light_amd import make_config
    c = make_config(2, 12, True)
    s = pc.spacing(c["a"])
    L = (2.0 * s, s + 0.7)
    rb = _body(c)
    r = rb.get_blob_positions().reshape(-1)
    F = np.random.default_rng(23).standard_normal(r.size)
    for n in (images, images[::-1]):
        if ("2xshell", n) not in _REF:
            _REF[("2xshell", n)] = po.dense_M(orc, r, c["a"], ETA, L, n)
    ref, swapped = _REF[("2xshell", images)] @ F, _REF[("2xshell", images[::-1])] @ F
    assert _rel(swapped, ref) > 1e-6                                  # the oracle's own two sums: a million tolerances apart
    rb.set_periodic(L[0], L[1], images=images)
    assert rb.periodic()["images"] == images
    for js in JSPLITS:
        rb.cb.set_option("ordered_jsplit", js)
        U = rb.apply_M(F, r)
        print("images %s, j-split %d: rel. error %.2e (the swapped counts' sum is %.2e away)" % (images, js, _rel(U, ref), _rel(swapped, ref)))
        assert _rel(U, ref) <= 1e-12 and np.array_equal(rb.apply_M(F, r), U)
    rb.cb.set_option("ordered_jsplit", 0)


def test_a_blob_touching_the_wall_at_the_origin_meets_no_padded_slot(orc):
    """the kernel cuts a ragged column tile short instead of padding it.  The unread slots of its LDS tile hold (0, 0, a) with no
    force: a sweep that read them would add exact zeros for every blob but one that sits right there, which it would report as two
    blobs in one place.  2 x shell_N_12 (one ragged tile) moved so that the lowest blob is at (0, 0, a) exactly, and by whole cells
    from there: served without an error flag, equal to the oracle"""
    from rigid_body_light_amd import make_config
    c = make_config(2, 12, True)
    a, L = c["a"], (8.0, 7.5)
    r = pc.blob_positions(c["cfg"], c["X"], c["Q"])
    k = int(np.argmin(r[:, 2]))
    rb = _body(c)
    rb.set_periodic(L[0], L[1], images=(1, 1))
    F = np.random.default_rng(25).standard_normal(r.size)
    for cells in ((0.0, 0.0), (1.0, -2.0)):
        r = r - r[k] + np.array([cells[0] * L[0], cells[1] * L[1], a])
        r[k] = [cells[0] * L[0], cells[1] * L[1], a]
        assert r[:, 2].min() == a
        ref = po.dense_M(orc, r, a, ETA, L, (1, 1)) @ F
        for js in (0, 3):
            rb.cb.set_option("ordered_jsplit", js)
            U = rb.apply_M(F, r.reshape(-1))                          # (raises on any error flag)
            print("lowest blob at (%g, %g, a), j-split %d: rel. error %.2e" % (r[k, 0], r[k, 1], js, _rel(U, ref)))
            assert _rel(U, ref) <= 1e-12
    rb.cb.set_option("ordered_jsplit", 0)


def test_two_bodies_exactly_half_a_cell_apart(orc):
    """twelve pairs of blobs exactly L / 2 = 4 apart in x (coordinates on a grid of 2^-30, so the differences are exact).  The
    oracle's rint(d / L) rounds the tie to even: the displacement stays as it is.  The kernel forms d / L from radius-scaled
    coordinates and a reciprocal, so each tie falls to whichever side the rounding of THAT pair lands on -- either is a nearest
    image, and at nx = 1 the truncated sums of the two differ.  Every block of the device's dense matrix must equal the oracle's
    with one of the two choices; the test prints which, pair by pair"""
    from rigid_body_light_amd import make_config
    c = make_config(2, 12, True)
    a, L = c["a"], (8.0, 7.5)
    r0 = pc.blob_positions(c["cfg"], c["X"][:1], c["Q"][:1])
    r0[:, 0] = np.round(r0[:, 0] * 2.0 ** 30) / 2.0 ** 30
    r = np.concatenate([r0, r0 + np.array([4.0, 0.3, 0.2])])
    assert np.array_equal(r[12:, 0] - r[:12, 0], np.full(12, 4.0)) and np.array_equal((r[12:, 0] - 8.0) + 8.0, r[12:, 0])
    keep = po.dense_M(orc, r, a, ETA, L, (1, 1))                      # d = -4 stays -4
    r_flip = r.copy()
    r_flip[12:, 0] -= 8.0                                             # a whole cell, exactly: the same system with d = +4 for the ties
    flip = po.dense_M(orc, r_flip, a, ETA, L, (1, 1))
    ties = [(k, k + 12) for k in range(12)]
    rest = np.ones((72, 72), dtype=bool)
    for i, j in ties:
        rest[3 * i:3 * i + 3, 3 * j:3 * j + 3] = rest[3 * j:3 * j + 3, 3 * i:3 * i + 3] = False
    assert np.abs((keep - flip)[rest]).max() <= 1e-13 * np.abs(keep).max()          # the two differ in the tie blocks ...
    assert min(np.abs((keep - flip)[3 * i:3 * i + 3, 3 * j:3 * j + 3]).max() for i, j in ties) > 1e-6 * np.abs(keep).max()   # ... and there they do
    rb = _body(c)
    rb.set_periodic(L[0], L[1], images=(1, 1))
    G = np.stack([rb.apply_M(e, r.reshape(-1)) for e in np.eye(72)], axis=1)
    mix, chosen = keep.copy(), []
    for i, j in ties:
        bi, bj = slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3)
        ek, ef = np.abs(G[bi, bj] - keep[bi, bj]).max(), np.abs(G[bi, bj] - flip[bi, bj]).max()
        chosen.append("stays" if ek <= ef else "flips")
        if ef < ek:
            mix[bi, bj], mix[bj, bi] = flip[bi, bj], flip[bj, bi]
    print("the twelve ties d = -L / 2 (row blob in the first body):", " ".join(chosen))
    print("dense matrix against the oracle with these choices: rel. error %.2e" % _rel(G, mix))
    assert _rel(G, mix) <= 1e-12
    F = np.random.default_rng(24).standard_normal(72)
    for js in (0, 3):
        rb.cb.set_option("ordered_jsplit", js)
        assert _rel(rb.apply_M(F, r.reshape(-1)), mix @ F) <= 1e-12
    rb.cb.set_option("ordered_jsplit", 0)
    assert np.abs(G - G.T).max() <= 1e-14 * np.abs(G).max()          # d_ji = -d_ij exactly, rint is odd: the mirror block takes the mirror choice
