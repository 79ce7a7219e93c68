"""The wall product kernels after the polynomial brackets of rbl_wall_coeffs stay un-multiplied (odd powers w^3, w^5 carry the factor u;
rbl_pair.hpp, shared length unit) and the far sweep advances its column offset last: every wall kernel that reaches the header's form, on the
systems of tests/test_pair_units_gpu.py with a layer of blobs put at heights between 1.0001 a and 1.5 a (w and u largest, the wall part
at its largest against the free-space part), each against the oracle's dense product.

1 100 blobs: the smallest system that reaches the four-row far sweep with four waves (18 tiles, two row groups); 300 blobs: the two-row
and diagonal paths and the wave-unit kernels.

Limits: the error of the build before the change on the same inputs (PARENT, measured with that build's library on one MI355X) times 1.5
-- another grouping of the same polynomial moves last bits, a lost digit shows as 10 x; the same reasoning as tests/test_pair_units_cpu.py
-- and never above the suite's 1e-12.  Four rows against two rows and against the ordered kernel: sums of the same pairs in other orders,
1.5 x what the build before gave.  This build's figures: profiles/wall_brackets.md, section 3; every test prints its own (-s)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_pair_units_gpu import A, ETA, _ctx, _far_map, _product, _rel, _system  # noqa: E402  (the same system, the same calls)

pytestmark = pytest.mark.gpu
FACTOR = 1.5
SUITE = 1e-12
# figure -> relative error in the maximum norm, build before the change (commit c748844), same inputs
PARENT = {
    "four_rows": 3.693e-15, "two_rows": 3.693e-15, "ordered": 5.088e-15, "two_rows_300": 1.216e-15, "ordered_300": 1.476e-15,
    "wave_units_1": 1.216e-15, "wave_units_2": 1.216e-15, "two_vectors_0": 3.693e-15, "two_vectors_1": 4.413e-15,
    "four_vs_two": 3.282e-16, "four_vs_ordered": 2.954e-15,
}
OPTS = {
    "four_rows": ({"sym_waves": 4, "sym_rows_per_lane": 4}, "k_apply_M_sym<true,4>"),
    "two_rows": ({"sym_waves": 4, "sym_rows_per_lane": 2}, "k_apply_M_sym<true,2>"),
    "wave_units_1": ({"sym_wave_units": 1, "sym_waves": 1, "sym_rows_per_lane": 1}, "k_apply_M_symw<true>"),
    "wave_units_2": ({"sym_wave_units": 1, "sym_waves": 1, "sym_rows_per_lane": 2}, "k_apply_M_symw<true,2>"),
    "ordered": ({"matvec_kernel": 1}, None),
}
TWO_VECTOR_KERNEL = "k_apply_M_symw2v<true,1>"    # what the default options pick for two vectors at 18 tiles: wave units, one row per lane
# (figure, N, kernel): each against the oracle
AGAINST_ORACLE = [("four_rows", 1100, "four_rows"), ("two_rows", 1100, "two_rows"), ("ordered", 1100, "ordered"),
                  ("two_rows_300", 300, "two_rows"), ("ordered_300", 300, "ordered"),
                  ("wave_units_1", 300, "wave_units_1"), ("wave_units_2", 300, "wave_units_2")]


def layered_system(N):
    """tests/test_pair_units_gpu.py's system with the bottom lattice layer of clusters 1 .. 3 (blobs from 150 on: behind the pairs of the near
    branch) moved to heights drawn from [1.0001 a, 1.5 a]; their lateral spacing stays 2.1 a or more"""
    r = _system(N, True)
    idx = np.array([i for i in range(150, min(N, 520)) if (i % 130) % 4 == 0])
    r[idx, 2] = np.random.default_rng(11 * N).uniform(1.0001, 1.5, len(idx)) * A
    return r, idx


@pytest.fixture(scope="module")
def gpu():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(orc):
    """{N: (positions, two force vectors, the oracle's two dense products)}, computed once"""
    out = {}
    for N in (1100, 300):
        r, _ = layered_system(N)
        F = np.random.default_rng(5 * N + 1).standard_normal((2, 3 * N))
        ref = np.stack([orc.apply_M(F[v], r.reshape(-1), A, ETA, True, mode="dense") for v in range(2)])
        out[N] = (r, F, ref)
    return out


@pytest.fixture(scope="module")
def products(gpu, cases):
    """every product of the module, computed once: {(N, kernel): result}, and the two-vector product at 1 100"""
    out = {}
    ctx = _ctx(gpu, True)
    for _, N, kern in AGAINST_ORACLE:
        r, F, _ = cases[N]
        opts, name = OPTS[kern]
        out[(N, kern)] = _product(gpu, ctx, r, F, dict(opts), kernel=name)[0]
    r, F, _ = cases[1100]
    out["two_vectors"] = _product(gpu, ctx, r, F, {}, nrhs=2, kernel=TWO_VECTOR_KERNEL)
    ctx.close()
    return out


def figures(cases, products):
    f = {}
    for fig, N, kern in AGAINST_ORACLE:
        f[fig] = _rel(products[(N, kern)], cases[N][2][0])
    for v in range(2):
        f["two_vectors_%d" % v] = _rel(products["two_vectors"][v], cases[1100][2][v])
    f["four_vs_two"] = _rel(products[(1100, "four_rows")], products[(1100, "two_rows")])
    f["four_vs_ordered"] = _rel(products[(1100, "four_rows")], products[(1100, "ordered")])
    return f


def limit(fig):
    return min(FACTOR * PARENT[fig], SUITE)


def test_the_layer_is_there_and_every_path_is_reached():
    for N, nlayer in ((1100, 90), (300, 35)):
        r, idx = layered_system(N)
        assert len(idx) >= nlayer and (r[idx, 2] >= 1.0001 * A).all() and (r[idx, 2] <= 1.5 * A).all()
        d = np.linalg.norm(r[:, None] - r[None], axis=2) / A + 10.0 * np.eye(N)
        assert (r[:, 2] > 0).all() and d.min() > 1.0 and 5 <= ((d < 2.0).sum() // 2) <= 12       # nothing coincides; the near branch, a few pairs
        assert d[idx][:, idx].min() > 2.0                                                         # the layer itself: far formula throughout
    r, idx = layered_system(1100)
    assert (1100 + 63) // 64 == 18
    for NI in (2, 4):
        far = _far_map(r, NI)
        upper = np.array([[J >= NI * S + NI for J in range(far.shape[1])] for S in range(far.shape[0])])
        assert (far & upper).any() and (~far & upper).any()                                       # both sweeps of the symmetric kernels
    # the layer meets far sweeps of the four-row kernel: its tiles (2 .. 8) are swept as columns by row group 0 (tiles 0 .. 3), far from it
    far4 = _far_map(r, 4)
    assert far4[0, 4:9].any() and set(idx // 64) >= {2, 3, 4, 5, 6, 7, 8}


@pytest.mark.parametrize("fig", [a[0] for a in AGAINST_ORACLE] + ["two_vectors_0", "two_vectors_1"])
def test_against_the_oracle(cases, products, fig):
    got = figures(cases, products)[fig]
    print("%s: %.3e (before %.3e, limit %.3e)" % (fig, got, PARENT[fig], limit(fig)))
    assert got <= limit(fig)


@pytest.mark.parametrize("fig", ["four_vs_two", "four_vs_ordered"])
def test_four_rows_against_the_other_kernels(cases, products, fig):
    got = figures(cases, products)[fig]
    print("%s: %.3e (before %.3e, limit %.3e)" % (fig, got, PARENT[fig], FACTOR * PARENT[fig]))
    assert got <= FACTOR * PARENT[fig]
