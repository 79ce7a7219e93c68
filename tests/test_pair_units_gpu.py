"""The product kernels after the wall pair arithmetic moved to the shared length unit of rbl_pair.hpp (coordinates times lambda / a when
loaded, sums times lambda nf when they leave; free-space kernels keep radii): every caller of the unit-scaled forms on the smallest
system that reaches its paths, against the oracle's dense product and against each other.

System: compact clusters far from each other, blobs sorted by cluster -- the far map of the symmetric kernels marks far AND near tile
pairs --, the lowest cluster below z = a (the damping zone), a few pairs closer than 2a (the near branch) and one pair across the
boundary of tiles 0 and 1 at exactly 2a (a = 0.5: the separation 1.0 and its coordinates are exact), one above the other.  1 100
blobs are 18 tiles with a ragged last one: two row groups of 4 waves x 4 tiles for the four-row kernel; 300 blobs for the wave-unit kernels.

Bounds: <= 1e-12 of the maximum norm against the oracle (the suite's bound), <= 1e-13 between kernels (sums of the same pairs in other
orders).  The verdicts -- two coinciding blobs, a blob below the wall -- are raised at the same inputs as before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
A, ETA = 0.5, 0.9


def _system(N, wall):
    """(N, 3) positions: clusters of 130 blobs on jittered 2.5a lattices, centres 60a apart; cluster 0 lies lowest"""
    rng = np.random.default_rng(N)
    per, pts = 130, []
    for c in range((N + per - 1) // per):
        g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(4), indexing="ij"), -1).reshape(-1, 3)[:per].astype(float)
        p = (g * 2.5 + rng.uniform(-0.2, 0.2, g.shape)) * A
        p += np.array([60.0 * (c % 3), 60.0 * (c // 3), 0.7 + 1.5 * c]) * A       # z from 0.5 a (cluster 0) upwards: no self term of 1 / h^5 size
                                                                                 # that would own the maximum norm
        pts.append(p)
    r = np.concatenate(pts)[:N]
    if not wall:
        r[:, 2] -= 3.0 * A                                                       # free space: heights of either sign
    # the near branch: five blobs of cluster 1 taken out of the lattice and put 1.2 a .. 1.9 a outside its x = 0 face, next to blob k
    for k, d in zip(range(140, 150, 2), (1.2, 1.4, 1.6, 1.8, 1.9)):
        r[k + 1] = r[k] - np.array([d * A, 0.0, 0.0])
    # exactly 2a across the boundary of tiles 0 and 1: blob 63 (top layer of cluster 0) on coordinates with few bits, blob 64 taken out
    # of the lattice and put 2a = 1.0 above it
    r[63] = np.round(r[63] * 64.0) / 64.0
    r[64] = r[63] + np.array([0.0, 0.0, 2.0 * A])
    return r


def _far_map(r, NI):
    """k_tile_far's rule on the host: far[S][J] -- every blob of tile J farther than 2a from every blob of row super-tile S"""
    T = (len(r) + 63) // 64
    lo = np.array([r[64 * t:64 * t + 64].min(0) for t in range(T)]) / A
    hi = np.array([r[64 * t:64 * t + 64].max(0) for t in range(T)]) / A
    far = np.zeros(((T + NI - 1) // NI, T), dtype=bool)
    for S in range(far.shape[0]):
        for J in range(T):
            g2 = min(float((np.maximum(np.maximum(lo[J] - hi[I], lo[I] - hi[J]), 0.0) ** 2).sum()) for I in range(NI * S, min(NI * S + NI, T)))
            far[S, J] = g2 > 4.0001
    return far


@pytest.fixture(scope="module")
def gpu():
    import torch
    return torch, torch.device("cuda:0")


def _ctx(gpu, wall):
    from rigid_body_light_amd._lib import DeviceContext
    torch, _ = gpu
    return DeviceContext(A, ETA, wall, stream_ptr=torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def cases(orc):
    """{(N, wall): (positions, two force vectors, the oracle's two dense products)}, computed once"""
    out = {}
    for N, wall in ((1100, True), (300, True), (1100, False)):
        r = _system(N, wall)
        F = np.random.default_rng(7 * N + wall).standard_normal((2, 3 * N))
        ref = np.stack([orc.apply_M(F[v], r.reshape(-1), A, ETA, wall, mode="dense") for v in range(2)])
        out[(N, wall)] = (r, F, ref)
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _product(gpu, ctx, r, F, opts, nrhs=1, kernel=None, wall=True):
    """one product under the options (restored afterwards); kernel: what the symmetric table must report for it"""
    torch, dev = gpu
    N = len(r)
    dr = torch.from_numpy(r.reshape(-1).copy()).to(dev)
    dF = torch.from_numpy(np.ascontiguousarray(F[:nrhs]).reshape(-1).copy()).to(dev)
    out = torch.full_like(dF, 7.25)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        if kernel is not None:
            assert ctx.apply_M_sym_kernel(N, wall, 1, nrhs) == kernel
        if nrhs == 1:
            ctx.apply_M(dF.data_ptr(), dr.data_ptr(), N, 0, N, out.data_ptr())
        else:
            ctx.apply_M_multi(dF.data_ptr(), dr.data_ptr(), N, nrhs, out.data_ptr())
        ctx.sync_check()
    finally:
        for k in opts:
            ctx.set_option(k, 1 if k == "sym_wave_units" else 0)
    return out.cpu().numpy().reshape(nrhs, 3 * N)


def test_the_system_reaches_every_path(cases):
    r, _, _ = cases[(1100, True)]
    N = len(r)
    assert (N + 63) // 64 == 18 and N % 64 != 0
    d = np.linalg.norm(r[:, None] - r[None], axis=2) / A + 10.0 * np.eye(N)
    assert (r[:, 2] > 0).all() and ((r[:, 2] < A).sum() >= 20) and ((r[:, 2] > A).sum() > 900)      # the damping zone and above it
    assert d[63, 64] == 2.0 and d.min() > 1.0                                                     # exactly 2a, tiles 0 | 1; nothing coincides
    assert 5 <= ((d < 2.0).sum() // 2) <= 12                                                      # the near branch, a few pairs
    for NI in (2, 4):
        far = _far_map(r, NI)
        upper = np.array([[J >= NI * S + NI for J in range(far.shape[1])] for S in range(far.shape[0])])
        assert (far & upper).any() and (~far & upper).any()                                       # both sweeps of the symmetric kernels


def test_wall_four_rows_per_lane(gpu, cases):
    r, F, ref = cases[(1100, True)]
    ctx = _ctx(gpu, True)
    four = _product(gpu, ctx, r, F, {"sym_waves": 4, "sym_rows_per_lane": 4}, kernel="k_apply_M_sym<true,4>")[0]
    two = _product(gpu, ctx, r, F, {"sym_waves": 4, "sym_rows_per_lane": 2}, kernel="k_apply_M_sym<true,2>")[0]
    ordered = _product(gpu, ctx, r, F, {"matvec_kernel": 1})[0]
    ctx.close()
    print("four rows vs oracle %.2e, vs two rows %.2e, vs ordered %.2e; ordered vs oracle %.2e" % (
        _rel(four, ref[0]), _rel(four, two), _rel(four, ordered), _rel(ordered, ref[0])))
    assert _rel(four, ref[0]) <= 1e-12 and _rel(two, ref[0]) <= 1e-12 and _rel(ordered, ref[0]) <= 1e-12
    assert _rel(four, two) <= 1e-13 and _rel(four, ordered) <= 1e-13


@pytest.mark.parametrize("rows", [1, 2])
def test_wall_wave_unit_kernels(gpu, cases, rows):
    r, F, ref = cases[(300, True)]
    ctx = _ctx(gpu, True)
    name = "k_apply_M_symw<true>" if rows == 1 else "k_apply_M_symw<true,2>"
    got = _product(gpu, ctx, r, F, {"sym_wave_units": 1, "sym_waves": 1, "sym_rows_per_lane": rows}, kernel=name)[0]
    ordered = _product(gpu, ctx, r, F, {"matvec_kernel": 1})[0]
    ctx.close()
    print("wave units, %d rows: vs oracle %.2e, vs ordered %.2e" % (rows, _rel(got, ref[0]), _rel(got, ordered)))
    assert _rel(got, ref[0]) <= 1e-12 and _rel(got, ordered) <= 1e-13


def test_wall_two_vectors(gpu, cases):
    r, F, ref = cases[(1100, True)]
    ctx = _ctx(gpu, True)
    got = _product(gpu, ctx, r, F, {}, nrhs=2)
    one = np.stack([_product(gpu, ctx, r, F[v:v + 1], {})[0] for v in range(2)])
    ctx.close()
    for v in range(2):
        print("two vectors, vector %d: vs oracle %.2e, vs the one-vector product %.2e" % (v, _rel(got[v], ref[v]), _rel(got[v], one[v])))
        assert _rel(got[v], ref[v]) <= 1e-12 and _rel(got[v], one[v]) <= 1e-13


def test_free_space(gpu, cases):
    r, F, ref = cases[(1100, False)]
    ctx = _ctx(gpu, False)
    sym = _product(gpu, ctx, r, F, {}, wall=False)[0]
    four = _product(gpu, ctx, r, F, {"sym_waves": 4, "sym_rows_per_lane": 4}, kernel="k_apply_M_sym<false,4>", wall=False)[0]
    ordered = _product(gpu, ctx, r, F, {"matvec_kernel": 1}, wall=False)[0]
    ctx.close()
    print("free space: vs oracle %.2e, four rows vs default %.2e, vs ordered %.2e" % (_rel(sym, ref[0]), _rel(four, sym), _rel(sym, ordered)))
    assert _rel(sym, ref[0]) <= 1e-12 and _rel(four, ref[0]) <= 1e-12
    assert _rel(four, sym) <= 1e-13 and _rel(sym, ordered) <= 1e-13


@pytest.mark.parametrize("opts", [{}, {"sym_waves": 4, "sym_rows_per_lane": 4}, {"matvec_kernel": 1}])
def test_refusals_at_the_same_inputs(gpu, cases, opts):
    """two coinciding blobs (r < 1e-12 a) and a blob below the wall still raise; a pair 1e-6 a apart and a blob 1e-6 a above the wall do not"""
    from rigid_body_light_amd._lib import RblError
    r, F, _ = cases[(300, True)]
    ctx = _ctx(gpu, True)
    bad = r.copy(); bad[201] = bad[200]                                          # one pair, inside a tile
    with pytest.raises(RblError, match="OVERLAPPING"):
        _product(gpu, ctx, bad, F, dict(opts))
    bad = r.copy(); bad[70] = bad[10]                            # ... and across tiles 0 | 1
    with pytest.raises(RblError, match="OVERLAPPING"):
        _product(gpu, ctx, bad, F, dict(opts))
    ok = r.copy(); ok[201] = ok[200] + np.array([1e-6 * A, 0.0, 0.0])
    assert np.isfinite(_product(gpu, ctx, ok, F, dict(opts))).all()
    bad = r.copy(); bad[17, 2] = -1e-9 * A
    with pytest.raises(RblError, match="below the wall"):
        _product(gpu, ctx, bad, F, dict(opts))
    ok = r.copy(); ok[17, 2] = 1e-6 * A
    assert np.isfinite(_product(gpu, ctx, ok, F, dict(opts))).all()
    ctx.close()
