"""Four rows per lane (k_apply_M_sym<wall, 4>, the default one-vector kernel of large single-GPU systems) against two rows per
lane (k_apply_M_sym<wall, 2>): the same unordered pairs, only their grouping into work units and the order of the column sums
differ.  Checked at cfg 3 size and at ragged sizes (N not a multiple of 256 blobs: a last super-tile of 1-3 tiles, a last tile
of fewer than 64 blobs): agreement to 1e-13 and bitwise run-to-run reproducibility of each."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _products(nb, nblb, wall, seed):
    import torch
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    dev = torch.device("cuda:0")
    c = make_config(nb, nblb, wall)
    N = nb * nblb
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    r = torch.empty(3 * N, dtype=torch.float64, device=dev)
    ctx.blob_positions(0, nb, r.data_ptr())
    F = torch.from_numpy(np.random.default_rng(seed).standard_normal(3 * N)).to(dev)
    res = {}
    ctx.set_option("sym_waves", 4)                              # two rows per lane in the same four-wave kernel at every size
    for rows in (2, 4):
        ctx.set_option("sym_rows_per_lane", rows)
        assert ctx.apply_M_sym_info(N, 1, 1)[0] == rows
        assert ctx.apply_M_sym_kernel(N, wall, 1, 1) == "k_apply_M_sym<%s,%d>" % ("true" if wall else "false", rows)
        outs = []
        for _ in range(2):
            out = torch.full_like(F, 7.25)
            ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, out.data_ptr())
            ctx.sync_check()
            outs.append(out.cpu().numpy())
        res[rows] = outs
    ctx.set_option("sym_rows_per_lane", 0); ctx.set_option("sym_waves", 0)
    default_rows = ctx.apply_M_sym_info(N, 1, 1)[0]
    ctx.close()
    return N, res, default_rows


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_four_rows_per_lane_matches_two_at_cfg3():
    N, res, default_rows = _products(200, 642, True, 11)
    assert N % 256 != 0
    assert default_rows == 4                                     # the heuristic's choice at cfg 3
    for rows in (2, 4):
        assert np.all(np.isfinite(res[rows][0]))
        assert np.array_equal(res[rows][0], res[rows][1])         # bitwise reproducible run to run
    assert _rel(res[4][0], res[2][0]) < 1e-13


@pytest.mark.parametrize("nb,nblb,wall", [(41, 642, True), (70, 642, True), (100, 162, False), (13, 2562, False)])
def test_four_rows_per_lane_matches_two_at_ragged_sizes(nb, nblb, wall):
    N, res, _ = _products(nb, nblb, wall, nb)
    assert N % 256 != 0
    for rows in (2, 4):
        assert np.all(np.isfinite(res[rows][0]))
        assert np.array_equal(res[rows][0], res[rows][1])
    assert _rel(res[4][0], res[2][0]) < 1e-13
