"""Work-queue schedules of the four-row symmetric kernel with one and with two chunk lengths (RBL_OPT_SYM_TAIL_CHUNK,
RBL_OPT_SYM_TAIL_SHARE) at 64*37+5 and 64*130+17 blobs, wall and free space: each agrees with the ordered-rows kernel to the 1e-13
that tests/test_sym_rows_per_lane_gpu.py holds four against two rows to, is bitwise reproducible run to run and bitwise the same
with the work queue off; one overlapping pair still raises the overlap flag."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [64 * 37 + 5, 64 * 130 + 17]
# (sym_tail_chunk, sym_tail_share): one length (the short length set to the chunk length); length 1 over half the tiles; 3 over a quarter
SCHEDULES = {"one": (None, 0), "fine1_half": (1, 500), "fine3_quarter": (3, 250)}
CHUNK = 7                      # (the heuristic's chunk is one tile at these sizes: a length the short ones can be shorter than)
_cache = {}


def _lattice(N, overlap=False):
    """N blobs of radius 0.1 on a cubic lattice 0.25 apart, x fastest (compact 64-blob tiles, most tile pairs far), jittered"""
    rng = np.random.default_rng(N)
    m = int(np.ceil(N ** (1.0 / 3.0)))
    i = np.arange(N)
    r = 0.25 * np.stack([i % m, (i // m) % m, i // (m * m)], axis=1) + 0.02 * rng.random((N, 3))
    r[:, 2] += 0.3
    if overlap:
        r[N - 3] = r[5]                                       # coincides with blob 5 (the overlap flag: r < 1e-12 a), first and last row group
    return r.reshape(-1)


def _run(N, wall, overlap=False):
    key = (N, wall, overlap)
    if key in _cache:
        return _cache[key]
    import torch
    from rigid_body_light_amd._lib import DeviceContext, RblError
    dev = torch.device("cuda:0")
    ctx = DeviceContext(0.1, 1.0, wall, stream_ptr=torch.cuda.current_stream().cuda_stream)
    r = torch.from_numpy(_lattice(N, overlap)).to(dev)
    F = torch.from_numpy(np.random.default_rng(N + 1).standard_normal(3 * N)).to(dev)

    def product():
        out = torch.full_like(F, 7.25)
        ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, out.data_ptr())
        flagged = False
        try:
            ctx.sync_check()
        except RblError as e:
            flagged = True
            assert "overlap" in str(e).lower(), str(e)
        return out.cpu().numpy(), flagged

    res = {}
    ctx.set_option("matvec_kernel", 1)
    res["ordered"] = product()
    ctx.set_option("matvec_kernel", 2)
    ctx.set_option("sym_rows_per_lane", 4); ctx.set_option("sym_waves", 4); ctx.set_option("sym_chunk", CHUNK)
    assert ctx.apply_M_sym_kernel(N, wall, 1, 1) == "k_apply_M_sym<%s,4>" % ("true" if wall else "false")
    for name, (tc, ts) in SCHEDULES.items():
        ctx.set_option("sym_tail_chunk", CHUNK if tc is None else tc); ctx.set_option("sym_tail_share", ts)
        units, info, _ = ctx.apply_M_sym_units(N, 256)
        assert info["work_queue"] and info["live_only"] and (info["tail_chunks"] > 0) == (tc is not None)
        ctx.set_option("sym_work_queue", 1)
        a = product(); b = product()
        ctx.set_option("sym_work_queue", 0)
        res[name] = (a, b, product())
        ctx.set_option("sym_work_queue", 1)
    ctx.close()
    _cache[key] = res
    return res


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("wall", [True, False])
@pytest.mark.parametrize("N", SIZES)
def test_schedule_matches_ordered_rows_and_is_reproducible(N, wall, schedule):
    res = _run(N, wall)
    ref, flagged = res["ordered"]
    assert not flagged and np.all(np.isfinite(ref))
    (a, fa), (b, _), (q, _) = res[schedule]
    err = np.linalg.norm(a - ref) / np.linalg.norm(ref)
    print("N=%d wall=%d %s: relative difference to the ordered-rows kernel %.3e" % (N, wall, schedule, err))
    assert not fa and err < 1e-13
    assert np.array_equal(a, b), "two runs of one schedule differ"
    assert np.array_equal(a, q), "work queue on and off differ"


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_overlap_flag_survives(schedule):
    res = _run(SIZES[0], True, overlap=True)
    assert res["ordered"][1], "the ordered-rows kernel did not flag the overlapping pair"
    assert all(flagged for _, flagged in res[schedule])
