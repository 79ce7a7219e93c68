"""The work units of the symmetric product (rbl_apply_M_sym_units: no device needed) under the work queue's two chunk lengths
(RBL_OPT_SYM_TAIL_CHUNK, RBL_OPT_SYM_TAIL_SHARE): every tile pair of the upper triangle is swept exactly once, no dead unit is
handed out, within a chunk length the tile counts never rise and the last unit drawn is the shortest of its length, the slab ranges
of the units are disjoint and inside the workspace, and both options set to one length reproduce the schedule of the one-length
kernel (tests/golden/sym_unit_sequence_2117.json, recorded from it)."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256
SIZES = [64, 1000, 64 * 33 + 5, 64 * 257 + 1, 128400]
# (sym_tail_chunk, sym_tail_share): heuristic; short length 1 (over the heuristic's share); no short chunks ("share 0": the short
# length set to the chunk length); every tile at the short length
# (and a short length that divides neither the chunk length nor the 8 or 16 row tiles of a row group, over a quarter of the tiles)
COMBOS = {"heuristic": (0, 0), "fine1": (1, 0), "share0": (-1, 0), "share1000": (0, 1000), "fine3_quarter": (3, 250)}
# (sym_rows_per_lane, sym_waves, sym_chunk): the heuristic's kernel, and the work queue's kernels forced at every size they exist
# for -- with the heuristic's chunk length (one tile below cfg 3) and with lengths that leave cut units of many sizes
SHAPES = {"auto": (0, 0, 0), "rows4": (4, 4, 0), "rows2": (2, 4, 0), "rows4_c7": (4, 4, 7), "rows2_c12": (2, 4, 12), "rows4_c16": (4, 4, 16)}


class Lib:
    def __init__(self):
        L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
        i64 = ctypes.c_int64
        L.rbl_create.restype = ctypes.c_void_p
        L.rbl_destroy.argtypes = [ctypes.c_void_p]
        L.rbl_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, i64]
        L.rbl_option_key.argtypes = [ctypes.c_char_p]
        L.rbl_apply_M_sym_units.argtypes = [ctypes.c_void_p, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, i64,
                                            ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(i64)]
        self.L = L

    def units(self, n_blobs, opts):
        """(units [n, 9], info, workspace bytes) under the named options, or None when no kernel has the forced shape"""
        L, i64 = self.L, ctypes.c_int64
        h = L.rbl_create()
        try:
            for k, v in opts.items():
                assert L.rbl_set_option(h, L.rbl_option_key(k.encode()), v) == 0, (k, v)
            n, wb, info = i64(0), i64(0), (ctypes.c_int * 8)()
            if L.rbl_apply_M_sym_units(h, n_blobs, N_CU, 1, 1, None, 0, ctypes.byref(n), info, ctypes.byref(wb)) != 0:
                return None
            u = np.zeros((n.value, 9), dtype=np.int64)
            assert L.rbl_apply_M_sym_units(h, n_blobs, N_CU, 1, 1, u.ctypes.data, n.value, ctypes.byref(n), info, ctypes.byref(wb)) == 0
            keys = ("rows_per_lane", "waves", "chunk", "tail_chunk", "tail_chunks", "chunks", "work_queue", "live_only")
            return u, dict(zip(keys, list(info))), wb.value
        finally:
            L.rbl_destroy(h)


@pytest.fixture(scope="module")
def lib():
    return Lib()


def _options(lib, n_blobs, shape, combo):
    rows, waves, chunk = SHAPES[shape]
    opts = {}
    if rows:
        opts["sym_rows_per_lane"] = rows
        opts["sym_waves"] = waves
    if chunk:
        opts["sym_chunk"] = chunk
    tc, ts = COMBOS[combo]
    if tc < 0:                                   # the chunk length itself: ask the layout for it
        got = lib.units(n_blobs, opts)
        if got is None:
            return None
        tc = got[1]["chunk"]
    if tc:
        opts["sym_tail_chunk"] = tc
    if ts:
        opts["sym_tail_share"] = ts
    return opts


@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n_blobs", SIZES)
def test_units_cover_the_triangle_once(lib, n_blobs, shape, combo):
    opts = _options(lib, n_blobs, shape, combo)
    got = lib.units(n_blobs, opts) if opts is not None else None
    if got is None:                              # (four waves need >= 2 rows per lane and that many row tiles: no kernel, RBL_ERR_ARG)
        assert shape != "auto"
        return
    u, info, wbytes = got
    T = (n_blobs + 63) // 64
    NI, SW = info["rows_per_lane"], info["waves"]
    tiles_per_group = NI * (SW if SW > 1 else 1)
    idx, g, c, j0, nt = u[:, 0], u[:, 1], u[:, 2], u[:, 3], u[:, 4]
    assert len(u) > 0 and np.all(np.diff(idx) > 0)
    assert np.all(nt >= 1), "a dead unit was listed"
    # chunk c's tiles under the layout the info describes
    C, Cf, nf = info["chunk"], info["tail_chunk"], info["tail_chunks"]
    first = np.where(c < nf, c * Cf, nf * Cf + (c - nf) * C)
    length = np.where(c < nf, Cf, C)
    it00 = g * tiles_per_group
    assert np.all(it00 < T)
    assert np.array_equal(j0, np.maximum(first, it00)) and np.array_equal(j0 + nt, np.minimum(first + length, T))
    # every (row tile I of the group, column tile J >= I) exactly once: a group's rows are tiles [it00, it00 + tiles_per_group)
    cover = np.zeros((T, T), dtype=np.int32)
    for gi, a, n in zip(g, j0, nt):
        r0, r1 = gi * tiles_per_group, min((gi + 1) * tiles_per_group, T)
        cover[r0:r1, a:a + n] += 1
    want = np.triu(np.ones((T, T), dtype=np.int32))
    # (a group's later row tiles lie behind the first column tiles of a unit the diagonal cuts: swept by nobody, J < I)
    assert np.array_equal(np.triu(cover), want)
    if T <= 600:
        assert np.all(np.tril(cover, -1) <= 1)
    # slab ranges: disjoint, inside the workspace
    ranges = [(o, o + l) for o, l in zip(u[:, 5], u[:, 6]) if l > 0] + [(o, o + l) for o, l in zip(u[:, 7], u[:, 8]) if l > 0]
    ranges.sort()
    r = np.array(ranges, dtype=np.int64)
    assert r[0, 0] >= 0 and r[-1, 1] * 8 <= wbytes
    assert np.all(r[1:, 0] >= r[:-1, 1]), "two units write the same slab entries"
    if info["live_only"]:
        assert np.array_equal(idx, np.arange(len(u)))          # the queue's limit is the live count
        fine = c < nf
        if nf and nf < info["chunks"]:
            assert not np.any(fine[:np.argmax(fine)]) and np.all(fine[np.argmax(fine):]), "the short chunks are drawn last"
        for cls in (fine, ~fine):
            if np.any(cls):
                assert np.all(np.diff(nt[cls]) <= 0), "tile counts rise within a chunk length"
        last = fine if np.any(fine) else ~fine
        assert nt[-1] == nt[last].min() and nt[-1] <= nt.max()


def test_queue_layouts_take_the_live_schedule(lib):
    """the sizes above reach the work queue's new schedule (heuristic: at cfg 3; forced shapes: from 2 117 blobs on)"""
    u, info, _ = lib.units(128400, {})
    assert info["rows_per_lane"] == 4 and info["work_queue"] and info["live_only"]
    u1, info1, _ = lib.units(128400, {"sym_tail_chunk": 1})
    assert info1["tail_chunk"] == 1 and info1["tail_chunks"] > 0 and len(u1) > len(u) - info["tail_chunks"]
    for n in SIZES[2:]:
        assert lib.units(n, {"sym_rows_per_lane": 4, "sym_waves": 4})[1]["live_only"]


@pytest.mark.parametrize("key,opts", [("heuristic", {}), ("rows4_waves4", {"sym_rows_per_lane": 4, "sym_waves": 4})])
def test_one_length_is_the_parents_schedule(lib, key, opts):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "sym_unit_sequence_2117.json")))[key]
    probe = lib.units(gold["n_blobs"], opts)[1]
    opts = dict(opts, sym_tail_chunk=probe["chunk"], sym_tail_share=1000)
    u, info, _ = lib.units(gold["n_blobs"], opts)
    assert (info["rows_per_lane"], info["waves"], info["chunk"], info["chunks"]) == (gold["rows_per_lane"], gold["waves"], gold["chunk"], gold["chunks"])
    assert info["tail_chunks"] == 0 and not info["live_only"]
    assert u[:, 1:3].tolist() == gold["units"]
