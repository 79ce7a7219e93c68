"""Blob types and the pair table per type pair of include/rbl.h section 4 without a GPU: every refusal of the two setters with its
message and the previous state kept, the round trips, bit 7 of rbl_interactions_active, the Python layer's own refusals, the
patch helper, and the numpy oracle (tests/typed_oracle.py) against tests/table_oracle.py and against its own energy."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import table_oracle  # noqa: E402
import typed_oracle  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)
ERR_ARG = 11


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = vp
    lib.rbl_destroy.argtypes = [vp]
    lib.rbl_last_error.restype = ctypes.c_char_p
    lib.rbl_last_error.argtypes = [vp]
    lib.rbl_set_blob_types.argtypes = [vp, vp, cint, cint, cint]
    lib.rbl_get_blob_types.argtypes = [vp, ip, ip, ip, vp]
    lib.rbl_set_type_table.argtypes = [vp, cint, cint, vp, vp, cint, dbl, dbl, cint]
    lib.rbl_get_type_table.argtypes = [vp, cint, cint, ip, dp, dp, ip, vp]
    lib.rbl_clear_type_tables.argtypes = [vp]
    lib.rbl_set_pair_table.argtypes = [vp, vp, vp, cint, dbl, dbl, cint]
    lib.rbl_set_bonds.argtypes = [vp, cint, vp, vp, vp, vp, cint, cint]
    lib.rbl_interactions_active.argtypes = [vp, ip]
    return lib


@pytest.fixture
def ctx():
    lib = _lib()
    h = lib.rbl_create()
    yield lib, h
    lib.rbl_destroy(h)


def _active(lib, h):
    m = cint(-1)
    assert lib.rbl_interactions_active(h, ctypes.byref(m)) == 0
    return m.value


def _types(lib, h):
    n, nt, on = cint(-1), cint(-1), cint(-1)
    assert lib.rbl_get_blob_types(h, ctypes.byref(n), ctypes.byref(nt), ctypes.byref(on), None) == 0
    t = np.full(max(n.value, 0), -1, dtype=np.int32)
    assert lib.rbl_get_blob_types(h, None, None, None, t.ctypes.data) == 0
    return n.value, nt.value, on.value, t


def _table(lib, h, ta, tb):
    n, lo, hi, on = cint(-1), dbl(0), dbl(0), cint(-1)
    assert lib.rbl_get_type_table(h, ta, tb, ctypes.byref(n), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(on), None) == 0
    coef = np.zeros((max(n.value - 1, 0), 4))
    assert lib.rbl_get_type_table(h, ta, tb, None, None, None, None, coef.ctypes.data) == 0
    return n.value, lo.value, hi.value, on.value, coef


def _lj(r, eps=1.3, sig=0.5):
    s6 = (sig / r) ** 6
    return 4 * eps * (s6 * s6 - s6), -24 * eps * (2 * s6 * s6 - s6) / r


def _set_types(lib, h, t, n_types, on=1):
    t = np.ascontiguousarray(t, dtype=np.int32)
    return lib.rbl_set_blob_types(h, t.ctypes.data, t.size, n_types, on)


def test_set_blob_types_refuses_and_keeps_the_previous_types(ctx):
    lib, h = ctx
    assert _types(lib, h)[:3] == (0, 0, 0)                                     # never set
    good = np.array([0, 2, 1, 1, 0, 2], dtype=np.int32)
    assert _set_types(lib, h, good, 3) == 0                                    # no rbl_set_parameters needed
    cases = [
        (good, 0, b"set_blob_types: n_types = 0 must lie in [1, 8]"),
        (good, 9, b"set_blob_types: n_types = 9 must lie in [1, 8]"),
        (good, -1, b"set_blob_types: n_types = -1 must lie in [1, 8]"),
        (good, 2, b"set_blob_types: type[1] = 2 must lie in [0, 2)"),             # the FIRST offending index
        (np.array([0, 1, 0, -4, 9]), 3, b"set_blob_types: type[3] = -4 must lie in [0, 3)"),
        (np.array([8]), 8, b"set_blob_types: type[0] = 8 must lie in [0, 8)"),
    ]
    for t, nt, msg in cases:
        for on in (0, 1):
            assert _set_types(lib, h, t, nt, on) == ERR_ARG, (t, nt)
            assert lib.rbl_last_error(h).startswith(msg), lib.rbl_last_error(h)
            n, nt_, on_, now = _types(lib, h)
            assert (n, nt_, on_) == (6, 3, 1) and np.array_equal(now, good)
    assert lib.rbl_set_blob_types(h, good.ctypes.data, 0, 3, 1) == ERR_ARG and lib.rbl_last_error(h).startswith(b"set_blob_types: n must be >= 1")
    assert lib.rbl_set_blob_types(h, None, 6, 3, 1) == ERR_ARG and lib.rbl_last_error(h).startswith(b"set_blob_types: type must not be NULL")
    assert _types(lib, h)[:3] == (6, 3, 1)
    assert lib.rbl_set_blob_types(h, None, 0, 0, 0) == 0                        # only the switch
    n, nt, on, now = _types(lib, h)
    assert (n, nt, on) == (6, 3, 0) and np.array_equal(now, good)
    assert _set_types(lib, h, np.arange(8), 8, 0) == 0                          # stored, switched off; 8 types are allowed
    n, nt, on, now = _types(lib, h)
    assert (n, nt, on) == (8, 8, 0) and np.array_equal(now, np.arange(8))


def test_set_type_table_refuses_and_keeps_the_previous_table(ctx):
    lib, h = ctx
    n = 9
    r = np.linspace(0.4, 1.5, n)
    U, dU = _lj(r)
    assert lib.rbl_set_type_table(h, 2, 1, U.ctypes.data, dU.ctypes.data, n, 0.4, 1.5, 1) == 0
    good = _table(lib, h, 1, 2)
    assert good[:4] == (n, 0.4, 1.5, 1)
    assert np.abs(good[4] - table_oracle.hermite_coef(U, dU, 0.4, 1.5)).max() <= 1e-15 * np.abs(U).max()
    for ta, tb in [(8, 0), (0, 8), (-1, 1), (3, 100)]:
        assert lib.rbl_set_type_table(h, ta, tb, U.ctypes.data, dU.ctypes.data, n, 0.4, 1.5, 1) == ERR_ARG
        assert lib.rbl_last_error(h).startswith(b"set_type_table: ta = %d, tb = %d: both types must lie in [0, 8)" % (ta, tb))
        assert lib.rbl_get_type_table(h, ta, tb, None, None, None, None, None) == ERR_ARG
    nan, inf = float("nan"), float("inf")
    Unan, Uinf, dUnan = U.copy(), U.copy(), dU.copy()
    Unan[3], Uinf[0], dUnan[n - 1] = nan, inf, nan
    bad = [                                                                     # rbl_set_pair_table's own refusals
        (U, dU, 1, 0.4, 1.5), (U, dU, 0, 0.4, 1.5), (U, dU, -3, 0.4, 1.5), (np.zeros(4), np.zeros(4), 65538, 0.4, 1.5),
        (U, dU, n, 1.5, 1.5), (U, dU, n, 1.6, 1.5),
        (Unan, dU, n, 0.4, 1.5), (Uinf, dU, n, 0.4, 1.5), (U, dUnan, n, 0.4, 1.5),
        (U, dU, n, -0.1, 1.5),
        (U, dU, n, nan, 1.5), (U, dU, n, 0.4, inf), (U, dU, n, 0.4, nan),
    ]
    for Ub, dUb, nb_, lo, hi in bad:
        for on in (0, 1):
            assert lib.rbl_set_type_table(h, 1, 2, Ub.ctypes.data, dUb.ctypes.data, nb_, lo, hi, on) == ERR_ARG, (nb_, lo, hi)
            assert lib.rbl_last_error(h).startswith(b"set_type_table")
            # ... the message of the pair table's entry point for the same arguments, under the new name
            assert lib.rbl_set_pair_table(h, Ub.ctypes.data, dUb.ctypes.data, nb_, lo, hi, on) == ERR_ARG
            assert lib.rbl_last_error(h) == b"set_pair_table" + msg_tail(lib, h, 1, 2, Ub, dUb, nb_, lo, hi, on)
            now = _table(lib, h, 2, 1)
            assert now[:4] == good[:4] and np.array_equal(now[4], good[4])
    assert lib.rbl_set_type_table(h, 1, 2, None, dU.ctypes.data, n, 0.4, 1.5, 1) == ERR_ARG
    assert lib.rbl_set_type_table(h, 1, 2, None, None, n, 0.4, 1.5, 1) == ERR_ARG
    assert _table(lib, h, 1, 2)[:4] == good[:4]
    assert _table(lib, h, 0, 0)[0] == 0 and _table(lib, h, 7, 7)[0] == 0        # the other pairs: never set


def msg_tail(lib, h, ta, tb, U, dU, n, lo, hi, on):
    """what rbl_set_type_table says after its name for these (refused) arguments"""
    assert lib.rbl_set_type_table(h, ta, tb, U.ctypes.data, dU.ctypes.data, n, lo, hi, on) == ERR_ARG
    msg = lib.rbl_last_error(h)
    assert msg.startswith(b"set_type_table")
    return msg[len(b"set_type_table"):]


def test_round_trips_and_the_unordered_pair(ctx):
    lib, h = ctx
    tabs = {}
    for q, (ta, tb) in enumerate([(0, 0), (0, 1), (3, 1), (7, 7), (7, 0)]):
        n = 5 + 3 * q
        lo, hi = 0.1 * (q + 1), 1.0 + 0.2 * q
        U, dU = _lj(np.linspace(lo, hi, n), eps=1.0 + q)
        assert lib.rbl_set_type_table(h, ta, tb, U.ctypes.data, dU.ctypes.data, n, lo, hi, q % 2) == 0
        tabs[(ta, tb)] = (n, lo, hi, q % 2, table_oracle.hermite_coef(U, dU, lo, hi))
    for (ta, tb), want in tabs.items():
        for x, y in ((ta, tb), (tb, ta)):                                       # one table under both orders
            got = _table(lib, h, x, y)
            assert got[:4] == want[:4] and np.abs(got[4] - want[4]).max() <= 1e-15 * np.abs(want[4]).max()
    n = 4
    U, dU = _lj(np.linspace(0.5, 0.9, n))
    assert lib.rbl_set_type_table(h, 1, 3, U.ctypes.data, dU.ctypes.data, n, 0.5, 0.9, 1) == 0     # (1, 3) replaces (3, 1)
    assert _table(lib, h, 3, 1)[:4] == (n, 0.5, 0.9, 1)
    assert lib.rbl_set_type_table(h, 3, 1, None, None, 0, 0.0, 0.0, 0) == 0                        # only the switch
    assert _table(lib, h, 1, 3)[:4] == (n, 0.5, 0.9, 0)
    assert _table(lib, h, 0, 1)[:4] == tabs[(0, 1)][:4]                                            # the others untouched
    assert lib.rbl_clear_type_tables(h) == 0
    for ta, tb in tabs:
        assert _table(lib, h, ta, tb)[:4] == (0, 0.0, 0.0, 0)


def test_bit_7_needs_types_on_and_a_usable_table_on(ctx):
    lib, h = ctx
    n = 6
    U, dU = _lj(np.linspace(0.4, 1.2, n))
    tab = (U.ctypes.data, dU.ctypes.data, n, 0.4, 1.2)
    assert _active(lib, h) == 0
    assert lib.rbl_set_type_table(h, 0, 1, *tab, 1) == 0
    assert _active(lib, h) == 0                                                 # a table, no types
    assert _set_types(lib, h, [0, 1, 0], 2, on=0) == 0
    assert _active(lib, h) == 0                                                 # types stored, off
    assert _set_types(lib, h, [0, 1, 0], 2) == 0
    assert _active(lib, h) == 128
    assert lib.rbl_set_type_table(h, 1, 0, None, None, 0, 0.0, 0.0, 0) == 0
    assert _active(lib, h) == 0                                                 # types on, the only table off
    assert lib.rbl_set_type_table(h, 2, 1, *tab, 1) == 0
    assert _active(lib, h) == 0                                                 # type 2 >= n_types = 2: stored and ignored
    assert _table(lib, h, 1, 2)[:4] == (n, 0.4, 1.2, 1)
    assert _set_types(lib, h, [0, 1, 2], 3) == 0
    assert _active(lib, h) == 128                                               # ... until there are three types
    assert _set_types(lib, h, [0, 0, 0], 1) == 0
    assert _active(lib, h) == 0
    assert lib.rbl_set_type_table(h, 0, 0, *tab, 1) == 0
    assert _active(lib, h) == 128
    assert lib.rbl_set_pair_table(h, *tab, 1) == 0
    assert _active(lib, h) == 130                                               # beside the untyped table's own bit
    assert lib.rbl_set_blob_types(h, None, 0, 0, 0) == 0
    assert _active(lib, h) == 2
    assert _set_types(lib, h, [0, 0, 0], 1) == 0 and lib.rbl_clear_type_tables(h) == 0
    assert _active(lib, h) == 2


def test_bonds_alone_still_report_64(ctx):
    lib, h = ctx
    body = np.array([0, 1], dtype=np.int32)
    anchor, param = np.zeros(6), np.array([1.0, 0.5])
    assert lib.rbl_set_bonds(h, 1, body.ctypes.data, anchor.ctypes.data, None, param.ctypes.data, 1, 1) == 0
    assert _active(lib, h) == 64
    assert _set_types(lib, h, [0, 1], 2) == 0                                   # types without a table change nothing
    assert _active(lib, h) == 64


# ------------------------------------------------------------------------------------------------------------ the Python layer
def _three():
    from rigid_body_light_amd import RigidBody, load_structure
    cfg = load_structure(12)[1]
    X = [[0.0, 0.0, 5.0], [4.0, 0.0, 5.0], [0.0, 4.0, 5.0]]
    return RigidBody(cfg, X, [[1.0, 0.0, 0.0, 0.0]] * 3, 1.0, 1.0, 0.01), cfg


def test_python_round_trips_and_refuses_shapes_and_dtypes_before_the_library():
    from rigid_body_light_amd._lib import RblError
    rb, cfg = _three()
    t = np.arange(12) % 3
    rb.set_blob_types(t)                                                        # n_types from the largest type
    got = rb.blob_types()
    assert got["on"] and got["n_types"] == 3 and np.array_equal(got["types"], t) and got["types"].dtype == np.int32
    per_body = np.stack([t, (t + 1) % 3, np.zeros(12, dtype=int)])
    rb.set_blob_types(per_body, n_types=5, on=False)
    got = rb.blob_types()
    assert not got["on"] and got["n_types"] == 5 and np.array_equal(got["types"], per_body.reshape(-1))
    before = rb.blob_types()
    for bad in (t.astype(float), t[:5], np.zeros((2, 12), dtype=int), np.zeros((3, 12, 1), dtype=int), np.zeros(0, dtype=int), 3):
        with pytest.raises(ValueError, match="set_blob_types"):
            rb.set_blob_types(bad)
    with pytest.raises(RblError, match=r"type\[2\] = 2 must lie in \[0, 2\)"):   # the range is the library's to refuse
        rb.set_blob_types(t, n_types=2)
    now = rb.blob_types()
    assert now["n_types"] == before["n_types"] and np.array_equal(now["types"], before["types"])
    rb.set_blob_types(None, on=False)
    x = np.linspace(0.5, 1.5, 7)
    U, dU = _lj(x)
    rb.set_type_table(2, 0, U, dU, 0.5, 1.5)
    for ta, tb in ((0, 2), (2, 0)):
        got = rb.type_table(ta, tb)
        assert (got["n"], got["lo"], got["hi"], got["on"]) == (7, 0.5, 1.5, True)
        assert np.abs(got["coef"] - table_oracle.hermite_coef(U, dU, 0.5, 1.5)).max() <= 1e-15 * np.abs(U).max()
    for ta, tb in ((0.0, 1), (1, "a"), (True, 0), (None, 0)):
        with pytest.raises(ValueError, match="set_type_table"):
            rb.set_type_table(ta, tb, U, dU, 0.5, 1.5)
        with pytest.raises(ValueError, match="type_table"):
            rb.type_table(ta, tb)
    with pytest.raises(ValueError, match="set_type_table: U and dU must be one-dimensional and of one length"):
        rb.set_type_table(0, 1, U, dU[:-1], 0.5, 1.5)
    with pytest.raises(RblError, match="ta = 8, tb = 0"):
        rb.set_type_table(8, 0, U, dU, 0.5, 1.5)
    rb.set_type_table(0, 2, None, None, 0.0, 0.0, on=False)
    assert not rb.type_table(2, 0)["on"] and rb.type_table(2, 0)["n"] == 7
    rb.clear_type_tables()
    assert rb.type_table(2, 0)["n"] == 0
    assert rb.ctx.interactions_active() == 0


def test_patch_types_marks_the_cap():
    from rigid_body_light_amd import load_structure, patch_types
    cfg = load_structure(42)[1]
    n = cfg - cfg.mean(axis=0)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    axis = np.array([0.3, -0.2, 0.9])
    for c in (0.0, 0.5, -0.5, 0.999):
        t = patch_types(cfg, axis, c)
        assert t.dtype == np.int32 and t.shape == (42,)
        assert np.array_equal(t == 1, n @ (axis / np.linalg.norm(axis)) >= c)
    janus = patch_types(cfg + [3.0, -1.0, 2.0], 5.0 * axis)                      # the mean is removed, the axis normalised
    assert np.array_equal(janus, patch_types(cfg, axis)) and 10 <= janus.sum() <= 32
    assert np.array_equal(janus + patch_types(cfg, -axis, 1e-12), np.ones(42))   # the two hemispheres (no blob on this equator)
    assert patch_types(cfg, axis, 1.0).sum() == 0 and patch_types(cfg, axis, -1.0).sum() == 42
    for bad in ((cfg[:, :2], axis, 0.0), (cfg, [0.0, 0.0, 0.0], 0.0), (cfg, [1.0, 0.0], 0.0), (cfg, axis, 1.5), (cfg, [np.nan, 0, 1], 0.0)):
        with pytest.raises(ValueError, match="patch_types"):
            patch_types(*bad)


# ------------------------------------------------------------------------------------------------------------ the oracle
def _packed():
    """test_interaction_tables_cpu's three 12-blob bodies"""
    nb, nblb = 3, 12
    X = np.array([[0.0, 0.0, 0.75], [0.9, 0.1, 0.8], [0.3, 0.8, 0.85]])
    rng = np.random.default_rng(4)
    cfg = rng.standard_normal((nblb, 3)) * 0.35
    cfg -= cfg.mean(axis=0)
    r = np.concatenate([X[b] + cfg @ np.linalg.qr(rng.standard_normal((3, 3)))[0] for b in range(nb)])
    return r, X, nblb


def _shifted_lj(lo, hi, n, eps=1.3):
    x = np.linspace(lo, hi, n)
    U, dU = _lj(x, eps=eps)
    return U - U[-1], dU, lo, hi


def test_one_type_with_T00_is_the_untyped_pair_table_exactly():
    r, X, nblb = _packed()
    a = 0.2
    tab = _shifted_lj(0.45, 1.4, 65)
    builtin = dict(w=0.7, eps_wall=1.3, b_wall=0.15, eps_blob=0.9, b_blob=0.1, r_cut=2 * a + 8 * 0.1)
    height = _shifted_lj(0.5, 1.1, 33)
    traps = (np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 3.0], [0.0, 0.0, 0.0]]), X + 0.1)
    for kw in (dict(), dict(builtin=builtin), dict(builtin=builtin, height=height, traps=traps)):
        f, FT, E, npairs = table_oracle.interactions(r, X, nblb, a, True, pair=tab, **kw)
        ft, FTt, Et, npt, nty = typed_oracle.interactions(r, X, nblb, a, True, types=np.zeros(r.shape[0], dtype=int), tables={(0, 0): tab}, **kw)
        assert np.array_equal(f, ft) and np.array_equal(FT, FTt) and E == Et and npairs == npt
        assert nty == 2 * int((typed_oracle.pair_distances(r, nblb) <= tab[3]).sum()) > 0
        # ... and without tables it is table_oracle's model
        f0, FT0, E0, np0, nty0 = typed_oracle.interactions(r, X, nblb, a, True, pair=tab, **kw)
        assert np.array_equal(f, f0) and np.array_equal(FT, FT0) and E == E0 and npairs == np0 and nty0 == 0


def test_typed_oracle_splits_by_type_pair_and_its_forces_are_minus_the_gradient():
    r, X, nblb = _packed()
    a = 0.2
    types = np.random.default_rng(8).integers(0, 3, r.shape[0])
    tables = {(0, 0): _shifted_lj(0.45, 1.4, 129), (2, 1): _shifted_lj(0.3, 0.9, 129, eps=0.4), (0, 2): _shifted_lj(0.5, 1.7, 129, eps=2.0)}
    pair = _shifted_lj(0.4, 1.1, 129, eps=0.7)
    builtin = dict(w=0.7, eps_wall=1.3, b_wall=0.15, eps_blob=0.9, b_blob=0.1, r_cut=2 * a + 8 * 0.1)
    kw = dict(types=types, tables=tables, builtin=builtin, pair=pair)
    f, FT, E, npairs, nty = typed_oracle.interactions(r, X, nblb, a, True, **kw)
    # the typed part is the sum over the type pairs of the untyped oracle restricted to the blobs of those types: by hand
    d = r[:, None, :] - r[None, :, :]
    dist = np.sqrt((d * d).sum(axis=2))
    body = np.arange(r.shape[0]) // nblb
    extra, cnt = np.zeros_like(r), 0
    for (s, t), tab in tables.items():
        m = (body[:, None] != body[None, :]) & (dist <= tab[3])
        m &= ((types[:, None] == s) & (types[None, :] == t)) | ((types[:, None] == t) & (types[None, :] == s))
        dUt = table_oracle.table_eval(tab, dist)[1]
        extra += (np.where(m, -dUt / np.where(dist > 0, dist, 1.0), 0.0)[:, :, None] * d).sum(axis=1)
        cnt += int(m.sum())
    f0 = table_oracle.interactions(r, X, nblb, a, True, builtin=builtin, pair=pair)[0]
    assert cnt == nty > 0 and np.abs(f - f0 - extra).max() <= 1e-13 * np.abs(f).max() and np.abs(extra).max() > 1e-3 * np.abs(f).max()
    # (1, 2) and (2, 1) name one table; giving both is refused
    f21 = typed_oracle.interactions(r, X, nblb, a, True, types=types, tables={(1, 2): tables[(2, 1)]})[0]
    assert np.array_equal(f21, typed_oracle.interactions(r, X, nblb, a, True, types=types, tables={(2, 1): tables[(2, 1)]})[0])
    with pytest.raises(AssertionError):
        typed_oracle.interactions(r, X, nblb, a, True, types=types, tables={(1, 2): pair, (2, 1): pair})
    eps = 1e-6
    g = np.zeros_like(r)
    for i in range(r.shape[0]):
        for k in range(3):
            rp, rm = r.copy(), r.copy()
            rp[i, k] += eps
            rm[i, k] -= eps
            g[i, k] = (typed_oracle.interactions(rp, X, nblb, a, True, **kw)[2] - typed_oracle.interactions(rm, X, nblb, a, True, **kw)[2]) / (2 * eps)
    assert np.abs(f + g).max() <= 1e-7 * np.abs(f).max()
    # minimum image: a cell far larger than the system changes nothing, one that brings an image closer does
    fL = typed_oracle.interactions(r, X, nblb, a, True, L=(50.0, 50.0), **kw)[0]
    assert np.abs(fL - f).max() <= 1e-13 * np.abs(f).max()
    shifted = r.copy()
    shifted[2 * nblb:, 0] += 10.0                                                # body 2 a whole cell away along x
    fs = typed_oracle.interactions(shifted, X + [[0, 0, 0], [0, 0, 0], [10.0, 0, 0]], nblb, a, True, L=(10.0, 0.0), **kw)[0]
    assert np.abs(fs - f).max() <= 1e-12 * np.abs(f).max()
