"""Bonds and tethers of include/rbl.h section 4 without a GPU: the numpy oracle (tests/bond_oracle.py) against central differences
of its own energy, and the argument checks, getters and activity bit of rbl_set_bonds and rbl_set_bond_table (host-only: no
device is touched), and the shape checks of the Python wrappers."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bond_oracle as bo  # noqa: E402
import magnetic_oracle as mo  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)
RBL_ERR_ARG = 11
INF, NAN = float("inf"), float("nan")


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = vp
    lib.rbl_destroy.argtypes = [vp]
    lib.rbl_last_error.restype = ctypes.c_char_p
    lib.rbl_last_error.argtypes = [vp]
    lib.rbl_interactions_active.argtypes = [vp, ip]
    lib.rbl_set_traps.argtypes = [vp, vp, vp, cint, cint]
    lib.rbl_set_pair_table.argtypes = [vp, vp, vp, cint, dbl, dbl, cint]
    lib.rbl_set_bonds.argtypes = [vp, cint, vp, vp, vp, vp, cint, cint]
    lib.rbl_get_bonds.argtypes = [vp, ip, ip, ip, vp, vp, vp, vp]
    lib.rbl_set_bond_table.argtypes = [vp, vp, vp, cint, dbl, dbl, cint]
    lib.rbl_get_bond_table.argtypes = [vp, ip, dp, dp, ip, vp]
    return lib


def test_the_error_code_of_the_header_is_the_one_used_here():
    import re
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    m = re.search(r"RBL_ERR_ARG\s*=\s*(-?\d+)", text) or re.search(r"#define\s+RBL_ERR_ARG\s+(-?\d+)", text)
    assert m and int(m.group(1)) == RBL_ERR_ARG


# ------------------------------------------------------------------------------------------------------------ 1: the oracle
def morse_table(lo=0.6, hi=1.8, n=129):
    """a Morse well with its minimum at d = 1, tabulated on lo .. hi"""
    x = np.linspace(lo, hi, n)
    return (np.exp(-2.0 * (x - 1.0)) - 2.0 * np.exp(-(x - 1.0)), -2.0 * np.exp(-2.0 * (x - 1.0)) + 2.0 * np.exp(-(x - 1.0)), lo, hi)


def _system():
    """four bodies, eight bonds: harmonic ones between bodies (one stored with the larger index first) and to a lab point, and
    tabulated ones whose lengths lie below r_min, inside the grid and beyond r_cut (one of each between bodies, one tether)"""
    X = np.array([[0.0, 0.0, 2.0], [1.3, 0.2, 2.2], [0.4, 1.6, 1.8], [2.3, 1.7, 2.6]])
    rng = np.random.default_rng(4)
    Q = rng.standard_normal((4, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    body = np.array([[0, 1], [2, 1], [3, -1], [1, 3], [0, 2], [3, 2], [1, -1], [0, 3]])
    anchor = 0.3 * rng.standard_normal((8, 6))
    anchor[2, 3:] = [2.9, 1.2, 3.1]                            # lab points
    anchor[6, 3:] = [1.5, 0.1, 1.2]
    kind = np.array([0, 0, 0, 1, 1, 1, 1, 0])
    k = np.array([3.0, 1.5, 2.0, 1.2, 0.8, 2.5, 1.1, 0.7])
    l0 = np.array([0.9, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 1.4])
    return X, Q, body, anchor, kind, k, l0


def _fit_table(X, Q, body, anchor, kind):
    """a grid that puts the tabulated bonds of _system below it, inside it and beyond it, none within 1e-3 of either end"""
    d = np.array([np.linalg.norm(np.subtract(*bo.end_points(X, Q, body, anchor, b)[2:])) for b in range(len(body)) if kind[b] == 1])
    ds = np.sort(d)
    assert ds.size >= 3 and ds[1] - ds[0] > 4e-3 and ds[-1] - ds[-2] > 4e-3
    lo, hi = 0.5 * (ds[0] + ds[1]), 0.5 * (ds[-1] + ds[-2])
    assert (d < lo).any() and ((d > lo) & (d < hi)).any() and (d > hi).any()
    assert np.abs(d - lo).min() > 1e-3 and np.abs(d - hi).min() > 1e-3
    return morse_table(lo, hi, 97)


def test_oracle_forces_and_torques_are_minus_the_gradient_of_its_energy():
    """h = 1e-6: truncation ~ h^2 |FT|, rounding ~ eps sum|terms| / h = 2e-10 sum|terms|; with sum|terms| <= 100 |FT|max (asserted)
    both stay below 1e-7 |FT|max -- the bound and its justification of tests/test_magnetic_cpu.py"""
    X, Q, body, anchor, kind, k, l0 = _system()
    table = _fit_table(X, Q, body, anchor, kind)
    kw = dict(kind=kind, table=table)
    FT, E, state, Eabs = bo.bonds(X, Q, body, anchor, k, l0, with_scale=True, **kw)
    assert Eabs <= 100 * np.abs(FT).max()
    h = 1e-6
    g = np.zeros((4, 6))
    for i in range(4):
        for c in range(3):
            Ep = []
            for s in (1.0, -1.0):
                Xs = X.copy()
                Xs[i, c] += s * h
                Ep.append(bo.bonds(Xs, Q, body, anchor, k, l0, **kw)[1])
            g[i, c] = (Ep[0] - Ep[1]) / (2 * h)
            Ep = []
            for s in (1.0, -1.0):
                Qs = Q.copy()
                delta = np.zeros(3)
                delta[c] = s * h
                Qs[i] = mo.rotate(Q[i], delta)
                Ep.append(bo.bonds(X, Qs, body, anchor, k, l0, **kw)[1])
            g[i, 3 + c] = (Ep[0] - Ep[1]) / (2 * h)
    err = np.abs(FT + g).max() / np.abs(FT).max()
    print("largest entry %.3e, worst relative difference %.2e" % (np.abs(FT).max(), err))
    assert err <= 1e-7
    # the bonds between bodies alone exert no net force and no net torque
    bb = body[:, 1] >= 0
    FTb = bo.bonds(X, Q, body[bb], anchor[bb], k[bb], l0[bb], kind=kind[bb], table=table)[0]
    total_F = FTb[:, :3].sum(axis=0)
    total_T = (FTb[:, 3:] + np.cross(X, FTb[:, :3])).sum(axis=0)
    scale = np.abs(FTb).max() * max(1.0, np.abs(X).max())
    assert np.abs(total_F).max() <= 1e-13 * scale and np.abs(total_T).max() <= 1e-13 * scale


def coincident():
    """two bodies with identity orientations whose anchors name the same point in the same doubles (every coordinate a short
    binary fraction: the sums are exact), a harmonic and a tabulated bond between them and a tether of each kind to that point"""
    X = np.array([[0.5, 0.25, 1.0], [0.25, 0.5, 1.0]])
    Q = np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    sA, sB, P = [0.25, 0.5, 0.125], [0.5, 0.25, 0.125], [0.75, 0.75, 1.125]
    body = np.array([[0, 1], [1, 0], [0, -1], [1, -1]])
    anchor = np.array([sA + sB, sB + sA, sA + P, sB + P])
    kind = np.array([0, 1, 1, 0])
    k, l0 = np.array([2.0, 1.5, 0.5, 3.0]), np.array([0.75, 0.0, 0.0, 0.5])
    return X, Q, body, anchor, kind, k, l0


def test_oracle_a_bond_of_length_zero_exerts_no_force_and_has_the_energy_at_zero():
    X, Q, body, anchor, kind, k, l0 = coincident()
    table = morse_table()
    FT, E, (length, tension, energy) = bo.bonds(X, Q, body, anchor, k, l0, kind=kind, table=table)
    assert np.array_equal(length, np.zeros(4))
    assert np.array_equal(FT, np.zeros((2, 6)))
    U0 = table[0][0] + table[1][0] * (0.0 - table[2])          # the tangent at r_min continued to d = 0
    want = np.array([0.5 * 2.0 * 0.75 ** 2, 1.5 * U0, 0.5 * U0, 0.5 * 3.0 * 0.5 ** 2])
    assert np.allclose(energy, want, rtol=1e-15, atol=0.0) and np.isclose(E, want.sum(), rtol=1e-15)
    assert np.allclose(tension, [-2.0 * 0.75, 1.5 * table[1][0], 0.5 * table[1][0], -3.0 * 0.5], rtol=1e-15, atol=0.0)


# ------------------------------------------------------------------------------------------------------------ 2: the C ABI
def _active(lib, h):
    m = cint(-1)
    assert lib.rbl_interactions_active(h, ctypes.byref(m)) == 0
    return m.value


def _get_bonds(lib, h):
    n, ns, on = cint(-1), cint(-1), cint(-1)
    assert lib.rbl_get_bonds(h, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(on), None, None, None, None) == 0
    body, anchor = np.full((n.value, 2), -7, dtype=np.int32), np.zeros((n.value, 6))
    kind, param = np.full(n.value, -7, dtype=np.int32), np.zeros((max(ns.value, 0), n.value, 2))
    assert lib.rbl_get_bonds(h, None, None, None, body.ctypes.data, anchor.ctypes.data, kind.ctypes.data, param.ctypes.data) == 0
    return n.value, ns.value, on.value, body, anchor, kind, param


def _get_table(lib, h):
    n, lo, hi, on = cint(-1), dbl(-1), dbl(-1), cint(-1)
    assert lib.rbl_get_bond_table(h, ctypes.byref(n), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(on), None) == 0
    coef = np.zeros((max(n.value - 1, 0), 4))
    assert lib.rbl_get_bond_table(h, None, None, None, None, coef.ctypes.data) == 0
    return n.value, lo.value, hi.value, on.value, coef


def _set(lib, h, body, anchor, kind, param, n_sets=1, on=1, n=None):
    body = None if body is None else np.ascontiguousarray(body, dtype=np.int32)
    anchor = None if anchor is None else np.ascontiguousarray(anchor, dtype=np.float64)
    kind = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    param = None if param is None else np.ascontiguousarray(param, dtype=np.float64)
    if n is None:
        n = body.shape[0]
    return lib.rbl_set_bonds(h, n, None if body is None else body.ctypes.data, None if anchor is None else anchor.ctypes.data,
                             None if kind is None else kind.ctypes.data, None if param is None else param.ctypes.data, n_sets, on)


GOOD = dict(body=np.array([[0, 1], [2, -1], [3, 1]], dtype=np.int32), anchor=np.arange(18.0).reshape(3, 6) / 8.0,
            kind=np.array([0, 1, 0], dtype=np.int32), param=np.array([[[1.0, 0.5], [2.0, 0.0], [0.0, 1.5]]]))


def test_getters_round_trip_and_defaults():
    lib = _lib()
    h = lib.rbl_create()
    try:
        n, ns, on, *_ = _get_bonds(lib, h)
        assert (n, ns, on) == (0, 0, 0)
        assert _get_table(lib, h)[0] == 0
        assert _set(lib, h, **GOOD) == 0                        # before any rbl_set_config, a body index of 3 included
        n, ns, on, body, anchor, kind, param = _get_bonds(lib, h)
        assert (n, ns, on) == (3, 1, 1)
        assert np.array_equal(body, GOOD["body"]) and np.array_equal(anchor, GOOD["anchor"])
        assert np.array_equal(kind, GOOD["kind"]) and np.array_equal(param, GOOD["param"])
        two = np.concatenate([GOOD["param"], GOOD["param"] + 0.25])             # two sets, kind NULL (all harmonic), stored off
        assert _set(lib, h, GOOD["body"][:2], GOOD["anchor"][:2], None, two[:, :2], n_sets=2, on=0) == 0
        n, ns, on, body, anchor, kind, param = _get_bonds(lib, h)
        assert (n, ns, on) == (2, 2, 0) and np.array_equal(kind, [0, 0]) and np.array_equal(param, two[:, :2])
        assert np.array_equal(body, GOOD["body"][:2])
        U, dU = np.array([1.0, 0.5, 0.25]), np.array([-1.0, -0.5, 0.0])
        assert lib.rbl_set_bond_table(h, U.ctypes.data, dU.ctypes.data, 3, 0.5, 1.5, 1) == 0
        n, lo, hi, on, coef = _get_table(lib, h)
        assert (n, lo, hi, on) == (3, 0.5, 1.5, 1)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import table_oracle
        assert np.array_equal(coef, table_oracle.hermite_coef(U, dU, 0.5, 1.5))  # the pair table's coefficient layout
        assert lib.rbl_set_bond_table(h, None, None, 0, 0.0, 0.0, 0) == 0       # only the switch
        n, lo, hi, on, coef2 = _get_table(lib, h)
        assert (n, lo, hi, on) == (3, 0.5, 1.5, 0) and np.array_equal(coef2, coef)
    finally:
        lib.rbl_destroy(h)


def test_activity_bit_six():
    lib = _lib()
    h = lib.rbl_create()
    try:
        assert _active(lib, h) == 0
        assert _set(lib, h, **GOOD) == 0
        assert _active(lib, h) == 64
        assert _set(lib, h, on=0, **GOOD) == 0                   # stored, switched off
        assert _active(lib, h) == 0
        assert _set(lib, h, **GOOD) == 0
        assert _set(lib, h, None, None, None, None, n_sets=0, on=0, n=0) == 0   # only the switch: the stored bonds stay
        assert _active(lib, h) == 0
        assert _get_bonds(lib, h)[:3] == (3, 1, 0)
        U, dU = np.array([1.0, 0.0]), np.array([-1.0, 0.0])
        assert lib.rbl_set_bond_table(h, U.ctypes.data, dU.ctypes.data, 2, 0.5, 1.5, 1) == 0
        assert _active(lib, h) == 0                              # a bond table alone acts on nothing
        k, X0 = np.ones(3), np.zeros(3)
        assert lib.rbl_set_traps(h, k.ctypes.data, X0.ctypes.data, 1, 1) == 0
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, 2, 0.5, 1.5, 1) == 0
        assert _active(lib, h) == 10                             # bits 1 and 3 as before
        assert _set(lib, h, **GOOD) == 0
        assert _active(lib, h) == 74
    finally:
        lib.rbl_destroy(h)


def _refused(lib, h, rc, word):
    assert rc == RBL_ERR_ARG
    msg = lib.rbl_last_error(h).decode()
    assert word in msg, msg


def test_every_refusal_names_its_argument_and_keeps_the_previous_model():
    lib = _lib()
    h = lib.rbl_create()
    try:
        assert _set(lib, h, **GOOD) == 0
        U, dU = np.array([1.0, 0.5, 0.25]), np.array([-1.0, -0.5, 0.0])
        assert lib.rbl_set_bond_table(h, U.ctypes.data, dU.ctypes.data, 3, 0.5, 1.5, 1) == 0
        before = (_get_bonds(lib, h), _get_table(lib, h), _active(lib, h))
        assert before[2] == 64

        def same():
            now = (_get_bonds(lib, h), _get_table(lib, h), _active(lib, h))
            assert now[0][:3] == before[0][:3] and all(np.array_equal(x, y) for x, y in zip(now[0][3:], before[0][3:]))
            assert now[1][:4] == before[1][:4] and np.array_equal(now[1][4], before[1][4]) and now[2] == before[2]

        def bad(word, **change):
            args = dict(GOOD, **change)
            extra = {q: args.pop(q) for q in ("n_sets", "on", "n") if q in args}
            _refused(lib, h, _set(lib, h, **args, **extra), word)

        bad("body", body=None, n=3)                              # NULL where an array is needed with on != 0
        bad("anchor", anchor=None)
        bad("param", param=None)
        bad("n_bonds", n=0)
        bad("n_bonds", n=-2)
        bad("n_bonds", n=(1 << 24) + 1)
        bad("n_sets", n_sets=0)
        bad("n_sets", n_sets=-1)
        for row, word in (([-1, 1], "first"), ([-5, 1], "first"), ([0, -2], "second"), ([2, 2], "one body")):
            b = GOOD["body"].copy()
            b[1] = row
            bad(word, body=b)
            bad("bond 1", body=b)                                # ... and the bond is named
        for kd in (2, -1):
            kk = GOOD["kind"].copy()
            kk[2] = kd
            bad("kind", kind=kk)
        for v in (NAN, INF, -INF):
            a = GOOD["anchor"].copy()
            a[1, 4] = v
            bad("anchor", anchor=a)
            for q in (0, 1):
                p = GOOD["param"].copy()
                p[0, 2, q] = v
                bad("param", param=p)
        p = GOOD["param"].copy()
        p[0, 1, 0] = -1e-3
        bad("k must", param=p)
        p = GOOD["param"].copy()
        p[0, 0, 1] = -0.5
        bad("l0 must", param=p)
        p = np.concatenate([GOOD["param"], GOOD["param"]])      # the second set is checked too
        p[1, 2, 0] = -2.0
        bad("set 1", param=p, n_sets=2)
        same()
        # the bond table: the pair table's refusals
        for args, word in (((None, dU.ctypes.data, 3, 0.5, 1.5, 1), "U and dU"), ((U.ctypes.data, dU.ctypes.data, 1, 0.5, 1.5, 1), "n must"),
                           ((U.ctypes.data, dU.ctypes.data, 3, -0.1, 1.5, 1), "r_min"), ((U.ctypes.data, dU.ctypes.data, 3, 1.5, 1.5, 1), "r_min")):
            _refused(lib, h, lib.rbl_set_bond_table(h, *args), word)
            assert "set_bond_table" in lib.rbl_last_error(h).decode()
        Ub = U.copy()
        Ub[1] = NAN
        _refused(lib, h, lib.rbl_set_bond_table(h, Ub.ctypes.data, dU.ctypes.data, 3, 0.5, 1.5, 1), "finite")
        same()
        # what is NOT refused: k = 0, l0 = 0, a body index far beyond any system (found at evaluation)
        b = GOOD["body"].copy()
        b[0] = [2 ** 31 - 1, 0]
        assert _set(lib, h, body=b, anchor=GOOD["anchor"], kind=None, param=np.zeros((1, 3, 2))) == 0
    finally:
        lib.rbl_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 3: Python
def test_python_wrappers_check_shapes_before_the_library():
    from rigid_body_light_amd._lib import blob_anchor, bond_args
    b, anchor, kind, param = bond_args("set_bonds", [[0, 1], [1, -1]], [0.0, 0.0, 0.5], [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]], 2.0, [0.5, 0.0], None)
    assert b.dtype == np.int32 and b.shape == (2, 2) and kind is None
    assert np.array_equal(anchor, [[0.0, 0.0, 0.5, 0.1, 0.2, 0.3], [0.0, 0.0, 0.5, 1.0, 2.0, 3.0]])
    assert np.array_equal(param, [[[2.0, 0.5], [2.0, 0.0]]])
    b, anchor, kind, param = bond_args("set_bonds", [0, 1], np.zeros(3), np.zeros(3), [[1.0], [2.0], [3.0]], 0.25, [1], sets=(1, 3))
    assert param.shape == (3, 1, 2) and np.array_equal(param[:, 0, 0], [1.0, 2.0, 3.0]) and np.array_equal(param[:, 0, 1], [0.25] * 3)
    assert kind.dtype == np.int32
    ok = dict(body=[[0, 1], [1, -1]], anchor_a=np.zeros(3), anchor_b=np.zeros((2, 3)), k=1.0, l0=0.0, kind=None)
    for name, value in (("body", [[0, 1, 2]]), ("body", [[0.0, 1.0]]), ("body", np.zeros((0, 2), dtype=int)), ("anchor_a", np.zeros((3, 3))),
                        ("anchor_b", np.zeros(2)), ("k", np.ones(3)), ("l0", np.ones((2, 2, 2))), ("kind", [0]), ("kind", [0.0, 1.0])):
        with pytest.raises(ValueError, match=name):
            bond_args("set_bonds", **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="k must"):              # a set count an ensemble of 3 replicas cannot use
        bond_args("set_bonds", **dict(ok, k=np.ones((2, 2))), sets=(1, 3))
    cfg = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 6.0]])
    assert np.allclose(blob_anchor(cfg, 2), [-1.0 / 3.0, -2.0 / 3.0, 4.0], rtol=1e-15)
