"""The dipole terms of include/rbl.h section 4 without a GPU: the numpy oracle (tests/magnetic_oracle.py) against central
differences of its own energy, and the argument checks, getters and activity bits of rbl_set_dipoles, rbl_set_magnetic_field and
rbl_set_field_time (host-only: no device is touched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
    lib.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    lib.rbl_set_interactions.argtypes = [vp] + [dbl] * 6 + [cint]
    lib.rbl_get_interactions.argtypes = [vp, dp, ip]
    lib.rbl_set_pair_table.argtypes = [vp, vp, vp, cint, dbl, dbl, cint]
    lib.rbl_set_traps.argtypes = [vp, vp, vp, cint, cint]
    lib.rbl_interactions_active.argtypes = [vp, ip]
    lib.rbl_set_dipoles.argtypes = [vp, vp, cint, dbl, dbl, dbl, cint]
    lib.rbl_get_dipoles.argtypes = [vp, ip, dp, dp, dp, ip, vp]
    lib.rbl_set_magnetic_field.argtypes = [vp, vp, vp, vp, dbl, cint]
    lib.rbl_get_magnetic_field.argtypes = [vp, vp, dp, ip]
    lib.rbl_set_field_time.argtypes = [vp, vp, cint]
    lib.rbl_get_field_time.argtypes = [vp, ip, vp]
    return lib


def test_the_error_code_of_the_header_is_the_one_used_here():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    assert "RBL_ERR_ARG" in text
    import re
    m = re.search(r"RBL_ERR_ARG\s*=\s*(-?\d+)", text) or re.search(r"#define\s+RBL_ERR_ARG\s+(-?\d+)", text)
    assert m and int(m.group(1)) == RBL_ERR_ARG


# ------------------------------------------------------------------------------------------------------------ 1: the oracle
def _cluster():
    """five bodies: pairs below r_core, between r_core and r_cut and beyond r_cut, none within 1e-3 of either radius"""
    X = np.array([[0.0, 0.0, 2.0], [0.7, 0.1, 2.1], [2.1, -0.3, 2.4], [0.2, 1.9, 1.7], [4.6, 0.4, 2.2]])
    rng = np.random.default_rng(8)
    Q = rng.standard_normal((5, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    m_body = rng.standard_normal((5, 3))
    return X, Q, m_body


def _regimes(X, r_core, r_cut):
    d = mo.pair_distances(X)
    assert (d < r_core).any() and ((d > r_core) & (d < r_cut)).any() and (d > r_cut).any()
    assert np.abs(d - r_core).min() > 1e-3 and np.abs(d - r_cut).min() > 1e-3
    return d


@pytest.mark.parametrize("with_field", [False, True])
def test_oracle_forces_and_torques_are_minus_the_gradient_of_its_energy(with_field):
    X, Q, m_body = _cluster()
    c_dd, r_core, r_cut = 1.7, 1.0, 3.0
    _regimes(X, r_core, r_cut)
    B = mo.field([0.3, -0.2, 0.5], [1.0, 0.0, 0.4], [0.0, 0.8, -0.1], 2.1, 3.4762) if with_field else None
    kw = dict(c_dd=c_dd, r_core=r_core, r_cut=r_cut, B=B)
    FT, E = mo.dipoles(X, Q, m_body, **kw)
    h = 1e-6
    g = np.zeros((5, 6))
    for i in range(5):
        for c in range(3):
            Ep = []
            for s in (1.0, -1.0):
                Xs = X.copy()
                Xs[i, c] += s * h
                Ep.append(mo.dipoles(Xs, Q, m_body, **kw)[1])
            g[i, c] = (Ep[0] - Ep[1]) / (2 * h)
            Ep = []
            for s in (1.0, -1.0):
                Qs = Q.copy()
                delta = np.zeros(3)
                delta[c] = s * h
                Qs[i] = mo.rotate(Q[i], delta)
                Ep.append(mo.dipoles(X, Qs, m_body, **kw)[1])
            g[i, 3 + c] = (Ep[0] - Ep[1]) / (2 * h)
    err = np.abs(FT + g).max() / np.abs(FT).max()
    print("largest entry %.3e, worst relative difference %.2e" % (np.abs(FT).max(), err))
    assert err <= 1e-7
    if not with_field:                                          # the pair term alone: no net force, no net torque
        total_F = FT[:, :3].sum(axis=0)
        total_T = (FT[:, 3:] + np.cross(X, FT[:, :3])).sum(axis=0)
        scale = np.abs(FT).max() * max(1.0, np.abs(X).max())
        assert np.abs(total_F).max() <= 1e-13 * scale and np.abs(total_T).max() <= 1e-13 * scale


def test_oracle_coincident_centres_exert_no_force_and_the_field_exerts_none():
    X = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    Q = np.array([[1.0, 0.0, 0.0, 0.0], [0.7, 0.1, -0.5, 0.5]])
    FT, E = mo.dipoles(X, Q, [0.2, 1.0, -0.4], c_dd=2.0, r_core=0.5, r_cut=np.inf)
    assert np.array_equal(FT[:, :3], np.zeros((2, 3))) and np.isfinite(FT).all() and np.abs(FT[:, 3:]).max() > 0.0
    FT, E = mo.dipoles(X[:1], Q[:1], [0.2, 1.0, -0.4], B=[0.0, 0.0, 2.0])
    m = mo.lab_moments(Q[:1], [0.2, 1.0, -0.4])[0]
    assert np.array_equal(FT[0, :3], np.zeros(3)) and np.allclose(FT[0, 3:], np.cross(m, [0.0, 0.0, 2.0])) and np.isclose(E, -2.0 * m[2])


# ------------------------------------------------------------------------------------------------------------ 2: the C ABI
def _active(lib, h):
    m = cint(-1)
    assert lib.rbl_interactions_active(h, ctypes.byref(m)) == 0
    return m.value


def _get_dipoles(lib, h):
    n, on, c, rc, ru = cint(-1), cint(-1), dbl(-1), dbl(-1), dbl(-1)
    assert lib.rbl_get_dipoles(h, ctypes.byref(n), ctypes.byref(c), ctypes.byref(rc), ctypes.byref(ru), ctypes.byref(on), None) == 0
    m = np.zeros((max(n.value, 0), 3))
    assert lib.rbl_get_dipoles(h, None, None, None, None, None, m.ctypes.data) == 0
    return n.value, c.value, rc.value, ru.value, on.value, m


def _get_field(lib, h):
    B, om, on = np.zeros(9), dbl(-1), cint(-1)
    assert lib.rbl_get_magnetic_field(h, B.ctypes.data, ctypes.byref(om), ctypes.byref(on)) == 0
    return B, om.value, on.value


def _get_time(lib, h):
    n = cint(-1)
    assert lib.rbl_get_field_time(h, ctypes.byref(n), None) == 0
    t = np.zeros(n.value)
    assert lib.rbl_get_field_time(h, None, t.ctypes.data) == 0
    return t


def test_getters_round_trip_and_defaults():
    lib = _lib()
    h = lib.rbl_create()
    try:
        n, c, rc, ru, on, m = _get_dipoles(lib, h)
        assert (n, c, on) == (0, 0.0, 0)
        assert np.array_equal(_get_time(lib, h), [0.0])            # the default: one shared entry, t = 0
        assert _get_field(lib, h)[2] == 0
        mb = np.random.default_rng(1).standard_normal((4, 3))
        assert lib.rbl_set_dipoles(h, mb.ctypes.data, 4, 1.5, 0.8, 3.5, 1) == 0
        n, c, rc, ru, on, m = _get_dipoles(lib, h)
        assert (n, c, rc, ru, on) == (4, 1.5, 0.8, 3.5, 1) and np.array_equal(m, mb)
        assert lib.rbl_set_dipoles(h, mb.ctypes.data, 1, 0.25, 0.5, INF, 0) == 0       # +inf is a cutoff; on = 0 stores, switched off
        n, c, rc, ru, on, m = _get_dipoles(lib, h)
        assert (n, c, rc, ru, on) == (1, 0.25, 0.5, INF, 0) and np.array_equal(m, mb[:1])
        B = np.arange(9.0) - 3.5
        assert lib.rbl_set_magnetic_field(h, B[0:3].ctypes.data, B[3:6].ctypes.data, B[6:9].ctypes.data, -2.5, 1) == 0
        Bg, om, on = _get_field(lib, h)
        assert np.array_equal(Bg, B) and (om, on) == (-2.5, 1)
        t = np.array([0.37, -1.0, 12.5])
        assert lib.rbl_set_field_time(h, t.ctypes.data, 3) == 0
        assert np.array_equal(_get_time(lib, h), t)
        assert lib.rbl_set_field_time(h, t.ctypes.data, 1) == 0
        assert np.array_equal(_get_time(lib, h), t[:1])
    finally:
        lib.rbl_destroy(h)


def test_activity_bits_four_and_five():
    lib = _lib()
    h = lib.rbl_create()
    try:
        z, one = np.zeros(3), np.array([0.0, 0.0, 1.0])
        assert _active(lib, h) == 0
        assert lib.rbl_set_magnetic_field(h, one.ctypes.data, z.ctypes.data, z.ctypes.data, 0.0, 1) == 0
        assert _active(lib, h) == 0                                 # a field without moments acts on nothing
        assert lib.rbl_set_dipoles(h, one.ctypes.data, 1, 0.0, 0.0, 0.0, 1) == 0
        assert _active(lib, h) == 32                                # moments and field: the torque; c_dd = 0: no pairs
        assert lib.rbl_set_dipoles(h, one.ctypes.data, 1, 2.0, 0.5, INF, 1) == 0
        assert _active(lib, h) == 48
        assert lib.rbl_set_magnetic_field(h, None, None, None, 0.0, 0) == 0           # only the switch
        assert _active(lib, h) == 16
        assert np.array_equal(_get_field(lib, h)[0][:3], one)       # ... the stored field stays
        assert lib.rbl_set_dipoles(h, None, 0, 0.0, 0.0, 0.0, 0) == 0                  # only the switch
        assert _active(lib, h) == 0
        n, c, rc, ru, on, m = _get_dipoles(lib, h)
        assert (n, c, rc, ru, on) == (1, 2.0, 0.5, INF, 0)
        # bits 0 - 3 as before, beside the new ones
        k, X0 = np.ones(3), np.zeros(3)
        assert lib.rbl_set_traps(h, k.ctypes.data, X0.ctypes.data, 1, 1) == 0
        assert _active(lib, h) == 8
        U, dU = np.array([1.0, 0.0]), np.array([-1.0, 0.0])
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, 2, 0.5, 1.5, 1) == 0
        assert _active(lib, h) == 10
        assert lib.rbl_set_dipoles(h, one.ctypes.data, 1, 2.0, 0.5, INF, 1) == 0
        assert lib.rbl_set_magnetic_field(h, one.ctypes.data, z.ctypes.data, z.ctypes.data, 0.0, 1) == 0
        assert _active(lib, h) == 58
        p6, on = (dbl * 6)(), cint(-1)
        assert lib.rbl_get_interactions(h, p6, ctypes.byref(on)) == 0 and on.value == 0   # the built-in term only, as before
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
        mb = np.array([[0.1, 0.2, 0.3], [-1.0, 0.5, 0.0]])
        B = np.array([0.5, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 2.0])
        t0 = np.array([0.25, 0.75])
        assert lib.rbl_set_dipoles(h, mb.ctypes.data, 2, 1.5, 0.8, 3.5, 1) == 0
        assert lib.rbl_set_magnetic_field(h, B[0:3].ctypes.data, B[3:6].ctypes.data, B[6:9].ctypes.data, 1.25, 1) == 0
        assert lib.rbl_set_field_time(h, t0.ctypes.data, 2) == 0
        before = (_get_dipoles(lib, h), _get_field(lib, h), _get_time(lib, h), _active(lib, h))
        assert before[3] == 48

        def same():
            now = (_get_dipoles(lib, h), _get_field(lib, h), _get_time(lib, h), _active(lib, h))
            assert now[0][:5] == before[0][:5] and np.array_equal(now[0][5], before[0][5])
            assert np.array_equal(now[1][0], before[1][0]) and now[1][1:] == before[1][1:]
            assert np.array_equal(now[2], before[2]) and now[3] == before[3]

        good = np.ones((2, 3))
        _refused(lib, h, lib.rbl_set_dipoles(h, None, 2, 1.0, 0.5, 2.0, 1), "m_body")
        for bad in (NAN, INF, -INF):
            m = good.copy()
            m[1, 2] = bad
            _refused(lib, h, lib.rbl_set_dipoles(h, m.ctypes.data, 2, 1.0, 0.5, 2.0, 1), "m_body")
        _refused(lib, h, lib.rbl_set_dipoles(h, good.ctypes.data, 0, 1.0, 0.5, 2.0, 1), "n_bodies")
        _refused(lib, h, lib.rbl_set_dipoles(h, good.ctypes.data, -3, 1.0, 0.5, 2.0, 1), "n_bodies")
        for c_dd in (-1e-3, NAN, INF):
            _refused(lib, h, lib.rbl_set_dipoles(h, good.ctypes.data, 2, c_dd, 0.5, 2.0, 1), "c_dd")
        for r_core in (0.0, -0.5, NAN, INF):
            _refused(lib, h, lib.rbl_set_dipoles(h, good.ctypes.data, 2, 1.0, r_core, 2.0, 1), "r_core")
        for r_cut in (0.5, 0.25, NAN, -INF):
            _refused(lib, h, lib.rbl_set_dipoles(h, good.ctypes.data, 2, 1.0, 0.5, r_cut, 1), "r_cut")
        same()
        z = np.zeros(3)
        _refused(lib, h, lib.rbl_set_magnetic_field(h, None, z.ctypes.data, z.ctypes.data, 0.0, 1), "B0")
        _refused(lib, h, lib.rbl_set_magnetic_field(h, z.ctypes.data, None, z.ctypes.data, 0.0, 1), "B1")
        _refused(lib, h, lib.rbl_set_magnetic_field(h, z.ctypes.data, z.ctypes.data, None, 0.0, 1), "B2")
        for k, name in enumerate(("B0", "B1", "B2")):
            for bad in (NAN, INF):
                v = [np.zeros(3), np.zeros(3), np.zeros(3)]
                v[k][1] = bad
                _refused(lib, h, lib.rbl_set_magnetic_field(h, v[0].ctypes.data, v[1].ctypes.data, v[2].ctypes.data, 0.0, 1), name)
        for bad in (NAN, INF, -INF):
            _refused(lib, h, lib.rbl_set_magnetic_field(h, z.ctypes.data, z.ctypes.data, z.ctypes.data, bad, 1), "omega")
        same()
        t = np.array([0.1, 0.2])
        _refused(lib, h, lib.rbl_set_field_time(h, None, 1), "set_field_time: t ")
        _refused(lib, h, lib.rbl_set_field_time(h, t.ctypes.data, 0), "set_field_time: n ")
        _refused(lib, h, lib.rbl_set_field_time(h, t.ctypes.data, -1), "set_field_time: n ")
        for bad in (NAN, INF, -INF):
            tb = t.copy()
            tb[1] = bad
            _refused(lib, h, lib.rbl_set_field_time(h, tb.ctypes.data, 2), "set_field_time: every value of t ")
        same()
        # what is NOT refused: c_dd = 0 needs no radii; r_cut = +inf
        assert lib.rbl_set_dipoles(h, good.ctypes.data, 2, 0.0, 0.0, 0.0, 1) == 0
        assert lib.rbl_set_dipoles(h, good.ctypes.data, 2, 1.0, 0.5, INF, 1) == 0
    finally:
        lib.rbl_destroy(h)


def test_python_wrappers_check_shapes_before_the_library():
    from rigid_body_light_amd._lib import dipole_args, field_args
    m, rc = dipole_args("set_dipoles", [0.0, 0.0, 1.0], 0.0, None)
    assert m.shape == (1, 3) and rc == 0.0
    with pytest.raises(ValueError, match="r_core"):
        dipole_args("set_dipoles", [0.0, 0.0, 1.0], 1.0, None)
    with pytest.raises(ValueError, match="m_body"):
        dipole_args("set_dipoles", np.zeros((2, 4)), 0.0, None)
    B0, B1, B2 = field_args("set_magnetic_field", [1.0, 0.0, 0.0], None, None)
    assert np.array_equal(B1, np.zeros(3)) and np.array_equal(B2, np.zeros(3))
    with pytest.raises(ValueError, match="B1"):
        field_args("set_magnetic_field", None, [1.0, 2.0], None)
