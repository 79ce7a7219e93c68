"""The tabulated terms and the traps of include/rbl.h section 4 without a GPU: the Hermite coefficients rbl_set_pair_table builds
against the numpy construction (tests/table_oracle.py), the numpy oracle against its own energy, and the argument checks of the
new entry points (host-only: no device is touched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import table_oracle  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = vp
    lib.rbl_destroy.argtypes = [vp]
    lib.rbl_last_error.restype = ctypes.c_char_p
    lib.rbl_last_error.argtypes = [vp]
    lib.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    lib.rbl_set_interactions.argtypes = [vp] + [dbl] * 6 + [cint]
    lib.rbl_get_interactions.argtypes = [vp, dp, ip]
    for name in ("pair", "height"):
        getattr(lib, "rbl_set_%s_table" % name).argtypes = [vp, vp, vp, cint, dbl, dbl, cint]
        getattr(lib, "rbl_get_%s_table" % name).argtypes = [vp, ip, dp, dp, ip, vp]
    lib.rbl_set_traps.argtypes = [vp, vp, vp, cint, cint]
    lib.rbl_get_traps.argtypes = [vp, ip, ip, vp, vp]
    lib.rbl_interactions_active.argtypes = [vp, ip]
    return lib


def _get_table(lib, h, which="pair"):
    n, lo, hi, on = cint(-1), dbl(0), dbl(0), cint(-1)
    get = getattr(lib, "rbl_get_%s_table" % which)
    assert get(h, ctypes.byref(n), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(on), None) == 0
    coef = np.zeros((max(n.value - 1, 0), 4))
    assert get(h, None, None, None, None, coef.ctypes.data) == 0
    return n.value, lo.value, hi.value, on.value, coef


def _active(lib, h):
    m = cint(-1)
    assert lib.rbl_interactions_active(h, ctypes.byref(m)) == 0
    return m.value


def _lj(r, eps=1.3, sig=0.5):
    s6 = (sig / r) ** 6
    return 4 * eps * (s6 * s6 - s6), -24 * eps * (2 * s6 * s6 - s6) / r


@pytest.mark.parametrize("n", [2, 3, 1025])
def test_coefficients_equal_the_numpy_construction(n):
    lib = _lib()
    h = lib.rbl_create()
    try:
        r_min, r_cut = 0.45, 1.6
        r = np.linspace(r_min, r_cut, n)
        U, dU = _lj(r)
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, n, r_min, r_cut, 1) == 0
        n_, lo, hi, on, coef = _get_table(lib, h)
        assert (n_, lo, hi, on) == (n, r_min, r_cut, 1)
        ref = table_oracle.hermite_coef(U, dU, r_min, r_cut)
        assert coef.shape == ref.shape == (n - 1, 4)
        assert np.abs(coef - ref).max() <= 1e-15 * np.abs(U).max()
        # what the coefficients mean: the interpolant and its derivative reproduce the nodes
        hh = (r_cut - r_min) / (n - 1)
        assert np.array_equal(coef[:, 0], U[:-1])
        assert np.abs(coef.sum(axis=1) - U[1:]).max() <= 1e-13 * np.abs(U).max()
        assert np.abs((coef[:, 1] + 2 * coef[:, 2] + 3 * coef[:, 3]) / hh - dU[1:]).max() <= 1e-12 * np.abs(dU).max()
        # the height table is the same construction
        assert lib.rbl_set_height_table(h, U.ctypes.data, dU.ctypes.data, n, -0.3, 0.9, 0) == 0
        n_, lo, hi, on, coef_h = _get_table(lib, h, "height")
        assert (n_, lo, hi, on) == (n, -0.3, 0.9, 0)
        assert np.abs(coef_h - table_oracle.hermite_coef(U, dU, -0.3, 0.9)).max() <= 1e-15 * np.abs(U).max()
    finally:
        lib.rbl_destroy(h)


def _packed():
    """three 12-blob bodies: blobs of different bodies closer than r_min, between r_min and r_cut and beyond r_cut, blobs below
    h_min and above h_cut"""
    nb, nblb = 3, 12
    X = np.array([[0.0, 0.0, 0.75], [0.9, 0.1, 0.8], [0.3, 0.8, 0.85]])
    rng = np.random.default_rng(4)
    cfg = rng.standard_normal((nblb, 3)) * 0.35
    cfg -= cfg.mean(axis=0)
    r = np.concatenate([X[b] + cfg @ np.linalg.qr(rng.standard_normal((3, 3)))[0] for b in range(nb)])
    return r, X, nblb


def test_oracle_forces_are_minus_the_gradient_of_its_energy():
    r, X, nblb = _packed()
    a = 0.2
    d = np.linalg.norm(r[:, None, :] - r[None, :, :], axis=2)
    body = np.arange(r.shape[0]) // nblb
    other = d[body[:, None] != body[None, :]]
    r_min, r_cut, h_min, h_cut = 0.45, 1.4, 0.5, 1.1
    assert (other < r_min).any() and ((other > r_min) & (other < r_cut)).any() and (other > r_cut).any()
    assert (r[:, 2] < h_min).any() and (r[:, 2] > h_cut).any() and ((r[:, 2] > h_min) & (r[:, 2] < h_cut)).any()
    # shifted tables (U = 0 at the cutoff): a central difference may straddle the cutoff of a pair
    x = np.linspace(r_min, r_cut, 257)
    U, dU = _lj(x)
    pair = (U - U[-1], dU, r_min, r_cut)
    z = np.linspace(h_min, h_cut, 65)
    height = (2.0 * (np.exp(-(z - h_min) / 0.2) - np.exp(-(h_cut - h_min) / 0.2)), -10.0 * np.exp(-(z - h_min) / 0.2), h_min, h_cut)
    builtin = dict(w=0.7, eps_wall=1.3, b_wall=0.15, eps_blob=0.9, b_blob=0.1, r_cut=2 * a + 8 * 0.1)
    traps = (np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 3.0], [0.0, 0.0, 0.0]]), X + 0.1)
    kw = dict(builtin=builtin, pair=pair, height=height, traps=traps)
    f, FT, E, npairs = table_oracle.interactions(r, X, nblb, a, True, **kw)
    assert npairs > 0
    eps = 1e-6
    g = np.zeros_like(r)
    for i in range(r.shape[0]):
        for k in range(3):
            rp, rm = r.copy(), r.copy()
            rp[i, k] += eps
            rm[i, k] -= eps
            g[i, k] = (table_oracle.interactions(rp, X, nblb, a, True, **kw)[2] -
                       table_oracle.interactions(rm, X, nblb, a, True, **kw)[2]) / (2 * eps)
    assert np.abs(f + g).max() <= 1e-7 * np.abs(f).max()
    # the traps: minus the gradient in the body centres, in the body force only
    Xp, Xm = X.copy(), X.copy()
    Xp[1, 2] += eps
    Xm[1, 2] -= eps
    gX = (table_oracle.interactions(r, Xp, nblb, a, True, **kw)[2] - table_oracle.interactions(r, Xm, nblb, a, True, **kw)[2]) / (2 * eps)
    assert abs(gX - 3.0 * (X[1, 2] - traps[1][1, 2])) <= 1e-7 * np.abs(FT).max()      # the bound of the blob forces, on the body forces
    FT0 = table_oracle.interactions(r, X, nblb, a, True, builtin=builtin, pair=pair, height=height)[1]
    dFT = (FT - FT0).reshape(3, 6)
    assert np.allclose(dFT[:, :3], -traps[0] * (X - traps[1]), rtol=0, atol=8 * np.finfo(float).eps * np.abs(FT).max()) and np.array_equal(dFT[:, 3:], np.zeros((3, 3)))
    # the built-in terms agree with the compiled restatement the existing tests use
    import interaction_oracle
    fb, FTb, Eb = interaction_oracle.interactions(r, X, nblb, a, True, **builtin)
    fn, FTn, En, _ = table_oracle.interactions(r, X, nblb, a, True, builtin=builtin)
    assert np.abs(fb - fn).max() <= 1e-12 * np.abs(fb).max() and abs(Eb - En) <= 1e-12 * abs(Eb)
    assert np.abs(FTb - FTn).max() <= 1e-12 * np.abs(FTb).max()


def test_table_and_trap_setters_validate_and_keep_what_was_there():
    lib = _lib()
    h = lib.rbl_create()
    try:
        assert _active(lib, h) == 0
        n = 9
        r = np.linspace(0.4, 1.5, n)
        U, dU = _lj(r)
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, n, 0.4, 1.5, 1) == 0      # no rbl_set_parameters needed
        good = _get_table(lib, h)
        assert _active(lib, h) == 2
        nan, inf = float("nan"), float("inf")
        Unan, Uinf, dUnan = U.copy(), U.copy(), dU.copy()
        Unan[3], Uinf[0], dUnan[n - 1] = nan, inf, nan
        bad = [
            (U, dU, 1, 0.4, 1.5), (U, dU, 0, 0.4, 1.5), (U, dU, -3, 0.4, 1.5), (np.zeros(4), np.zeros(4), 65538, 0.4, 1.5),   # n
            (U, dU, n, 1.5, 1.5), (U, dU, n, 1.6, 1.5),                                                                 # r_min >= r_cut
            (Unan, dU, n, 0.4, 1.5), (Uinf, dU, n, 0.4, 1.5), (U, dUnan, n, 0.4, 1.5),                                  # a NaN in U ...
            (U, dU, n, -0.1, 1.5),                                                                                      # negative r_min
            (U, dU, n, nan, 1.5), (U, dU, n, 0.4, inf), (U, dU, n, 0.4, nan),
        ]
        for Ub, dUb, nb_, lo, hi in bad:
            for on in (0, 1):
                assert lib.rbl_set_pair_table(h, Ub.ctypes.data, dUb.ctypes.data, nb_, lo, hi, on) == 11, (nb_, lo, hi)   # RBL_ERR_ARG
                assert lib.rbl_last_error(h).startswith(b"set_pair_table")
                now = _get_table(lib, h)
                assert now[:4] == good[:4] and np.array_equal(now[4], good[4])                 # the previous table, unchanged
                assert _active(lib, h) == 2
        assert lib.rbl_set_pair_table(h, None, dU.ctypes.data, n, 0.4, 1.5, 1) == 11
        assert lib.rbl_set_pair_table(h, None, None, n, 0.4, 1.5, 1) == 11
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, n, 0.0, 1.5, 1) == 0          # r_min = 0: allowed
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, n, 0.4, 1.5, 1) == 0
        # the height table: h_min may be negative, everything else as the pair table
        assert lib.rbl_set_height_table(h, U.ctypes.data, dU.ctypes.data, n, -0.5, 0.5, 1) == 0
        assert _active(lib, h) == 6
        for args in [(U, dU, 1, 0.0, 1.0), (U, dU, n, 1.0, 1.0), (Unan, dU, n, 0.0, 1.0), (U, dU, n, 0.0, inf)]:
            assert lib.rbl_set_height_table(h, args[0].ctypes.data, args[1].ctypes.data, *args[2:], 1) == 11
            assert lib.rbl_last_error(h).startswith(b"set_height_table")
            assert _get_table(lib, h, "height")[:4] == (n, -0.5, 0.5, 1)
        # traps
        k = np.array([[1.0, 0.0, 2.0], [0.5, 0.5, 0.5]])
        X0 = np.array([[0.1, 0.2, 0.3], [1.0, 1.1, 1.2]])
        assert lib.rbl_set_traps(h, k.ctypes.data, X0.ctypes.data, 2, 1) == 0
        assert _active(lib, h) == 14

        def traps():
            nb_, on = cint(-1), cint(-1)
            ko, Xo = np.zeros((2, 3)), np.zeros((2, 3))
            assert lib.rbl_get_traps(h, ctypes.byref(nb_), ctypes.byref(on), ko.ctypes.data, Xo.ctypes.data) == 0
            return nb_.value, on.value, ko, Xo

        knan, Xinf = k.copy(), X0.copy()
        knan[1, 1], Xinf[0, 0] = nan, inf
        for kb, Xb, nb_ in [(k, X0, 0), (k, X0, -1), (knan, X0, 2), (k, Xinf, 2)]:
            assert lib.rbl_set_traps(h, kb.ctypes.data, Xb.ctypes.data, nb_, 1) == 11
            assert lib.rbl_last_error(h).startswith(b"set_traps")
            t = traps()
            assert t[:2] == (2, 1) and np.array_equal(t[2], k) and np.array_equal(t[3], X0)
        assert lib.rbl_set_traps(h, None, X0.ctypes.data, 2, 1) == 11
        # the built-in term keeps its own switch and its own report
        a = 0.25
        cfg = np.ascontiguousarray(np.random.default_rng(0).standard_normal((12, 3)))
        assert lib.rbl_set_parameters(h, a, 0.01, 1.0, 1.0, cfg.ctypes.data, 12) == 0
        on = cint(-1)
        assert lib.rbl_get_interactions(h, None, ctypes.byref(on)) == 0 and on.value == 0    # the tables do not show here
        assert lib.rbl_set_interactions(h, 0.5, 2.0, 0.1, 1.0, 0.05, 2 * a + 1.0, 1) == 0
        assert _active(lib, h) == 15
        # off: with the arrays (stored, off) or without them (only the switch)
        assert lib.rbl_set_pair_table(h, U.ctypes.data, dU.ctypes.data, n, 0.4, 1.5, 0) == 0 and _active(lib, h) == 13
        assert lib.rbl_set_height_table(h, None, None, 0, 0.0, 0.0, 0) == 0 and _active(lib, h) == 9
        assert _get_table(lib, h, "height")[:4] == (n, -0.5, 0.5, 0)
        assert lib.rbl_set_traps(h, None, None, 0, 0) == 0 and _active(lib, h) == 1
        assert traps()[0] == 2
        assert lib.rbl_set_interactions(h, 0.5, 2.0, 0.1, 1.0, 0.05, 2 * a + 1.0, 0) == 0 and _active(lib, h) == 0
        assert lib.rbl_interactions_active(h, None) == 11
    finally:
        lib.rbl_destroy(h)


def test_tabulate_returns_the_grid_values():
    from rigid_body_light_amd import tabulate
    U, dU = tabulate(lambda r: _lj(r)[0], lambda r: _lj(r)[1], 0.4, 1.5, 17)
    r = np.linspace(0.4, 1.5, 17)
    assert np.array_equal(U, _lj(r)[0]) and np.array_equal(dU, _lj(r)[1])
    U, dU = tabulate(lambda r: 2.0, lambda r: 0.0 * r, 0.0, 1.0, 5)            # a constant comes back as an array
    assert U.shape == dU.shape == (5,) and np.array_equal(U, np.full(5, 2.0))
