"""The periodic cell of include/rbl.h section 10 without a GPU: the properties of the truncated image sum M_per that the section
quotes (tests/periodic_oracle.py, the CPU oracle's pair block: symmetry, positivity for n >= 1, the indefinite n = 0 matrix, the
slow convergence in n), every host refusal of rbl_set_periodic with the value named, the set / get round trip and the checks of the
Python wrappers.  No device is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_oracle as po  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)
ERR_STATE, ERR_ARG = 7, 11
INF, NAN = float("inf"), float("nan")
ETA = 1.0


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    L.rbl_set_config.argtypes = [vp, vp, vp, cint]
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    L.rbl_set_periodic.argtypes = [vp, dbl, dbl, cint, cint, cint]
    L.rbl_get_periodic.argtypes = [vp, dp, dp, ip, ip, ip]
    return L


def test_the_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in ("rbl_set_periodic", "rbl_get_periodic"):
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    assert "10. Periodic cell" in text
    for said in ("pseudo-periodic", "observed, not proven", "UNWRAPPED", "Ewald", "free-space", "minimum-image"):   # scope and caveats are written down
        assert said in text, said


# ------------------------------------------------------------------------------------------------------------ 1: the operator
CELL = (7.0, 7.5)


@pytest.fixture(scope="module")
def layer(orc):
    """make_config(4, 12, wall) in a cell of 7.0 x 7.5: the image terms up to n = 4, every pair evaluated once"""
    from oracle import oracle as O
    from rigid_body_light_amd.synth import make_config
    c = make_config(4, 12, True)
    cfg = O.remove_mean(c["cfg"])
    r = orc.multi_body_pos(c["X"], O.normalize_quats(c["Q"]), cfg)
    T = po.image_terms(orc, r, c["a"], ETA, CELL, (4, 4))
    B = orc.damp(r, c["a"])
    M_open = orc.rotne_prager_tensor(r, c["a"], ETA, True)
    return dict(r=r, a=c["a"], T=T, B=B, M_open=B[:, None] * M_open * B[None, :])


def test_M_per_is_symmetric_and_positive_definite_for_n_of_1_to_4_and_indefinite_at_0(layer):
    """the figures of include/rbl.h section 10: symmetric to rounding for every n; the smallest eigenvalue of the damped matrix is
    negative with the nearest image alone and positive, rising towards the open system's, for n = 1 ... 4.  Positivity is OBSERVED
    here, not proven: only its sign is asserted"""
    lam_open = np.linalg.eigvalsh(layer["M_open"]).min()
    print("open system: smallest eigenvalue %.5f" % lam_open)
    lam = []
    for n in range(5):
        M = po.truncated(layer["T"], (n, n), layer["B"])
        asym = np.abs(M - M.T).max()
        lam.append(np.linalg.eigvalsh(0.5 * (M + M.T)).min())
        print("n = %d: asymmetry %.1e, smallest eigenvalue %.5f" % (n, asym, lam[-1]))
        assert asym <= 1e-15 * np.abs(M).max()
    assert lam[0] < 0.0, "the nearest image alone was expected to be indefinite: the reason a periodic axis takes n >= 1"
    assert all(x > 0.0 for x in lam[1:])
    assert lam_open > 0.0


def test_the_change_of_U_from_one_image_count_to_the_next_decreases(layer):
    """the r^-3 tail in two dimensions: the remainder of the truncated sum falls like 1 / n, slowly but monotonically"""
    F = np.random.default_rng(5).standard_normal(layer["r"].size)
    U = [po.truncated(layer["T"], (n, n), layer["B"]) @ F for n in range(5)]
    change = [np.linalg.norm(U[n] - U[n - 1]) / np.linalg.norm(U[n]) for n in range(1, 5)]
    print("relative change of U from n - 1 to n, n = 1 ... 4: " + " ".join("%.3f" % c for c in change))
    assert all(change[k + 1] < change[k] for k in range(3))
    assert change[-1] < 0.05                                  # 0.006 in the header; anything near 1 would mean a diverging sum


def test_oracle_forms_agree_with_each_other(orc, layer):
    """the dense form and rows() are two walks over one definition; an open axis leaves its coordinate alone"""
    r, a = layer["r"].reshape(-1, 3)[:9], layer["a"]
    M = po.dense_M(orc, r, a, ETA, CELL, (2, 1))
    which = [0, 4, 8]
    R = po.rows(orc, r, which, a, ETA, CELL, (2, 1))
    idx = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in which])
    assert np.abs(R - M[idx]).max() <= 1e-16
    assert np.array_equal(po.nearest([5.0, -5.0, 1.0], (7.0, 0.0)), [-2.0, -5.0, 1.0])
    assert np.array_equal(po.nearest([3.5, 10.5, 1.0], (7.0, 7.0)), [3.5, -3.5, 1.0])      # round half to even, an odd function
    assert np.array_equal(po.nearest([-3.5, -10.5, 1.0], (7.0, 7.0)), [-3.5, 3.5, 1.0])


def test_M_per_is_positive_definite_where_the_gpu_tests_take_roots(orc):
    """10 x shell_N_12 in three lattice spacings by three plus 0.7 with (1, 1) images: the configuration of the GPU tests' Lanczos
    root and Brownian steps.  The smallest eigenvalue is recorded; only its sign is asserted"""
    import periodic_cases as pc
    c = pc.layer10()
    M = po.dense_M(orc, c["r"], c["a"], ETA, c["L"], (1, 1))
    lam = np.linalg.eigvalsh(0.5 * (M + M.T)).min()
    print("10 x shell_N_12, cell %.3f x %.3f, images (1, 1): smallest eigenvalue %.5f" % (c["L"][0], c["L"][1], lam))
    assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
    assert lam > 0.0


# ------------------------------------------------------------------------------------------------------------ 2: the C ABI
def _get(L, h):
    Lx, Ly, nx, ny, on = dbl(-1.0), dbl(-1.0), cint(-1), cint(-1), cint(-1)
    assert L.rbl_get_periodic(h, ctypes.byref(Lx), ctypes.byref(Ly), ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(on)) == 0
    return Lx.value, Ly.value, nx.value, ny.value, on.value


def _context(L, a=0.25):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5
    assert L.rbl_set_parameters(h, a, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    return h


def test_set_get_round_trip_and_the_switch():
    L = _lib()
    h = L.rbl_create()
    try:
        assert _get(L, h) == (0.0, 0.0, 0, 0, 0)                  # never set
        assert L.rbl_get_periodic(h, None, None, None, None, None) == 0
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0      # before any rbl_set_parameters
        assert _get(L, h) == (7.0, 7.5, 2, 3, 1)
        assert L.rbl_set_periodic(h, 9.0, 0.0, 1, 5, 0) == 0      # stored switched off; n of the open axis is ignored, stored as 0
        assert _get(L, h) == (9.0, 0.0, 1, 0, 0)
        assert L.rbl_set_periodic(h, 0.0, 6.0, -4, 16, 1) == 0
        assert _get(L, h) == (0.0, 6.0, 0, 16, 1)
        assert L.rbl_set_periodic(h, 0.0, 0.0, 0, 0, 0) == 0      # both axes open is fine while the cell is off
        assert _get(L, h) == (0.0, 0.0, 0, 0, 0)
        assert L.rbl_set_periodic(None, 7.0, 7.0, 1, 1, 1) == ERR_ARG
    finally:
        L.rbl_destroy(h)


def test_every_refusal_names_its_value_and_keeps_the_previous_cell():
    L = _lib()
    h = _context(L, a=0.25)                                       # 4a = 1
    try:
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0
        before = _get(L, h)

        def bad(args, *words, code=ERR_ARG):
            assert L.rbl_set_periodic(h, *args) == code, args
            msg = L.rbl_last_error(h).decode()
            for w in words:
                assert w in msg, (w, msg)
            assert _get(L, h) == before

        for v in (NAN, INF, -INF, -1.0):
            bad((v, 7.0, 1, 1, 1), "Lx")
            bad((7.0, v, 1, 1, 1), "Ly")
            bad((v, 7.0, 1, 1, 0), "Lx")                          # also while it would be stored switched off
        bad((0.0, 0.0, 1, 1, 1), "Lx = 0", "Ly = 0")
        bad((1.0, 7.0, 1, 1, 1), "Lx", "4a", "1.0")               # L = 4a exactly is refused, a hair above is not
        bad((7.0, 0.5, 1, 1, 1), "Ly", "4a", "0.5")
        assert L.rbl_set_periodic(h, 1.0 + 1e-9, 7.5, 2, 3, 1) == 0
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0
        for n in (0, -1, 17):
            bad((7.0, 7.0, n, 1, 1), "nx = %d" % n, "[1, 16]")
            bad((7.0, 7.0, 1, n, 1), "ny = %d" % n, "[1, 16]")
            bad((0.0, 7.0, 1, n, 1), "ny = %d" % n)
        assert L.rbl_set_periodic(h, 0.0, 7.5, 17, 3, 1) == 0     # ... and ignored on an open axis
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0
        # a context with a communicator
        CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
        cb = CB(lambda user, buf, n: 0)
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 0) == 0      # (a cell that is on refuses the communicator: below)
        before = _get(L, h)
        assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
        bad((8.0, 8.0, 1, 1, 1), "communicator")
        assert L.rbl_set_comm_ops(h, 0, 1, None, None, None) == 0
        # ... and the other way round: attaching one while the cell is on, RBL_ERR_STATE with "periodic"; detaching stays possible
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0
        assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == ERR_STATE
        assert b"periodic" in L.rbl_last_error(h)
        assert L.rbl_set_comm_ops(h, 0, 1, None, None, None) == 0
        assert _get(L, h) == (7.0, 7.5, 2, 3, 1)
    finally:
        L.rbl_destroy(h)
    # before rbl_set_parameters no radius is known: a short cell is stored ... and found at use (the GPU tests)
    h = L.rbl_create()
    try:
        assert L.rbl_set_periodic(h, 1e-3, 0.0, 1, 0, 1) == 0
    finally:
        L.rbl_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 3: Python
class _NoLibrary:
    """stands where the extension object would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_python_wrappers_check_before_the_library():
    from rigid_body_light_amd import Ensemble, RigidBody
    from rigid_body_light_amd._lib import DeviceContext, periodic_args
    assert periodic_args("set_periodic", 7, 7.5, (1, 2)) == (7.0, 7.5, 1, 2)
    assert periodic_args("set_periodic", np.float64(7.0), 0, [np.int32(3), 0]) == (7.0, 0.0, 3, 0)
    for Lx, Ly, images, exc, word in (("7", 7.0, (1, 1), TypeError, "Lx"), (7.0, None, (1, 1), TypeError, "Ly"),
                                      (7.0, True, (1, 1), TypeError, "Ly"), (7.0, 7.0, 1, TypeError, "images"),
                                      (7.0, 7.0, (1, 1, 1), ValueError, "images"), (7.0, 7.0, (1.0, 1), TypeError, "images"),
                                      (7.0, 7.0, (1,), ValueError, "images")):
        with pytest.raises(exc, match=word):
            periodic_args("set_periodic", Lx, Ly, images)
    rb = RigidBody.__new__(RigidBody)
    rb.cb = rb.ctx = _NoLibrary()
    with pytest.raises(ValueError, match="images"):
        rb.set_periodic(7.0, 7.0, images=(1, 2, 3))
    ctx = DeviceContext.__new__(DeviceContext)
    ctx.L = ctx.h = _NoLibrary()
    ctx._borrowed = True
    with pytest.raises(TypeError, match="Lx"):
        ctx.set_periodic("wide", 7.0)
    for name in ("set_periodic", "periodic"):
        assert callable(getattr(RigidBody, name)) and callable(getattr(DeviceContext, name)), name
    ens = Ensemble.__new__(Ensemble)
    ens.ctx = _NoLibrary()
    with pytest.raises(ValueError, match="not offered for ensembles"):
        ens.set_periodic(7.0, 7.0)
