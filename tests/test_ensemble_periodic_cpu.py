"""The cell of an ensemble (include/rbl.h section 5: rbl_ensemble_set_periodic) without a GPU: the entry points are declared and
exported, every argument refusal has its status and its message on a context that has never seen a device -- they stand before the
"no ensemble" refusal, which is pinned too --, and the Python wrappers check their arguments before the library is called.  No
device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)
ERR_STATE, ERR_ARG = 7, 11
INF, NAN = float("inf"), float("nan")


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    L.rbl_set_periodic.argtypes = L.rbl_ensemble_set_periodic.argtypes = [vp, dbl, dbl, cint, cint, cint]
    L.rbl_get_periodic.argtypes = L.rbl_ensemble_get_periodic.argtypes = [vp, dp, dp, ip, ip, ip]
    return L


def _get(L, h, which="rbl_ensemble_get_periodic"):
    Lx, Ly, nx, ny, on = dbl(-1.0), dbl(-1.0), cint(-1), cint(-1), cint(-1)
    assert getattr(L, which)(h, ctypes.byref(Lx), ctypes.byref(Ly), ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(on)) == 0
    return Lx.value, Ly.value, nx.value, ny.value, on.value


def _context(L, a):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5
    assert L.rbl_set_parameters(h, a, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    return h


def test_the_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in ("rbl_ensemble_set_periodic", "rbl_ensemble_get_periodic"):
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    assert "rbl_ensemble_set_periodic" in sec5                     # documented with the ensembles ...
    assert "rbl_ensemble_set_periodic" in text[text.index("10. Periodic cell"):]   # ... and cross-referenced from the cell's section


def test_every_argument_refusal_has_its_status_and_message_and_stands_before_the_ensemble_check():
    """none of these contexts holds an ensemble, and none has a device: an argument refusal is what comes back, RBL_ERR_ARG with
    the value named under the new name; arguments that pass meet the "no ensemble" refusal, RBL_ERR_STATE"""
    L = _lib()
    h = _context(L, a=0.25)                                       # 4a = 1
    try:
        def bad(args, *words, code=ERR_ARG):
            assert L.rbl_ensemble_set_periodic(h, *args) == code, args
            msg = L.rbl_last_error(h).decode()
            for w in ("ensemble_set_periodic",) + words:
                assert w in msg, (w, msg)
            assert _get(L, h) == (0.0, 0.0, 0, 0, 0)              # nothing is stored unless every check passes

        for v in (NAN, INF, -INF, -1.0):
            bad((v, 7.0, 1, 1, 1), "Lx", "finite")
            bad((7.0, v, 1, 1, 1), "Ly", "finite")
            bad((v, 7.0, 1, 1, 0), "Lx")                          # also while it would be stored switched off
        bad((0.0, 0.0, 1, 1, 1), "Lx = 0", "Ly = 0")
        bad((1.0, 7.0, 1, 1, 1), "Lx", "4a", "1.0")               # L = 4a exactly is refused
        bad((7.0, 0.5, 1, 1, 1), "Ly", "4a", "0.5")
        for n in (0, -1, 17):
            bad((7.0, 7.0, n, 1, 1), "nx = %d" % n, "[1, 16]")
            bad((7.0, 7.0, 1, n, 1), "ny = %d" % n, "[1, 16]")
            bad((0.0, 7.0, 1, n, 1), "ny = %d" % n)
        # arguments that pass: the context holds no ensemble
        for args in ((7.0, 7.5, 2, 3, 1), (1.0 + 1e-9, 7.5, 1, 1, 1), (0.0, 7.5, 17, 3, 1), (0.0, 0.0, 0, 0, 0)):
            bad(args, "ensemble", "rbl_ensemble_set_config", code=ERR_STATE)
        # a communicator is refused before the ensemble is looked for, after the arguments
        CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
        cb = CB(lambda user, buf, n: 0)
        assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
        bad((8.0, 8.0, 1, 1, 1), "communicator")
        bad((8.0, 8.0, 0, 1, 1), "nx = 0")
        assert L.rbl_set_comm_ops(h, 0, 1, None, None, None) == 0
        # the single context's cell is other state: setting it leaves the ensemble's alone, and the other way round
        assert L.rbl_set_periodic(h, 7.0, 7.5, 2, 3, 1) == 0
        assert _get(L, h) == (0.0, 0.0, 0, 0, 0) and _get(L, h, "rbl_get_periodic") == (7.0, 7.5, 2, 3, 1)
        assert L.rbl_ensemble_get_periodic(h, None, None, None, None, None) == 0
        assert L.rbl_ensemble_set_periodic(None, 7.0, 7.0, 1, 1, 1) == ERR_ARG
        assert L.rbl_ensemble_get_periodic(None, None, None, None, None, None) == ERR_ARG
    finally:
        L.rbl_destroy(h)
    # before rbl_set_parameters no radius is known: the 4a check waits, the "no ensemble" refusal does not
    h = L.rbl_create()
    try:
        assert L.rbl_ensemble_set_periodic(h, 1e-3, 0.0, 1, 0, 1) == ERR_STATE
        assert b"ensemble" in L.rbl_last_error(h)
        assert L.rbl_ensemble_set_periodic(h, -1.0, 0.0, 1, 0, 1) == ERR_ARG
    finally:
        L.rbl_destroy(h)


class _NoLibrary:
    """stands where the extension object would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_python_wrappers_check_before_the_library():
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext.__new__(DeviceContext)
    ctx.L = ctx.h = _NoLibrary()
    ctx._borrowed = True
    ens = Ensemble.__new__(Ensemble)
    ens.ctx = _NoLibrary()
    for Lx, Ly, images, exc, word in (("7", 7.0, (1, 1), TypeError, "Lx"), (7.0, None, (1, 1), TypeError, "Ly"),
                                      (7.0, True, (1, 1), TypeError, "Ly"), (7.0, 7.0, 1, TypeError, "images"),
                                      (7.0, 7.0, (1, 1, 1), ValueError, "images"), (7.0, 7.0, (1.0, 1), TypeError, "images"),
                                      (7.0, 7.0, (1,), ValueError, "images")):
        with pytest.raises(exc, match=word):
            ctx.ensemble_set_periodic(Lx, Ly, images=images)
        with pytest.raises(exc, match=word):
            ens.set_cell(Lx, Ly, images=images)
    for name in ("ensemble_set_periodic", "ensemble_periodic"):
        assert callable(getattr(DeviceContext, name)), name
    for name in ("set_cell", "cell"):
        assert callable(getattr(Ensemble, name)), name
    # the single context's name still raises for an ensemble, and now says where to go
    with pytest.raises(ValueError, match="not offered for ensembles") as e:
        ens.set_periodic(7.0, 7.0)
    assert "set_cell" in str(e.value)
