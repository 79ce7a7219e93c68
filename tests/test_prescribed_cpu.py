"""Prescribed kinematics (include/rbl.h section 7), the parts that need no device: the three entry points are declared and
exported, bad arguments are RBL_ERR_ARG before any device work, a box without a device answers RBL_ERR_NO_DEVICE, and
RigidBody.solve_mixed rejects a bad `prescribed` set or bad shapes before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_solve_mixed", "rbl_solve_mixed_dev", "rbl_step_mixed")
ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 5, 7, 11


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    vp, dbl, ip, dp = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, ctypes.c_int]
    L.rbl_set_config.argtypes = [vp, vp, vp, ctypes.c_int]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_set_comm_ops.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.rbl_solve_mixed.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, vp, vp, ip, dp]
    L.rbl_solve_mixed_dev.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, vp, vp, ip, dp]
    L.rbl_step_mixed.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, ip, dp]
    return L


def test_the_three_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed" % n, code), n
        assert hasattr(L, n), n
    assert "7. Prescribed kinematics" in text
    for said in ("communicator", "Brownian", "per-component", "TOTAL load"):     # scope and conventions are written down
        assert said in text, said


def _context(L, nb=3):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    X = np.arange(3.0 * nb).reshape(nb, 3) * 3.0
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    assert L.rbl_set_config(h, X.ctypes.data, Q.ctypes.data, nb) == 0
    assert L.rbl_set_K_mats(h) == 0
    return h


def test_bad_arguments_are_refused_before_any_device_work():
    """every refusal below must come back as RBL_ERR_ARG on a box WITHOUT a device too: a call that touched the device first
    would answer RBL_ERR_NO_DEVICE there"""
    import torch
    L = _lib()
    nb = 3
    h = _context(L, nb)
    mask = np.array([0, 1, 0], dtype=np.uint8)
    bi, U, F, lam = np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(3 * nb * 4)
    it, res = ctypes.c_int(0), ctypes.c_double(0.0)
    tail = (ctypes.byref(it), ctypes.byref(res))
    m, b, u, f, l = mask.ctypes.data, bi.ctypes.data, U.ctypes.data, F.ctypes.data, lam.ctypes.data

    def solve(fn, mm=m, bb=b, mi=50, rt=1e-8, uu=u, ff=f):
        return fn(h, mm, bb, None, mi, rt, l, uu, ff, *tail)

    for fn in (L.rbl_solve_mixed, L.rbl_solve_mixed_dev):
        assert fn(None, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
        assert solve(fn, mm=None) == ERR_ARG and b"NULL" in L.rbl_last_error(h)
        assert solve(fn, bb=None) == ERR_ARG
        assert solve(fn, uu=None) == ERR_ARG
        assert solve(fn, ff=None) == ERR_ARG
        assert solve(fn, mi=0) == ERR_ARG
        assert solve(fn, mi=-3) == ERR_ARG
        assert solve(fn, mi=256) == ERR_ARG                # no restart: at most 255 iterations
        assert solve(fn, rt=-1.0) == ERR_ARG
        assert solve(fn, rt=float("nan")) == ERR_ARG
        bad = np.array([0, 2, 0], dtype=np.uint8)
        assert solve(fn, mm=bad.ctypes.data) == ERR_ARG and b"0 or 1" in L.rbl_last_error(h)
    assert L.rbl_step_mixed(None, m, b, None, 50, 1e-8, f, *tail) == ERR_ARG
    assert L.rbl_step_mixed(h, None, b, None, 50, 1e-8, f, *tail) == ERR_ARG
    assert L.rbl_step_mixed(h, m, None, None, 50, 1e-8, f, *tail) == ERR_ARG
    assert L.rbl_step_mixed(h, m, b, None, 0, 1e-8, f, *tail) == ERR_ARG
    assert L.rbl_step_mixed(h, m, b, None, 50, -1e-8, None, *tail) == ERR_ARG
    bad = np.array([255, 0, 0], dtype=np.uint8)
    assert L.rbl_step_mixed(h, bad.ctypes.data, b, None, 50, 1e-8, None, *tail) == ERR_ARG
    # no configuration yet: RBL_ERR_STATE, as the other solvers
    h2 = L.rbl_create()
    assert L.rbl_solve_mixed(h2, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_STATE
    L.rbl_destroy(h2)
    # a context with a communicator: RBL_ERR_ARG from all three, before any device work
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    assert L.rbl_solve_mixed(h3, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    assert L.rbl_solve_mixed_dev(h3, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
    assert L.rbl_step_mixed(h3, m, b, None, 50, 1e-8, f, *tail) == ERR_ARG
    L.rbl_destroy(h3)
    if torch.cuda.device_count() == 0:                    # good arguments, no device: loud, and the configuration is untouched
        assert solve(L.rbl_solve_mixed) == ERR_NO_DEVICE and b"no CPU fallback" in L.rbl_last_error(h)
        assert L.rbl_step_mixed(h, m, b, None, 50, 1e-8, f, *tail) == ERR_NO_DEVICE
    L.rbl_destroy(h)


class _NoLibrary:
    """stands where the extension object would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _wrapper(nb=4, nblb=2):
    from rigid_body_light_amd import RigidBody
    rb = RigidBody.__new__(RigidBody)
    rb.cb = rb.ctx = _NoLibrary()          # the extension object and the view of its context
    rb.N_bodies, rb.blobs_per_body, rb.total_blobs = nb, nblb, nb * nblb
    rb.X_shape, rb.Q_shape = (nb, 3), (nb, 4)
    return rb


def test_wrapper_rejects_bad_sets_and_shapes_before_calling_the_library():
    rb = _wrapper()
    bi = np.zeros(24)
    for bad in ([0, 4], [-1], [1, 1], [0, 2, 2], np.array([True, False, True]), np.ones(5, dtype=bool), [0.5, 1.0], "ab"):
        with pytest.raises(ValueError):
            rb.solve_mixed(bad, bi)
        with pytest.raises(ValueError):
            rb.step_mixed(bad, bi)
    with pytest.raises(ValueError):
        rb.solve_mixed([0], np.zeros(23))
    with pytest.raises(ValueError):
        rb.solve_mixed([0], bi, slip=np.zeros(7))
    with pytest.raises(ValueError):
        rb.step_mixed([0], bi.reshape(4, 6)[:3])
    # good arguments reach the library (here: the stand-in's refusal), with the set as a 0/1 byte mask
    seen = {}

    class _Record:
        def solve_mixed(self, mask, body_in, slip, max_iter, rtol):
            seen["args"] = (mask, body_in, slip, max_iter, rtol)
            return "solved"
    rb.ctx = _Record()
    assert rb.solve_mixed([3, 1], bi.reshape(4, 6), max_iter=7) == "solved"
    mask, body_in, slip, max_iter, rtol = seen["args"]
    assert mask.dtype == np.uint8 and mask.tolist() == [0, 1, 0, 1] and body_in.shape == (24,) and slip is None and max_iter == 7
    assert rb.solve_mixed(np.array([False, True, False, True]), bi, slip=np.zeros((8, 3))) == "solved"
    assert seen["args"][0].tolist() == [0, 1, 0, 1] and seen["args"][2].shape == (24,)
    assert rb.solve_mixed([], bi) == "solved" and seen["args"][0].tolist() == [0, 0, 0, 0]      # nobody prescribed: a mobility solve
