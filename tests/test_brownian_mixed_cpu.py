"""The Brownian midpoint step with prescribed bodies (include/rbl.h section 7), the parts that need no device: the three entry
points are declared and exported, bad arguments are RBL_ERR_ARG before any device work, a box without a device answers
RBL_ERR_NO_DEVICE, and RigidBody.step_brownian_mixed / RHS_and_Midpoint_mixed reject a bad `prescribed` set or bad shapes before
the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_RHS_and_Midpoint_mixed", "rbl_RHS_and_Midpoint_mixed_dev", "rbl_step_brownian_mixed")
ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 5, 7, 11


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    vp, dbl, ip, dp, u64, ci = (ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                                ctypes.c_uint64, ctypes.c_int)
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, ci]
    L.rbl_set_config.argtypes = [vp, vp, vp, ci]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_set_comm_ops.argtypes = [vp, ci, ci, vp, vp, vp]
    L.rbl_RHS_and_Midpoint_mixed.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, vp, vp, vp]
    L.rbl_RHS_and_Midpoint_mixed_dev.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, vp, vp, vp]
    L.rbl_step_brownian_mixed.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, ci, dbl, vp, ip, dp]
    return L


def test_the_three_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed" % n, code), n
        assert hasattr(L, n), n
    for said in ("Brownian midpoint step with prescribed bodies", "D_f Kinv W_rfd", "(dt/2) U_p", "instantaneous load",
                 "dt <= 0 or delta <= 0"):                                # the scheme and its conventions are written down
        assert said in text, said
    assert "Not offered: the Brownian midpoint step" not in text


def _context(L, nb=3, dt=0.01, kBT=1.0):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, dt, kBT, 1.0, cfg.ctypes.data, 4) == 0
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
    bi, F, s, Xh, Qh = np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(3 * nb * 4), np.zeros(3 * nb), np.zeros(4 * nb)
    it, res = ctypes.c_int(0), ctypes.c_double(0.0)
    tail = (ctypes.byref(it), ctypes.byref(res))
    m, b, f = mask.ctypes.data, bi.ctypes.data, F.ctypes.data
    out = (s.ctypes.data, Xh.ctypes.data, Qh.ctypes.data)

    def step(hh=h, mm=m, bb=b, delta=1e-4, mi=50, rt=1e-8, ff=f):
        return L.rbl_step_brownian_mixed(hh, mm, bb, None, None, 0, 0, 1, delta, mi, rt, ff, *tail)

    def rhs(fn, hh=h, mm=m, bb=b, delta=1e-4, oo=out):
        return fn(hh, mm, bb, None, None, 0, 0, 1, delta, *oo)

    assert step(hh=None) == ERR_ARG
    assert step(mm=None) == ERR_ARG and b"NULL" in L.rbl_last_error(h)
    assert step(bb=None) == ERR_ARG
    bad = np.array([0, 2, 0], dtype=np.uint8)
    assert step(mm=bad.ctypes.data) == ERR_ARG and b"0 or 1" in L.rbl_last_error(h)
    assert step(mi=0) == ERR_ARG
    assert step(mi=-3) == ERR_ARG
    assert step(mi=255) == ERR_ARG                         # no restart: at most 254 iterations
    assert step(rt=-1.0) == ERR_ARG
    assert step(rt=float("nan")) == ERR_ARG
    assert step(delta=0.0) == ERR_ARG and b"delta" in L.rbl_last_error(h)
    assert step(delta=-1e-4) == ERR_ARG
    assert step(delta=float("nan")) == ERR_ARG
    for fn in (L.rbl_RHS_and_Midpoint_mixed, L.rbl_RHS_and_Midpoint_mixed_dev):
        assert rhs(fn, hh=None) == ERR_ARG
        assert rhs(fn, mm=None) == ERR_ARG and b"NULL" in L.rbl_last_error(h)
        assert rhs(fn, bb=None) == ERR_ARG
        assert rhs(fn, mm=bad.ctypes.data) == ERR_ARG and b"0 or 1" in L.rbl_last_error(h)
        assert rhs(fn, delta=0.0) == ERR_ARG and b"delta" in L.rbl_last_error(h)
        assert rhs(fn, delta=-1.0) == ERR_ARG
        for k in range(3):
            assert rhs(fn, oo=tuple(None if j == k else o for j, o in enumerate(out))) == ERR_ARG
    # dt <= 0 with kBT > 0
    h0 = _context(L, nb, dt=0.0)
    assert step(hh=h0) == ERR_ARG and b"dt" in L.rbl_last_error(h0)
    assert rhs(L.rbl_RHS_and_Midpoint_mixed, hh=h0) == ERR_ARG
    assert rhs(L.rbl_RHS_and_Midpoint_mixed_dev, hh=h0) == ERR_ARG
    L.rbl_destroy(h0)
    # no configuration yet: RBL_ERR_STATE, as the other solvers
    h2 = L.rbl_create()
    assert step(hh=h2) == ERR_STATE
    assert rhs(L.rbl_RHS_and_Midpoint_mixed, hh=h2) == ERR_STATE
    L.rbl_destroy(h2)
    # a context with a communicator: RBL_ERR_ARG from all three, before any device work
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    assert step(hh=h3) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    assert rhs(L.rbl_RHS_and_Midpoint_mixed, hh=h3) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    assert rhs(L.rbl_RHS_and_Midpoint_mixed_dev, hh=h3) == ERR_ARG
    L.rbl_destroy(h3)
    # kBT = 0 is rbl_step_mixed: its refusals, and no quarrel with delta
    h4 = _context(L, nb, kBT=0.0)
    assert step(hh=h4, mi=0) == ERR_ARG
    assert step(hh=h4, mm=None) == ERR_ARG
    if torch.cuda.device_count() == 0:
        assert step(hh=h4, delta=0.0) == ERR_NO_DEVICE
    L.rbl_destroy(h4)
    if torch.cuda.device_count() == 0:                    # good arguments, no device: loud, and the configuration is untouched
        assert step() == ERR_NO_DEVICE and b"no CPU fallback" in L.rbl_last_error(h)
        assert rhs(L.rbl_RHS_and_Midpoint_mixed) == ERR_NO_DEVICE
        assert rhs(L.rbl_RHS_and_Midpoint_mixed_dev) == ERR_NO_DEVICE
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
            rb.step_brownian_mixed(bad, bi)
        with pytest.raises(ValueError):
            rb.RHS_and_Midpoint_mixed(bad, bi)
    for fn in (rb.step_brownian_mixed, rb.RHS_and_Midpoint_mixed):
        with pytest.raises(ValueError):
            fn([0], np.zeros(23))
        with pytest.raises(ValueError):
            fn([0], bi, slip=np.zeros(7))
        with pytest.raises(ValueError):
            fn([0], bi, W=np.zeros(24))                    # W is [W1 | W2 | W_rfd]: 9 N_blobs = 72 numbers
        with pytest.raises(ValueError):
            fn([0], bi.reshape(4, 6)[:3])
    # good arguments reach the library with the set as a 0/1 byte mask and flat arrays
    seen = {}

    class _Record:
        def step_brownian_mixed(self, mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol):
            seen["step"] = (mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol)
            return "stepped"

        def RHS_and_Midpoint_mixed(self, mask, body_in, slip, W, seed, method, split_rand, delta):
            seen["rhs"] = (mask, body_in, slip, W, seed, method, split_rand, delta)
            return "rhs"
    rb.ctx = _Record()
    assert rb.step_brownian_mixed([3, 1], bi.reshape(4, 6), W=np.zeros((3, 24)), seed=5, max_iter=7) == "stepped"
    mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol = seen["step"]
    assert mask.dtype == np.uint8 and mask.tolist() == [0, 1, 0, 1] and body_in.shape == (24,) and slip is None
    assert W.shape == (72,) and seed == 5 and method == "lanczos_pc" and split_rand is True and delta == 1e-4
    assert max_iter == 7 and rtol == 1e-8
    assert rb.RHS_and_Midpoint_mixed(np.array([False, True, False, True]), bi, slip=np.zeros((8, 3)), split_rand=False) == "rhs"
    mask, body_in, slip, W, seed, method, split_rand, delta = seen["rhs"]
    assert mask.tolist() == [0, 1, 0, 1] and slip.shape == (24,) and W is None and method == "cholesky" and split_rand is False
    assert rb.step_brownian_mixed([], bi) == "stepped" and seen["step"][0].tolist() == [0, 0, 0, 0]     # nobody prescribed
