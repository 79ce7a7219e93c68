"""Prescribed kinematics per velocity component (include/rbl.h section 7, the _dof entry points), the parts that need no device:
the three entry points are declared and exported, bad arguments are RBL_ERR_ARG with a message that names the entry point before
any device work, and RigidBody.solve_mixed_dof / step_mixed_dof reject anything but a bool array of shape (N_bodies, 6) before
the library is called.  Modelled on test_prescribed_cpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_solve_mixed_dof", "rbl_solve_mixed_dof_dev", "rbl_step_mixed_dof")
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
    L.rbl_solve_mixed_dof.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, vp, vp, ip, dp]
    L.rbl_solve_mixed_dof_dev.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, vp, vp, ip, dp]
    L.rbl_step_mixed_dof.argtypes = [vp, vp, vp, vp, ctypes.c_int, dbl, vp, ip, dp]
    return L


def test_the_three_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed6" % n, code), n
        assert hasattr(L, n), n
    # what the component masks do not cover is written down, and whole-body-only is no longer listed as a limit
    for said in ("Brownian step", "ensembles", "body frame", "lock-step"):
        assert said in text.split("Not offered:")[-1], said
    assert "only whole bodies are prescribed" not in text


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
    """every refusal must come back as RBL_ERR_ARG, naming the entry point, on a box WITHOUT a device too: a call that touched the
    device first would answer RBL_ERR_NO_DEVICE there"""
    import torch
    L = _lib()
    nb = 3
    h = _context(L, nb)
    mask = np.zeros((nb, 6), dtype=np.uint8)
    mask[1, 3:] = 1
    bi, U, F, lam = np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(3 * nb * 4)
    it, res = ctypes.c_int(0), ctypes.c_double(0.0)
    tail = (ctypes.byref(it), ctypes.byref(res))
    m, b, u, f, l = mask.ctypes.data, bi.ctypes.data, U.ctypes.data, F.ctypes.data, lam.ctypes.data
    bad = np.zeros((nb, 6), dtype=np.uint8)
    bad[2, 5] = 2                                          # the LAST entry: all 6 N_bod entries are checked, not the first N_bod

    def refused(rc, name):
        return rc == ERR_ARG and name.encode() + b":" in L.rbl_last_error(h)

    for name in ("solve_mixed_dof", "solve_mixed_dof_dev"):
        fn = getattr(L, "rbl_" + name)

        def solve(mm=m, bb=b, mi=50, rt=1e-8, uu=u, ff=f):
            return fn(h, mm, bb, None, mi, rt, l, uu, ff, *tail)
        assert fn(None, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
        assert refused(solve(mm=None), name) and b"NULL" in L.rbl_last_error(h)
        assert refused(solve(bb=None), name)
        assert refused(solve(uu=None), name)
        assert refused(solve(ff=None), name)
        assert refused(solve(mi=0), name)
        assert refused(solve(mi=-3), name)
        assert refused(solve(mi=256), name)                # no restart: at most 255 iterations
        assert refused(solve(rt=-1.0), name)
        assert refused(solve(rt=float("nan")), name)
        assert refused(solve(mm=bad.ctypes.data), name) and b"0 or 1" in L.rbl_last_error(h)
    name = "step_mixed_dof"
    assert L.rbl_step_mixed_dof(None, m, b, None, 50, 1e-8, f, *tail) == ERR_ARG
    assert refused(L.rbl_step_mixed_dof(h, None, b, None, 50, 1e-8, f, *tail), name)
    assert refused(L.rbl_step_mixed_dof(h, m, None, None, 50, 1e-8, f, *tail), name)
    assert refused(L.rbl_step_mixed_dof(h, m, b, None, 0, 1e-8, f, *tail), name)
    assert refused(L.rbl_step_mixed_dof(h, m, b, None, 256, 1e-8, f, *tail), name)
    assert refused(L.rbl_step_mixed_dof(h, m, b, None, 50, -1e-8, None, *tail), name)
    assert refused(L.rbl_step_mixed_dof(h, bad.ctypes.data, b, None, 50, 1e-8, None, *tail), name)
    # no configuration yet: RBL_ERR_STATE, as the other solvers
    h2 = L.rbl_create()
    assert L.rbl_solve_mixed_dof(h2, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_STATE
    L.rbl_destroy(h2)
    # a context with a communicator: RBL_ERR_ARG from all three, before any device work
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    assert L.rbl_solve_mixed_dof(h3, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
    assert b"solve_mixed_dof:" in L.rbl_last_error(h3) and b"communicator" in L.rbl_last_error(h3)
    assert L.rbl_solve_mixed_dof_dev(h3, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    assert L.rbl_step_mixed_dof(h3, m, b, None, 50, 1e-8, f, *tail) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    L.rbl_destroy(h3)
    if torch.cuda.device_count() == 0:                    # good arguments, no device: loud, and the configuration is untouched
        assert L.rbl_solve_mixed_dof(h, m, b, None, 50, 1e-8, l, u, f, *tail) == ERR_NO_DEVICE
        assert L.rbl_step_mixed_dof(h, m, b, None, 50, 1e-8, f, *tail) == ERR_NO_DEVICE
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


def test_wrapper_takes_a_bool_array_of_shape_nbodies_by_6_and_nothing_else():
    rb = _wrapper()
    bi = np.zeros(24)
    good = np.zeros((4, 6), dtype=bool)
    good[1, 3:] = True
    good[3, 2] = True
    bads = (good.astype(np.uint8), good.astype(np.int64), good.astype(float), good.reshape(-1), good.T, good[:3], np.zeros((4, 5), dtype=bool),
            np.zeros(4, dtype=bool), [1, 3], [], good.tolist()[:2], "ab", None)
    for bad in bads:
        with pytest.raises(ValueError):
            rb.solve_mixed_dof(bad, bi)
        with pytest.raises(ValueError):
            rb.step_mixed_dof(bad, bi)
    with pytest.raises(ValueError):
        rb.solve_mixed_dof(good, np.zeros(23))
    with pytest.raises(ValueError):
        rb.solve_mixed_dof(good, bi, slip=np.zeros(7))
    with pytest.raises(ValueError):
        rb.step_mixed_dof(good, bi.reshape(4, 6)[:3])
    # good arguments reach the library (here: the stand-in), the mask as 6 N_bodies bytes in body_in's order
    seen = {}

    class _Record:
        def solve_mixed_dof(self, mask, body_in, slip, max_iter, rtol):
            seen["args"] = (mask, body_in, slip, max_iter, rtol)
            return "solved"

        def step_mixed_dof(self, mask, body_in, slip, max_iter, rtol):
            seen["args"] = (mask, body_in, slip, max_iter, rtol)
            return "stepped"
    rb.ctx = _Record()
    assert rb.solve_mixed_dof(good, bi.reshape(4, 6), max_iter=7) == "solved"
    mask, body_in, slip, max_iter, rtol = seen["args"]
    assert mask.dtype == np.uint8 and mask.shape == (24,) and mask.tolist() == good.reshape(-1).astype(int).tolist()
    assert body_in.shape == (24,) and slip is None and max_iter == 7
    assert rb.step_mixed_dof(np.asfortranarray(good), bi, slip=np.zeros((8, 3))) == "stepped"      # any memory layout, read by index
    assert seen["args"][0].tolist() == good.reshape(-1).astype(int).tolist() and seen["args"][2].shape == (24,)
    assert rb.solve_mixed_dof(good.tolist(), bi) == "solved"                                        # a nested list of bools is such an array
    # solve_mixed keeps reading a mask of N_bodies entries
    with pytest.raises(ValueError):
        rb.solve_mixed(good, bi)
