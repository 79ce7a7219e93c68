"""Prescribed kinematics for many right-hand sides in lock step (include/rbl.h section 7, the _multi entry points), the parts that
need no device: the four entry points are declared and exported, every bad argument is RBL_ERR_ARG with a message that names the
entry point before any device work, and RigidBody.solve_mixed_multi / solve_mixed_dof_multi reject wrong shapes and dtypes before
the library is called.  Modelled on test_prescribed_dof_cpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_solve_mixed_multi", "rbl_solve_mixed_multi_dev", "rbl_solve_mixed_dof_multi", "rbl_solve_mixed_dof_multi_dev")
ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 5, 7, 11


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, ctypes.c_int]
    L.rbl_set_config.argtypes = [vp, vp, vp, ctypes.c_int]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_set_comm_ops.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    for n in NAMES:
        getattr(L, n).argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, dbl, vp, vp, vp, vp, vp]
    return L


def test_the_four_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        mask = "prescribed6" if "_dof_" in n else "prescribed"
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*%s\s*,\s*int\s+nrhs\s*," % (n, mask), code), n
        assert hasattr(L, n), n
    # lock-step solves under one mask are offered now; what stays out is written down
    assert "Not offered: lock-step multi-right-hand-side mixed solves" not in text
    assert "differs from column to" in text.split("Not offered:")[-1]


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
    """every refusal must come back as RBL_ERR_ARG, naming the entry point, on a machine WITHOUT a device too: a call that touched
    the device first would answer RBL_ERR_NO_DEVICE there"""
    import torch
    L = _lib()
    nb, k = 3, 5
    h = _context(L, nb)
    bi, U, F, lam = np.zeros(6 * nb * k), np.zeros(6 * nb * k), np.zeros(6 * nb * k), np.zeros(3 * nb * 4 * k)
    it, res = np.zeros(k, dtype=np.int32), np.zeros(k)
    tail = (it.ctypes.data, res.ctypes.data)
    b, u, f, l = bi.ctypes.data, U.ctypes.data, F.ctypes.data, lam.ctypes.data
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    h2 = L.rbl_create()

    def refused(rc, name):
        return rc == ERR_ARG and name.encode() + b":" in L.rbl_last_error(h)

    for n in NAMES:
        name, per = n[4:], (6 if "_dof_" in n else 1)
        fn = getattr(L, n)
        mask = np.zeros(per * nb, dtype=np.uint8)
        mask[per:2 * per] = 1
        bad = np.zeros(per * nb, dtype=np.uint8)
        bad[-1] = 2                                        # the LAST entry: every entry is checked
        m = mask.ctypes.data

        def solve(mm=m, kk=k, bb=b, mi=50, rt=1e-8, uu=u, ff=f):
            return fn(h, mm, kk, bb, None, mi, rt, l, uu, ff, *tail)
        assert fn(None, m, k, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
        assert refused(solve(mm=None), name) and b"NULL" in L.rbl_last_error(h)
        assert refused(solve(bb=None), name)
        assert refused(solve(uu=None), name)
        assert refused(solve(ff=None), name)
        assert refused(solve(kk=0), name) and b"nrhs" in L.rbl_last_error(h)
        assert refused(solve(kk=-2), name) and b"nrhs" in L.rbl_last_error(h)
        assert refused(solve(mi=0), name)
        assert refused(solve(mi=-3), name)
        assert refused(solve(mi=256), name)                # no restart: at most 255 iterations
        assert refused(solve(rt=-1.0), name)
        assert refused(solve(rt=float("nan")), name)
        assert refused(solve(mm=bad.ctypes.data), name) and b"0 or 1" in L.rbl_last_error(h)
        # no configuration yet: RBL_ERR_STATE, as the other solvers
        assert fn(h2, m, k, b, None, 50, 1e-8, l, u, f, *tail) == ERR_STATE
        # a context with a communicator
        assert fn(h3, m, k, b, None, 50, 1e-8, l, u, f, *tail) == ERR_ARG
        assert name.encode() + b":" in L.rbl_last_error(h3) and b"communicator" in L.rbl_last_error(h3)
        if torch.cuda.device_count() == 0:                # good arguments, no device: loud
            assert solve() == ERR_NO_DEVICE
    L.rbl_destroy(h2)
    L.rbl_destroy(h3)
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


def test_wrappers_reject_wrong_shapes_and_dtypes_before_calling_down():
    rb = _wrapper()
    k = 3
    bi = np.zeros((k, 24))
    p = np.array([False, True, False, True])
    P = np.zeros((4, 6), dtype=bool)
    P[1, 3:] = True
    for fn, good, bad_masks in ((rb.solve_mixed_multi, p, (p.astype(float), np.zeros(5, dtype=bool), [0, 0], [7], P)),
                                (rb.solve_mixed_dof_multi, P, (P.astype(np.uint8), P.reshape(-1), P.T, p, [1, 3], None))):
        for bad in bad_masks:
            with pytest.raises(ValueError):
                fn(bad, bi)
        for bad_bi in (np.zeros(24), np.zeros(k * 24), np.zeros((k, 23)), np.zeros((0, 24)), np.zeros((k, 4, 6)), np.zeros((24, k)),
                       np.zeros((k, 24), dtype=complex), np.full((k, 24), "a"), None):
            with pytest.raises(ValueError):
                fn(good, bad_bi)
        for bad_slip in (np.zeros(24), np.zeros(k * 24), np.zeros((k, 23)), np.zeros((k + 1, 24)), np.zeros((24, k)), np.zeros((k, 8, 3)),
                         np.zeros((k, 24), dtype=complex)):
            with pytest.raises(ValueError):
                fn(good, bi, slip=bad_slip)
    # good arguments reach the library (here: a stand-in): the mask as bytes, body_in and slip as C-contiguous float64 rows
    seen = {}

    class _Record:
        def solve_mixed_multi(self, mask, body_in, slip, max_iter, rtol):
            seen["args"] = (mask, body_in, slip, max_iter, rtol)
            return "multi"

        def solve_mixed_dof_multi(self, mask, body_in, slip, max_iter, rtol):
            seen["args"] = (mask, body_in, slip, max_iter, rtol)
            return "dof_multi"
    rb.ctx = _Record()
    assert rb.solve_mixed_multi([1, 3], np.asfortranarray(bi), max_iter=7) == "multi"
    mask, body_in, slip, max_iter, rtol = seen["args"]
    assert mask.dtype == np.uint8 and mask.tolist() == [0, 1, 0, 1]
    assert body_in.shape == (k, 24) and body_in.flags.c_contiguous and body_in.dtype == np.float64 and slip is None and max_iter == 7
    assert rb.solve_mixed_dof_multi(P, np.zeros((k, 24), dtype=np.float32), slip=np.zeros((k, 24), dtype=int), rtol=1e-3) == "dof_multi"
    mask, body_in, slip, max_iter, rtol = seen["args"]
    assert mask.dtype == np.uint8 and mask.shape == (24,) and mask.tolist() == P.reshape(-1).astype(int).tolist()
    assert body_in.dtype == np.float64 and slip.dtype == np.float64 and slip.shape == (k, 24) and rtol == 1e-3
    # the resistance matrix keeps its sequential loop unless asked: lock_step=True goes through solve_mixed_multi
    calls = []

    class _Count:
        def solve_mixed(self, mask, body_in, slip, max_iter, rtol):
            calls.append("one")
            return None, None, np.zeros(24), 1, 0.0

        def solve_mixed_multi(self, mask, body_in, slip, max_iter, rtol):
            calls.append(("multi", body_in.copy()))
            return None, None, np.arange(body_in.size, dtype=float).reshape(body_in.shape), np.ones(body_in.shape[0], dtype=np.int32), None
    rb.ctx = _Count()
    R, its = rb.body_resistance_matrix(columns=[2, 17])
    assert calls == ["one", "one"] and R.shape == (24, 2)
    del calls[:]
    R, its = rb.body_resistance_matrix(columns=[2, 17], lock_step=True)
    assert len(calls) == 1 and calls[0][0] == "multi"
    U = calls[0][1]
    assert U.shape == (2, 24) and U[0, 2] == 1.0 and U[1, 17] == 1.0 and U.sum() == 2.0
    assert R.shape == (24, 2) and np.array_equal(R[:, 1], -np.arange(24.0, 48.0)) and its.tolist() == [1, 1]
