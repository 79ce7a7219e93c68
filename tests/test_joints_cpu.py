"""Hard joints of include/rbl.h section 9 without a GPU: the numpy restatement the GPU tests trust (tests/joint_oracle.py) against
central differences of its own gaps, every host refusal of rbl_set_joints with the joint named, the set / get round trip, the
refusals for contexts with a communicator and for ensembles, and the shape checks of the Python wrappers.  No device is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_oracle as jo  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
dp, ip = ctypes.POINTER(dbl), ctypes.POINTER(cint)
ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 5, 7, 11
INF, NAN = float("inf"), float("nan")
NAMES = ("rbl_set_joints", "rbl_get_joints", "rbl_solve_jointed", "rbl_solve_jointed_dev", "rbl_step_jointed", "rbl_joint_state")


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    L.rbl_set_config.argtypes = [vp, vp, vp, cint]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    L.rbl_set_joints.argtypes = [vp, cint, vp, vp, cint]
    L.rbl_get_joints.argtypes = [vp, ip, ip, vp, vp]
    L.rbl_solve_jointed.argtypes = L.rbl_solve_jointed_dev.argtypes = [vp, vp, vp, vp, cint, dbl, vp, vp, vp, ip, dp]
    L.rbl_step_jointed.argtypes = [vp, vp, vp, vp, dbl, cint, dbl, vp, ip, dp]
    L.rbl_joint_state.argtypes = [vp, vp, vp]
    return L


def test_the_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    assert "9. Hard joints" in text
    for said in ("redundant", "communicator", "ensemble", "Brownian", "IGNORED"):      # scope and conventions are written down
        assert said in text, said
    m = re.search(r"#define\s+RBL_ERR_ARG\s+(-?\d+)", text)
    assert m and int(m.group(1)) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------ 1: the oracle
def _system():
    rng = np.random.default_rng(8)
    X = np.array([[0.0, 0.0, 2.0], [1.3, 0.2, 2.2], [0.4, 1.6, 1.8], [2.3, 1.7, 2.6]])
    Q = jo.unit(rng.standard_normal((4, 4)))
    body = np.array([[0, 1], [2, 1], [3, -1], [1, 3], [1, 2], [0, -1]])
    anchor = 0.4 * rng.standard_normal((6, 6))
    anchor[2, 3:] = [2.9, 1.2, 3.1]
    anchor[5, 3:] = [-0.3, 0.2, 1.4]
    anchor[3, :3] = 0.0                                           # a centre anchor
    return X, Q, body, anchor


def test_J_is_the_rate_of_change_of_the_gaps():
    """d gap / dt = J U along the motion the library's update makes (X += h u, Q <- exp(h w) Q): central differences with
    h = 1e-5 have truncation ~ h^2 |w|^2 |l| |w| / 6 ~ 1e-11 and rounding ~ eps |gap| / h ~ 1e-10 on gaps of order one, so
    1e-8 of the largest entry of J U leaves two orders in hand"""
    from oracle import oracle as O
    X, Q, body, anchor = _system()
    J = jo.J_matrix(X, Q, body, anchor)
    assert J.shape == (18, 24)
    rng = np.random.default_rng(9)
    h = 1e-5
    for _ in range(3):
        U = rng.standard_normal(24)
        g = []
        for s in (1.0, -1.0):
            Xs, Qs = O.evolve(X, Q, s * U, h)
            g.append(jo.geometry(Xs, Qs, body, anchor)[2].reshape(-1))
        fd = (g[0] - g[1]) / (2 * h)
        err = np.abs(fd - J @ U).max() / np.abs(J @ U).max()
        print("J U against central differences of the gap: %.2e" % err)
        assert err <= 1e-8
    # a pivot's rows hold no second body, a joint's two halves are opposite in the translations
    assert not J[6:9, :18].any() and np.array_equal(J[0:3, 0:3], np.eye(3)) and np.array_equal(J[0:3, 6:9], -np.eye(3))
    # rigid motion of everything joined by body-body joints leaves their gaps' rates zero: J (u, w) = 0 for a common translation
    Ut = np.tile([0.3, -0.2, 0.5, 0.0, 0.0, 0.0], 4)
    bb = np.repeat(body[:, 1] >= 0, 3)
    assert np.abs((J @ Ut)[bb]).max() <= 1e-15


def test_dense_jointed_solution_satisfies_its_three_blocks():
    rng = np.random.default_rng(10)
    n3, nb6, nj3 = 24, 12, 6
    A = rng.standard_normal((n3, n3))
    M = A @ A.T + n3 * np.eye(n3)
    K, J = rng.standard_normal((n3, nb6)), rng.standard_normal((nj3, nb6))
    F, slip, c = rng.standard_normal(nb6), rng.standard_normal(n3), rng.standard_normal(nj3)
    lam, U, phi = jo.dense_jointed(M, K, J, F, slip, c)
    assert np.abs(M @ lam - K @ U - slip).max() <= 1e-12 and np.abs(K.T @ lam + J.T @ phi + F).max() <= 1e-12
    assert np.abs(J @ U - c).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 2: the C ABI
def _get(L, h):
    n, on = cint(-1), cint(-1)
    assert L.rbl_get_joints(h, ctypes.byref(n), ctypes.byref(on), None, None) == 0
    body, anchor = np.full((n.value, 2), -7, dtype=np.int32), np.zeros((n.value, 6))
    assert L.rbl_get_joints(h, None, None, body.ctypes.data, anchor.ctypes.data) == 0
    return n.value, on.value, body, anchor


def _set(L, h, body, anchor, on=1, n=None):
    body = None if body is None else np.ascontiguousarray(body, dtype=np.int32)
    anchor = None if anchor is None else np.ascontiguousarray(anchor, dtype=np.float64)
    if n is None:
        n = body.shape[0]
    return L.rbl_set_joints(h, n, None if body is None else body.ctypes.data, None if anchor is None else anchor.ctypes.data, on)


GOOD = dict(body=np.array([[0, 1], [2, -1], [3, 1], [1, 0]], dtype=np.int32), anchor=np.arange(24.0).reshape(4, 6) / 8.0)


def _context(L, nb=4):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    X = np.arange(3.0 * nb).reshape(nb, 3) * 3.0
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    assert L.rbl_set_config(h, X.ctypes.data, Q.ctypes.data, nb) == 0
    assert L.rbl_set_K_mats(h) == 0
    return h


def test_set_get_round_trip_and_the_switch():
    L = _lib()
    h = L.rbl_create()
    try:
        assert _get(L, h)[:2] == (0, 0)
        assert _set(L, h, **GOOD) == 0                            # before any rbl_set_config
        n, on, body, anchor = _get(L, h)
        assert (n, on) == (4, 1) and np.array_equal(body, GOOD["body"]) and np.array_equal(anchor, GOOD["anchor"])
        assert _set(L, h, GOOD["body"][:2], GOOD["anchor"][:2], on=0) == 0       # stored, switched off
        n, on, body, anchor = _get(L, h)
        assert (n, on) == (2, 0) and np.array_equal(body, GOOD["body"][:2]) and np.array_equal(anchor, GOOD["anchor"][:2])
        assert _set(L, h, **GOOD) == 0
        assert _set(L, h, None, None, on=0, n=0) == 0             # only the switch: the stored joints stay
        n, on, body, _ = _get(L, h)
        assert (n, on) == (4, 0) and np.array_equal(body, GOOD["body"])
    finally:
        L.rbl_destroy(h)


def test_every_refusal_names_its_joint_and_keeps_the_previous_joints():
    L = _lib()
    h = _context(L, 4)
    try:
        assert _set(L, h, **GOOD) == 0
        before = _get(L, h)

        def bad(*words, **change):
            args = dict(GOOD, **change)
            assert _set(L, h, **args) == ERR_ARG
            msg = L.rbl_last_error(h).decode()
            for w in words:
                assert w in msg, (w, msg)
            now = _get(L, h)
            assert now[:2] == before[:2] and np.array_equal(now[2], before[2]) and np.array_equal(now[3], before[3])

        bad("body", body=None, n=4)                               # NULL where an array is needed
        bad("anchor", anchor=None)
        bad("n_joints", n=0)
        bad("n_joints", n=-3)
        bad("n_joints", n=2049)
        for row, word in (([-2, 1], "out of range"), ([0, -2], "out of range"), ([4, 1], "out of range"), ([0, 4], "out of range"),
                          ([0, 77], "out of range"), ([-1, 2], "pivot"), ([2, 2], "one body")):
            b = GOOD["body"].copy()
            b[2] = row
            bad(word, "joint 2", body=b)
        for v in (NAN, INF, -INF):
            for q in (1, 4):
                a = GOOD["anchor"].copy()
                a[1, q] = v
                bad("anchor", "joint 1", anchor=a)
        # a third joint between one pair of bodies (in either order), a third pivot on one body
        b = np.array([[0, 1], [1, 0], [2, 3], [0, 1]], dtype=np.int32)
        bad("third joint", "joint 3", "0 and 1", body=b)
        b = np.array([[2, -1], [0, 1], [2, -1], [2, -1]], dtype=np.int32)
        bad("third pivot", "joint 3", "body 2", body=b)
        # what is NOT refused: two joints between a pair (a hinge), two pivots on a body, one pivot on every body
        b = np.array([[0, 1], [1, 0], [2, -1], [2, -1]], dtype=np.int32)
        assert _set(L, h, b, GOOD["anchor"]) == 0
        b = np.array([[0, -1], [1, -1], [2, -1], [3, -1]], dtype=np.int32)
        assert _set(L, h, b, GOOD["anchor"]) == 0
    finally:
        L.rbl_destroy(h)
    # without a configuration an index beyond any system is stored ... and found at the solve
    h = L.rbl_create()
    try:
        b = GOOD["body"].copy()
        b[0] = [50, 1]
        assert _set(L, h, b, GOOD["anchor"]) == 0
        b[0] = [-3, 1]
        assert _set(L, h, b, GOOD["anchor"]) == ERR_ARG and b"joint 0" in L.rbl_last_error(h)
    finally:
        L.rbl_destroy(h)


def _solve_args(nb, nj):
    F, U, lam, phi, c = np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(3 * nb * 4), np.zeros(3 * nj), np.zeros(3 * nj)
    it, res = cint(0), dbl(0.0)
    return F, U, lam, phi, c, it, res


def test_the_solves_refuse_before_any_device_work():
    """every refusal below must come back as it does on a box WITHOUT a device too: a call that touched the device first would
    answer RBL_ERR_NO_DEVICE there"""
    import torch
    L = _lib()
    nb = 4
    h = _context(L, nb)
    F, U, lam, phi, c, it, res = _solve_args(nb, 4)
    tail = (ctypes.byref(it), ctypes.byref(res))
    f, u, l, p = F.ctypes.data, U.ctypes.data, lam.ctypes.data, phi.ctypes.data

    def solve(fn, ff=f, mi=50, rt=1e-8, hh=None):
        return fn(h if hh is None else hh, ff, None, None, mi, rt, l, u, p, *tail)

    def step(ff=f, gamma=1.0, mi=50, rt=1e-8, hh=None):
        return L.rbl_step_jointed(h if hh is None else hh, ff, None, None, gamma, mi, rt, p, *tail)

    assert _set(L, h, **GOOD) == 0
    for fn in (L.rbl_solve_jointed, L.rbl_solve_jointed_dev):
        assert fn(None, f, None, None, 50, 1e-8, l, u, p, *tail) == ERR_ARG
        assert solve(fn, ff=None) == ERR_ARG and b"NULL" in L.rbl_last_error(h)
        for mi in (0, -3, 256):                               # no restart: at most 255 iterations
            assert solve(fn, mi=mi) == ERR_ARG
        for rt in (-1.0, NAN):
            assert solve(fn, rt=rt) == ERR_ARG
    assert L.rbl_solve_jointed_dev(h, f, None, None, 50, 1e-8, l, None, p, *tail) == ERR_ARG
    assert L.rbl_step_jointed(None, f, None, None, 1.0, 50, 1e-8, p, *tail) == ERR_ARG
    assert step(ff=None) == ERR_ARG
    for g in (-0.1, 1.5, NAN):
        assert step(gamma=g) == ERR_ARG and b"gamma" in L.rbl_last_error(h)
    assert step(mi=0) == ERR_ARG and step(rt=-1e-8) == ERR_ARG
    # no configuration yet: RBL_ERR_STATE, as the other solvers; a joint that names a body the configuration lacks: the same
    h2 = L.rbl_create()
    assert solve(L.rbl_solve_jointed, hh=h2) == ERR_STATE and step(hh=h2) == ERR_STATE
    assert L.rbl_joint_state(h2, p, None) == ERR_STATE
    L.rbl_destroy(h2)
    h2 = L.rbl_create()
    b = GOOD["body"].copy()
    b[3] = [1, 9]
    assert _set(L, h2, b, GOOD["anchor"]) == 0                 # no configuration yet: stored
    L.rbl_destroy(h2)
    h2 = _context(L, nb)
    assert L.rbl_joint_state(h2, p, None) == ERR_STATE and b"no joints" in L.rbl_last_error(h2)
    assert _set(L, h2, **GOOD) == 0
    assert L.rbl_joint_state(h2, None, p) == ERR_STATE and b"no jointed solve" in L.rbl_last_error(h2)
    X = np.arange(6.0).reshape(2, 3) * 3.0                     # the configuration shrinks under the stored joints
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    assert L.rbl_set_config(h2, X.ctypes.data, Q.ctypes.data, 2) == 0
    assert solve(L.rbl_solve_jointed, hh=h2) == ERR_STATE and b"joint 1 names body 2" in L.rbl_last_error(h2)
    assert step(hh=h2) == ERR_STATE and L.rbl_joint_state(h2, p, None) == ERR_STATE
    L.rbl_destroy(h2)
    # a context with a communicator: RBL_ERR_ARG from all three, joints on or off
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    for with_joints in (False, True):
        if with_joints:
            assert _set(L, h3, **GOOD) == 0
        assert solve(L.rbl_solve_jointed, hh=h3) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
        assert solve(L.rbl_solve_jointed_dev, hh=h3) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
        assert step(hh=h3) == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    L.rbl_destroy(h3)
    if torch.cuda.device_count() == 0:                        # good arguments, no device: loud, and the configuration is untouched
        assert solve(L.rbl_solve_jointed) == ERR_NO_DEVICE and b"no CPU fallback" in L.rbl_last_error(h)
        assert step() == ERR_NO_DEVICE
    L.rbl_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 3: Python
class _NoLibrary:
    """stands where the extension object would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_python_wrappers_check_shapes_before_the_library():
    from rigid_body_light_amd import Ensemble, RigidBody
    from rigid_body_light_amd._lib import DeviceContext, joint_args
    b, anchor = joint_args("set_joints", [[0, 1], [1, -1]], [0.0, 0.0, 0.5], [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    assert b.dtype == np.int32 and b.shape == (2, 2)
    assert np.array_equal(anchor, [[0.0, 0.0, 0.5, 0.1, 0.2, 0.3], [0.0, 0.0, 0.5, 1.0, 2.0, 3.0]])
    ok = dict(body=[[0, 1], [1, -1]], anchor_a=np.zeros(3), anchor_b=np.zeros((2, 3)))
    for name, value in (("body", [[0, 1, 2]]), ("body", [[0.0, 1.0]]), ("body", np.zeros((0, 2), dtype=int)), ("anchor_a", np.zeros((3, 3))),
                        ("anchor_b", np.zeros(2))):
        with pytest.raises(ValueError, match=name):
            joint_args("set_joints", **dict(ok, **{name: value}))
    rb = RigidBody.__new__(RigidBody)
    rb.cb = _NoLibrary()
    rb.N_bodies, rb.blobs_per_body, rb.total_blobs = 4, 2, 8
    with pytest.raises(ValueError, match="body"):
        rb.set_joints([[0, 1, 2]], np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError, match="6\\*N_bodies"):
        rb.solve_jointed(np.zeros(23))
    with pytest.raises(ValueError, match="slip"):
        rb.step_jointed(np.zeros(24), slip=np.zeros(5))
    for name in ("set_joints", "joints", "solve_jointed", "step_jointed", "joint_state"):
        assert callable(getattr(RigidBody, name)) and callable(getattr(DeviceContext, name)), name
    assert callable(DeviceContext.solve_jointed_dev)
    # ensembles: refused before anything is called
    ens = Ensemble.__new__(Ensemble)
    ens.ctx = _NoLibrary()
    with pytest.raises(ValueError, match="not offered for ensembles"):
        ens.set_joints([[0, 1]], np.zeros(3), np.zeros(3))
