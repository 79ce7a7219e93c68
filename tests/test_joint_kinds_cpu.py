"""Joint kinds of include/rbl.h section 9 (ball, lock, axis) without a GPU: every host refusal of rbl_set_joint_kinds and
rbl_set_joint_rates with the joint named and the previous set left in place, the set / get round trip, the Python checks before
the library is called, the numpy restatement (tests/joint_kinds_oracle.py) against central differences of its own angular gaps
and on a welded pair's rigid motion, and the dense jointed matrices of the GPU cases.  No device is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_kinds_oracle as jk  # noqa: E402
import joint_oracle as jo  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
ip = ctypes.POINTER(cint)
ERR_STATE, ERR_ARG = 7, 11
INF, NAN = float("inf"), float("nan")
NAMES = ("rbl_set_joint_kinds", "rbl_get_joint_kinds", "rbl_set_joint_rates", "rbl_joint_state_kinds")
BALL, LOCK, AXIS = 0, 1, 2


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    L.rbl_set_config.argtypes = [vp, vp, vp, cint]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_set_joints.argtypes = [vp, cint, vp, vp, cint]
    L.rbl_get_joints.argtypes = [vp, ip, ip, vp, vp]
    L.rbl_set_joint_kinds.argtypes = [vp, cint, vp, vp, vp, vp, vp, cint]
    L.rbl_get_joint_kinds.argtypes = [vp, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp]
    L.rbl_set_joint_rates.argtypes = [vp, vp]
    L.rbl_joint_state_kinds.argtypes = [vp, vp, vp, vp]
    return L


def _context(L, nb=4):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    X = np.arange(3.0 * nb).reshape(nb, 3) * 3.0
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    assert L.rbl_set_config(h, X.ctypes.data, Q.ctypes.data, nb) == 0
    assert L.rbl_set_K_mats(h) == 0
    return h


def _p(v, dtype):
    return None if v is None else np.ascontiguousarray(v, dtype=dtype)


def _set(L, h, s, on=1, n=None):
    a = [_p(s.get("body"), np.int32), _p(s.get("anchor"), np.float64), _p(s.get("kind"), np.int32), _p(s.get("axis"), np.float64),
         _p(s.get("q_rel"), np.float64)]
    if n is None:
        n = a[0].shape[0]
    return L.rbl_set_joint_kinds(h, n, a[0] if a[0] is None else a[0].ctypes.data, *(None if v is None else v.ctypes.data for v in a[1:]), on)


def _get(L, h):
    n, on, by = cint(-1), cint(-1), cint(-1)
    assert L.rbl_get_joint_kinds(h, ctypes.byref(n), ctypes.byref(on), ctypes.byref(by), *([None] * 7)) == 0
    m = n.value
    o = dict(n=m, on=on.value, by_kinds=by.value, body=np.full((m, 2), -7, dtype=np.int32), anchor=np.zeros((m, 6)),
             kind=np.full(m, -7, dtype=np.int32), axis=np.zeros((m, 3)), q_rel=np.zeros((m, 4)), theta=np.full(m, NAN), rate=np.full(m, NAN))
    assert L.rbl_get_joint_kinds(h, None, None, None, *(o[k].ctypes.data for k in ("body", "anchor", "kind", "axis", "q_rel", "theta", "rate"))) == 0
    return o


def _good():
    """5 joints on 4 bodies: a hinge 0-1 (ball + axis), a weld 2-lab (ball + lock), a ball joint 3-1"""
    return dict(body=np.array([[0, 1], [0, 1], [2, -1], [2, -1], [3, 1]], dtype=np.int32),
                anchor=np.arange(30.0).reshape(5, 6) / 8.0, kind=np.array([BALL, AXIS, BALL, LOCK, BALL], dtype=np.int32),
                axis=np.array([[9.0, 9.0, 9.0], [0.0, 3.0, 4.0], [NAN, 0.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]]),
                q_rel=np.array([[0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0], [NAN, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]))


def test_the_entry_points_are_declared_exported_and_described():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    for name, value in (("RBL_JOINT_BALL", 0), ("RBL_JOINT_LOCK", 1), ("RBL_JOINT_AXIS", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == value
    for said in ("five-row hinge", "weld", "motor", "Omega_j", "theta_j += Omega_j dt", "the short way round", "IGNORED", "slider", "universal joint"):
        assert said in text, said


# ------------------------------------------------------------------------------------------------------------ 1: the C ABI
def test_set_get_round_trip_normalisation_and_the_switch():
    L = _lib()
    h = _context(L)
    g = _good()
    assert _set(L, h, g) == 0, L.rbl_last_error(h)
    o = _get(L, h)
    assert (o["n"], o["on"], o["by_kinds"]) == (5, 1, 1)
    assert np.array_equal(o["body"], g["body"]) and np.array_equal(o["kind"], g["kind"])
    ball = g["kind"] == BALL
    assert np.array_equal(o["anchor"][ball], g["anchor"][ball]) and not o["anchor"][~ball].any()      # anchors of angular joints: not read
    assert np.array_equal(o["axis"][1], [0.0, 0.6, 0.8]) and np.array_equal(o["axis"][3], [0.0, 0.0, 1.0])   # normalised
    assert np.array_equal(o["q_rel"][1], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(o["q_rel"][3], [0.5, 0.5, 0.5, 0.5])
    assert not o["axis"][ball].any() and np.array_equal(o["q_rel"][ball], np.tile([1.0, 0.0, 0.0, 0.0], (3, 1)))   # not read for a ball joint
    assert not o["theta"].any() and not o["rate"].any()
    # the ball-only getter serves the same set
    n, on = cint(0), cint(0)
    body = np.zeros((5, 2), dtype=np.int32)
    assert L.rbl_get_joints(h, ctypes.byref(n), ctypes.byref(on), body.ctypes.data, None) == 0 and n.value == 5 and np.array_equal(body, g["body"])
    # rates: stored, read back, cleared by the next set
    rate = np.array([0.0, 0.0, 0.0, 1.5, 0.0])
    assert L.rbl_set_joint_rates(h, rate.ctypes.data) == 0 and np.array_equal(_get(L, h)["rate"], rate)
    assert L.rbl_set_joint_kinds(h, 0, None, None, None, None, None, 0) == 0                              # only the switch
    o = _get(L, h)
    assert (o["n"], o["on"]) == (5, 0) and np.array_equal(o["rate"], rate)
    assert _set(L, h, g) == 0 and not _get(L, h)["rate"].any() and _get(L, h)["on"] == 1
    # rbl_set_joints replaces the set: it reads back as ball joints, by_kinds 0
    assert L.rbl_set_joints(h, 2, g["body"][[0, 4]].copy().ctypes.data, g["anchor"][[0, 4]].copy().ctypes.data, 1) == 0
    o = _get(L, h)
    assert (o["n"], o["by_kinds"]) == (2, 0) and not o["kind"].any() and np.array_equal(o["q_rel"], np.tile([1.0, 0.0, 0.0, 0.0], (2, 1)))
    # no ball joint: anchor may be NULL; no angular joint: axis and q_rel may be
    assert _set(L, h, dict(body=[[0, 1]], kind=[LOCK], axis=[[1.0, 0.0, 0.0]], q_rel=[[1.0, 0.0, 0.0, 0.0]])) == 0
    assert _set(L, h, dict(body=[[0, 1]], kind=[BALL], anchor=np.zeros((1, 6)))) == 0
    L.rbl_destroy(h)


def _variant(**change):
    g = _good()
    for k, (j, v) in change.items():
        g[k] = np.array(g[k])
        g[k][j] = v
    return g


REFUSED = [
    ("unknown kind 3", _variant(kind=(1, 3)), 1, "unknown kind"),
    ("unknown kind -1", _variant(kind=(4, -1)), 4, "unknown kind"),
    ("axis NaN", _variant(axis=(1, [0.0, NAN, 1.0])), 1, "axis"),
    ("axis inf", _variant(axis=(3, [INF, 0.0, 0.0])), 3, "axis"),
    ("axis too short", _variant(axis=(1, [1e-13, 0.0, 0.0])), 1, "axis"),
    ("q_rel zero", _variant(q_rel=(3, [0.0, 0.0, 0.0, 0.0])), 3, "q_rel"),
    ("q_rel NaN", _variant(q_rel=(1, [1.0, NAN, 0.0, 0.0])), 1, "q_rel"),
    ("A = B", _variant(body=(1, [1, 1])), 1, "one body"),
    ("A = -1", _variant(body=(3, [-1, 2])), 3, "second slot"),
    ("body out of range", _variant(body=(3, [4, -1])), 3, "out of range"),
    ("anchor NaN on a ball joint", _variant(anchor=(4, [0.0, NAN, 0.0, 0.0, 0.0, 0.0])), 4, "anchor"),
    ("a second angular joint on a pair", _variant(kind=(0, LOCK), axis=(0, [1.0, 0.0, 0.0]), q_rel=(0, [1.0, 0.0, 0.0, 0.0])), 1, "second angular"),
    ("a second angular joint to the lab", _variant(kind=(2, AXIS), axis=(2, [1.0, 0.0, 0.0]), q_rel=(2, [1.0, 0.0, 0.0, 0.0])), 3, "second angular"),
    ("a second angular joint, bodies swapped", _variant(body=(4, [1, 0]), kind=(4, LOCK), axis=(4, [1.0, 0.0, 0.0]), q_rel=(4, [1.0, 0.0, 0.0, 0.0])),
     4, "second angular"),
    ("angular + two balls", _variant(body=(4, [1, 0])), 4, "two ball joints"),
]


@pytest.mark.parametrize("label,bad,joint,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_refusal_names_its_joint_and_leaves_the_previous_set(label, bad, joint, word):
    L = _lib()
    h = _context(L)
    g = _good()
    assert _set(L, h, g) == 0
    rate = np.array([0.0, 0.0, 0.0, -0.5, 0.0])
    assert L.rbl_set_joint_rates(h, rate.ctypes.data) == 0
    before = _get(L, h)
    assert _set(L, h, bad) == ERR_ARG, label
    msg = L.rbl_last_error(h).decode()
    assert msg.startswith("set_joint_kinds: joint %d: " % joint) and word in msg, msg
    after = _get(L, h)
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    L.rbl_destroy(h)


def test_refusals_without_a_joint_index_and_of_the_rates():
    L = _lib()
    h = _context(L)
    g = _good()
    rate = np.zeros(5)
    assert L.rbl_set_joint_rates(h, rate.ctypes.data) == ERR_STATE and "no joints" in L.rbl_last_error(h).decode()
    assert _set(L, h, g) == 0
    before = _get(L, h)
    for label, s, n in (("NULL body", dict(g, body=None), 5), ("NULL kind", dict(g, kind=None), 5), ("n = 0", g, 0), ("n = 2049", g, 2049)):
        assert _set(L, h, s, n=n) == ERR_ARG and "set_joint_kinds" in L.rbl_last_error(h).decode(), label
    for label, s, joint in (("NULL anchor", dict(g, anchor=None), 0), ("NULL axis", dict(g, axis=None), 1), ("NULL q_rel", dict(g, q_rel=None), 1)):
        assert _set(L, h, s) == ERR_ARG and ("joint %d: " % joint) in L.rbl_last_error(h).decode(), label
    # three ball joints between one pair, as rbl_set_joints refuses them
    three = dict(body=[[0, 1], [1, 0], [0, 1]], kind=[BALL] * 3, anchor=np.zeros((3, 6)))
    assert _set(L, h, three) == ERR_ARG and "joint 2: a third joint" in L.rbl_last_error(h).decode()
    # rates: only a lock joint takes one; finite; nothing stored on a refusal
    for j, v, word in ((1, 0.5, "only a lock joint"), (0, -1.0, "only a lock joint"), (3, NAN, "finite"), (3, INF, "finite")):
        r = np.zeros(5)
        r[3] = 0.25
        r[j] = v
        assert L.rbl_set_joint_rates(h, r.ctypes.data) == ERR_ARG
        msg = L.rbl_last_error(h).decode()
        assert msg.startswith("set_joint_rates: joint %d: " % j) and word in msg, msg
    assert L.rbl_set_joint_rates(h, None) == ERR_ARG
    after = _get(L, h)
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    # the cap holds: 2048 joints are taken (ball joints body - lab would exceed two a body: 1024 bodies, two pivots each)
    nb = 1024
    L.rbl_destroy(h)
    h = _context(L, nb)
    body = np.array([[i // 2, -1] for i in range(2048)], dtype=np.int32)
    kind = np.array([BALL, LOCK] * 1024, dtype=np.int32)
    full = dict(body=body, kind=kind, anchor=np.zeros((2048, 6)), axis=np.tile([0.0, 0.0, 1.0], (2048, 1)), q_rel=np.tile([1.0, 0.0, 0.0, 0.0], (2048, 1)))
    assert _set(L, h, full) == 0 and _get(L, h)["n"] == 2048
    L.rbl_destroy(h)


def test_a_communicator_context_refuses_the_jointed_calls_with_kinds_set():
    """as with rbl_set_joints: the set is context state and is taken, the solve and the step are refused before any device work"""
    L = _lib()
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    L.rbl_solve_jointed.argtypes = L.rbl_solve_jointed_dev.argtypes = [vp, vp, vp, vp, cint, dbl, vp, vp, vp, ip, ctypes.POINTER(dbl)]
    L.rbl_step_jointed.argtypes = [vp, vp, vp, vp, dbl, cint, dbl, vp, ip, ctypes.POINTER(dbl)]
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = _context(L)
    assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    assert _set(L, h, _good()) == 0
    F, U, phi = np.zeros(24), np.zeros(24), np.zeros(15)
    it, res = cint(0), dbl(0.0)
    for f in (L.rbl_solve_jointed, L.rbl_solve_jointed_dev):
        assert f(h, F.ctypes.data, None, None, 50, 1e-8, None, U.ctypes.data, phi.ctypes.data, ctypes.byref(it), ctypes.byref(res)) == ERR_ARG
        assert b"communicator" in L.rbl_last_error(h)
    assert L.rbl_step_jointed(h, F.ctypes.data, None, None, 1.0, 50, 1e-8, phi.ctypes.data, ctypes.byref(it), ctypes.byref(res)) == ERR_ARG
    assert b"communicator" in L.rbl_last_error(h) and not _get(L, h)["theta"].any()
    L.rbl_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 2: the Python checks
class _NoLibrary:
    """stands where the extension object or the device context would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_the_python_checks_run_before_the_library_is_called():
    from rigid_body_light_amd import RigidBody
    from rigid_body_light_amd._lib import DeviceContext
    rb = RigidBody.__new__(RigidBody)
    rb.cb = rb.ctx = _NoLibrary()
    ctx = DeviceContext.__new__(DeviceContext)
    ctx.L = ctx.h = _NoLibrary()
    ok = dict(body=[[0, 1], [0, 1]], kind=[BALL, AXIS], anchor_a=np.zeros(3), anchor_b=np.zeros(3), axis=[0.0, 0.0, 1.0], q_rel=[1.0, 0.0, 0.0, 0.0])
    bad = [dict(ok, kind=[BALL, 3]), dict(ok, kind=[BALL]), dict(ok, kind=[0.0, 2.0]), dict(ok, body=[[0, 1, 2]]), dict(ok, body=[[0.5, 1], [0, 1]]),
           dict(ok, anchor_a=None), dict(ok, axis=None), dict(ok, axis=[0.0, 0.0, 0.0]), dict(ok, axis=[NAN, 0.0, 1.0]), dict(ok, axis=np.zeros((3, 3))),
           dict(ok, q_rel=[0.0, 0.0, 0.0, 0.0]), dict(ok, q_rel=np.ones(3)), dict(ok, anchor_b=[INF, 0.0, 0.0]), dict(ok, anchor_a=np.zeros((2, 2)))]
    for who in (rb, ctx):
        for kw in bad:
            with pytest.raises(ValueError, match="set_joint_kinds"):
                who.set_joint_kinds(**kw)
    with pytest.raises((ValueError, RuntimeError), match="finite"):
        rb.set_joint_rates([0.0, NAN])
    # the message names the joint
    with pytest.raises(ValueError, match="joint 1: axis"):
        rb.set_joint_kinds(**dict(ok, axis=[[1.0, 0.0, 0.0], [0.0, 0.0, 1e-13]]))
    with pytest.raises(ValueError, match="joint 1: unknown kind 7"):
        ctx.set_joint_kinds(**dict(ok, kind=[BALL, 7]))


def test_the_builders_make_the_oracle_s_rows():
    from rigid_body_light_amd import _lib as lib
    X, Q = jk.spread(3, seed=9)
    p, ax = jk.mid(X, 0, 1), [0.3, -0.5, 0.8]
    for mine, theirs in ((lib.hinge(X, Q, 0, 1, p, ax), jk.hinge(X, Q, 0, 1, p, ax)), (lib.weld(X, Q, 2, 1, p), jk.weld(X, Q, 2, 1, p)),
                         (lib.motor(X, Q, 1, -1, p, ax), jk.motor(X, Q, 1, -1, p, ax))):
        for k in ("body", "kind", "anchor_a", "anchor_b", "axis", "q_rel"):
            assert np.allclose(mine[k], theirs[k], rtol=0.0, atol=1e-14), k
    both = lib.joint_rows(lib.hinge(X, Q, 0, 1, p, ax), lib.weld(X, Q, 2, 1, p))
    assert both["body"].shape == (4, 2) and list(both["kind"]) == [BALL, AXIS, BALL, LOCK] and both["q_rel"].shape == (4, 4)
    b, k, anchor, axis, q_rel = lib.joint_kind_args("t", **both)
    assert b.dtype == np.int32 and k.dtype == np.int32 and anchor.shape == (4, 6) and not anchor[[1, 3]].any()
    for bad in (dict(a=0, b=0), dict(a=3, b=0), dict(a=-1, b=0)):
        with pytest.raises(ValueError, match="builder"):
            lib.hinge(X, Q, bad["a"], bad["b"], p, ax)
    with pytest.raises(ValueError, match="builder"):
        lib.motor(X, Q, 0, 1, p, [0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------------------ 3: the oracle
def test_J_is_the_rate_of_change_of_the_gaps_angular_rows_included():
    """d gap / dt = J U along the library's update (X += h u, Q <- exp(h w) Q) for small gaps, where de/dt = w_A - w_B holds to
    first order in e: gaps of the order 1e-3 leave a relative error of that order in the angular rows' rates, so those are
    compared at 5e-3 of the largest entry of J U; central differences with h = 1e-5 add 1e-8 (tests/test_joints_cpu.py)."""
    from oracle import oracle as O
    X, Q, r = jk.case_mixed42()
    r = jk.perturbed(jk.concat(jk.weld(X, Q, 0, 1, jk.mid(X, 0, 1)), jk.hinge(X, Q, 2, 1, jk.mid(X, 1, 2), [0.2, 0.9, -0.4]),
                               jk.motor(X, Q, 3, -1, X[3] + [0.3, 0.3, 0.5], [1.0, 0.1, 0.2])), 3, 1e-3)
    J = jk.J_matrix(X, Q, r)
    assert J.shape == (18, 24)
    rng = np.random.default_rng(9)
    h = 1e-5
    for _ in range(3):
        U = rng.standard_normal(24)
        g = []
        for s in (1.0, -1.0):
            Xs, Qs = O.evolve(X, Q, s * U, h)
            g.append(jk.geometry(Xs, Qs, r)[1].reshape(-1))
        fd = (g[0] - g[1]) / (2 * h)
        err = np.abs(fd - J @ U).max() / np.abs(J @ U).max()
        print("J U against central differences of the gaps: %.2e" % err)
        assert err <= 5e-3
    # at a closed joint the first-order statement is exact to the differences' own error
    X, Q = jk.spread(2, seed=1)
    r = jk.weld(X, Q, 0, 1, jk.mid(X, 0, 1))
    assert np.abs(jk.geometry(X, Q, r)[1]).max() <= 1e-14                     # rounding of coordinates of a few units
    U = rng.standard_normal(12)
    g = [jk.geometry(*O.evolve(X, Q, s * U, h), r)[1].reshape(-1) for s in (1.0, -1.0)]
    assert np.abs((g[0] - g[1]) / (2 * h) - jk.J_matrix(X, Q, r) @ U).max() <= 1e-8 * np.abs(U).max()


def test_the_motor_angle_enters_the_gap_with_its_sign():
    """theta > 0 moves the target of body B by +theta about ah: with B where it was, e = +theta ah; once B has turned by +theta
    about ah relative to A, e = 0"""
    X, Q, r = jk.case_motor(False)
    ah, gap = jk.geometry(X, Q, r, theta=[0.0, 0.3])
    assert np.allclose(gap[1], 0.3 * ah[1], rtol=0.0, atol=1e-15) and np.abs(jk.geometry(X, Q, r)[1][1]).max() <= 1e-15
    Q2 = np.array(Q)
    Q2[1] = jk.qmul(jk.qrot(0.3, ah[1]), Q[1])
    assert np.abs(jk.geometry(X, Q2, r, theta=[0.0, 0.3])[1][1]).max() <= 1e-15
    # the step's right-hand side asks for w_A - w_B = -rate ah: B turns at +rate about ah
    c = jk.step_rhs(X, Q, r, [0.0, 0.0], [0.0, 0.7], 1.0, 0.01, np.zeros(6)).reshape(-1, 3)
    assert np.allclose(c[1], -0.7 * ah[1], rtol=0.0, atol=1e-13)


def test_a_rigid_motion_of_a_welded_pair_lies_in_the_null_space_of_J():
    X, Q = jk.spread(2, seed=1)
    r = jk.weld(X, Q, 0, 1, jk.mid(X, 0, 1))                     # closed: both anchors are one lab point
    J = jk.J_matrix(X, Q, r)
    rng = np.random.default_rng(12)
    for _ in range(3):
        u, w = rng.standard_normal(3), rng.standard_normal(3)
        U = np.concatenate([u, w, u + np.cross(w, X[1] - X[0]), w])
        assert np.abs(J @ U).max() <= 1e-14 * np.abs(U).max() * 10
    assert np.linalg.matrix_rank(J) == 6                         # and nothing else does: six rows hold six relative coordinates
    # a hinge leaves exactly the rotation about its axis through its point
    X, Q, five, two = jk.case_hinge()
    J5 = jk.J_matrix(X, Q, five)[:6, :12]
    ah = jk.geometry(X, Q, five)[0][1]
    p = jk.mid(X, 0, 1)
    U = np.concatenate([np.zeros(6), np.cross(ah, X[1] - p), ah])
    assert np.abs(J5 @ U).max() <= 1e-14 and np.linalg.matrix_rank(J5) == 5
    assert np.abs(jo.J_matrix(X, Q, two["body"], jk.anchor6(two))[:6, :12] @ U).max() <= 1e-14     # the two-ball hinge on the same axis agrees


CASES = {"weld": lambda: jk.case_weld(), "hinge": lambda: jk.case_hinge()[:3], "motor": lambda: jk.case_motor(False),
         "motor_lab": lambda: jk.case_motor(True), "mixed42": jk.case_mixed42, "hub": jk.case_hub, "steps": jk.case_steps,
         "driven": jk.case_driven}


@pytest.mark.parametrize("wall", [False, True])
def test_the_dense_jointed_matrix_of_every_gpu_case_is_regular(orc, wall):
    """[M -K 0; K^T 0 J^T; 0 J -D] of every configuration of tests/test_joint_kinds_gpu.py, with D = sigma ah ah^T of the block
    preconditioner: full rank, and a condition number (2-norm, numpy.linalg.cond) far from the 1e16 of a singular matrix.  Without D
    the matrix of every case with an axis joint is singular: its smallest singular value is rounding.

    Recorded (free / wall): weld 2.86e2 / 2.85e2, hinge 2.92e2 / 3.29e2, motor 2.85e2 / 2.85e2, motor_lab 2.81e2 / 2.73e2,
    mixed42 1.13e3 / 1.30e3, hub 6.63e3 / 7.07e3, steps 2.99e2 / 2.99e2, driven 2.85e2 / 2.84e2 (orders 90 ... 1722).
    Asserted: below 1e6."""
    from rigid_body_light_amd import load_structure
    for name, make in CASES.items():
        X, Q, r = make()
        p, cfg = load_structure(42 if name == "mixed42" else 12)
        M, K = jo.dense_matrices(orc, cfg, X, Q, p["sep"] / 2.0, 1.0, wall)
        J = jk.J_matrix(X, Q, r)
        D = jk.D_matrix(X, Q, r, jo.pc_M(M, cfg.shape[0], True), K, cfg.shape[0])
        A = jk.jointed_matrix(M, K, J, D)
        cond = np.linalg.cond(A)
        print("%s wall=%s: order %d, cond %.2e" % (name, wall, A.shape[0], cond))
        assert np.isfinite(cond) and cond < 1e6, name
        S = jk.schur(M, K, J, D, cfg.shape[0], True)
        assert np.linalg.eigvalsh(0.5 * (S + S.T))[0] > 0.0, name
        if (r["kind"] == jk.AXIS).any():
            s = np.linalg.svd(jk.jointed_matrix(M, K, J, 0.0 * D), compute_uv=False)
            assert s[-1] <= 1e-12 * s[0], name
