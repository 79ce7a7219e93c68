"""Imposed flow, body-frame slip and first moments (include/rbl.h section 8), the parts that need no device: every entry point is
declared and exported, bad arguments are RBL_ERR_ARG and leave the previous model in place, the wall refusal and the n_scale
mismatch fire at the use before the device is touched, the state errors fire, record_moments is a named option, a box without a
device answers RBL_ERR_NO_DEVICE, and the Python wrappers reject bad shapes before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_set_background_flow", "rbl_set_body_slip", "rbl_get_flow_model", "rbl_flow_slip_dev", "rbl_flow_slip",
         "rbl_ensemble_flow_slip", "rbl_first_moments_dev", "rbl_first_moments", "rbl_step_moments", "rbl_ensemble_step_moments")
OK, ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 0, 5, 7, 11
NBLB = 4


def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    vp, dbl, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    ip, dp = ctypes.POINTER(ci), ctypes.POINTER(dbl)
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, ci]
    L.rbl_set_wall_pc.argtypes = [vp, ci]
    L.rbl_set_config.argtypes = [vp, vp, vp, ci]
    L.rbl_set_K_mats.argtypes = [vp]
    L.rbl_step_deterministic.argtypes = [vp, vp, vp, ci, dbl, ci, ip, dp]
    L.rbl_step_mixed.argtypes = [vp, vp, vp, vp, ci, dbl, vp, ip, dp]
    L.rbl_set_background_flow.argtypes = [vp, vp, vp, ci]
    L.rbl_set_body_slip.argtypes = [vp, vp, vp, ci, ci]
    L.rbl_get_flow_model.argtypes = [vp, vp, ip, ip]
    for n in ("rbl_flow_slip_dev", "rbl_flow_slip", "rbl_ensemble_flow_slip", "rbl_step_moments", "rbl_ensemble_step_moments"):
        getattr(L, n).argtypes = [vp, vp]
    L.rbl_first_moments_dev.argtypes = L.rbl_first_moments.argtypes = [vp, vp, vp]
    L.rbl_set_option.argtypes = [vp, ci, ctypes.c_int64]
    L.rbl_get_option.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_int64)]
    L.rbl_option_info.argtypes = [ci, ctypes.POINTER(ctypes.c_char_p)] + [ctypes.POINTER(ctypes.c_int64)] * 3
    L.rbl_option_key.argtypes = [ctypes.c_char_p]
    return L


def _no_device():
    import torch
    return torch.cuda.device_count() == 0


def _context(L, nb=3, wall=False, config=True):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, 0.01, 1.0, 1.0, cfg.ctypes.data, NBLB) == OK
    assert L.rbl_set_wall_pc(h, int(wall)) == OK
    if config:
        X = np.arange(3.0 * nb).reshape(nb, 3) * 3.0 + np.array([0.0, 0.0, 3.0])
        Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
        assert L.rbl_set_config(h, X.ctypes.data, Q.ctypes.data, nb) == OK
        assert L.rbl_set_K_mats(h) == OK
    return h


def _model(L, h):
    v, f, b = np.full(12, np.nan), ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.rbl_get_flow_model(h, v.ctypes.data, ctypes.byref(f), ctypes.byref(b)) == OK
    return v, f.value, b.value


def test_every_entry_point_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    assert "8. Imposed flow and active slip" in text
    for said in ("M lambda - K U = slip", "drift", "q^{n+1/2}", "not linear in r", "n_scale"):    # conventions and scope are written down
        assert said in text, said


def test_bad_arguments_leave_the_previous_model_in_place():
    L = _lib()
    h = _context(L)
    u0, G = np.array([0.1, 0.2, 0.3]), np.arange(9.0)
    assert L.rbl_set_background_flow(None, u0.ctypes.data, G.ctypes.data, 1) == ERR_ARG
    assert L.rbl_set_background_flow(h, u0.ctypes.data, G.ctypes.data, 1) == OK
    v, f, b = _model(L, h)
    assert np.array_equal(v, np.concatenate([u0, G])) and (f, b) == (1, 0)
    assert L.rbl_set_background_flow(h, None, G.ctypes.data, 1) == ERR_ARG
    assert L.rbl_set_background_flow(h, u0.ctypes.data, None, 1) == ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            ub = np.zeros(3); ub[k] = bad
            assert L.rbl_set_background_flow(h, ub.ctypes.data, G.ctypes.data, 0) == ERR_ARG
        for k in range(9):
            Gb = np.zeros(9); Gb[k] = bad
            assert L.rbl_set_background_flow(h, u0.ctypes.data, Gb.ctypes.data, 0) == ERR_ARG
            assert b"finite" in L.rbl_last_error(h)
    v, f, b = _model(L, h)
    assert np.array_equal(v, np.concatenate([u0, G])) and (f, b) == (1, 0)                # nothing moved, still on
    assert L.rbl_set_background_flow(h, u0.ctypes.data, G.ctypes.data, 0) == OK
    assert _model(L, h)[1:] == (0, 0)
    # the pattern
    s, sc = np.ones(3 * NBLB), np.array([1.0, 0.0, 2.0])
    assert L.rbl_set_body_slip(None, s.ctypes.data, None, 0, 1) == ERR_ARG
    assert L.rbl_set_body_slip(h, None, None, 0, 1) == ERR_ARG
    assert L.rbl_set_body_slip(h, s.ctypes.data, sc.ctypes.data, 0, 1) == ERR_ARG
    assert _model(L, h)[2] == 0
    assert L.rbl_set_body_slip(h, s.ctypes.data, sc.ctypes.data, 3, 1) == OK
    sb = s.copy(); sb[5] = np.nan
    assert L.rbl_set_body_slip(h, sb.ctypes.data, None, 0, 0) == ERR_ARG
    scb = sc.copy(); scb[1] = np.inf
    assert L.rbl_set_body_slip(h, s.ctypes.data, scb.ctypes.data, 3, 0) == ERR_ARG
    assert _model(L, h)[2] == 1                                                            # the failed sets did not switch it off
    assert L.rbl_get_flow_model(None, None, None, None) == ERR_ARG
    assert L.rbl_get_flow_model(h, None, None, None) == OK                                 # any pointer may be NULL
    # the queries and the moments
    out, lam, D = np.zeros(3 * 3 * NBLB), np.zeros(3 * 3 * NBLB), np.zeros(27)
    for fn in (L.rbl_flow_slip, L.rbl_flow_slip_dev, L.rbl_ensemble_flow_slip, L.rbl_step_moments, L.rbl_ensemble_step_moments):
        assert fn(None, out.ctypes.data) == ERR_ARG
    for fn in (L.rbl_flow_slip, L.rbl_flow_slip_dev, L.rbl_step_moments, L.rbl_ensemble_step_moments):
        assert fn(h, None) == ERR_ARG
    for fn in (L.rbl_first_moments, L.rbl_first_moments_dev):
        assert fn(None, lam.ctypes.data, D.ctypes.data) == ERR_ARG
        assert fn(h, None, D.ctypes.data) == ERR_ARG
        assert fn(h, lam.ctypes.data, None) == ERR_ARG
    L.rbl_destroy(h)


def test_state_errors():
    L = _lib()
    h = L.rbl_create()
    s = np.ones(3 * NBLB)
    assert L.rbl_set_body_slip(h, s.ctypes.data, None, 0, 1) == ERR_STATE and b"setParameters" in L.rbl_last_error(h)
    out = np.zeros(64)
    assert L.rbl_flow_slip(h, out.ctypes.data) == ERR_STATE
    assert L.rbl_first_moments(h, out.ctypes.data, out.ctypes.data) == ERR_STATE
    L.rbl_destroy(h)
    h = _context(L, config=False)
    assert L.rbl_flow_slip(h, out.ctypes.data) == ERR_STATE                               # parameters, no configuration
    assert L.rbl_ensemble_flow_slip(h, out.ctypes.data) == ERR_STATE                      # no ensemble
    L.rbl_destroy(h)
    # nothing recorded: before the option, after the option, and again after the option is set once more
    h = _context(L)
    D = np.zeros(27)
    key = L.rbl_option_key(b"record_moments")
    assert L.rbl_step_moments(h, D.ctypes.data) == ERR_STATE and b"record" in L.rbl_last_error(h)
    assert L.rbl_ensemble_step_moments(h, D.ctypes.data) == ERR_STATE
    assert L.rbl_set_option(h, key, 1) == OK
    assert L.rbl_step_moments(h, D.ctypes.data) == ERR_STATE
    assert L.rbl_ensemble_step_moments(h, D.ctypes.data) == ERR_STATE
    L.rbl_destroy(h)


def test_record_moments_is_a_named_option():
    L = _lib()
    key = L.rbl_option_key(b"record_moments")
    assert key > 0
    nm, lo, hi, df = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.rbl_option_info(key, ctypes.byref(nm), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(df)) == OK
    assert (nm.value, lo.value, hi.value, df.value) == (b"record_moments", 0, 1, 0)
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    assert re.search(r"RBL_OPT_RECORD_MOMENTS\s*=\s*%d\b" % key, text)
    h = L.rbl_create()
    v = ctypes.c_int64(-1)
    assert L.rbl_get_option(h, key, ctypes.byref(v)) == OK and v.value == 0
    assert L.rbl_set_option(h, key, 1) == OK and L.rbl_get_option(h, key, ctypes.byref(v)) == OK and v.value == 1
    assert L.rbl_set_option(h, key, 2) == ERR_ARG
    L.rbl_destroy(h)


def _uses(L, h, nb):
    """every kind of use that can run without an ensemble: the two queries, a plain step, a mixed step -> their status codes.
    (The device form is handed a host array, so it is only called where it cannot get as far as writing to it.)"""
    out = np.zeros(3 * nb * NBLB)
    F, mask = np.zeros(6 * nb), np.zeros(nb, dtype=np.uint8)
    it, res = ctypes.c_int(0), ctypes.c_double(0.0)
    query_dev = L.rbl_flow_slip_dev if _no_device() else L.rbl_flow_slip
    return [L.rbl_flow_slip(h, out.ctypes.data),
            query_dev(h, out.ctypes.data),
            L.rbl_step_deterministic(h, F.ctypes.data, None, 50, 1e-8, 0, ctypes.byref(it), ctypes.byref(res)),
            L.rbl_step_mixed(h, mask.ctypes.data, F.ctypes.data, None, 50, 1e-8, None, ctypes.byref(it), ctypes.byref(res))]


def _G(i, j, v=0.5):
    G = np.zeros(9)
    G[3 * i + j] = v
    return G


def test_wall_refusal_fires_at_every_use_before_the_device():
    """with the wall flag only u = (G02 z, G12 z, 0) vanishes at z = 0: u0, the lateral gradients G[.][0], G[.][1] and G22 are
    RBL_ERR_ARG at a query and at a step -- on a box without a device too, where a call that reached the device answers
    RBL_ERR_NO_DEVICE"""
    L = _lib()
    nb = 3
    zero3, zero9 = np.zeros(3), np.zeros(9)
    offending = [(np.eye(3)[k] * 0.3, zero9) for k in range(3)]
    offending += [(zero3, _G(i, j)) for i in range(3) for j in range(2)] + [(zero3, _G(2, 2))]
    for wall in (True, False):
        h = _context(L, nb, wall=wall)
        for u0, G in offending:
            assert L.rbl_set_background_flow(h, u0.ctypes.data, G.ctypes.data, 1) == OK      # the set accepts it: the use refuses
            codes = _uses(L, h, nb)
            if wall:
                assert codes == [ERR_ARG] * 4, (u0, G, codes)
                assert b"z = 0" in L.rbl_last_error(h)
            else:                                                                               # free space: any G
                assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in codes), (u0, G, codes)
        for G in (_G(0, 2), _G(1, 2), _G(0, 2) + _G(1, 2, -0.7)):
            assert L.rbl_set_background_flow(h, zero3.ctypes.data, G.ctypes.data, 1) == OK
            codes = _uses(L, h, nb)
            assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in codes), (wall, G, codes)
        # switched off, an offending flow is no flow
        assert L.rbl_set_background_flow(h, offending[0][0].ctypes.data, zero9.ctypes.data, 0) == OK
        codes = _uses(L, h, nb)
        assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in codes), codes
        L.rbl_destroy(h)


def test_n_scale_mismatch_is_refused_at_the_use():
    L = _lib()
    nb = 3
    h = _context(L, nb)
    s = np.ones(3 * NBLB)
    for n in (2, 4):
        sc = np.ones(n)
        assert L.rbl_set_body_slip(h, s.ctypes.data, sc.ctypes.data, n, 1) == OK              # not at the set
        assert _uses(L, h, nb) == [ERR_ARG] * 4
        assert b"n_scale" in L.rbl_last_error(h)
    sc = np.ones(nb)
    assert L.rbl_set_body_slip(h, s.ctypes.data, sc.ctypes.data, nb, 1) == OK
    assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in _uses(L, h, nb))
    assert L.rbl_set_body_slip(h, s.ctypes.data, None, 0, 1) == OK                             # NULL: 1 for every body, any count
    assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in _uses(L, h, nb))
    L.rbl_destroy(h)


def test_a_pattern_goes_stale_with_the_structure():
    """the pattern belongs to the structure: after another rbl_set_parameters -- even one with the same blob count -- a pattern
    that is still on is RBL_ERR_STATE at every use until it is set again"""
    L = _lib()
    nb = 3
    h = _context(L, nb)
    s = np.ones(3 * NBLB)
    assert L.rbl_set_body_slip(h, s.ctypes.data, None, 0, 1) == OK
    cfg = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]) * 0.6          # another structure of four blobs
    assert L.rbl_set_parameters(h, 0.25, 0.01, 1.0, 1.0, cfg.ctypes.data, NBLB) == OK
    assert L.rbl_set_K_mats(h) == OK
    assert _uses(L, h, nb) == [ERR_STATE] * 4 and b"rbl_set_body_slip" in L.rbl_last_error(h)
    assert L.rbl_set_body_slip(h, s.ctypes.data, None, 0, 0) == OK                         # switched off: nothing to refuse
    assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in _uses(L, h, nb))
    assert L.rbl_set_body_slip(h, s.ctypes.data, None, 0, 1) == OK                         # set again for this structure
    assert all(c == (ERR_NO_DEVICE if _no_device() else OK) for c in _uses(L, h, nb))
    L.rbl_destroy(h)


def test_valid_calls_without_a_device_fail_loudly():
    if not _no_device():
        return                                               # a device is present: tests/test_flow_gpu.py covers the calls
    L = _lib()
    nb = 3
    h = _context(L, nb)
    out, lam, D = np.zeros(3 * nb * NBLB), np.zeros(3 * nb * NBLB), np.zeros(9 * nb)
    assert L.rbl_flow_slip(h, out.ctypes.data) == ERR_NO_DEVICE and b"no CPU fallback" in L.rbl_last_error(h)   # both parts off too
    G = _G(0, 2)
    assert L.rbl_set_background_flow(h, np.zeros(3).ctypes.data, G.ctypes.data, 1) == OK
    assert L.rbl_flow_slip(h, out.ctypes.data) == ERR_NO_DEVICE
    assert L.rbl_flow_slip_dev(h, out.ctypes.data) == ERR_NO_DEVICE
    assert L.rbl_first_moments(h, lam.ctypes.data, D.ctypes.data) == ERR_NO_DEVICE
    assert L.rbl_first_moments_dev(h, lam.ctypes.data, D.ctypes.data) == ERR_NO_DEVICE
    L.rbl_destroy(h)


class _NoLibrary:
    """stands where the extension object or the context would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _wrapper(nb=4, nblb=2):
    from rigid_body_light_amd import RigidBody
    rb = RigidBody.__new__(RigidBody)
    rb.cb = rb.ctx = _NoLibrary()          # the extension object and the view of its context
    rb.N_bodies, rb.blobs_per_body, rb.total_blobs = nb, nblb, nb * nblb
    rb.X_shape, rb.Q_shape = (nb, 3), (nb, 4)
    rb._wall = False
    return rb


def test_rigid_body_shape_errors_raise_before_the_library():
    rb = _wrapper()
    for u0, G in ((np.zeros(2), None), (np.zeros((3, 1)), None), (None, np.zeros(9)), (None, np.zeros((3, 2))), (np.zeros(4), np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            rb.set_background_flow(u0, G)
    for sb, sc in ((np.zeros(5), None), (np.zeros((3, 2)), None), (np.zeros((2, 3, 1)), None), (np.zeros((2, 3)), np.zeros(3)),
                   (np.zeros(6), np.zeros((4, 1))), (np.zeros(6), np.zeros(5))):
        with pytest.raises(ValueError):
            rb.set_body_slip(sb, sc)
    for lam in (np.zeros(23), np.zeros((7, 3)), np.zeros(0)):
        with pytest.raises(ValueError):
            rb.first_moments(lam)
        with pytest.raises(ValueError):
            rb.stresslets(lam)
    with pytest.raises(ValueError):
        rb.velocity_field(np.zeros((4, 2)), np.zeros(24), with_flow=True)
    # good arguments reach the library in the C layout
    seen = {}

    class _Record:
        def set_background_flow(self, u0, G, on):
            seen["flow"] = (u0, G, on)

        def set_body_slip(self, sb, sc, on):
            seen["slip"] = (sb, sc, on)

        def first_moments(self, lam):
            seen["lam"] = lam
            return np.arange(36.0)
    rb.ctx = _Record()
    rb.set_background_flow(G=np.arange(9.0).reshape(3, 3), on=False)
    assert seen["flow"][0].tolist() == [0, 0, 0] and seen["flow"][1].reshape(-1).tolist() == list(range(9)) and seen["flow"][1].flags.c_contiguous and seen["flow"][2] is False
    rb.set_body_slip(np.arange(6.0).reshape(2, 3), scale=[1, 0, 2, 3])
    assert seen["slip"][0].shape == (6,) and seen["slip"][1].tolist() == [1, 0, 2, 3] and seen["slip"][2] is True
    D = rb.first_moments(np.zeros((8, 3)))
    assert seen["lam"].shape == (24,) and D.shape == (4, 3, 3)
    S = rb.stresslets(np.zeros(24))
    assert np.allclose(S, S.transpose(0, 2, 1)) and np.allclose(np.trace(S, axis1=1, axis2=2), 0.0)


def test_ensemble_shape_errors_raise_before_the_library():
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.ctx = _NoLibrary()
    e.R, e.N_bodies, e.blobs_per_body = 3, 4, 2
    for u0, G in ((np.zeros(2), None), (None, np.zeros(9)), (None, np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            e.set_background_flow(u0, G)
    for sb, sc in ((np.zeros(5), None), (np.zeros((3, 2)), None), (np.zeros(6), np.zeros(3)), (np.zeros(6), np.zeros((3, 4)))):
        with pytest.raises(ValueError):
            e.set_body_slip(sb, sc)


def test_rigid_alias_exposes_the_new_methods():
    from Rigid import RigidBody
    for name in ("set_background_flow", "set_body_slip", "flow_model", "flow_slip", "first_moments", "stresslets", "record_moments",
                 "step_moments"):
        assert callable(getattr(RigidBody, name, None)), name
