"""The Brownian midpoint step with prescribed velocity components (include/rbl.h sections 5 and 7: rbl_RHS_and_Midpoint_mixed_dof,
rbl_RHS_and_Midpoint_mixed_dof_dev, rbl_step_brownian_mixed_dof, rbl_ensemble_step_brownian_mixed_dof), the parts that need no
device: the entry points are declared and exported; every refusal is RBL_ERR_ARG before any device work -- those of the whole-body
Brownian calls, those of the _dof calls, and the rule that is new here: in every body's row of prescribed6 the three rotation
entries are all 0 or all 1; the Python layer repeats that rule with the library's wording before the library is called; and the
block structure of K^T K that the rule's argument rests on.  Modelled on test_brownian_mixed_cpu.py and test_ensemble_dof_cpu.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_RHS_and_Midpoint_mixed_dof", "rbl_RHS_and_Midpoint_mixed_dof_dev", "rbl_step_brownian_mixed_dof")
ENS = "rbl_ensemble_step_brownian_mixed_dof"
ERR_SIZE, ERR_NO_DEVICE, ERR_STATE, ERR_ARG = 4, 5, 7, 11
# the rotation entries (3..5) of an inadmissible row: one or two of the three set
PARTIAL = [r for r in itertools.product((0, 1), repeat=3) if 0 < sum(r) < 3]
SAID = b"the rotation is partly prescribed"


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
    L.rbl_RHS_and_Midpoint_mixed_dof.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, vp, vp, vp]
    L.rbl_RHS_and_Midpoint_mixed_dof_dev.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, vp, vp, vp]
    L.rbl_step_brownian_mixed_dof.argtypes = [vp, vp, vp, vp, vp, u64, ci, ci, dbl, ci, dbl, vp, ip, dp]
    L.rbl_ensemble_step_brownian_mixed_dof.argtypes = [vp, vp, vp, vp, vp, u64, ci, dbl, ci, dbl, vp, vp, vp]
    return L


def test_the_entry_points_are_declared_and_exported_and_the_class_is_written_down():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES + (ENS,):
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed6" % n, code), n
        assert hasattr(L, n), n
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    assert re.search(r"\bint\s+%s\s*\(" % ENS, re.sub(r"/\*.*?\*/", "", sec5, flags=re.S))       # declared in section 5
    for said in ("all 0 or all 1", "(K D_f)^+ = D_f Kinv", "subset of the coordinates", "partly prescribed rotation"):
        assert said in text, said
    not_offered = text.split("Not offered:")[-1].split("*/")[0]
    assert "partly prescribed rotation" in not_offered and "rbl_ensemble_run" in not_offered and "follow-up" in not_offered
    assert "rbl_step_brownian_mixed takes whole bodies only" not in text
    assert "There is no Brownian step with component masks" not in text


def _context(L, nb=3, dt=0.01, kBT=1.0):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5     # a tetrahedron
    assert L.rbl_set_parameters(h, 0.25, dt, kBT, 1.0, cfg.ctypes.data, 4) == 0
    X = np.arange(3.0 * nb).reshape(nb, 3) * 3.0
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    assert L.rbl_set_config(h, X.ctypes.data, Q.ctypes.data, nb) == 0
    assert L.rbl_set_K_mats(h) == 0
    return h


class _Calls:
    """the three single-context entry points on one context and one set of good arguments, each changeable by keyword"""
    def __init__(self, L, h, nb):
        self.L, self.h, self.nb = L, h, nb
        mask = np.zeros((nb, 6), dtype=np.uint8)
        mask[:, 2] = 1                                     # z of every body: admissible
        mask[1, 3:] = 1                                    # and the rotation of one
        self.keep = [mask, np.zeros(6 * nb), np.zeros(6 * nb), np.zeros(3 * nb * 4), np.zeros(3 * nb), np.zeros(4 * nb)]
        self.it, self.res = ctypes.c_int(0), ctypes.c_double(0.0)
        self.m, self.b, self.f = (v.ctypes.data for v in self.keep[:3])
        self.out = tuple(v.ctypes.data for v in self.keep[3:])

    def step(self, hh=0, mm=0, bb=0, delta=1e-4, mi=50, rt=1e-8):
        hh, mm, bb = (self.h if hh == 0 else hh), (self.m if mm == 0 else mm), (self.b if bb == 0 else bb)
        return self.L.rbl_step_brownian_mixed_dof(hh, mm, bb, None, None, 0, 0, 1, delta, mi, rt, self.f, ctypes.byref(self.it),
                                                  ctypes.byref(self.res))

    def rhs(self, name, hh=0, mm=0, bb=0, delta=1e-4, oo=None):
        hh, mm, bb = (self.h if hh == 0 else hh), (self.m if mm == 0 else mm), (self.b if bb == 0 else bb)
        return getattr(self.L, name)(hh, mm, bb, None, None, 0, 0, 1, delta, *(self.out if oo is None else oo))

    def all(self, **kw):
        """(entry point's name in messages, status) of the three on the same changed arguments, one call at a time: the context's
        last error is the yielded call's"""
        yield b"step_brownian_mixed_dof", self.step(**kw)
        for n in NAMES[:2]:
            yield n[4:].encode(), self.rhs(n, **kw)


def test_the_refusals_of_the_whole_body_brownian_calls_and_of_the_dof_calls():
    """every refusal below must come back as RBL_ERR_ARG on a box WITHOUT a device too: a call that touched the device first would
    answer RBL_ERR_NO_DEVICE there"""
    import torch
    L = _lib()
    nb = 3
    h = _context(L, nb)
    c = _Calls(L, h, nb)
    err = lambda: L.rbl_last_error(h)
    for name, rc in c.all(hh=None):
        assert rc == ERR_ARG
    for name, rc in c.all(mm=None):
        assert rc == ERR_ARG and b"NULL" in err()
    for name, rc in c.all(bb=None):
        assert rc == ERR_ARG
    bad = np.zeros((nb, 6), dtype=np.uint8)
    bad[1, 0] = 2
    for name, rc in c.all(mm=bad.ctypes.data):
        assert rc == ERR_ARG and b"0 or 1" in err()
    for mi in (0, -3, 255):                                # no restart: at most 254 iterations
        assert c.step(mi=mi) == ERR_ARG
    for rt in (-1.0, float("nan")):
        assert c.step(rt=rt) == ERR_ARG
    for delta in (0.0, -1e-4, float("nan")):
        for name, rc in c.all(delta=delta):
            assert rc == ERR_ARG and b"delta" in err() and name in err()
    for n in NAMES[:2]:
        for k in range(3):
            assert c.rhs(n, oo=tuple(None if j == k else o for j, o in enumerate(c.out))) == ERR_ARG and b"NULL" in err()
    # dt <= 0 with kBT > 0
    h0 = _context(L, nb, dt=0.0)
    for name, rc in c.all(hh=h0):
        assert rc == ERR_ARG and b"dt" in L.rbl_last_error(h0)
    L.rbl_destroy(h0)
    # no configuration yet: RBL_ERR_STATE, as the other solvers
    h2 = L.rbl_create()
    assert c.step(hh=h2) == ERR_STATE and c.rhs(NAMES[0], hh=h2) == ERR_STATE
    L.rbl_destroy(h2)
    # a context with a communicator: RBL_ERR_ARG from all three
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L, nb)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    for name, rc in c.all(hh=h3):
        assert rc == ERR_ARG and b"communicator" in L.rbl_last_error(h3)
    L.rbl_destroy(h3)
    # kBT = 0 is rbl_step_mixed_dof: its refusals, and no quarrel with delta
    h4 = _context(L, nb, kBT=0.0)
    assert c.step(hh=h4, mi=0) == ERR_ARG and c.step(hh=h4, mm=None) == ERR_ARG
    if torch.cuda.device_count() == 0:
        assert c.step(hh=h4, delta=0.0) == ERR_NO_DEVICE
    L.rbl_destroy(h4)
    if torch.cuda.device_count() == 0:                     # good arguments, no device: loud
        for name, rc in c.all():
            assert rc == ERR_NO_DEVICE and b"no CPU fallback" in err()
    L.rbl_destroy(h)


@pytest.mark.parametrize("body", [0, 2, 4])                # the first, a middle and the last of five bodies
@pytest.mark.parametrize("rot", PARTIAL)
def test_a_partly_prescribed_rotation_is_refused_and_named(rot, body):
    import torch
    L = _lib()
    nb = 5
    h = _context(L, nb)
    c = _Calls(L, h, nb)
    mask = np.zeros((nb, 6), dtype=np.uint8)
    mask[:, 2] = 1
    mask[body, 3:] = rot
    mask[body, :3] = np.random.default_rng(sum(rot) + body).integers(0, 2, 3)      # the translation entries do not matter
    if body < nb - 1:
        mask[nb - 1, 3:] = [1, 0, 1]                        # a later offender: the FIRST one is named
    for name, rc in c.all(mm=mask.ctypes.data):
        msg = L.rbl_last_error(h)
        assert rc == ERR_ARG, (name, rc, msg)
        assert msg.startswith(name + b": body %d: " % body) and SAID in msg and b"all 0 or all 1" in msg and b"not been derived" in msg
    # the same refusal whatever kBT is: the entry points' masks are one class
    h0 = _context(L, nb, kBT=0.0)
    assert c.step(hh=h0, mm=mask.ctypes.data) == ERR_ARG and SAID in L.rbl_last_error(h0)
    L.rbl_destroy(h0)
    # an entry above 1 is the older refusal and comes first
    two = mask.copy()
    two[0, 0] = 3
    assert c.step(mm=two.ctypes.data) == ERR_ARG and b"0 or 1" in L.rbl_last_error(h)
    # the repaired mask passes every argument check: what is left is the missing device (or, with one, nothing)
    mask[:, 3:] = mask[:, 3:4]
    for name, rc in c.all(mm=mask.ctypes.data):
        assert rc == (ERR_NO_DEVICE if torch.cuda.device_count() == 0 else 0), (name, rc, L.rbl_last_error(h))
    L.rbl_destroy(h)


def test_admissible_masks_reach_the_state_error_not_the_argument_error():
    L = _lib()
    h = L.rbl_create()                                     # no parameters, no configuration
    c = _Calls(L, h, 3)
    for name, rc in c.all():
        assert rc == ERR_STATE
    L.rbl_destroy(h)


def test_the_ensemble_entry_point_refuses_before_a_device_is_touched():
    """what needs no ensemble configuration (an entry above 1 and the rotation rule are counted from the ensemble's R and N_bod,
    hence need one and a device: test_brownian_dof_gpu.py)"""
    from rigid_body_light_amd import load_structure
    L = _lib()
    p, cfg = load_structure(12)
    cfg = np.ascontiguousarray(cfg, dtype=np.float64)

    def ctx(kBT=1.0, dt=0.01):
        h = L.rbl_create()
        assert L.rbl_set_parameters(h, p["sep"] / 2.0, dt, kBT, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
        return h
    mask, bi, F = np.zeros(48, dtype=np.uint8), np.zeros(48), np.zeros(48)
    it, res = np.zeros(4, dtype=np.int32), np.zeros(4)

    def call(h, m=mask, b=bi, delta=1e-4, mi=10, rt=1e-8):
        rc = L.rbl_ensemble_step_brownian_mixed_dof(h, None if m is None else m.ctypes.data, None if b is None else b.ctypes.data, None,
                                                    None, 0, 1, delta, mi, rt, F.ctypes.data, it.ctypes.data, res.ctypes.data)
        return rc, (L.rbl_last_error(h) if h else b"")
    who = b"ensemble_step_brownian_mixed_dof"
    h = ctx()
    assert call(None)[0] == ERR_ARG
    rc, msg = call(h, m=None)
    assert rc == ERR_ARG and b"NULL" in msg and who in msg and b"prescribed6" in msg
    rc, msg = call(h, b=None)
    assert rc == ERR_ARG and b"NULL" in msg and who in msg
    for mi in (0, -3):
        rc, msg = call(h, mi=mi)
        assert rc == ERR_ARG and b"max_iter" in msg and who in msg
    for rt in (-1.0, float("nan")):
        rc, msg = call(h, rt=rt)
        assert rc == ERR_ARG and b"rtol" in msg and who in msg
    rc, msg = call(h, mi=256)
    assert rc == ERR_SIZE and b"max_iter <= 255" in msg and who in msg
    rc, msg = call(h)
    assert rc == ERR_STATE and b"no ensemble configuration" in msg and who in msg
    L.rbl_destroy(h)
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = ctx()
    assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    rc, msg = call(h)
    assert rc == ERR_ARG and b"communicator" in msg and who in msg
    L.rbl_destroy(h)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------

class _NoLibrary:
    """stands where the extension object or the device context would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _wrapper(nb=5, nblb=2):
    from rigid_body_light_amd import RigidBody
    rb = RigidBody.__new__(RigidBody)
    rb.cb = rb.ctx = _NoLibrary()          # the extension object and the view of its context
    rb.N_bodies, rb.blobs_per_body, rb.total_blobs = nb, nblb, nb * nblb
    rb.X_shape, rb.Q_shape = (nb, 3), (nb, 4)
    return rb


def _c_message(who, mask):
    """the library's own refusal of this mask (a context with a configuration, no device needed)"""
    L = _lib()
    nb = mask.shape[0]
    h = _context(L, nb)
    c = _Calls(L, h, nb)
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    rc = c.step(mm=m.ctypes.data) if who == "step_brownian_mixed_dof" else c.rhs("rbl_" + who, mm=m.ctypes.data)
    msg = L.rbl_last_error(h).decode()
    L.rbl_destroy(h)
    assert rc == ERR_ARG
    return msg


@pytest.mark.parametrize("body", [0, 2, 4])
@pytest.mark.parametrize("rot", PARTIAL)
def test_wrapper_refuses_a_partly_prescribed_rotation_with_the_librarys_words(rot, body):
    rb = _wrapper()
    bi = np.zeros(30)
    mask = np.zeros((5, 6), dtype=bool)
    mask[:, 2] = True
    mask[body, 3:] = rot
    for who, fn in (("step_brownian_mixed_dof", rb.step_brownian_mixed_dof), ("RHS_and_Midpoint_mixed_dof", rb.RHS_and_Midpoint_mixed_dof)):
        with pytest.raises(ValueError) as e:
            fn(mask, bi)
        assert str(e.value) == _c_message(who, mask)
        assert ("%s: body %d: the rotation is partly prescribed" % (who, body)) in str(e.value)


def test_wrapper_rejects_bad_shapes_and_passes_admissible_masks_on():
    rb = _wrapper()
    bi = np.zeros(30)
    good = np.zeros((5, 6), dtype=bool)
    good[:, 2] = True
    good[3, 3:] = True
    good[4, :3] = True
    for fn in (rb.step_brownian_mixed_dof, rb.RHS_and_Midpoint_mixed_dof):
        for bad in (np.zeros(5, dtype=bool), np.zeros((5, 6), dtype=np.uint8), np.zeros((4, 6), dtype=bool), [0, 1], np.zeros((6, 5), dtype=bool)):
            with pytest.raises(ValueError):
                fn(bad, bi)
        with pytest.raises(ValueError):
            fn(good, np.zeros(29))
        with pytest.raises(ValueError):
            fn(good, bi, slip=np.zeros(7))
        with pytest.raises(ValueError):
            fn(good, bi, W=np.zeros(30))                   # W is [W1 | W2 | W_rfd]: 9 N_blobs = 90 numbers
    seen = {}

    class _Record:
        def step_brownian_mixed_dof(self, mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol):
            seen["step"] = (mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol)
            return "stepped"

        def RHS_and_Midpoint_mixed_dof(self, mask, body_in, slip, W, seed, method, split_rand, delta):
            seen["rhs"] = (mask, body_in, slip, W, seed, method, split_rand, delta)
            return "rhs"
    rb.ctx = _Record()
    assert rb.step_brownian_mixed_dof(good, bi.reshape(5, 6), W=np.zeros((3, 30)), seed=5, max_iter=7) == "stepped"
    mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol = seen["step"]
    assert mask.dtype == np.uint8 and mask.shape == (30,) and np.array_equal(mask.reshape(5, 6), good) and body_in.shape == (30,)
    assert slip is None and W.shape == (90,) and seed == 5 and method == "lanczos_pc" and split_rand is True and delta == 1e-4
    assert max_iter == 7 and rtol == 1e-8
    assert rb.RHS_and_Midpoint_mixed_dof(good, bi, slip=np.zeros((10, 3)), split_rand=False) == "rhs"
    mask, body_in, slip, W, seed, method, split_rand, delta = seen["rhs"]
    assert np.array_equal(mask.reshape(5, 6), good) and slip.shape == (30,) and W is None and method == "cholesky" and split_rand is False
    assert rb.step_brownian_mixed_dof(np.zeros((5, 6), dtype=bool), bi) == "stepped" and not seen["step"][0].any()   # nothing prescribed


def test_ensemble_wrapper_names_the_replica_and_the_body():
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = 3, 4, 12, _NoLibrary()
    bi = np.zeros(24)
    for rot in PARTIAL:
        for r, b in ((0, 0), (1, 2), (2, 3)):
            mask = np.zeros((3, 4, 6), dtype=bool)
            mask[:, :, 2] = True
            mask[r, b, 3:] = rot
            with pytest.raises(ValueError) as err:
                e.step_brownian_mixed_dof(mask, bi)
            assert str(err.value).startswith("ensemble_step_brownian_mixed_dof: replica %d, body %d: the rotation is partly prescribed" % (r, b))
            assert "all 0 or all 1" in str(err.value) and "not been derived" in str(err.value)
    one = np.zeros((4, 6), dtype=bool)                      # a mask for all replicas: the first replica is the first offender
    one[1, 4] = True
    with pytest.raises(ValueError) as err:
        e.step_brownian_mixed_dof(one, bi)
    assert "replica 0, body 1" in str(err.value)
    for bad in (np.zeros((3, 4), dtype=bool), np.zeros((4, 6), dtype=np.uint8), np.zeros((2, 4, 6), dtype=bool)):
        with pytest.raises(ValueError):
            e.step_brownian_mixed_dof(bad, bi)
    good = np.zeros((3, 4, 6), dtype=bool)
    good[0, :, 2] = True
    good[1, 2, 3:] = True
    good[2, 1] = True
    with pytest.raises(ValueError):
        e.step_brownian_mixed_dof(good, bi, W=np.zeros((3, 100)))
    calls = []

    class _Rec:
        def ensemble_step_brownian_mixed_dof(self, m, b, **k):
            calls.append((m, b, k))
            return "stepped"
    e.ctx = _Rec()
    assert e.step_brownian_mixed_dof(good, bi, seed=4, max_iter=9) == "stepped"
    m, b, k = calls[-1]
    assert m.dtype == np.uint8 and m.shape == (3, 4, 6) and np.array_equal(m, good) and k["seed"] == 4 and k["max_iter"] == 9
    # the device context's own check (the ctypes layer under the Ensemble), with the library replaced as well
    from rigid_body_light_amd._lib import check_brownian_mask6
    check_brownian_mask6("x", good, 4, 3)
    bad = good.copy()
    bad[2, 1, 5] = False
    with pytest.raises(ValueError) as err:
        check_brownian_mask6("ensemble_step_brownian_mixed_dof", bad, 4, 3)
    assert "replica 2, body 1" in str(err.value)


# ---- the block structure the argument rests on --------------------------------------------------------------------------------------

@pytest.mark.parametrize("nblb", [12, 162])
def test_KTK_is_block_diagonal_and_pinv_of_K_Df_is_Df_Kinv(nblb):
    """K^T K of a body whose reference configuration has its mean removed: the translation block is n I and the
    translation-rotation blocks vanish (sum of the lever arms = 0), at any orientation.  Hence for a mask whose rotation entries
    are all equal within a body pinv(K D_f) = D_f Kinv, Kinv = (K^T K)^-1 K^T: the masked random displacements stay in the free
    coordinates."""
    from oracle import oracle as O
    from rigid_body_light_amd import load_structure
    cfg = O.remove_mean(load_structure(nblb)[1])
    nb = 3
    rng = np.random.default_rng(nblb)
    X = rng.uniform(-5.0, 5.0, (nb, 3))
    Q = O.normalize_quats(rng.standard_normal((nb, 4)))
    K = O.K_matrix(X, Q, cfg)
    Kinv = O.Kinv_matrix(X, Q, cfg)
    KTK = K.T @ K
    scale = np.abs(KTK).max()
    for b in range(nb):
        B = KTK[6 * b:6 * b + 6, 6 * b:6 * b + 6]
        assert np.abs(B[:3, :3] - nblb * np.eye(3)).max() <= 1e-13 * nblb
        assert np.abs(B[:3, 3:]).max() <= 1e-13 * scale and np.abs(B[3:, :3]).max() <= 1e-13 * scale
        off = KTK[6 * b:6 * b + 6].copy()
        off[:, 6 * b:6 * b + 6] = 0.0
        assert np.abs(off).max() <= 1e-13 * scale                                       # bodies do not couple
    masks = {"z of all": np.tile([0, 0, 1, 0, 0, 0], (nb, 1)), "a rotation driven": np.array([[0] * 6, [0, 0, 0, 1, 1, 1], [0] * 6]),
             "held and whole": np.array([[1, 1, 1, 0, 0, 0], [1] * 6, [0, 1, 0, 1, 1, 1]]), "nothing": np.zeros((nb, 6), dtype=int)}
    for name, m in masks.items():
        Df = np.diag(1.0 - m.reshape(-1).astype(np.float64))
        P = np.linalg.pinv(K @ Df)
        err = np.abs(P - Df @ Kinv).max() / np.abs(Kinv).max()
        print("shell_N_%d, %s: |pinv(K D_f) - D_f Kinv| / |Kinv| = %.2e" % (nblb, name, err))
        assert err <= 1e-12
