"""Replica ensembles with prescribed velocity components (include/rbl.h section 5, rbl_ensemble_solve_mixed_dof /
rbl_ensemble_step_mixed_dof, rbl_run_opts.prescribed_per; Ensemble.solve_mixed_dof / step_mixed_dof / run(prescribed_dof=)): what
can be checked without a device -- the declarations, every refusal that is decided before the library touches the GPU, the
per-component field of a run, and the shape rules of the Python layer.  Modelled on test_ensemble_mixed_cpu.py and
test_ensemble_run_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_ensemble_solve_mixed_dof", "rbl_ensemble_step_mixed_dof")
RBL_ERR_SIZE, RBL_ERR_STATE, RBL_ERR_ARG = 4, 7, 11


def _lib():
    from rigid_body_light_amd._lib import lib
    L = lib()
    L.rbl_set_comm_ops.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _ctx(L, params=True, kBT=1.0):
    from rigid_body_light_amd import load_structure
    h = L.rbl_create()
    if params:
        p, cfg = load_structure(12)
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)
        assert L.rbl_set_parameters(h, p["sep"] / 2.0, 0.01, kBT, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    return h


def _calls(L, h, mask, body_in, max_iter=10, rtol=1e-8):
    """the two entry points on one set of arguments -> [(name, status code, message)]"""
    m = None if mask is None else mask.ctypes.data
    b = None if body_in is None else body_in.ctypes.data
    U, F, lam = np.zeros(64), np.zeros(64), np.zeros(512)
    it, res = np.zeros(4, dtype=np.int32), np.zeros(4)
    out = []
    out.append((b"ensemble_solve_mixed_dof",
                L.rbl_ensemble_solve_mixed_dof(h, m, b, None, max_iter, rtol, lam.ctypes.data, U.ctypes.data, F.ctypes.data,
                                               it.ctypes.data, res.ctypes.data), L.rbl_last_error(h)))
    out.append((b"ensemble_step_mixed_dof",
                L.rbl_ensemble_step_mixed_dof(h, m, b, None, max_iter, rtol, F.ctypes.data, it.ctypes.data, res.ctypes.data),
                L.rbl_last_error(h)))
    return out


def test_the_two_entry_points_are_declared_in_section_5_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    code5 = re.sub(r"/\*.*?\*/", "", sec5, flags=re.S)
    for n in NAMES:
        pat = r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed6\s*,\s*const\s+double\s*\*\s*body_in" % n
        assert re.search(pat, code), n
        assert re.search(pat, code5), n                    # declared in section 5, not only mentioned there
        assert hasattr(L, n), n
    assert "prescribed_per" in code5
    # section 7 no longer lists ensembles with component masks as unavailable; what remains is their Brownian step
    not_offered = text.split("Not offered:")[-1].split("*/")[0]
    assert "rbl_ensemble_*_mixed take whole bodies only" not in not_offered
    assert "ensembles" in not_offered and "Brownian" in not_offered


def test_every_refusal_is_decided_before_a_device_is_touched_and_names_the_entry_point():
    L = _lib()
    mask, bi = np.zeros(48, dtype=np.uint8), np.zeros(48)
    h = _ctx(L)                                           # parameters, no ensemble: this context never initialises a device
    for name, rc, msg in _calls(L, h, None, bi):
        assert rc == RBL_ERR_ARG and b"NULL" in msg and name in msg and b"prescribed6" in msg
    for name, rc, msg in _calls(L, h, mask, None):
        assert rc == RBL_ERR_ARG and b"NULL" in msg and name in msg
    for bad in (0, -3):
        for name, rc, msg in _calls(L, h, mask, bi, max_iter=bad):
            assert rc == RBL_ERR_ARG and b"max_iter" in msg and name in msg
    for rtol in (-1.0, float("nan")):
        for name, rc, msg in _calls(L, h, mask, bi, rtol=rtol):
            assert rc == RBL_ERR_ARG and b"rtol" in msg and name in msg
    for name, rc, msg in _calls(L, h, mask, bi, max_iter=256):
        assert rc == RBL_ERR_SIZE and b"max_iter <= 255" in msg and name in msg
    for name, rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg and name in msg
    # Two refusals need an ensemble configuration, hence a device, and are checked in test_ensemble_dof_gpu.py: an entry of
    # prescribed6 above 1 (RBL_ERR_ARG; the entries are counted from the ensemble's R and N_bod) and a masked solve that does not
    # fit the LDS (RBL_ERR_SIZE; the shape is the ensemble's)
    # U or F of the solve
    it, res = np.zeros(4, dtype=np.int32), np.zeros(4)
    U = np.zeros(64)
    for Uo, Fo in ((None, U.ctypes.data), (U.ctypes.data, None)):
        rc = L.rbl_ensemble_solve_mixed_dof(h, mask.ctypes.data, bi.ctypes.data, None, 10, 1e-8, None, Uo, Fo, it.ctypes.data, res.ctypes.data)
        assert rc == RBL_ERR_ARG and b"ensemble_solve_mixed_dof" in L.rbl_last_error(h) and b"NULL" in L.rbl_last_error(h)
    assert L.rbl_ensemble_solve_mixed_dof(None, mask.ctypes.data, bi.ctypes.data, None, 10, 1e-8, None, None, None, it.ctypes.data,
                                          res.ctypes.data) == RBL_ERR_ARG
    assert L.rbl_ensemble_step_mixed_dof(None, mask.ctypes.data, bi.ctypes.data, None, 10, 1e-8, None, it.ctypes.data,
                                         res.ctypes.data) == RBL_ERR_ARG
    L.rbl_destroy(h)
    h = _ctx(L, params=False)                             # no parameters at all
    for name, rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_STATE
    L.rbl_destroy(h)
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = _ctx(L)
    assert L.rbl_set_comm_ops(h, 0, 2, C.cast(cb, C.c_void_p), None, None) == 0
    for name, rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_ARG and b"communicator" in msg and name in msg
    L.rbl_destroy(h)


# ---- the per-component field of a run -----------------------------------------------------------------------------------------------
_KEEP = []


def _run(L, h, **change):
    """a valid masked deterministic run of 4 steps with the named fields changed -> (status, message)"""
    from rigid_body_light_amd._lib import RunOpts, RunOut
    mask, bi = np.zeros(4096, dtype=np.uint8), np.zeros(4096)
    _KEEP.extend([mask, bi])
    o, out = RunOpts(), RunOut()
    o.size, out.size = C.sizeof(RunOpts), C.sizeof(RunOut)
    o.n_steps, o.brownian, o.split_rand, o.max_iter, o.stride, o.on_error, o.check_every = 4, 0, 1, 10, 0, 0, 0
    o.seed, o.delta, o.rtol = 1, 1e-4, 1e-8
    o.prescribed, o.body_in = mask.ctypes.data, bi.ctypes.data
    for k, v in change.items():
        setattr(o, k, v)
    rc = L.rbl_ensemble_run(h, C.byref(o), C.byref(out))
    return rc, L.rbl_last_error(h)


def test_run_mask_entries_per_body():
    from rigid_body_light_amd._lib import RunOpts
    assert C.sizeof(RunOpts) == 8 + 8 * 4 + 8 + 2 * 8 + 4 * 8            # the field took the reserved int32's place
    L = _lib()
    h = _ctx(L)                                           # kBT = 1; no ensemble, no device
    for per in (0, 1, 6):                                 # accepted: nothing wrong but the state
        rc, msg = _run(L, h, prescribed_per=per)
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (per, rc, msg)
    for per in (0, 1):                                    # whole bodies: a Brownian run is theirs to make
        rc, msg = _run(L, h, prescribed_per=per, brownian=1)
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (per, rc, msg)
    for per in (-1, 2, 3, 5, 7, 12):
        rc, msg = _run(L, h, prescribed_per=per)
        assert rc == RBL_ERR_ARG and b"ensemble_run" in msg and b"prescribed_per" in msg, (per, rc, msg)
    rc, msg = _run(L, h, prescribed_per=6, brownian=1)    # kBT > 0: refused, and the message says why
    assert rc == RBL_ERR_ARG and b"ensemble_run" in msg and b"Brownian" in msg and b"not been derived" in msg, (rc, msg)
    L.rbl_destroy(h)
    h = _ctx(L, kBT=0.0)                                  # kBT <= 1e-10: the deterministic step, as elsewhere
    rc, msg = _run(L, h, prescribed_per=6, brownian=1)
    assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (rc, msg)
    L.rbl_destroy(h)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    """stands where the device context would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Recorder:
    """stands where the device context would and keeps what it is handed"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            return (None, 0) if name == "ensemble_run" else None
        return call


def _ensemble(R=3, nb=4, ctx=None):
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = R, nb, 12, ctx or _NoLibrary()
    return e


def test_accepted_shapes_reach_the_library_as_R_by_N_bod_by_6():
    rec = _Recorder()
    e = _ensemble(ctx=rec)
    one = np.zeros((4, 6), dtype=bool)
    one[1, 3:] = True
    per = np.zeros((3, 4, 6), dtype=bool)
    per[2, 0, 2] = True
    for given, want in ((one, np.broadcast_to(one, (3, 4, 6))), (per, per)):
        e.solve_mixed_dof(given, np.zeros(24))
        e.step_mixed_dof(given, np.zeros(24))
        e.run(4, prescribed_dof=given, body_in=np.zeros(24), brownian=False)
        for name, a, k in rec.calls[-3:]:
            m = k["prescribed"] if name == "ensemble_run" else a[0]
            assert m.dtype == np.uint8 and m.shape == (3, 4, 6) and m.flags.c_contiguous and np.array_equal(m, want.astype(np.uint8))
    assert [c[0] for c in rec.calls[-3:]] == ["ensemble_solve_mixed_dof", "ensemble_step_mixed_dof", "ensemble_run"]
    assert rec.calls[-1][2]["per"] == 6
    e.run(4, prescribed=[1], body_in=np.zeros(24))        # the whole-body keyword keeps its meaning
    assert rec.calls[-1][2]["per"] == 1 and rec.calls[-1][2]["prescribed"].shape == (3, 4)


@pytest.mark.parametrize("prescribed", [
    np.zeros((3, 4), dtype=bool),                         # (R, N_bod): a whole-body mask
    np.zeros(4, dtype=bool),
    np.zeros(24, dtype=bool),
    np.zeros((2, 4, 6), dtype=bool),                      # replicas differ
    np.zeros((4, 5), dtype=bool),
    np.zeros((6, 4), dtype=bool),
    np.zeros((4, 6), dtype=np.uint8),                     # the wrong dtype
    np.zeros((4, 6)),
    np.zeros((3, 4, 6), dtype=np.int64),
    [1, 2],                                               # body indices are the whole-body calls'
])
def test_other_shapes_and_dtypes_raise_before_the_library_is_called(prescribed):
    e = _ensemble()
    for call in (e.solve_mixed_dof, e.step_mixed_dof):
        with pytest.raises(ValueError):
            call(prescribed, np.zeros(24))
    with pytest.raises(ValueError):
        e.run(4, prescribed_dof=prescribed, body_in=np.zeros(24), brownian=False)


def test_R_equal_N_bod_equal_6_is_read_per_component_only_through_the_dof_names():
    """(R, N_bod) and (N_bod, 6) are one shape here: the separate methods and keyword decide, nothing is guessed"""
    rec = _Recorder()
    e = _ensemble(R=6, nb=6, ctx=rec)
    m = np.zeros((6, 6), dtype=bool)
    m[1, 4] = True
    e.step_mixed(m, np.zeros(36))
    assert rec.calls[-1][1][0].shape == (6, 6)            # replica 1, body 4
    e.step_mixed_dof(m, np.zeros(36))
    got = rec.calls[-1][1][0]
    assert got.shape == (6, 6, 6) and np.all(got[:, 1, 4] == 1) and got.sum() == 6   # body 1, rotation y, in every replica


@pytest.mark.parametrize("kwargs", [
    dict(prescribed_dof=np.zeros((4, 6), dtype=bool), body_in=np.zeros(24), F=np.zeros(24)),
    dict(prescribed_dof=np.zeros((4, 6), dtype=bool), body_in=np.zeros(24), prescribed=[0]),
    dict(prescribed_dof=np.zeros((4, 6), dtype=bool), body_in=np.zeros(24), prescribed=np.zeros(4, dtype=bool)),
    dict(prescribed_dof=np.zeros((4, 6), dtype=bool)),                                  # no body_in
    dict(prescribed_dof=np.zeros((4, 6), dtype=bool), body_in=np.zeros(25)),
])
def test_prescribed_dof_excludes_F_and_prescribed(kwargs):
    e = _ensemble()
    with pytest.raises(ValueError):
        e.run(4, brownian=False, **kwargs)
