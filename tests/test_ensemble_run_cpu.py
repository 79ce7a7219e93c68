"""Runs of ensemble steps (include/rbl.h section 5, rbl_ensemble_run; Ensemble.run): what can be checked without a device -- the
declaration, the layout of the two structs as Python passes them, every refusal that is decided before the library touches the
GPU, and the shape rules of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBL_ERR_SIZE, RBL_ERR_STATE, RBL_ERR_ARG = 4, 7, 11


def _lib():
    from rigid_body_light_amd._lib import lib
    L = lib()
    L.rbl_set_comm_ops.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _ctx(L, params=True):
    from rigid_body_light_amd import load_structure
    h = L.rbl_create()
    if params:
        p, cfg = load_structure(12)
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)
        assert L.rbl_set_parameters(h, p["sep"] / 2.0, 0.01, 1.0, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    return h


_KEEP = []                                              # the arrays behind the pointers of the structs


def _args(**change):
    """valid options and outputs for a free Brownian run of 4 steps, with the named fields changed"""
    from rigid_body_light_amd._lib import RunOpts, RunOut
    F, fr = np.zeros(64), np.zeros(4096)
    _KEEP.extend([F, fr])
    o, out = RunOpts(), RunOut()
    o.size, out.size = C.sizeof(RunOpts), C.sizeof(RunOut)
    o.n_steps, o.brownian, o.split_rand, o.max_iter, o.stride, o.on_error, o.check_every = 4, 1, 1, 10, 0, 0, 0
    o.seed, o.delta, o.rtol = 1, 1e-4, 1e-8
    o.F_body = F.ctypes.data
    for k, v in change.items():
        if k.startswith("out_"):
            setattr(out, k[4:], v)
        else:
            setattr(o, k, v)
    return o, out


def _run(L, h, **change):
    o, out = _args(**change)
    rc = L.rbl_ensemble_run(h, C.byref(o), C.byref(out))
    return rc, L.rbl_last_error(h)


def test_the_entry_point_and_its_structs_are_declared_and_exported():
    from rigid_body_light_amd._lib import RunOpts, RunOut
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    assert re.search(r"\bint\s+rbl_ensemble_run\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+rbl_run_opts\s*\*\s*opts\s*,\s*rbl_run_out\s*\*\s*out\s*\)", code)
    assert hasattr(L, "rbl_ensemble_run")
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    assert "rbl_ensemble_run" in sec5 and "RBL_RUN_REJECT" in sec5 and "redrawn" in sec5.lower()
    for name, cls in (("rbl_run_opts", RunOpts), ("rbl_run_out", RunOut)):   # the ctypes mirror has the header's fields, in order
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(RunOpts) == 8 + 8 * 4 + 8 + 2 * 8 + 4 * 8 and C.sizeof(RunOut) == 8 + 11 * 8 + 4 * 4


def test_every_refusal_is_decided_before_a_device_is_touched():
    L = _lib()
    h = _ctx(L)                                          # parameters, no ensemble: this context never initialises a device
    o, out = _args()
    assert L.rbl_ensemble_run(h, None, C.byref(out)) == RBL_ERR_ARG and b"NULL" in L.rbl_last_error(h)
    assert L.rbl_ensemble_run(h, C.byref(o), None) == RBL_ERR_ARG and b"NULL" in L.rbl_last_error(h)
    assert L.rbl_ensemble_run(None, C.byref(o), C.byref(out)) == RBL_ERR_ARG
    mask, bi = np.zeros(8, dtype=np.uint8), np.zeros(48)
    for change, word in (
            (dict(size=8), b"opts.size"), (dict(out_size=0), b"out.size"),
            (dict(n_steps=0), b"n_steps"), (dict(n_steps=-2), b"n_steps"),
            (dict(stride=-1), b"stride"), (dict(check_every=-1), b"check_every"),
            (dict(on_error=2), b"on_error"), (dict(on_error=-1), b"on_error"),
            (dict(F_body=None), b"F_body"),                                                        # neither
            (dict(prescribed=mask.ctypes.data, body_in=bi.ctypes.data), b"F_body"),                # both
            (dict(body_in=bi.ctypes.data), b"F_body"),
            (dict(F_body=None, prescribed=mask.ctypes.data), b"NULL"),                             # half of the masked pair
            (dict(F_body=None, body_in=bi.ctypes.data), b"NULL"),
            (dict(max_iter=0), b"max_iter"), (dict(max_iter=-3), b"max_iter"),
            (dict(rtol=-1.0), b"rtol"), (dict(rtol=float("nan")), b"rtol"),
            (dict(stride=2), b"frame_X"),                                                          # 2 frames, no arrays
            (dict(stride=1, out_frame_X=1, out_frame_Q=1), b"frame_accepted_at"),
    ):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_ARG and word in msg, (change, rc, msg)
    fr = np.zeros(64)
    masked = dict(F_body=None, prescribed=mask.ctypes.data, body_in=bi.ctypes.data)
    rc, msg = _run(L, h, stride=1, out_frame_X=fr.ctypes.data, out_frame_Q=fr.ctypes.data, out_frame_accepted_at=fr.ctypes.data, **masked)
    assert rc == RBL_ERR_ARG and b"frame_F" in msg
    for change in (dict(max_iter=256), dict(max_iter=256, **masked)):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_SIZE and b"max_iter <= 255" in msg, (change, rc, msg)
    for change in (dict(), masked, dict(stride=5), dict(brownian=0, on_error=1)):   # nothing wrong but the state (5 > 4 steps: no frame)
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (change, rc, msg)
    L.rbl_destroy(h)
    h = _ctx(L, params=False)
    for change in (dict(), masked):
        assert _run(L, h, **change)[0] == RBL_ERR_STATE
    L.rbl_destroy(h)
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = _ctx(L)
    assert L.rbl_set_comm_ops(h, 0, 2, C.cast(cb, C.c_void_p), None, None) == 0
    for change in (dict(), masked):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_ARG and b"communicator" in msg
    L.rbl_destroy(h)


class _NoLibrary:
    """stands where the device context would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _ensemble(R=3, nb=4):
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = R, nb, 12, _NoLibrary()
    return e


@pytest.mark.parametrize("kwargs", [
    dict(n_steps=0, F=np.zeros(24)),
    dict(n_steps=4),                                                               # neither F nor prescribed
    dict(n_steps=4, F=np.zeros(24), prescribed=[0], body_in=np.zeros(24)),         # both
    dict(n_steps=4, prescribed=[0]),                                               # no body_in
    dict(n_steps=4, body_in=np.zeros(24)),                                         # no mask
    dict(n_steps=4, F=np.zeros(23)),
    dict(n_steps=4, F=np.zeros((2, 24))),                                          # replicas differ
    dict(n_steps=4, prescribed=[4], body_in=np.zeros(24)),                         # no such body
    dict(n_steps=4, prescribed=np.zeros((2, 4), dtype=bool), body_in=np.zeros(24)),
    dict(n_steps=4, prescribed=[0], body_in=np.zeros(25)),
    dict(n_steps=4, F=np.zeros(24), slip=np.zeros(7)),
    dict(n_steps=4, F=np.zeros(24), stride=-1),
    dict(n_steps=4, F=np.zeros(24), check_every=-1),
    dict(n_steps=4, F=np.zeros(24), on_error="retry"),
    dict(n_steps=4, F=np.zeros(24), on_error=1),
])
def test_run_shape_and_option_errors_raise_before_the_library_is_called(kwargs):
    e = _ensemble()
    with pytest.raises(ValueError):
        e.run(**kwargs)


def test_the_default_poll_interval_is_the_header_s():
    import inspect
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import RUN_CHECK_DEFAULT
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    assert int(re.search(r"#define\s+RBL_RUN_CHECK_DEFAULT\s+(\d+)", text).group(1)) == RUN_CHECK_DEFAULT
    assert inspect.signature(Ensemble.run).parameters["check_every"].default == RUN_CHECK_DEFAULT
    assert inspect.signature(Ensemble.run).parameters["on_error"].default == "stop"
