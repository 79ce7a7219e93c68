"""Observers of ensemble runs and the ensemble's flow field (include/rbl.h section 5: rbl_ensemble_run_observed,
rbl_ensemble_velocity_field, rbl_ensemble_probe_info; Ensemble.run / run_jointed with probes, probe_body, moments;
Ensemble.velocity_field): what can be checked without a device -- the declarations, the structs as Python passes them, every
refusal that is decided before the library touches the GPU, the shape rules of the Python layer, and the self-consistency of
the CPU restatement (tests/ensemble_probe_oracle.py) that the GPU tests compare against.

A context without a device cannot hold an ensemble, so R and N_bod are unknown here: of the refusals of point_sets and probe_body
the halves that need neither (point_sets < 1, probe_body < -1) are checked here, the other halves (point_sets = 2 with R = 3,
probe_body = N_bod) in tests/test_ensemble_observed_gpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_probe_oracle as epo  # noqa: E402
import periodic_oracle as po  # noqa: E402

RBL_OK, RBL_ERR_STATE, RBL_ERR_ARG = 0, 7, 11


def _lib():
    from rigid_body_light_amd._lib import lib
    return lib()


def _ctx(L):
    from rigid_body_light_amd import load_structure
    h = L.rbl_create()
    p, cfg = load_structure(12)
    cfg = np.ascontiguousarray(cfg, dtype=np.float64)
    assert L.rbl_set_parameters(h, p["sep"] / 2.0, 0.01, 1.0, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    return h


_KEEP = []


def _args(jointed=False, **change):
    """valid arguments of an observed deterministic run of 4 steps with 5 probes and moments; o_ / out_ / obs_ / oout_ name the
    struct a changed field belongs to"""
    from rigid_body_light_amd._lib import RunJointOpts, RunJointOut, RunObsOpts, RunObsOut, RunOpts, RunOut
    F, fr, pts = np.zeros(64), np.zeros(4096), np.arange(15.0) + 1.0
    _KEEP.extend([F, fr, pts])
    o, out, jo, jout, obs, oout = RunOpts(), RunOut(), RunJointOpts(), RunJointOut(), RunObsOpts(), RunObsOut()
    for s in (o, out, jo, jout, obs, oout):
        s.size = C.sizeof(type(s))
    o.n_steps, o.brownian, o.max_iter, o.stride, o.on_error, o.check_every, o.rtol = 4, 0, 10, 0, 0, 0, 1e-8
    o.F_body = F.ctypes.data
    jo.gamma = 1.0
    obs.n_probes, obs.point_sets, obs.probe_body, obs.moments, obs.points = 5, 1, -1, 1, pts.ctypes.data
    S = dict(o=o, out=out, obs=obs, oout=oout)
    for k, v in change.items():
        tag, name = k.split("_", 1)
        setattr(S[tag], name, v)
    return o, (jo if jointed else None), obs, out, (jout if jointed else None), oout


def _run(L, h, jointed=False, **change):
    o, jo, obs, out, jout, oout = _args(jointed, **change)
    rc = L.rbl_ensemble_run_observed(h, C.byref(o), None if jo is None else C.byref(jo), C.byref(obs), C.byref(out),
                                     None if jout is None else C.byref(jout), C.byref(oout))
    return rc, L.rbl_last_error(h)


def test_the_entry_points_and_structs_are_declared_and_exported():
    from rigid_body_light_amd._lib import RunObsOpts, RunObsOut
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    for name in ("rbl_ensemble_run_observed", "rbl_ensemble_velocity_field", "rbl_ensemble_velocity_field_dev", "rbl_ensemble_probe_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in sec5, name
    for name, cls in (("rbl_run_obs_opts", RunObsOpts), ("rbl_run_obs_out", RunObsOut)):   # the ctypes mirror has the header's fields, in order
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(RunObsOpts) == 8 + 4 * 4 + 8 and C.sizeof(RunObsOut) == 8 + 4 * 8
    # no existing struct changed size
    from rigid_body_light_amd._lib import RunJointOpts, RunJointOut, RunOpts, RunOut
    assert C.sizeof(RunOpts) == 8 + 8 * 4 + 8 + 2 * 8 + 4 * 8 and C.sizeof(RunOut) == 8 + 11 * 8 + 4 * 4
    assert C.sizeof(RunJointOpts) == 8 + 8 + 8 + 4 * 4 + 3 * 8 and C.sizeof(RunJointOut) == 8 + 6 * 8


@pytest.mark.parametrize("jointed", [False, True])
def test_every_refusal_of_an_observed_run_is_decided_before_a_device_is_touched(jointed):
    L = _lib()
    h = _ctx(L)                                          # parameters, no ensemble: this context never initialises a device
    o, jo, obs, out, jout, oout = _args(jointed)
    pj, pjo = (None if jo is None else C.byref(jo)), (None if jout is None else C.byref(jout))
    assert L.rbl_ensemble_run_observed(None, C.byref(o), pj, C.byref(obs), C.byref(out), pjo, C.byref(oout)) == RBL_ERR_ARG
    assert L.rbl_ensemble_run_observed(h, C.byref(o), pj, None, C.byref(out), pjo, C.byref(oout)) == RBL_ERR_ARG and b"obs" in L.rbl_last_error(h)
    assert L.rbl_ensemble_run_observed(h, C.byref(o), pj, C.byref(obs), C.byref(out), pjo, None) == RBL_ERR_ARG and b"oout" in L.rbl_last_error(h)
    bad = np.arange(15.0)
    bad[3 * 3 + 1] = np.inf
    nan = np.arange(15.0)
    nan[14] = np.nan
    fr = np.zeros(4096)
    frames = dict(out_frame_X=fr.ctypes.data, out_frame_Q=fr.ctypes.data, out_frame_accepted_at=fr.ctypes.data)
    for change, word in (
            (dict(obs_size=8), b"obs.size"), (dict(oout_size=0), b"oout.size"),
            (dict(obs_n_probes=-1), b"n_probes"),
            (dict(obs_points=None), b"points is NULL"),
            (dict(obs_point_sets=0), b"point_sets"), (dict(obs_point_sets=-3), b"point_sets"),
            (dict(obs_probe_body=-2), b"probe_body"),
            (dict(obs_points=bad.ctypes.data), b"set 0, point 3"),
            (dict(obs_points=nan.ctypes.data), b"set 0, point 4"),
            (dict(o_stride=2, oout_frame_D=fr.ctypes.data, **frames), b"frame_u"),
            (dict(o_stride=2, oout_frame_u=fr.ctypes.data, **frames), b"frame_D"),
            (dict(o_stride=2, obs_moments=0, **frames), b"frame_u"),
            (dict(o_stride=2, obs_n_probes=0, **frames), b"frame_D"),
            # ... then everything the underlying run refuses
            (dict(o_n_steps=0), b"n_steps"), (dict(o_size=8), b"opts.size"), (dict(out_size=0), b"out.size"),
            (dict(o_stride=-1), b"stride"), (dict(o_on_error=2), b"on_error"), (dict(o_F_body=None), b"F_body"),
            (dict(o_max_iter=0), b"max_iter"), (dict(o_rtol=-1.0), b"rtol"),
    ) + (() if jointed else (          # (a jointed run looks at its state before its frame arrays, as rbl_ensemble_run_jointed does)
            (dict(o_stride=2, oout_frame_u=fr.ctypes.data, oout_frame_D=fr.ctypes.data), b"frame_X"),)):
        rc, msg = _run(L, h, jointed, **change)
        assert rc == RBL_ERR_ARG and word in msg, (change, rc, msg)
        if change and next(iter(change)).startswith(("obs_", "oout_")):
            assert b"ensemble_run_observed" in msg, msg   # the observers' refusals name the call
    # nothing wrong but the state: with observers, and with none (then the call is the underlying run)
    for change in (dict(), dict(obs_n_probes=0, obs_moments=0), dict(obs_moments=0), dict(obs_n_probes=0),
                   dict(o_stride=5), dict(obs_n_probes=0, obs_moments=0, obs_point_sets=-7, obs_probe_body=-9, obs_points=None)):
        rc, msg = _run(L, h, jointed, **change)
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (change, rc, msg)
    L.rbl_destroy(h)


def test_the_field_s_refusals_and_its_no_op_need_no_device():
    L = _lib()
    h = _ctx(L)
    x, lam, u = np.ones(6), np.zeros(360), np.zeros(6)
    f = L.rbl_ensemble_velocity_field
    for fn in (f, L.rbl_ensemble_velocity_field_dev):
        assert fn(None, x.ctypes.data, 2, 1, -1, lam.ctypes.data, u.ctypes.data) == RBL_ERR_ARG
        assert fn(h, x.ctypes.data, -1, 1, -1, lam.ctypes.data, u.ctypes.data) == RBL_ERR_ARG and b"n_points" in L.rbl_last_error(h)
        assert fn(h, None, 0, 7, -5, None, None) == RBL_OK                      # n_points == 0: nothing is read
        for args, word in (((None, 2, 1, -1, lam.ctypes.data, u.ctypes.data), b"NULL"),
                           ((x.ctypes.data, 2, 1, -1, None, u.ctypes.data), b"NULL"),
                           ((x.ctypes.data, 2, 1, -1, lam.ctypes.data, None), b"NULL"),
                           ((x.ctypes.data, 2, 0, -1, lam.ctypes.data, u.ctypes.data), b"point_sets"),
                           ((x.ctypes.data, 2, 1, -2, lam.ctypes.data, u.ctypes.data), b"probe_body")):
            assert fn(h, *args) == RBL_ERR_ARG and word in L.rbl_last_error(h), (args, L.rbl_last_error(h))
        assert fn(h, x.ctypes.data, 2, 1, -1, lam.ctypes.data, u.ctypes.data) == RBL_ERR_STATE
        assert b"no ensemble configuration" in L.rbl_last_error(h)
    ni, wv, tl = C.c_int(0), C.c_int(0), C.c_int64(0)
    assert L.rbl_ensemble_probe_info(h, -1, C.byref(ni), C.byref(wv), C.byref(tl)) == RBL_ERR_ARG
    assert L.rbl_ensemble_probe_info(h, 64, C.byref(ni), C.byref(wv), C.byref(tl)) == RBL_ERR_STATE
    assert L.rbl_ensemble_probe_info(None, 64, C.byref(ni), C.byref(wv), C.byref(tl)) == RBL_ERR_ARG
    L.rbl_destroy(h)


# ---- the Python layer -----------------------------------------------------------------------------------------------------
class _Recorder:
    """stands where the device context would and records what Ensemble calls"""
    def __init__(self):
        self.calls = []

    def joints(self):
        return dict(on=False, body=np.zeros((0, 2), dtype=np.int32))

    def __getattr__(self, name):
        def call(*args, **kwargs):
            from rigid_body_light_amd._lib import RunResult
            self.calls.append((name, args, kwargs))
            return RunResult(), 0
        return call


def _ensemble(R=3, nb=4, ctx=None):
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = R, nb, 12, ctx if ctx is not None else _Recorder()
    return e


_INF = np.ones((5, 3))
_INF[2, 1] = np.inf


@pytest.mark.parametrize("kwargs", [
    dict(probes=np.zeros(15)),                               # not (P, 3)
    dict(probes=np.zeros((5, 2))),
    dict(probes=np.zeros((2, 5, 3))),                        # neither one set nor R = 3
    dict(probes=np.zeros((3, 2, 5, 3))),
    dict(probes=_INF),
    dict(probes=np.full((3, 5, 3), np.nan)),
    dict(probes=np.zeros((5, 3)), probe_body=4),             # no such body
    dict(probes=np.zeros((5, 3)), probe_body=-1),
    dict(probes=np.zeros((5, 3)), probe_body=1.5),
    dict(probe_body=0),                                      # a body without probes
    dict(probe_body=0, moments=True),
])
def test_observer_shape_errors_raise_before_the_library_is_called(kwargs):
    for method in ("run", "run_jointed"):
        e = _ensemble()
        with pytest.raises(ValueError):
            getattr(e, method)(4, F=np.zeros(24), **kwargs)
        assert not [c for c in e.ctx.calls if c[0].startswith("ensemble_run")]
    if "probes" in kwargs:
        e = _ensemble()
        with pytest.raises(ValueError):
            e.velocity_field(kwargs["probes"], np.zeros((3, 3 * 4 * 12)), body=kwargs.get("probe_body"))
        assert not e.ctx.calls


def test_velocity_field_checks_lambda_s_shape():
    e = _ensemble()
    for lam in (np.zeros(3 * 4 * 12), np.zeros((2, 3 * 4 * 12)), np.zeros((3, 100))):
        with pytest.raises(ValueError):
            e.velocity_field(np.zeros((5, 3)), lam)
    assert not e.ctx.calls


def test_a_non_finite_probe_is_named():
    e = _ensemble()
    with pytest.raises(ValueError, match="point 2"):
        e.run(4, F=np.zeros(24), probes=_INF)
    p = np.zeros((3, 5, 3))
    p[1, 4, 0] = np.nan
    with pytest.raises(ValueError, match="set 1, point 4"):
        e.run(4, F=np.zeros(24), probes=p)


def test_without_observers_run_and_run_jointed_call_today_s_bindings():
    e = _ensemble()
    e.run(4, F=np.zeros(24))
    e.run_jointed(4, np.zeros(24))
    assert [c[0] for c in e.ctx.calls] == ["ensemble_run", "ensemble_run_jointed"]
    assert all("_obs" not in c[2] for c in e.ctx.calls)
    e = _ensemble()
    e.run(4, F=np.zeros(24), probes=np.zeros((5, 3)))
    e.run(4, F=np.zeros(24), moments=True)
    e.run_jointed(4, np.zeros(24), probes=np.zeros((3, 5, 3)), probe_body=3, moments=True)
    assert [c[0] for c in e.ctx.calls] == ["ensemble_run_observed"] * 3      # the single binding
    assert e.ctx.calls[2][2]["jointed"] is True and e.ctx.calls[2][1][2] == 3 and e.ctx.calls[2][1][3] is True
    assert e.ctx.calls[1][1][1] is None and e.ctx.calls[1][1][3] is True


def test_the_single_binding_is_the_only_caller_of_the_observed_entry_point():
    text = open(os.path.join(ROOT, "rigid_body_light_amd", "_lib.py")).read()
    assert len(re.findall(r"self\.L\.rbl_ensemble_run_observed\(", text)) == 1
    assert "rbl_ensemble_run_observed" not in open(os.path.join(ROOT, "rigid_body_light_amd", "ensemble.py")).read()


# ---- the restatement's self-consistency (CPU oracle only) ---------------------------------------------------------------------
A, ETA = 0.5, 1.0
CELL, IMAGES = (7.0, 7.5), (1, 1)


@pytest.fixture(scope="module")
def blobs24():
    """24 random blobs at least 2a apart, 0.2 .. 4 above the wall (some inside the damped layer), random forces"""
    rng = np.random.default_rng(11)
    r = np.empty((24, 3))
    n = 0
    while n < 24:
        x = rng.uniform([0.0, 0.0, 0.2], [7.0, 7.5, 4.0])
        d = po.nearest(r[:n] - x, CELL) if n else np.zeros((0, 3))
        if n == 0 or np.min(np.linalg.norm(d, axis=1)) > 2 * A:
            r[n] = x
            n += 1
    return r, rng.standard_normal(72)


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def test_the_oracle_refuses_a_point_appended_on_a_blob(orc, blobs24):
    """why the restatement does not append a coincident point: the oracle raises its overlap error at distance 0"""
    from oracle.oracle import OracleError
    r, lam = blobs24
    with pytest.raises(OracleError):
        orc.apply_M_rows(np.concatenate([lam, np.zeros(3)]), np.concatenate([r.reshape(-1), r[5]]), 24, 25, A, ETA, True)


def test_restated_field_is_invariant_under_a_lattice_translation_and_differs_from_the_open_one(orc, blobs24):
    r, lam = blobs24
    pts = np.random.default_rng(12).uniform([0.0, 0.0, 0.1], [7.0, 7.5, 5.0], (6, 3))
    u = epo.field_cell(orc, r, lam, pts, A, ETA, CELL, IMAGES)
    v = epo.field_cell(orc, r, lam, pts + np.array([CELL[0], -CELL[1], 0.0]), A, ETA, CELL, IMAGES)
    assert _rel(v, u) <= 1e-13
    w = epo.field_open(orc, r, lam, pts, A, ETA, True)
    assert _rel(w, u) > 0.05                               # O(1): the cell tests discriminate


def test_a_restated_probe_on_a_blob_is_that_blob_s_row(orc, blobs24):
    r, lam = blobs24
    M = po.dense_M(orc, r, A, ETA, CELL, IMAGES)
    U = (M @ lam).reshape(-1, 3)
    ks = [0, 7, 23]
    shifted = r[ks] + np.array([[0.0, 0.0, 0.0], [CELL[0], 0.0, 0.0], [-CELL[0], 2 * CELL[1], 0.0]])   # on the blob, and on its images
    assert _rel(epo.field_cell(orc, r, lam, shifted, A, ETA, CELL, IMAGES), U[ks]) <= 1e-13
    Uo = orc.apply_M(lam, r.reshape(-1), A, ETA, True).reshape(-1, 3)
    assert _rel(epo.field_open(orc, r, lam, r[ks], A, ETA, True), Uo[ks]) <= 1e-13


def test_restated_points_at_or_below_the_wall_get_zero(orc, blobs24):
    r, lam = blobs24
    pts = np.array([[1.0, 1.0, 0.0], [2.0, 3.0, -0.5], [3.0, 3.0, 1.5]])
    for u in (epo.field_open(orc, r, lam, pts, A, ETA, True), epo.field_cell(orc, r, lam, pts, A, ETA, CELL, IMAGES)):
        assert np.all(u[:2] == 0.0) and np.linalg.norm(u[2]) > 0.0


def test_body_frame_points_of_an_unrotated_body_are_lab_points_shifted_by_its_centre():
    X = np.array([[0.5, 1.0, 2.0], [3.0, -1.0, 4.0]])
    Q = np.array([[2.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])          # body 0 unrotated (and not normalised), body 1 turned by 90 degrees about x
    s = np.random.default_rng(13).standard_normal((5, 3))
    assert np.array_equal(epo.place(s, X, Q), s)
    assert np.allclose(epo.place(s, X, Q, 0), s + X[0], rtol=0, atol=1e-15)
    turned = epo.place(s, X, Q, 1) - X[1]
    assert np.allclose(turned, np.stack([s[:, 0], -s[:, 2], s[:, 1]], axis=1), rtol=0, atol=1e-15)
