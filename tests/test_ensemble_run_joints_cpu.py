"""Ensemble runs with hard joints (include/rbl.h section 5, rbl_ensemble_run_jointed) without a GPU: the declarations and exports,
the refusals a context without a device reaches, the motor schedule's map from a cycle position to its phase, and the Python
layer's shape and value checks.  No device is touched.

The position-to-phase map is written once, as a __host__ __device__ function in rigid_body_light_amd/csrc/rbl_schedule.hpp; the
run's kernel calls it on the device and the library exports the host's copy of the same statements as rbl_run_schedule_phase,
which is what is tested here against a cycle unrolled by brute force.  (The refusals that need an ensemble configuration -- the
schedule's own, the cell, a Brownian run with a real ensemble -- are in the GPU file.)"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_ensemble_joints_cpu import _context, _ensemble, _lib, _set_motor  # noqa: E402

ERR_STATE, ERR_ARG = 7, 11


def _structs(F=None, n_steps=4):
    from rigid_body_light_amd._lib import RunJointOpts, RunJointOut, RunOpts, RunOut
    o, jo, out, jout = RunOpts(), RunJointOpts(), RunOut(), RunJointOut()
    for s in (o, jo, out, jout):
        s.size = ctypes.sizeof(s)
    o.n_steps, o.max_iter, o.rtol = n_steps, 50, 1e-8
    o.F_body = None if F is None else F.ctypes.data
    jo.gamma = 1.0
    return o, jo, out, jout


def test_the_entry_point_is_declared_and_exported_and_the_documents_name_it():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    assert re.search(r"\bint\s+rbl_ensemble_run_jointed\s*\(\s*rbl_ctx\s*\*\s*ctx", code) and hasattr(L, "rbl_ensemble_run_jointed")
    assert re.search(r"\bint\s+rbl_run_schedule_phase\s*\(", code) and hasattr(L, "rbl_run_schedule_phase")
    for name in ("rbl_run_joint_opts", "rbl_run_joint_out"):
        assert re.search(r"\}\s*%s\s*;" % name, code), name
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import DeviceContext, RunJointOpts, RunJointOut, RunOpts, RunOut
    assert callable(Ensemble.run_jointed) and callable(DeviceContext.ensemble_run_jointed)
    # the structs of rbl_ensemble_run keep their size and layout; the new ones are what the header declares (LP64)
    assert ctypes.sizeof(RunOpts) == 96 and ctypes.sizeof(RunOut) == 112
    assert ctypes.sizeof(RunJointOpts) == 64 and ctypes.sizeof(RunJointOut) == 56
    for doc in ("README.md", "DESIGN.md"):
        assert "run_jointed" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_run_refuses_before_any_device_work():
    L = _lib()
    h = _context(L)
    F = np.zeros(12)
    run = L.rbl_ensemble_run_jointed

    def said(hh=None):
        return L.rbl_last_error(h if hh is None else hh)

    o, jo, out, jout = _structs(F)
    assert run(None, o, jo, out, jout) == ERR_ARG
    for k in range(4):
        a = [ctypes.byref(s) for s in (o, jo, out, jout)]
        a[k] = None
        assert run(h, *a) == ERR_ARG and b"NULL" in said()
    for k, name in enumerate((b"rbl_run_opts", b"rbl_run_joint_opts", b"rbl_run_out", b"rbl_run_joint_out")):
        s = _structs(F)
        s[k].size += 8
        assert run(h, *s) == ERR_ARG and name in said(), name
    for with_joints in (False, True):
        if with_joints:
            _set_motor(L, h)
        for field, value, word in (("n_steps", 0, b"n_steps"), ("stride", -1, b"stride"), ("check_every", -1, b"check_every"),
                                   ("on_error", 2, b"on_error"), ("prescribed_per", 6, b"prescribed_per"), ("max_iter", 0, b"max_iter"),
                                   ("max_iter", 256, b"max_iter"), ("rtol", -1.0, b"rtol")):
            o, jo, out, jout = _structs(F)
            setattr(o, field, value)
            assert run(h, o, jo, out, jout) == ERR_ARG and word in said(), field
            assert (out.steps_done, out.stopped_at, out.stop_replica) == (0, -1, -1)
        mask = np.zeros(2, dtype=np.uint8)
        for field in ("prescribed", "body_in"):
            o, jo, out, jout = _structs(F)
            setattr(o, field, mask.ctypes.data if field == "prescribed" else F.ctypes.data)
            assert run(h, o, jo, out, jout) == ERR_ARG and b"prescribed" in said() and b"masks" in said()
        for g in (-0.1, 1.5, float("nan")):
            o, jo, out, jout = _structs(F)
            jo.gamma = g
            assert run(h, o, jo, out, jout) == ERR_ARG and b"gamma" in said()
        o, jo, out, jout = _structs(None)
        assert run(h, o, jo, out, jout) == ERR_ARG and b"F_body is NULL" in said()
        o, jo, out, jout = _structs(F)
        assert run(h, o, jo, out, jout) == ERR_STATE and b"no ensemble configuration" in said()
    # a Brownian run at kBT > 0: refused, the message says why; at kBT = 0 (the context above) brownian is ignored
    from rigid_body_light_amd import load_structure
    cfg = np.ascontiguousarray(load_structure(12)[1])
    hb = L.rbl_create()
    assert L.rbl_set_parameters(hb, 0.4, 0.01, 0.01, 1.0, cfg.ctypes.data, 12) == 0
    o, jo, out, jout = _structs(F)
    o.brownian = 1
    assert run(hb, o, jo, out, jout) == ERR_ARG and b"drift" in said(hb) and b"brownian" in said(hb)
    assert run(h, o, jo, out, jout) == ERR_STATE and b"no ensemble configuration" in said()
    L.rbl_destroy(hb)
    # dt <= 0 with the joints on
    h0 = _context(L, dt=0.0)
    _set_motor(L, h0)
    o, jo, out, jout = _structs(F)
    assert run(h0, o, jo, out, jout) == ERR_ARG and b"dt must be positive" in said(h0)
    L.rbl_destroy(h0)
    # a communicator
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h3 = _context(L)
    _set_motor(L, h3)
    assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    o, jo, out, jout = _structs(F)
    assert run(h3, o, jo, out, jout) == ERR_ARG and b"communicator" in said(h3)
    L.rbl_destroy(h3)
    L.rbl_destroy(h)


@pytest.mark.parametrize("steps", [(3, 1, 4, 2), (5,), (1, 1, 7), (1,)])
def test_the_position_to_phase_map_against_the_unrolled_cycle(steps):
    """every position of the cycle, and the positions outside it: the table is the cycle written out phase by phase"""
    L = _lib()
    ps = np.array(steps, dtype=np.int32)
    table = [k for k, n in enumerate(steps) for _ in range(n)]
    assert len(table) == sum(steps)
    for p, k in enumerate(table):
        assert L.rbl_run_schedule_phase(ps.ctypes.data, len(steps), p) == k, (steps, p)
    for p in (-1, len(table), len(table) + 3):
        assert L.rbl_run_schedule_phase(ps.ctypes.data, len(steps), p) == -1, (steps, p)
    assert L.rbl_run_schedule_phase(None, len(steps), 0) == -1 and L.rbl_run_schedule_phase(ps.ctypes.data, 0, 0) == -1
    bad = np.array(list(steps) + [0], dtype=np.int32)
    assert L.rbl_run_schedule_phase(bad.ctypes.data, len(bad), 0) == -1


def test_shape_and_value_errors_raise_before_the_library_is_called():
    e = _ensemble(R=3, nb=4, nj=5)
    F = np.zeros(24)
    ok = ([3, 1, 4, 2], np.zeros((4, 5)))
    for bad in (dict(n_steps=0), dict(stride=-1), dict(check_every=-1), dict(on_error="ignore"), dict(gamma=1.5), dict(gamma=-0.1),
                dict(gamma=float("nan"))):
        kw = dict(n_steps=4, F=F, schedule=ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            e.run_jointed(**kw)
    for Fb in (np.zeros(23), np.zeros((2, 24)), np.zeros((3, 4, 6))):
        with pytest.raises(ValueError):
            e.run_jointed(4, Fb)
    with pytest.raises(ValueError):
        e.run_jointed(4, F, slip=np.zeros(7))
    for rows in (np.zeros(14), np.zeros((5, 2)), np.zeros((2, 15)), np.zeros((3, 3, 5))):
        with pytest.raises(ValueError):
            e.run_jointed(4, F, joint_velocity=rows)
    for sched in (([3, 1], np.zeros((3, 5))),            # a phase without rates
                  ([3, 1], np.zeros((2, 4))),            # not n_joints rates
                  ([3, 1], np.zeros((2, 2, 5))),         # neither shared nor one set per replica
                  ([3, 1], np.zeros(5)),
                  ([], np.zeros((0, 5))),                # an empty cycle
                  ([3, 0], np.zeros((2, 5))),            # a phase of no steps
                  ([3, -1], np.zeros((2, 5))),
                  ([3.0, 1.0], np.zeros((2, 5))),        # lengths are integers
                  ([[3, 1]], np.zeros((2, 5))),
                  ([2**30, 2**30], np.zeros((2, 5))),    # the cycle's length fits 31 bits
                  ([3, 1], np.full((2, 5), np.inf)),
                  [3, 1],                                # no pair
                  ([3, 1], np.zeros((2, 5)), 0)):
        with pytest.raises(ValueError):
            e.run_jointed(4, F, schedule=sched)
    for start in (4, -1, [0, 1], [0, 1, 4], [0.0, 1.0, 2.0], [[0, 1, 2]]):      # the cycle of [3, 1] has the positions 0 .. 3
        with pytest.raises(ValueError):
            e.run_jointed(4, F, schedule=([3, 1], np.zeros((2, 5))), cycle_start=start)
    with pytest.raises(ValueError):
        e.run_jointed(4, F, cycle_start=1)                # no schedule: only 0
    with pytest.raises(ValueError):
        _ensemble(R=3, nb=4, nj=0).run_jointed(4, F, schedule=([3, 1], np.zeros((2, 0))))       # no joints are stored
    # what the wrapper hands on
    ps, pr, cs = e._schedule(([3, 1, 4, 2], np.ones((4, 3, 5))), [0, 4, 9])
    assert ps.dtype == np.int32 and list(ps) == [3, 1, 4, 2] and pr.shape == (4, 3, 5) and cs.dtype == np.int32 and list(cs) == [0, 4, 9]
    assert e._schedule(None, None) == (None, None, None) and list(e._schedule(None, 0)[2]) == [0]
