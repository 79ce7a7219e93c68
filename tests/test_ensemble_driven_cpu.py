"""Driven ensemble runs (include/rbl.h section 5, rbl_ensemble_run_driven / rbl_ensemble_drive_eval; Ensemble.run_driven,
Ensemble.drive_eval): what can be checked without a device -- the declarations and the layout of the two structs as Python passes
them, the refusals that are decided before the library touches the GPU (a context without an ensemble never initialises one),
the shape and value rules of the Python layer, and the numpy restatement of the drive formula that the GPU tests compare with."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_drive_oracle as edo  # noqa: E402

RBL_ERR_STATE, RBL_ERR_ARG = 7, 11


def _lib():
    from rigid_body_light_amd._lib import lib
    return lib()


def _ctx(L, dt=0.01):
    from rigid_body_light_amd import load_structure
    h = L.rbl_create()
    p, cfg = load_structure(12)
    cfg = np.ascontiguousarray(cfg, dtype=np.float64)
    assert L.rbl_set_parameters(h, p["sep"] / 2.0, dt, 1.0, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    return h


_KEEP = []


def _structs(**change):
    """valid options of a free deterministic run of 2 steps and a drive with one set of everything (the only set count whose
    arrays have a known length without an ensemble), the named fields of the drive changed"""
    from rigid_body_light_amd._lib import RunDriveOpts, RunDriveOut, RunOpts, RunOut
    F, om, t0, ps, pi, cs = np.zeros(64), np.array([2.0]), np.array([0.5]), np.array([1, 2, 1], dtype=np.int32), np.zeros(192), np.array([3], dtype=np.int32)
    _KEEP.extend([F, om, t0, ps, pi, cs])
    o, out, d, dq = RunOpts(), RunOut(), RunDriveOpts(), RunDriveOut()
    o.size, out.size, d.size, dq.size = C.sizeof(RunOpts), C.sizeof(RunOut), C.sizeof(RunDriveOpts), C.sizeof(RunDriveOut)
    o.n_steps, o.max_iter, o.rtol, o.F_body = 2, 10, 1e-8, F.ctypes.data
    d.amp_sets = d.omega_sets = d.t0_sets = d.phase_sets = d.start_sets = 1
    d.n_phases, d.lockin = 3, 1
    d.cos_amp, d.omega, d.t0, d.phase_steps, d.phase_in, d.cycle_start = F.ctypes.data, om.ctypes.data, t0.ctypes.data, ps.ctypes.data, pi.ctypes.data, cs.ctypes.data
    for k, v in change.items():
        if k == "dq_size":
            dq.size = v
        else:
            if isinstance(v, np.ndarray):
                _KEEP.append(v)
                v = v.ctypes.data
            setattr(d, k, v)
    return o, out, d, dq


def _run(L, h, **change):
    o, out, d, dq = _structs(**change)
    rc = L.rbl_ensemble_run_driven(h, C.byref(o), C.byref(d), None, C.byref(out), C.byref(dq), None)
    return rc, L.rbl_last_error(h).decode()


def test_the_entry_points_and_their_structs_are_declared_and_exported():
    from rigid_body_light_amd._lib import RunDriveOpts, RunDriveOut
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    assert re.search(r"\bint\s+rbl_ensemble_run_driven\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+rbl_run_opts\s*\*\s*opts\s*,\s*const\s+"
                     r"rbl_run_drive_opts\s*\*\s*drive\s*,\s*const\s+rbl_run_obs_opts\s*\*\s*obs\s*,\s*rbl_run_out\s*\*\s*out\s*,\s*"
                     r"rbl_run_drive_out\s*\*\s*dout\s*,\s*rbl_run_obs_out\s*\*\s*oout\s*\)", code)
    assert re.search(r"\bint\s+rbl_ensemble_drive_eval\s*\(", code)
    assert hasattr(L, "rbl_ensemble_run_driven") and hasattr(L, "rbl_ensemble_drive_eval")
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    assert "rbl_ensemble_run_driven" in sec5 and "lockin" in sec5 and "rbl_ensemble_drive_eval" in sec5
    for name, cls in (("rbl_run_drive_opts", RunDriveOpts), ("rbl_run_drive_out", RunDriveOut)):   # the header's fields, in order
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(RunDriveOpts) == 8 + 8 * 4 + 7 * 8 and C.sizeof(RunDriveOut) == 8 + 9 * 8
    assert [getattr(RunDriveOpts, n).offset for n in ("amp_sets", "lockin", "cos_amp", "omega", "phase_steps", "cycle_start")] == [8, 32, 40, 56, 72, 88]
    assert [getattr(RunDriveOut, n).offset for n in ("X_c", "U_c", "F_c", "norm", "cycle_pos", "t_end")] == [8, 24, 40, 56, 64, 72]


def test_the_refusals_that_need_no_ensemble_are_decided_before_a_device_is_touched():
    L = _lib()
    h = _ctx(L)                                          # parameters, no ensemble: this context never initialises a device
    nan1 = np.array([np.nan])
    for change, word in (
            (dict(size=8), "drive.size"), (dict(dq_size=16), "dout.size"), (dict(n_phases=-1), "n_phases"),
            (dict(omega=None), "omega is NULL"), (dict(t0=None), "t0 is NULL"), (dict(phase_steps=None), "phase_steps or phase_in"),
            (dict(phase_in=None), "phase_steps or phase_in"), (dict(cycle_start=None), "cycle_start is NULL"),
            (dict(omega=nan1), "omega: set 0"), (dict(t0=np.array([np.inf])), "t0: set 0"),
            (dict(phase_steps=np.array([1, 0, 1], dtype=np.int32)), "phase_steps[1] = 0"),
            (dict(phase_steps=np.array([2**30, 2**30, 5], dtype=np.int32)), "31 bits"),
            (dict(cycle_start=np.array([4], dtype=np.int32)), "cycle_start[0] = 4"),
            (dict(cycle_start=np.array([-1], dtype=np.int32)), "cycle_start[0] = -1"),
            (dict(n_phases=0, cycle_start=np.array([1], dtype=np.int32)), "no phases")):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_ARG and word in msg, (change, rc, msg)
    rc, msg = _run(L, h)                                 # the drive is sound: the underlying run's own refusal, unchanged
    assert rc == RBL_ERR_STATE and "no ensemble configuration" in msg
    o, out, d, dq = _structs()
    assert L.rbl_ensemble_run_driven(h, C.byref(o), None, None, C.byref(out), None, None) == RBL_ERR_STATE
    assert L.rbl_ensemble_run_driven(h, None, C.byref(d), None, C.byref(out), C.byref(dq), None) == RBL_ERR_ARG
    assert "NULL" in L.rbl_last_error(h).decode()
    assert L.rbl_ensemble_run_driven(None, C.byref(o), C.byref(d), None, C.byref(out), C.byref(dq), None) == RBL_ERR_ARG
    assert L.rbl_ensemble_run_driven(h, C.byref(o), C.byref(d), None, C.byref(out), None, None) == RBL_ERR_ARG
    assert "dout is NULL" in L.rbl_last_error(h).decode()
    L.rbl_destroy(h)
    h = _ctx(L, dt=0.0)                                  # a harmonic part or lockin needs a clock that runs
    rc, msg = _run(L, h)
    assert rc == RBL_ERR_ARG and "dt must be positive" in msg
    rc, msg = _run(L, h, cos_amp=None, lockin=0)         # phases alone do not
    assert rc == RBL_ERR_STATE
    L.rbl_destroy(h)


def test_drive_eval_refuses_null_arguments_and_a_context_without_an_ensemble():
    L = _lib()
    h = _ctx(L)
    _, _, d, _ = _structs()
    base, out = np.zeros(64), np.zeros(64)
    assert L.rbl_ensemble_drive_eval(h, None, base.ctypes.data, None, None, out.ctypes.data, None) == RBL_ERR_ARG
    assert L.rbl_ensemble_drive_eval(h, C.byref(d), None, None, None, out.ctypes.data, None) == RBL_ERR_ARG
    assert L.rbl_ensemble_drive_eval(h, C.byref(d), base.ctypes.data, None, None, None, None) == RBL_ERR_ARG
    assert "NULL" in L.rbl_last_error(h).decode()
    assert L.rbl_ensemble_drive_eval(h, C.byref(d), base.ctypes.data, None, None, out.ctypes.data, None) == RBL_ERR_STATE
    assert "no ensemble configuration" in L.rbl_last_error(h).decode()
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


_F = np.zeros(24)


@pytest.mark.parametrize("kwargs", [
    dict(n_steps=0, F=_F),
    dict(n_steps=4),                                                               # neither F nor prescribed: run's own rules hold
    dict(n_steps=4, F=_F, on_error="retry"),
    dict(n_steps=4, F=_F, cos=np.zeros(23)),
    dict(n_steps=4, F=_F, cos=np.zeros((2, 24))),                                  # neither one set nor R
    dict(n_steps=4, F=_F, sin=np.zeros((3, 4, 5))),
    dict(n_steps=4, F=_F, cos=np.full(24, np.nan)),
    dict(n_steps=4, F=_F, cos=np.zeros(24), omega=None),                           # a harmonic part without a frequency
    dict(n_steps=4, F=_F, lockin=True, omega=None),
    dict(n_steps=4, F=_F, omega=np.zeros(2)),
    dict(n_steps=4, F=_F, omega=np.inf),
    dict(n_steps=4, F=_F, t0=np.zeros((3, 1))),
    dict(n_steps=4, F=_F, schedule=([1, 2], np.zeros((3, 24)))),                   # phases and inputs differ
    dict(n_steps=4, F=_F, schedule=([1, 0], np.zeros((2, 24)))),
    dict(n_steps=4, F=_F, schedule=([1.5, 2], np.zeros((2, 24)))),
    dict(n_steps=4, F=_F, schedule=([], np.zeros((0, 24)))),
    dict(n_steps=4, F=_F, schedule=([1, 2], np.zeros((2, 2, 24)))),                # sets neither 1 nor R
    dict(n_steps=4, F=_F, schedule=([2**30, 2**30], np.zeros((2, 24)))),
    dict(n_steps=4, F=_F, schedule=([1, 2], np.full((2, 24), np.inf))),
    dict(n_steps=4, F=_F, schedule=np.zeros(3)),
    dict(n_steps=4, F=_F, schedule=([1, 2], np.zeros((2, 24))), cycle_start=3),    # outside the cycle
    dict(n_steps=4, F=_F, cycle_start=1),                                          # no schedule: only 0
    dict(n_steps=4, F=_F, cycle_start=[0, 0]),
    dict(n_steps=4, F=_F, cycle_start=0.5),
])
def test_run_driven_shape_and_value_errors_raise_before_the_library_is_called(kwargs):
    e = _ensemble()
    with pytest.raises(ValueError):
        e.run_driven(**kwargs)


@pytest.mark.parametrize("kwargs", [
    dict(base=np.zeros(23)),
    dict(base=_F, accepted=np.zeros(2, dtype=np.int32)),
    dict(base=_F, accepted=np.zeros(3)),                                           # not integers
    dict(base=_F, accepted=np.array([0, -1, 0])),
    dict(base=_F, cycle_pos=np.zeros((3, 1), dtype=np.int32)),
    dict(base=_F, cos=np.zeros(5), omega=1.0),
])
def test_drive_eval_shape_errors_raise_before_the_library_is_called(kwargs):
    e = _ensemble()
    with pytest.raises(ValueError):
        e.drive_eval(**kwargs)


def test_run_keeps_its_keywords_and_run_driven_has_run_s():
    import inspect
    from rigid_body_light_amd import Ensemble
    run, driven = inspect.signature(Ensemble.run).parameters, inspect.signature(Ensemble.run_driven).parameters
    assert not {"cos", "sin", "omega", "t0", "schedule", "cycle_start", "lockin"} & set(run)
    assert set(run) <= set(driven)
    for name in run:
        assert run[name].default == driven[name].default or name == "n_steps", name


# ---- the numpy restatement (tests/ensemble_drive_oracle.py) ---------------------------------------------------------
def test_the_oracle_s_clock_is_the_two_rounding_clock():
    """t0 = 0.37, dt = 0.01: the separately rounded t0 + dt * n differs from the fused one first at n = 9 (the case the field
    clock's comment in rbl_forces.hip records); exact rational arithmetic says which is which"""
    from fractions import Fraction
    t0, dt = 0.37, 0.01
    first = None
    for n in range(40):
        two = float(edo.clock(t0, dt, np.array([n]))[0])
        assert two == t0 + float(np.float64(dt) * np.float64(n))
        exact = Fraction(t0) + Fraction(dt) * n
        lo, hi = np.nextafter(two, -np.inf), np.nextafter(two, np.inf)
        fused = min((two, lo, hi), key=lambda v: abs(Fraction(float(v)) - exact))       # the correctly rounded exact sum
        if fused != two and first is None:
            first = n
    assert first == 9
    assert np.array_equal(edo.clock(None, dt, np.arange(5)), dt * np.arange(5.0))


def test_the_oracle_s_formula_order_and_limits():
    rng = np.random.default_rng(0)
    R, per = 3, 12
    A0, Cc, Ss, P = rng.standard_normal((R, per)), rng.standard_normal((R, per)), rng.standard_normal(per), rng.standard_normal((3, R, per))
    n, pos = np.array([0, 3, 9]), np.array([0, 1, 3])
    # omega = 0, S = 0: the bits of (A0 + P) + C
    v, cs_sn, parts = edo.drive_eval(A0, 0.01, n, cos=Cc, omega=0.0, t0=0.37, phase_steps=[1, 2, 1], phase_in=P, cycle_pos=pos)
    Pk = np.stack([P[0, 0], P[1, 1], P[2, 2]])
    assert np.array_equal(v, (A0 + Pk) + Cc) and np.array_equal(cs_sn, np.tile([1.0, 0.0], (R, 1)))
    assert np.array_equal(parts, np.abs(A0) + np.abs(Pk) + np.abs(Cc))
    # the additions in the order written, entry by entry, with python floats
    om, t0 = np.array([3.0, 5.0, 7.0]), np.array([0.1, 0.2, 0.3])
    v, cs_sn, _ = edo.drive_eval(A0, 0.01, n, cos=Cc, sin=Ss, omega=om, t0=t0)
    for r in range(R):
        t = float(t0[r]) + 0.01 * float(n[r])
        cs, sn = float(np.cos(om[r] * t)), float(np.sin(om[r] * t))
        assert (cs, sn) == tuple(cs_sn[r])
        for e in range(per):
            assert v[r, e] == ((float(A0[r, e]) + 0.0) + float(Cc[r, e]) * cs) + float(Ss[e]) * sn
    # given cs, sn stand for libm's
    w, _, _ = edo.drive_eval(A0, 0.01, n, cos=Cc, sin=Ss, cs_sn=cs_sn)
    assert np.array_equal(v, w)


def test_the_oracle_s_schedule_map_is_the_library_s():
    L = _lib()
    L.rbl_run_schedule_phase.restype = C.c_int
    steps = np.array([1, 2, 1, 3], dtype=np.int32)
    pos = 0
    for _ in range(2 * int(steps.sum())):
        assert edo.schedule_phase(steps, pos) == L.rbl_run_schedule_phase(steps.ctypes.data, steps.size, pos)
        nxt = edo.schedule_next(steps, pos)
        assert nxt == (pos + 1) % int(steps.sum())
        pos = nxt


def test_the_oracle_s_lockin_sums_skip_uncommitted_steps_and_keep_step_order():
    rng = np.random.default_rng(1)
    steps, R = 6, 2
    vals, cs_sn = rng.standard_normal((steps, R, 2, 3)), [rng.standard_normal((R, 2)) for _ in range(steps)]
    ok = [np.array([True, n % 2 == 0]) for n in range(steps)]
    sc, ss = edo.lockin_sums(vals, cs_sn, ok)
    norm = edo.lockin_norm(cs_sn, ok)
    for r in range(R):
        acc_c, acc_s, nn = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(5)
        for n in range(steps):
            if ok[n][r]:
                c, s = cs_sn[n][r]
                acc_c, acc_s = acc_c + vals[n, r] * c, acc_s + vals[n, r] * s
                nn = nn + np.array([c, s, c * c, s * s, c * s])
        assert np.array_equal(sc[r], acc_c) and np.array_equal(ss[r], acc_s) and np.array_equal(norm[r], nn)
