"""Ensemble runs with hard joints (include/rbl.h section 5: rbl_ensemble_run_jointed, Ensemble.run_jointed): n jointed steps in one
call, the motors' angles, a periodic piecewise-constant motor schedule and the records of phi and of the gaps kept on the device.

The reference is the loop the run replaces: set_joint_rates with the rates of the replica's phase, then step_jointed, with
joint_state() where a frame falls.  The run enqueues that step's very launches and advances theta with the statements of the
one-step call's host loop, so everything is compared BITWISE; there is no tolerance in this file.  The set is
tests/joint_kinds_oracle.py's case_steps (3 bodies of 12 blobs; a motor 0-1 -- joint 1 is its lock --, a hinge 1-2, a pivot on
body 0), three replicas a little apart, 12 steps of a cycle of 3 + 1 + 4 + 2 = 10, so that every replica's position wraps."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_kinds_oracle as jk  # noqa: E402
import joint_oracle as jo  # noqa: E402

MAXIT, RTOL, DT = 100, 1e-10, 0.01
STEPS, STRIDE = 12, 5
PHASES = np.array([3, 1, 4, 2])
START = np.array([0, 4, 9])
KW = dict(max_iter=MAXIT, rtol=RTOL)


def _params():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return cfg, p["sep"] / 2.0


def _ensemble(X, Q, wall, kBT=0.0):
    from rigid_body_light_amd import Ensemble
    cfg, a = _params()
    return Ensemble(cfg, np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64), a, 1.0, DT, kBT=kBT, wall=wall)


def _turned(X, Q, angle, axis, shift):
    q = jk.qrot(angle, jo._unit(axis))
    return np.asarray(X) @ jo.rot(q).T + shift, np.array([jk.qmul(q, p) for p in jo.unit(Q)])


@functools.lru_cache(maxsize=None)
def _case():
    """three replicas of case_steps' bodies, loads, slip, a joint_velocity on the pivot's (ball) rows, rates per phase and replica
    on the motor's lock"""
    X0, Q0, r = jk.case_steps()
    reps = [(X0, jo.unit(Q0)), _turned(X0, Q0, 0.01, [0.2, 1.0, -0.3], [0.01, -0.005, 0.02]),
            _turned(X0, Q0, -0.015, [1.0, 0.1, 0.4], [-0.008, 0.012, 0.015])]
    X, Q = np.array([p[0] for p in reps]), np.array([p[1] for p in reps])
    rng = np.random.default_rng(2024)
    F, slip = rng.standard_normal((3, 18)), 0.1 * rng.standard_normal((3, 108))
    v = np.zeros((5, 3))
    v[4] = [0.2, -0.1, 0.3]
    rates = np.zeros((4, 3, 5))
    rates[:, :, 1] = rng.uniform(0.3, 1.0, (4, 3)) * rng.choice([-1.0, 1.0], (4, 3))
    assert list(r["kind"]) == [jk.BALL, jk.LOCK, jk.BALL, jk.AXIS, jk.BALL]
    return dict(X=X, Q=Q, r=r, F=F, slip=slip, v=v, rates=rates)


def _phase(p):
    return int(np.searchsorted(np.cumsum(PHASES), p, side="right"))


def _loop(ens, sel, steps=STEPS, stride=STRIDE, start=START, before_step=None):
    """the loop a run replaces, for the replicas sel of the case -> what the run returns, gathered on the host"""
    c = _case()
    F, slip, rates = c["F"][sel], c["slip"][sel], c["rates"][:, sel]
    R = F.shape[0]
    pos = np.array(start)[sel].copy()
    out = dict(phi_sum=np.zeros((R, 5, 3)), iters_sum=np.zeros(R, dtype=np.int64), resid_max=np.zeros(R), X=[], Q=[], theta=[], phi=[], gap=[])
    for n in range(steps):
        if before_step is not None:
            before_step(ens, n)
        ens.set_joint_rates(np.array([rates[_phase(pos[k]), k] for k in range(R)]))
        phi, its, res = ens.step_jointed(F, slip=slip, joint_velocity=c["v"], gamma=1.0, **KW)
        assert (its > 0).all() and (its < MAXIT).all() and (res < RTOL).all()
        out["phi_sum"] += phi.reshape(R, 5, 3)
        out["iters_sum"] += its
        out["resid_max"] = np.maximum(out["resid_max"], res)
        pos = (pos + 1) % PHASES.sum()
        if stride and (n + 1) % stride == 0:
            Xn, Qn = ens.get_config()
            gap, ph, theta = ens.joint_state()
            for k, val in (("X", Xn), ("Q", Qn), ("theta", theta), ("phi", ph), ("gap", gap)):
                out[k].append(np.array(val))
    out["Xf"], out["Qf"] = ens.get_config()
    out["gapf"], out["phif"], out["thetaf"] = (np.array(p) for p in ens.joint_state())
    out["cycle_pos"] = pos.astype(np.int32)
    return out


def _run(ens, sel, steps=STEPS, stride=STRIDE, start=START, **kw):
    c = _case()
    res = ens.run_jointed(steps, c["F"][sel], slip=c["slip"][sel], joint_velocity=c["v"], gamma=1.0,
                          schedule=(PHASES, c["rates"][:, sel]), cycle_start=np.array(start)[sel], stride=stride, **KW, **kw)
    return res


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _run_is_loop(res, ens, ref, what):
    """every record of a run against the loop's, bit for bit"""
    X, Q = ens.get_config()
    gap, phi, theta = ens.joint_state()                          # after the run: the gaps now, the last accepted phi, the angles
    pairs = [("X", X, ref["Xf"]), ("Q", Q, ref["Qf"]), ("theta", res.theta, ref["thetaf"]), ("cycle_pos", res.cycle_pos, ref["cycle_pos"]),
             ("iters_sum", res.iters_sum, ref["iters_sum"]), ("resid_max", res.resid_max, ref["resid_max"]),
             ("phi_sum", res.phi_sum, ref["phi_sum"]), ("joint_state gap", gap, ref["gapf"]), ("joint_state phi", phi, ref["phif"]),
             ("joint_state theta", theta, ref["thetaf"])]
    if ref["X"]:
        pairs += [("frame X", res.X, np.array(ref["X"])), ("frame Q", res.Q, np.array(ref["Q"])),
                  ("frame theta", res.frame_theta, np.array(ref["theta"])), ("frame phi", res.frame_phi, np.array(ref["phi"])),
                  ("frame gap", res.frame_gap, np.array(ref["gap"]))]
    for name, mine, theirs in pairs:
        assert _bits(mine, theirs), "%s: %s differs from the loop's" % (what, name)


@functools.lru_cache(maxsize=None)
def _together(wall):
    """the run of the three replicas, once per wall flag -> (result, X, Q, joint_state)"""
    c = _case()
    ens = _ensemble(c["X"], c["Q"], wall)
    ens.set_joint_kinds(**c["r"])
    res = _run(ens, slice(0, 3))
    out = (res,) + tuple(ens.get_config()) + (ens.joint_state(),)
    _run_is_loop(res, ens, _loop_together(wall), "R = 3, wall=%s" % wall)
    ens.close()
    return out


@functools.lru_cache(maxsize=None)
def _loop_together(wall):
    c = _case()
    ens = _ensemble(c["X"], c["Q"], wall)
    ens.set_joint_kinds(**c["r"])
    ref = _loop(ens, slice(0, 3))
    ens.close()
    return ref


# ------------------------------------------------------------------------------------------------ 1: a run is the loop
@pytest.mark.parametrize("wall", [False, True])
def test_a_run_is_the_loop_bitwise(wall):
    res, X, Q, state = _together(wall)                        # (compares every record with the loop's)
    c, ref = _case(), _loop_together(wall)
    assert res.accepted.tolist() == [STEPS] * 3 and not res.rejected.any() and res.steps_done == STEPS and res.stopped_at == -1
    assert res.cycle_pos.tolist() == ((START + STEPS) % 10).tolist() == [2, 6, 1]
    assert res.X.shape == (2, 3, 3, 3) and res.frame_theta.shape == (2, 3, 5) and res.frame_gap.shape == (2, 3, 5, 3)
    assert res.accepted_at.tolist() == [[5] * 3, [10] * 3]
    # the run did something: the motor turned by the schedule's rates, replica by replica, and only the motor
    want = np.zeros(3)
    for k in range(3):
        for n in range(STEPS):
            want[k] += c["rates"][_phase((START[k] + n) % 10), k, 1] * DT
    assert np.abs(res.theta[:, 1] - want).max() <= 1e-15 * STEPS and np.abs(res.theta[:, 1]).min() > 1e-3
    assert not res.theta[:, [0, 2, 3, 4]].any() and np.abs(X - c["X"]).max() > 1e-3
    assert _bits(res.phi_mean, res.phi_sum / STEPS) and np.abs(res.phi_sum).max() > 1e-3
    assert _bits(state[1], ref["phif"]) and res.phi is res.frame_phi and res.gap is res.frame_gap


# ------------------------------------------------------------------------------------------------ 2: replica r of R
@pytest.mark.parametrize("wall", [False, True])
def test_replica_r_of_three_is_the_run_of_that_replica_alone(wall):
    c = _case()
    res, X, Q, state = _together(wall)
    for k in range(3):
        sel = slice(k, k + 1)
        ens = _ensemble(c["X"][sel], c["Q"][sel], wall)
        ens.set_joint_kinds(**c["r"])
        one = _run(ens, sel)
        X1, Q1 = ens.get_config()
        s1 = ens.joint_state()
        ens.close()
        for name in ("theta", "cycle_pos", "iters_sum", "resid_max", "phi_sum", "accepted"):
            assert _bits(getattr(res, name)[sel], getattr(one, name)), (k, name)
        for name in ("X", "Q", "frame_theta", "frame_phi", "frame_gap", "accepted_at"):
            assert _bits(getattr(res, name)[:, sel], getattr(one, name)), (k, name)
        assert _bits(X[sel], X1) and _bits(Q[sel], Q1)
        for p, q in zip(state, s1):
            assert _bits(p[sel], q), k


# ------------------------------------------------------------------------------------------------ 3: a second run continues the first
def test_a_second_run_continues_the_first():
    c = _case()
    res, X, Q, state = _together(True)
    ens = _ensemble(c["X"], c["Q"], True)
    ens.set_joint_kinds(**c["r"])
    first = _run(ens, slice(0, 3), steps=7, stride=0)
    assert first.cycle_pos.tolist() == ((START + 7) % 10).tolist() and first.X.shape[0] == 0
    second = _run(ens, slice(0, 3), steps=5, stride=0, start=first.cycle_pos)
    X2, Q2 = ens.get_config()
    s2 = ens.joint_state()
    ens.close()
    assert _bits(X2, X) and _bits(Q2, Q) and _bits(second.theta, res.theta) and _bits(second.cycle_pos, res.cycle_pos)
    assert _bits(first.iters_sum + second.iters_sum, res.iters_sum) and _bits(np.maximum(first.resid_max, second.resid_max), res.resid_max)
    for p, q in zip(s2, state):                                # gaps, the last phi, theta
        assert _bits(p, q)


# ------------------------------------------------------------------------------------------------ 4: joints off or never set
@pytest.mark.parametrize("state", ["never", "off"])
def test_joints_off_or_never_set_is_the_plain_deterministic_run(state):
    from rigid_body_light_amd._lib import RblError
    c = _case()
    twin = _ensemble(c["X"], c["Q"], True)
    ref = twin.run(STEPS, F=c["F"], slip=c["slip"], brownian=False, stride=STRIDE, **KW)
    Xr, Qr = twin.get_config()
    twin.close()
    ens = _ensemble(c["X"], c["Q"], True)
    if state == "off":
        ens.set_joint_kinds(**c["r"], on=False)
    before = ens.get_config()
    with pytest.raises(ValueError if state == "never" else RblError, match="phase_rates" if state == "never" else "switched off or were never set.*status 7"):
        ens.run_jointed(STEPS, c["F"], slip=c["slip"], schedule=(PHASES, np.zeros((4, 5))), **KW)
    assert all(_bits(p, q) for p, q in zip(before, ens.get_config()))
    res = ens.run_jointed(STEPS, c["F"], slip=c["slip"], stride=STRIDE, **KW)
    X, Q = ens.get_config()
    ens.close()
    assert _bits(X, Xr) and _bits(Q, Qr) and np.abs(X - c["X"]).max() > 1e-3
    for name in ("accepted", "rejected", "iters_sum", "resid_max", "X", "Q", "accepted_at"):
        assert _bits(getattr(res, name), getattr(ref, name)), name
    assert res.theta.shape == (3, 0) and not res.cycle_pos.any()


# ------------------------------------------------------------------------------------------------ 5: stop
def _ring_with_a_motor():
    """jo.redundant_set's ring on two bodies and, on another pair, a running motor whose angle is not zero"""
    X2, Q2, body, anchor = jo.redundant_set()
    X, Q = np.concatenate([X2, [[8.0, 0.0, 4.0]]]), np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    ring = jk.rows(body, np.zeros(5, dtype=np.int32), anchor_a=anchor[:, :3], anchor_b=anchor[:, 3:])
    r = jk.concat(ring, jk.motor(X, Q, 1, 2, jk.mid(X, 1, 2), [0.0, 0.0, 1.0]))
    assert list(r["kind"]) == [jk.BALL] * 6 + [jk.LOCK]
    return X, Q, r


def test_a_redundant_ring_stops_the_run_at_step_0_and_turns_no_motor():
    from rigid_body_light_amd._lib import RblError
    X, Q, r = _ring_with_a_motor()
    rates, theta = np.zeros((2, 2, 7)), np.zeros((2, 7))
    rates[0, :, 6], rates[1, :, 6], theta[:, 6] = [0.8, -0.5], [0.3, 0.2], [0.05, -0.02]
    ens = _ensemble(np.array([X, X]), np.array([Q, Q]), True)
    ens.set_joint_kinds(**r)
    ens.set_joint_angles(theta)
    F = np.random.default_rng(72).standard_normal(18)
    before = ens.get_config()
    with pytest.raises(RblError, match=r"step 0.*replica 0.*redundant"):
        ens.run_jointed(6, F, schedule=([2, 1], rates), stride=2, **KW)
    last = ens.last_run
    assert last.steps_done == 0 and last.stopped_at == 0 and last.stop_replica == 0 and last.status == 3      # RBL_ERR_NOT_SPD
    assert not last.accepted.any() and last.rejected.tolist() == [1, 1]
    assert all(_bits(p, q) for p, q in zip(before, ens.get_config()))
    assert _bits(ens.joint_state(phi=False)[2], theta) and _bits(last.theta, theta) and not last.cycle_pos.any() and not last.phi_sum.any()
    with pytest.raises(RblError, match="no jointed ensemble solve or step has succeeded"):
        ens.joint_state()                                        # phi is invalid after a stopped run, as after a failed step
    keep = [0, 4, 5, 6]                                          # a pivot, the joint 0-1 and the motor 1-2: no loop is left
    ens.set_joint_kinds(**{k: v[keep] for k, v in r.items()})
    ens.set_joint_angles(theta[:, keep])
    res = ens.run_jointed(6, F, schedule=([2, 1], rates[:, :, keep]), stride=2, **KW)
    assert res.accepted.tolist() == [6, 6] and (res.resid_max < RTOL).all() and not all(_bits(p, q) for p, q in zip(before, ens.get_config()))
    # four steps of the first phase and two of the second
    assert np.abs(res.theta[:, 3] - (theta[:, 6] + (4 * rates[0, :, 6] + 2 * rates[1, :, 6]) * DT)).max() <= 1e-15
    ens.close()


# ------------------------------------------------------------------------------------------------ 6: reject
def test_reject_keeps_a_failed_replicas_motor_still(orc):
    """replica 1 carries a load that puts a blob below the wall in one step -- shown first on the numpy restatement of the step
    --, the others the ordinary loads.  Rejected in every step, it keeps its configuration, angle and place in the cycle; the
    others are bitwise the loop"""
    c = _case()
    cfg, a = _params()
    bad = 1
    F = c["F"].copy()
    F[bad] = 0.0
    F[bad, 2::6] = 3.0e4                                        # (F_body is the load the fluid resists: +z pushes down)
    k0 = _phase(START[bad])
    cc = dict(cfg=cfg, X=c["X"][bad], Q=c["Q"][bad], a=a, eta=1.0)
    Xo, Qo, _ = jk.numpy_steps(orc, cc, c["r"], True, F[bad], c["slip"][bad], c["v"], 1.0, DT, c["rates"][k0, bad][None])
    lowest = min((Xo[b][None, :] + cfg @ jo.rot(Qo[b]).T)[:, 2].min() for b in range(3))
    print("numpy restatement: the lowest blob of the loaded replica after one step is at z = %.3f" % lowest)
    assert lowest < -1.0
    ens = _ensemble(c["X"], c["Q"], True)
    ens.set_joint_kinds(**c["r"])
    theta0 = np.zeros((3, 5))
    theta0[:, 1] = [0.0, 0.02, -0.03]
    ens.set_joint_angles(theta0)
    X0, Q0 = ens.get_config()                                    # (the quaternions as set_config normalised them)
    res = ens.run_jointed(STEPS, F, slip=c["slip"], joint_velocity=c["v"], gamma=1.0, schedule=(PHASES, c["rates"]), cycle_start=START,
                          stride=STRIDE, on_error="reject", **KW)
    X, Q = ens.get_config()
    state = ens.joint_state()
    ens.close()
    assert res.accepted.tolist() == [STEPS, 0, STEPS] and res.rejected.tolist() == [0, STEPS, 0] and res.stopped_at == -1
    assert res.first_status.tolist() == [0, 2, 0]                # RBL_ERR_BELOW_WALL
    assert _bits(X[bad], X0[bad]) and _bits(Q[bad], Q0[bad]) and _bits(res.theta[bad], theta0[bad]) and res.cycle_pos[bad] == START[bad]
    assert _bits(res.X[:, bad], np.array([X0[bad]] * 2)) and _bits(res.Q[:, bad], np.array([Q0[bad]] * 2))
    assert not res.phi_sum[bad].any() and not res.frame_phi[:, bad].any() and _bits(res.frame_theta[:, bad], np.array([theta0[bad]] * 2))
    assert np.isnan(res.phi_mean[bad]).all() and res.accepted_at[:, bad].tolist() == [0, 0]
    # the others: the loop on a twin ensemble of the two
    good = [0, 2]
    twin = _ensemble(c["X"][good], c["Q"][good], True)
    twin.set_joint_kinds(**c["r"])
    twin.set_joint_angles(theta0[good])
    ref = _loop(twin, good)
    twin.close()
    for name, mine, theirs in (("X", X[good], ref["Xf"]), ("Q", Q[good], ref["Qf"]), ("theta", res.theta[good], ref["thetaf"]),
                               ("cycle_pos", res.cycle_pos[good], ref["cycle_pos"]), ("iters_sum", res.iters_sum[good], ref["iters_sum"]),
                               ("resid_max", res.resid_max[good], ref["resid_max"]), ("phi_sum", res.phi_sum[good], ref["phi_sum"]),
                               ("frame X", res.X[:, good], np.array(ref["X"])), ("frame theta", res.frame_theta[:, good], np.array(ref["theta"])),
                               ("frame phi", res.frame_phi[:, good], np.array(ref["phi"])), ("frame gap", res.frame_gap[:, good], np.array(ref["gap"])),
                               ("joint_state phi", state[1][good], ref["phif"]), ("joint_state gap", state[0][good], ref["gapf"])):
        assert _bits(mine, theirs), name


# ------------------------------------------------------------------------------------------------ 7: the field clock and the schedule
def test_the_field_clock_and_the_schedule_run_together():
    c = _case()
    t0 = np.array([0.37, -0.2, 1.05])

    def driven():
        ens = _ensemble(c["X"], c["Q"], True)
        ens.set_joint_kinds(**c["r"])
        ens.set_dipoles(3.0 * np.array([0.6, 0.0, 0.8]))
        ens.set_magnetic_field(B1=[2.0, 0.0, 0.0], B2=[0.0, 0.0, 2.0], omega=2.0)
        ens.set_field_time(t0)
        return ens

    ens = driven()
    assert np.abs(ens.interaction_forces()).max() > 0.1
    ref = _loop(ens, slice(0, 3), before_step=lambda e, n: e.set_field_time(t0 + DT * n))
    ens.close()
    ens = driven()
    res = _run(ens, slice(0, 3))
    assert np.array_equal(ens.field_time(), t0)                  # the run leaves the context's field times as they were
    _run_is_loop(res, ens, ref, "with a rotating field")
    ens.close()
    assert not _bits(ref["Xf"], _loop_together(True)["Xf"])      # the field mattered


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_come_before_any_motion():
    from rigid_body_light_amd._lib import RblError, RunJointOpts, RunJointOut, RunOpts, RunOut
    c = _case()
    F, sched = c["F"], (PHASES, c["rates"])
    hot = _ensemble(c["X"], c["Q"], True, kBT=0.01)
    hot.set_joint_kinds(**c["r"])
    before = hot.get_config()
    with pytest.raises(RblError, match=r"brownian.*drift.*status 11"):
        hot.ctx.ensemble_run_jointed(STEPS, F, phase_steps=PHASES, phase_rates=c["rates"], brownian=True, **KW)
    assert all(_bits(p, q) for p, q in zip(before, hot.get_config()))
    hot.close()
    ens = _ensemble(c["X"], c["Q"], True)
    ens.set_joint_kinds(**c["r"])
    before = ens.get_config()
    ctx = ens.ctx
    on_the_ball = c["rates"].copy()
    on_the_ball[2, 1, 4] = 0.25
    for match, call in (
            (r"prescribed.*masks.*status 11", lambda: ctx.ensemble_run_jointed(STEPS, F, prescribed=np.zeros((3, 3), dtype=np.uint8), **KW)),
            (r"phase 2, set 1, joint 4.*only a lock joint.*status 11",
             lambda: ctx.ensemble_run_jointed(STEPS, F, phase_steps=PHASES, phase_rates=on_the_ball, **KW)),
            (r"phase_steps\[1\] = 0.*status 11", lambda: ctx.ensemble_run_jointed(STEPS, F, phase_steps=[3, 0, 4, 2], phase_rates=c["rates"], **KW)),
            (r"cycle_start\[2\] = 10.*outside the cycle.*status 11",
             lambda: ctx.ensemble_run_jointed(STEPS, F, phase_steps=PHASES, phase_rates=c["rates"], cycle_start=[0, 4, 10], **KW)),
            (r"cycle_start\[0\] = -1.*status 11",
             lambda: ctx.ensemble_run_jointed(STEPS, F, phase_steps=PHASES, phase_rates=c["rates"], cycle_start=-1, **KW))):
        with pytest.raises(RblError, match=match):
            call()
        assert all(_bits(p, q) for p, q in zip(before, ens.get_config()))
    # the ensemble's periodic cell
    ens.set_cell(40.0, 40.0)
    with pytest.raises(RblError, match=r"periodic.*status 7"):
        ens.run_jointed(STEPS, F, schedule=sched, **KW)
    ens.set_cell(40.0, 40.0, on=False)
    assert all(_bits(p, q) for p, q in zip(before, ens.get_config()))
    # wrong struct sizes, through the raw call
    Fc = np.ascontiguousarray(F)
    for k, name in enumerate(("rbl_run_opts", "rbl_run_joint_opts", "rbl_run_out", "rbl_run_joint_out")):
        s = [RunOpts(), RunJointOpts(), RunOut(), RunJointOut()]
        for x in s:
            x.size = ctypes.sizeof(x)
        s[0].n_steps, s[0].max_iter, s[0].rtol, s[0].F_body, s[1].gamma = STEPS, MAXIT, RTOL, Fc.ctypes.data, 1.0
        s[k].size -= 8
        rc = ctx.L.rbl_ensemble_run_jointed(ctx.h, *[ctypes.byref(x) for x in s])
        assert rc == 11 and name in ctx.L.rbl_last_error(ctx.h).decode(), name
    assert all(_bits(p, q) for p, q in zip(before, ens.get_config())) and not ens.joint_state(phi=False)[2].any()
    # and the ensemble still runs; the first moments a one-step call recorded are not there after a run, as after Ensemble.run
    ens.record_moments(True)
    ens.step_jointed(F, **KW)
    assert np.isfinite(ens.step_moments()).all()
    res = ens.run_jointed(2, F, schedule=sched, **KW)
    assert res.accepted.tolist() == [2, 2, 2]
    with pytest.raises(RblError, match=r"no ensemble step has recorded first moments.*status 7"):
        ens.step_moments()
    ens.close()


# ------------------------------------------------------------------------------------------------ 9: existing paths unmoved
def test_the_one_step_call_and_a_plain_run_after_a_jointed_run_are_those_of_a_fresh_twin():
    c = _case()
    res, X, Q, state = _together(True)
    rate = np.zeros((3, 5))
    rate[:, 1] = [0.4, -0.7, 0.2]

    def after(ens):
        stepped = ens.step_jointed(c["F"], slip=c["slip"], joint_velocity=c["v"], gamma=0.5, **KW)
        mid = tuple(ens.get_config()) + tuple(ens.joint_state())
        plain = ens.run(4, F=c["F"], slip=c["slip"], brownian=True, seed=9, stride=2, **KW)
        return tuple(stepped) + mid + tuple(ens.get_config()) + (plain.X, plain.Q, plain.iters_sum, plain.resid_max, plain.accepted)

    # the rates are stored BEFORE the run: its schedule is an argument, never state, so the step after it turns the motors by these
    ens = _ensemble(c["X"], c["Q"], True, kBT=0.01)
    ens.set_joint_kinds(**c["r"])
    ens.set_joint_rates(rate)
    mine_run = _run(ens, slice(0, 3))
    assert _bits(mine_run.theta, res.theta)                      # (kBT plays no part in a jointed run)
    mine = after(ens)
    ens.close()
    # the twin never saw a run: it gets to the same configuration and angles by the loop of one-step calls (test 1: the same bits)
    twin = _ensemble(c["X"], c["Q"], True, kBT=0.01)
    twin.set_joint_kinds(**c["r"])
    _loop(twin, slice(0, 3), stride=0)
    twin.set_joint_rates(rate)
    theirs = after(twin)
    twin.close()
    for k, (p, q) in enumerate(zip(mine, theirs)):
        assert _bits(p, q), k
    assert _bits(mine[7], res.theta + rate * DT)                 # phi, its, res, X, Q, gap, phi, theta: the angles after the step
