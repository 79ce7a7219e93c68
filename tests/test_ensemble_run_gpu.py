"""Runs of ensemble steps on the GPU (include/rbl.h section 5, rbl_ensemble_run; Ensemble.run): a run is the loop of one-step calls,
bitwise -- configurations, frames, iteration sums, loads; the stop policy leaves what the loop leaves when it raises; the reject
policy freezes the failing replica and no other, validates a new configuration before it commits and keeps a clock per replica; a
run goes on from where the last one ended and leaves the one-step calls as they were; and the example runs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import random_positions  # noqa: E402


def _shell12():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return {"cfg": cfg, "a": p["sep"] / 2.0, "eta": 1.0, "dt": 0.01}


def _configs(R, nb, wall=True):
    X, Q = np.zeros((R, nb, 3)), np.zeros((R, nb, 4))
    for r in range(R):
        x, q = random_positions(nb, wall=wall, seed=100 + r, min_dist=4.0)
        if wall:
            x[:, 2] += 1.5
        X[r], Q[r] = x, q
    return X, Q


def _model(a):
    return dict(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=2 * a + 20 * 0.05)


def _ens(c, X, Q, dt=None, kBT=1.0, model=False, flow=False):
    from rigid_body_light_amd import Ensemble
    e = Ensemble(c["cfg"], X, Q, a=c["a"], eta=c["eta"], dt=c["dt"] if dt is None else dt, kBT=kBT, wall=True)
    if model:
        e.set_interactions(**_model(c["a"]))
    if flow:                                            # with the wall only u = (G02 z, G12 z, 0) is a flow
        G = np.zeros((3, 3)); G[0, 2], G[1, 2] = 0.3, -0.1
        e.set_background_flow(G=G)
        e.set_body_slip(0.05 * np.random.default_rng(8).standard_normal((12, 3)), scale=np.linspace(0.5, 1.5, X.shape[1]))
    return e


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("family", ["brownian", "deterministic", "masked"])
def test_a_run_is_the_loop_bitwise(family):
    c = _shell12()
    R, nb, steps = 5, 3, 6
    X0, Q0 = _configs(R, nb)
    rng = np.random.default_rng(11)
    F = 0.5 * rng.standard_normal((R, 6 * nb))
    slip = 0.01 * rng.standard_normal((R, 3 * nb * 12))
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 0] = True
    mask[1] = [False, False, True]                      # another body in replica 1
    body_in = F.copy().reshape(R, nb, 6)
    body_in[mask] = [0.02, 0.0, 0.01, 0.0, 0.03, 0.0]   # driven
    body_in = body_in.reshape(R, 6 * nb)
    kw = dict(max_iter=50, rtol=1e-8)
    # the loop of one-step calls
    ens = _ens(c, X0, Q0, model=True, flow=True)
    its, res, Fs, cfgs = [], [], [], []
    for n in range(steps):
        if family == "brownian":
            it, rs = ens.step_brownian(F, seed=40 + n, slip=slip, **kw)
        elif family == "deterministic":
            it, rs = ens.step_deterministic(F, slip=slip, **kw)
        else:
            Fn, it, rs = ens.step_brownian_mixed(mask, body_in, seed=40 + n, slip=slip, **kw)
            Fs.append(Fn)
        its.append(it); res.append(rs); cfgs.append(ens.get_config())
    ens.close()
    outs = []
    for check_every in (0, 2):
        ens = _ens(c, X0, Q0, model=True, flow=True)
        if family == "masked":
            out = ens.run(steps, prescribed=mask, body_in=body_in, seed=40, stride=2, slip=slip, check_every=check_every, **kw)
        else:
            out = ens.run(steps, F=F, brownian=family == "brownian", seed=40, stride=2, slip=slip, check_every=check_every, **kw)
        Xr, Qr = ens.get_config()
        ens.close()
        assert np.array_equal(Xr, cfgs[-1][0]) and np.array_equal(Qr, cfgs[-1][1])
        assert out.X.shape == (3, R, nb, 3) and out.Q.shape == (3, R, nb, 4)
        for k in range(3):
            assert np.array_equal(out.X[k], cfgs[2 * k + 1][0]) and np.array_equal(out.Q[k], cfgs[2 * k + 1][1]), k
            assert np.array_equal(out.accepted_at[k], np.full(R, 2 * k + 2))
        assert np.array_equal(out.iters_sum, np.sum(its, axis=0))
        assert np.array_equal(out.resid_max, np.max(res, axis=0))
        assert np.array_equal(out.accepted, np.full(R, steps)) and not out.rejected.any() and not out.first_status.any()
        assert (out.steps_done, out.stopped_at) == (steps, -1)
        if family == "masked":
            Fsum = np.zeros((R, 6 * nb))
            for Fn in Fs:
                Fsum += Fn                              # in step order, as the device adds them
            assert np.array_equal(out.F_sum, Fsum)
            assert np.array_equal(out.F_mean, Fsum / steps)
            for k in range(3):
                assert np.array_equal(out.F[k], Fs[2 * k + 1]), k
        else:
            assert out.F_mean is None and out.F is None
        outs.append(out)
    assert np.array_equal(outs[0].X, outs[1].X) and np.array_equal(outs[0].Q, outs[1].Q)   # check_every changes no bit


# ---------------------------------------------------------------------------------------------------------------- 2, 3, 5
_F_BAD = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], 3)


def _bad_start():
    """R = 4, N_bod = 3; replica 1 has a body below the wall from the start (tests/test_ensemble_gpu.py's error test)"""
    c = _shell12()
    X0, Q0 = _configs(4, 3)
    ens = _ens(c, X0, Q0)
    Xa, Qa = ens.get_config()                           # normalised quaternions
    ens.close()
    Xb = Xa.copy()
    Xb[1, 0, 2] = -0.5
    return c, Xa, Qa, Xb


@functools.lru_cache(maxsize=None)
def _reject_and_reference():
    """the reject run from the bad start (5 Brownian steps, a frame per step) and the stop run of the same ensemble with a valid
    replica 1: computed once, shared"""
    c, Xa, Qa, Xb = _bad_start()
    ens = _ens(c, Xb, Qa)
    out = ens.run(5, F=_F_BAD, seed=7, stride=1, on_error="reject", max_iter=40)       # does not raise
    end = ens.get_config()
    ens.close()
    ens = _ens(c, Xa, Qa)
    ref = ens.run(5, F=_F_BAD, seed=7, stride=1, on_error="stop", max_iter=40)
    ref_end = ens.get_config()
    ens.close()
    return Xb, Qa, out, end, ref, ref_end


def test_stop_leaves_what_the_loop_leaves():
    from rigid_body_light_amd._lib import RblError
    c, Xa, Qa, Xb = _bad_start()
    ens = _ens(c, Xb, Qa)
    with pytest.raises(RblError) as e:
        ens.run(4, F=_F_BAD, seed=7, stride=1, max_iter=40)
    msg = str(e.value)
    assert "[rbl status 2]" in msg and "replica 1" in msg and "step 0" in msg
    Xc, Qc = ens.get_config()
    assert np.array_equal(Xc, Xb) and np.array_equal(Qc, Qa)
    last = ens.last_run
    assert last.stopped_at == 0 and last.steps_done == 0 and last.stop_replica == 1
    assert not last.accepted.any()
    assert last.first_status[1] == 2 and last.rejected[1] == 1
    ens.set_config(Xa, Qa)                              # repaired: the one-step calls go on
    ens.step_brownian(_F_BAD, seed=3, max_iter=40)
    assert ens.run(2, F=_F_BAD, seed=4, max_iter=40).accepted.tolist() == [2, 2, 2, 2]
    ens.close()


def test_reject_freezes_the_failing_replica_and_no_other():
    Xb, Qa, out, (Xe, Qe), ref, (Xr, Qr) = _reject_and_reference()
    assert out.rejected[1] == 5 and out.accepted[1] == 0
    assert out.first_status[1] == 2                     # RBL_ERR_BELOW_WALL
    assert np.array_equal(Xe[1], Xb[1]) and np.array_equal(Qe[1], Qa[1])
    for k in range(5):
        assert np.array_equal(out.X[k, 1], Xb[1]) and np.array_equal(out.Q[k, 1], Qa[1])
    assert (out.stopped_at, out.steps_done) == (-1, 5)
    assert ref.accepted.tolist() == [5, 5, 5, 5] and ref.stopped_at == -1
    for r in (0, 2, 3):                                 # replicas do not interact, the noise depends on r and the step only
        assert out.accepted[r] == 5 and out.rejected[r] == 0 and out.first_status[r] == 0
        assert np.array_equal(Xe[r], Xr[r]) and np.array_equal(Qe[r], Qr[r])
        assert np.array_equal(out.X[:, r], ref.X[:, r]) and np.array_equal(out.Q[:, r], ref.Q[:, r])
        assert not np.array_equal(Xe[r], Xb[r])         # they moved


def test_frames_keep_a_clock_per_replica():
    _, _, out, _, _, _ = _reject_and_reference()
    assert out.accepted_at.shape == (5, 4)
    assert not out.accepted_at[:, 1].any()
    for r in (0, 2, 3):
        assert out.accepted_at[:, r].tolist() == [1, 2, 3, 4, 5]


# ---------------------------------------------------------------------------------------------------------------- 4
def test_a_new_configuration_is_validated_before_it_commits():
    """replica 2's lowest blob sits 0.02 above the wall and is pushed toward it (U = -N F_body: F_z > 0 pushes down); one step of
    dt = 40 carries it far below z = 0 -- the free-space displacement is dt F / (6 pi eta R_h) = 2.1, a hundred times the gap,
    so the wall's reduction of the mobility cannot save it"""
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, dt = 3, 40.0
    X0 = np.zeros((R, 1, 3)); Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (R, 1, 1))
    X0[0, 0], X0[1, 0] = [0.0, 0.0, 5.0], [1.0, 2.0, 6.0]
    X0[2, 0, 2] = -c["cfg"][:, 2].min() + 0.02
    F = np.zeros((R, 6))
    F[0], F[1], F[2] = [0.05, 0, 0, 0, 0, 0], [0, 0.03, -0.02, 0, 0.01, 0], [0, 0, 1.0, 0, 0, 0]
    # the premise, with the one-step calls: the first step succeeds and leaves replica 2 below the wall, the second says so
    ens = _ens(c, X0, Q0, dt=dt)
    ens.step_deterministic(F)
    X1, Q1 = ens.get_config()
    with pytest.raises(RblError) as e:
        ens.step_deterministic(F)
    assert "[rbl status 2]" in str(e.value) and "replica 2" in str(e.value)
    ens.close()
    # the loop of replicas 0 and 1 beside a harmless replica 2
    Xs = X0.copy(); Xs[2, 0, 2] = 7.0
    ens = _ens(c, Xs, Q0, dt=dt)
    for _ in range(4):
        ens.step_deterministic(F)
    Xl, Ql = ens.get_config()
    ens.close()
    # reject: the bad configuration never commits
    ens = _ens(c, X0, Q0, dt=dt)
    Xa, Qa = ens.get_config()
    out = ens.run(4, F=F, brownian=False, on_error="reject")
    Xe, Qe = ens.get_config()
    ens.close()
    assert out.accepted.tolist() == [4, 4, 0] and out.rejected.tolist() == [0, 0, 4]
    assert out.first_status.tolist() == [0, 0, 2]
    assert np.array_equal(Xe[2], Xa[2]) and np.array_equal(Qe[2], Qa[2])
    assert np.array_equal(Xe[:2], Xl[:2]) and np.array_equal(Qe[:2], Ql[:2])
    # stop reproduces the loop: step 0 commits (no validation, by design), step 1 stops the run
    ens = _ens(c, X0, Q0, dt=dt)
    with pytest.raises(RblError) as e:
        ens.run(4, F=F, brownian=False, on_error="stop")
    assert "[rbl status 2]" in str(e.value) and "replica 2" in str(e.value) and "step 1" in str(e.value)
    assert ens.last_run.stopped_at == 1 and ens.last_run.accepted.tolist() == [1, 1, 1]
    Xe, Qe = ens.get_config()
    ens.close()
    assert np.array_equal(Xe, X1) and np.array_equal(Qe, Q1)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_a_run_goes_on_from_where_it_ended_and_leaves_the_one_step_calls_alone():
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, nb = 3, 2
    X0, Q0 = _configs(R, nb)
    F = 0.3 * np.random.default_rng(12).standard_normal((R, 6 * nb))
    ens = _ens(c, X0, Q0, model=True)
    ens.run(6, F=F, seed=40)
    X6, Q6 = ens.get_config()
    ens.close()
    ens = _ens(c, X0, Q0, model=True)
    ens.record_moments(True)
    ens.step_brownian(F, seed=1)
    assert ens.step_moments().shape == (R, nb, 3, 3)
    ens.set_config(X0, Q0)
    ens.run(3, F=F, seed=40)
    with pytest.raises(RblError) as e:                  # a run records none
        ens.step_moments()
    assert "[rbl status 7]" in str(e.value)
    for n in range(3):
        ens.step_brownian(F, seed=43 + n)
    assert np.isfinite(ens.step_moments()).all()        # a one-step call has recorded again
    Xe, Qe = ens.get_config()
    ens.close()
    assert np.array_equal(Xe, X6) and np.array_equal(Qe, Q6)


def test_an_entry_of_prescribed_above_one_is_refused():
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    X0, Q0 = _configs(2, 2)
    ens = _ens(c, X0, Q0)
    mask = np.array([[0, 1], [2, 0]], dtype=np.uint8)
    with pytest.raises(RblError) as e:
        ens.ctx.ensemble_run(2, prescribed=mask, body_in=np.zeros(12))
    assert "[rbl status 11]" in str(e.value) and "prescribed" in str(e.value)
    Xe, Qe = ens.get_config()
    assert np.array_equal(Xe, X0)
    ens.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_example_ensemble_run_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_run.py"), "--replicas", "32", "--steps", "40",
                          "--burn", "10"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "rejected" in out.stdout and "mean" in out.stdout and "var" in out.stdout
