"""Driven ensemble runs on the GPU (include/rbl.h section 5, rbl_ensemble_run_driven / rbl_ensemble_drive_eval; Ensemble.run_driven,
Ensemble.drive_eval): an empty drive is the existing run, a driven run is the loop of drive_eval and the one-step call bit for
bit -- under both error policies --, replica r of R is the R = 1 run, a run goes on from another's cycle_pos and t_end, the kernel
agrees with the numpy restatement of the formula (tests/ensemble_drive_oracle.py), the lock-in sums are numpy's sums in step order,
a trapped shell under an oscillating force follows the explicit recursion, and every refusal leaves the ensemble as it was."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_drive_oracle as edo  # noqa: E402
from body_shapes import trimer  # noqa: E402
from conftest import random_positions  # noqa: E402

EPS = np.finfo(np.float64).eps
DT = 0.01
KW = dict(max_iter=50, rtol=1e-8)
PHASES = np.array([1, 2, 1], dtype=np.int32)
FAMILIES = ["deterministic", "brownian", "mixed", "brownian_mixed", "mixed_dof"]


def _shell12():
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    return cfg, p["sep"] / 2.0


def _configs(R, nb, wall=True):
    X, Q = np.zeros((R, nb, 3)), np.zeros((R, nb, 4))
    for r in range(R):
        x, q = random_positions(nb, wall=wall, seed=100 + r, min_dist=4.0)
        if wall:
            x[:, 2] += 1.5
        X[r], Q[r] = x, q
    return X, Q / np.linalg.norm(Q, axis=2, keepdims=True)


def _ens(X, Q, kBT=1.0, wall=True, cfg=None, a=None, dt=DT):
    from rigid_body_light_amd import Ensemble
    if cfg is None:
        cfg, a = _shell12()
    return Ensemble(cfg, X, Q, a=a, eta=1.0, dt=dt, kBT=kBT, wall=wall)


def _inputs(R, nb, seed=3):
    """A0, the mask of the masked families (body 0, in replica 1 the last body), the dof mask, C, S, omega and t0 per replica, a
    three-phase schedule of lengths 1, 2, 1 with inputs per replica, cycle starts per replica"""
    rng = np.random.default_rng(seed)
    d = dict(A0=0.5 * rng.standard_normal((R, 6 * nb)), C=0.3 * rng.standard_normal((R, 6 * nb)), S=0.2 * rng.standard_normal((R, 6 * nb)),
             omega=3.0 + 2.0 * np.arange(R), t0=0.37 + 0.11 * np.arange(R), P=0.1 * rng.standard_normal((3, R, 6 * nb)),
             start=np.arange(R, dtype=np.int32) % 4)
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 0] = True
    if R > 1:
        mask[1] = False
        mask[1, nb - 1] = True
    d["mask"] = mask
    dof = np.zeros((R, nb, 6), dtype=bool)
    dof[:, :, 2] = True                                 # z of every body prescribed
    dof[:, 0, 3:] = True                                # and the rotation of body 0
    d["dof"] = dof
    for key, m in (("bi", np.repeat(mask, 6, axis=1)), ("bi_dof", dof.reshape(R, 6 * nb))):
        for name in ("A0", "C", "S"):                   # prescribed entries are velocities: small ones
            v = d[name].copy()
            v[m] *= 0.05
            d[key + "_" + name] = v
    return d


def _family_args(family, d):
    """(run_driven's keywords naming A0 and the mask, the suffix of the inputs, brownian)"""
    if family in ("deterministic", "brownian"):
        return dict(F=d["A0"]), "", family == "brownian"
    if family == "mixed_dof":
        return dict(prescribed_dof=d["dof"], body_in=d["bi_dof_A0"]), "bi_dof_", False
    return dict(prescribed=d["mask"], body_in=d["bi_A0"]), "bi_", family == "brownian_mixed"


def _step(ens, family, d, inp, seed):
    """the one-step call of the family with the evaluated input -> F (R, 6 N_bod) or None"""
    if family == "deterministic":
        ens.step_deterministic(inp, **KW)
    elif family == "brownian":
        ens.step_brownian(inp, seed=seed, **KW)
    elif family == "mixed":
        return ens.step_mixed(d["mask"], inp, **KW)[0]
    elif family == "brownian_mixed":
        return ens.step_brownian_mixed(d["mask"], inp, seed=seed, **KW)[0]
    else:
        return ens.step_mixed_dof(d["dof"], inp, **KW)[0]
    return None


def _amps(d, pre):
    return (d[pre + "A0"], d[pre + "C"], d[pre + "S"]) if pre else (d["A0"], d["C"], d["S"])


def _loop(ens, family, d, steps, seed, pre, start=None, t0=None, first=0):
    """the loop a driven run replaces: drive_eval with the loop's own counters, then the one-step call -> (configurations after
    every step, F per step, cs_sn per step, the final cycle positions)"""
    A0, Cc, Ss = _amps(d, pre)
    R = A0.shape[0]
    pos = np.array(d["start"] if start is None else start, dtype=np.int32)
    t0 = d["t0"] if t0 is None else t0
    cfgs, Fs, cs = [], [], []
    for n in range(steps):
        inp, cs_sn = ens.drive_eval(A0, accepted=np.full(R, n, dtype=np.int32), cycle_pos=pos, cos=Cc, sin=Ss, omega=d["omega"], t0=t0,
                                    schedule=(PHASES, d["P"]))
        Fs.append(_step(ens, family, d, inp, seed + first + n))
        cs.append(cs_sn)
        cfgs.append(ens.get_config())
        pos = np.array([edo.schedule_next(PHASES, int(p)) for p in pos], dtype=np.int32)
    return cfgs, Fs, cs, pos


def _driven(ens, family, d, steps, seed, **more):
    args, pre, brownian = _family_args(family, d)
    A0, Cc, Ss = _amps(d, pre)
    kw = dict(cos=Cc, sin=Ss, omega=d["omega"], t0=d["t0"], schedule=(PHASES, d["P"]), cycle_start=d["start"], brownian=brownian, seed=seed,
              stride=1, **KW)
    kw.update(more)
    return ens.run_driven(steps, **args, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("family", ["deterministic", "brownian", "mixed", "brownian_mixed"])
def test_an_empty_drive_is_the_existing_run_bitwise(family):
    R, nb, steps = 3, 2, 5
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    args, _, brownian = _family_args(family, d)
    outs = []
    for driven in (False, True):
        ens = _ens(X0, Q0)
        run = ens.run_driven if driven else ens.run
        out = run(steps, brownian=brownian, seed=21, stride=2, **args, **KW)
        outs.append((out, ens.get_config()))
        ens.close()
    (a, ca), (b, cb) = outs
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])
    assert np.array_equal(a.X, b.X) and np.array_equal(a.Q, b.Q) and np.array_equal(a.accepted_at, b.accepted_at)
    for name in ("accepted", "rejected", "first_flags", "first_status", "iters_sum", "resid_max"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    if "mixed" in family:
        assert np.array_equal(a.F_sum, b.F_sum) and np.array_equal(a.F, b.F)
    assert b.cycle_pos.tolist() == [0] * R and np.array_equal(b.t_end, edo.clock(None, DT, b.accepted))
    assert b.X_c is None and b.norm is None


def test_an_empty_drive_with_observers_is_the_observed_run_bitwise():
    R, nb, steps = 3, 2, 4
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    pts = np.array([[0.0, 0.0, 3.0], [1.0, 2.0, 0.5]])
    outs = []
    for driven in (False, True):
        ens = _ens(X0, Q0)
        run = ens.run_driven if driven else ens.run
        outs.append(run(steps, F=d["A0"], seed=5, stride=1, probes=pts, moments=True, **KW))
        ens.close()
    a, b = outs
    for name in ("X", "Q", "u_sum", "D_sum", "frame_u", "frame_D", "iters_sum"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("family", FAMILIES)
def test_a_driven_run_is_the_loop_bitwise(family):
    R, nb, steps = 3, 2, 6
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    _, pre, _ = _family_args(family, d)
    ens = _ens(X0, Q0)
    cfgs, Fs, _, pos = _loop(ens, family, d, steps, 40, pre)
    ens.close()
    ens = _ens(X0, Q0)
    out = _driven(ens, family, d, steps, 40)
    Xr, Qr = ens.get_config()
    ens.close()
    assert np.array_equal(Xr, cfgs[-1][0]) and np.array_equal(Qr, cfgs[-1][1])
    for n in range(steps):
        assert np.array_equal(out.X[n], cfgs[n][0]) and np.array_equal(out.Q[n], cfgs[n][1]), n
    if Fs[0] is not None:
        Fsum = np.zeros_like(Fs[0])
        for n, Fn in enumerate(Fs):
            Fsum += Fn
            assert np.array_equal(out.F[n], Fn), n
        assert np.array_equal(out.F_sum, Fsum)
    assert np.array_equal(out.cycle_pos, pos)
    assert np.array_equal(out.t_end, edo.clock(d["t0"], DT, np.full(R, steps)))
    assert out.accepted.tolist() == [steps] * R


def test_under_reject_a_rejected_replica_s_clock_and_position_wait():
    """replica 1 starts with a body below the wall (tests/test_ensemble_run_gpu.py's bad start): every step of it is rejected, its
    cycle position and clock stay; the other replicas are the replicas of the run from a valid start"""
    R, nb, steps = 3, 2, 5
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    Xb = X0.copy()
    Xb[1, 0, 2] = -0.5
    ens = _ens(Xb, Q0)
    out = _driven(ens, "brownian", d, steps, 9, on_error="reject", lockin=True)
    ens.close()
    ens = _ens(X0, Q0)
    ref = _driven(ens, "brownian", d, steps, 9, lockin=True)
    ens.close()
    assert out.rejected.tolist() == [0, steps, 0] and out.accepted.tolist() == [steps, 0, steps]
    assert out.cycle_pos[1] == d["start"][1] and out.t_end[1] == d["t0"][1]      # lag by the rejected count: all of them
    assert not out.X_c[1].any() and not out.U_c[1].any() and not out.norm[1].any()
    for r in (0, 2):
        assert np.array_equal(out.X[:, r], ref.X[:, r]) and np.array_equal(out.Q[:, r], ref.Q[:, r])
        assert out.cycle_pos[r] == ref.cycle_pos[r] and out.t_end[r] == ref.t_end[r]
        for name in ("X_c", "X_s", "U_c", "U_s", "norm"):
            assert np.array_equal(getattr(out, name)[r], getattr(ref, name)[r]), name
    assert np.array_equal(out.X[:, 1], np.broadcast_to(Xb[1], (steps, nb, 3)))


def test_under_stop_nothing_moves_or_is_added_from_the_stopping_step_on():
    """a schedule whose second phase pushes replica 1 through the wall in one step: that step commits (the stop policy does not
    look ahead), the next one finds the blobs below the wall and stops the run.  What the run leaves is what the loop left when it
    raised, and the sums hold the steps before the stopping one"""
    from rigid_body_light_amd._lib import RblError
    R, nb, steps = 3, 1, 6
    X0, Q0 = _configs(R, nb)
    rng = np.random.default_rng(5)
    A0 = 0.2 * rng.standard_normal((R, 6))
    P = np.zeros((2, R, 6))
    P[1, 1, 2] = 4.0e5                                  # U = -N F_body: a positive entry pushes down
    C1, om, t0 = 0.1 * rng.standard_normal((R, 6)), np.array([2.0, 5.0, 9.0]), np.array([0.1, 0.2, 0.3])
    sched = (np.array([2, 1], dtype=np.int32), P)
    kw = dict(cos=C1, omega=om, t0=t0, schedule=sched)
    ens = _ens(X0, Q0, kBT=0.0)
    pos, cfgs, cs, failed = np.zeros(R, dtype=np.int32), [ens.get_config()], [], None
    for n in range(steps):
        inp, cs_sn = ens.drive_eval(A0, accepted=np.full(R, n, dtype=np.int32), cycle_pos=pos, **kw)
        try:
            ens.step_deterministic(inp, **KW)
        except RblError:
            failed = n
            break
        cs.append(cs_sn)
        cfgs.append(ens.get_config())
        pos = np.array([edo.schedule_next(sched[0], int(p)) for p in pos], dtype=np.int32)
    ens.close()
    assert failed == 3, failed                          # steps 0, 1 gentle, step 2 pushes, step 3 meets the wall
    ens = _ens(X0, Q0, kBT=0.0)
    with pytest.raises(RblError):
        ens.run_driven(steps, F=A0, brownian=False, stride=1, lockin=True, check_every=0, **kw, **KW)
    out = ens.last_run
    Xe, Qe = ens.get_config()
    ens.close()
    assert (out.stopped_at, out.steps_done, out.stop_replica) == (failed, failed, 1)
    assert np.array_equal(Xe, cfgs[-1][0]) and np.array_equal(Qe, cfgs[-1][1])
    for n in range(steps):                              # frames after the stop repeat the stopped configuration
        k = min(n + 1, failed)
        assert np.array_equal(out.X[n], cfgs[k][0]), n
    assert out.accepted.tolist() == [failed] * R
    assert np.array_equal(out.cycle_pos, pos) and np.array_equal(out.t_end, edo.clock(t0, DT, np.full(R, failed)))
    ok = [np.ones(R, dtype=bool)] * failed
    Xc, Xs = edo.lockin_sums([c[0] for c in cfgs[:failed]], cs, ok)
    assert np.array_equal(out.X_c, Xc) and np.array_equal(out.X_s, Xs)
    assert np.array_equal(out.norm, edo.lockin_norm(cs, ok))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("one_phase", [False, True])
def test_zero_frequency_is_the_run_with_the_summed_force(one_phase):
    R, nb, steps = 3, 2, 4
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    P = d["P"][:1]
    F = (d["A0"] + (P[0] if one_phase else 0.0)) + d["C"]
    ens = _ens(X0, Q0)
    ref = ens.run(steps, F=F, seed=2, stride=1, **KW)
    ens.close()
    for S in (None, np.zeros((R, 6 * nb))):
        ens = _ens(X0, Q0)
        out = ens.run_driven(steps, F=d["A0"], cos=d["C"], sin=S, omega=0.0, t0=d["t0"], schedule=([1], P) if one_phase else None, seed=2,
                             stride=1, **KW)
        ens.close()
        assert np.array_equal(out.X, ref.X) and np.array_equal(out.Q, ref.Q) and np.array_equal(out.iters_sum, ref.iters_sum)


# ---------------------------------------------------------------------------------------------------------------- 4
DT2 = 2.0 ** -7                                         # a dyadic dt and dyadic t0: every clock below is exact, so a run continued from
                                                        # t_end has the clocks of the long run bit for bit, not only up to rounding


def _dyadic(d):
    return dict(d, t0=0.375 + 0.125 * np.arange(d["A0"].shape[0]))


@functools.lru_cache(maxsize=None)
def _long_run(family):
    """the masked run of R = 3 over 8 steps that the replica and continuation tests compare with: computed once per family"""
    R, nb, steps = 3, 2, 8
    X0, Q0 = _configs(R, nb)
    d = _dyadic(_inputs(R, nb))
    ens = _ens(X0, Q0, dt=DT2)
    out = _driven(ens, family, d, steps, 17, lockin=True)
    ens.close()
    return X0, Q0, d, out


# (a replica's noise is drawn from its own counters, offset r of the batch: only replica 0 shares the R = 1 run's noise, so the
# Brownian family is compared for replica 0 and the deterministic one for the others)
@pytest.mark.parametrize("family,r", [("mixed", 0), ("mixed", 2), ("brownian_mixed", 0)])
def test_replica_r_of_R_is_the_single_replica_run(family, r):
    X0, Q0, d, ref = _long_run(family)
    one = {k: (v[:, r:r + 1] if k == "P" else v[r:r + 1]) for k, v in d.items()}
    ens = _ens(X0[r:r + 1], Q0[r:r + 1], dt=DT2)
    out = _driven(ens, family, one, 8, 17, lockin=True)
    ens.close()
    assert np.array_equal(out.X[:, 0], ref.X[:, r]) and np.array_equal(out.Q[:, 0], ref.Q[:, r]) and np.array_equal(out.F[:, 0], ref.F[:, r])
    for name in ("F_sum", "X_c", "X_s", "U_c", "U_s", "F_c", "F_s", "norm", "cycle_pos", "t_end"):
        assert np.array_equal(getattr(out, name)[0], getattr(ref, name)[r]), name


def test_a_second_run_continues_the_first():
    X0, Q0, d, ref = _long_run("brownian_mixed")
    ens = _ens(X0, Q0, dt=DT2)
    first = _driven(ens, "brownian_mixed", d, 3, 17)
    more = dict(d, start=first.cycle_pos, t0=first.t_end)
    second = _driven(ens, "brownian_mixed", more, 5, 17 + 3)
    ens.close()
    assert np.array_equal(first.X, ref.X[:3]) and np.array_equal(second.X, ref.X[3:]) and np.array_equal(second.Q, ref.Q[3:])
    assert np.array_equal(second.F, ref.F[3:])
    assert np.array_equal(second.cycle_pos, ref.cycle_pos) and np.array_equal(second.t_end, ref.t_end)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_drive_eval_agrees_with_numpy_within_the_rounding_bound():
    """per entry within 16 eps (|A0| + |P| + |C| + |S|): the argument omega t is bit-identical on both sides, the device's sincos
    and libm are each within 2 ulp, three roundings on each side -- about 8 eps, doubled.  Cases: moderate clocks; n = 9 with
    t0 = 0.37, dt = 0.01 (where a fused clock first differed); omega t about 1e6.  With the device's own cs, sn put into the numpy
    formula the agreement must be exact"""
    R, nb = 5, 2
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    ens = _ens(X0, Q0)
    worst = 0.0
    cases = [(np.arange(R) * 7, d["t0"], d["omega"]), (np.full(R, 9), np.full(R, 0.37), d["omega"]),
             (np.arange(R) + 30, 1.0e6 / d["omega"], d["omega"]), (np.full(R, 9), None, d["omega"])]
    for n, t0, om in cases:
        n = n.astype(np.int32)
        pos = (n % 4).astype(np.int32)
        got, cs_sn = ens.drive_eval(d["A0"], accepted=n, cycle_pos=pos, cos=d["C"], sin=d["S"], omega=om, t0=t0, schedule=(PHASES, d["P"]))
        ref, cs_ref, parts = edo.drive_eval(d["A0"], DT, n, cos=d["C"], sin=d["S"], omega=om, t0=t0, phase_steps=PHASES, phase_in=d["P"],
                                            cycle_pos=pos)
        ratio = (np.abs(got - ref) / (EPS * parts)).max()
        worst = max(worst, ratio)
        print("drive_eval vs numpy: worst |diff| / (eps * parts) = %.3f, cs/sn diff %.3g" % (ratio, np.abs(cs_sn - cs_ref).max()))
        assert ratio <= 16.0
        assert np.abs(cs_sn - cs_ref).max() <= 4 * EPS
        same, _, _ = edo.drive_eval(d["A0"], DT, n, cos=d["C"], sin=d["S"], phase_steps=PHASES, phase_in=d["P"], cycle_pos=pos, cs_sn=cs_sn)
        assert np.array_equal(got, same)
    ens.close()
    print("drive_eval vs numpy: worst ratio over the cases %.3f of the bound's 16" % worst)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_lockin_sums_are_numpy_s_sums_in_step_order():
    R, nb, steps = 3, 2, 7
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    ens = _ens(X0, Q0, kBT=0.0)
    out = _driven(ens, "mixed", d, steps, 0, lockin=True)
    # the cs, sn of every step, from the run's own kernel (every step accepted: the counters are the step numbers)
    cs = [ens.drive_eval(d["bi_A0"], accepted=np.full(R, n, dtype=np.int32), omega=d["omega"], t0=d["t0"])[1] for n in range(steps)]
    ens.close()
    ok = [np.ones(R, dtype=bool)] * steps
    Xn = np.concatenate([X0[None], out.X[:-1]])         # q^n: the frames shifted by one step
    Xc, Xs = edo.lockin_sums(Xn, cs, ok)
    assert np.array_equal(out.X_c, Xc) and np.array_equal(out.X_s, Xs)
    Fc, Fs = edo.lockin_sums(out.F, cs, ok)
    assert np.array_equal(out.F_c, Fc) and np.array_equal(out.F_s, Fs)
    assert np.array_equal(out.norm, edo.lockin_norm(cs, ok))
    # U from the frames: (X^{n+1} - X^n) / dt, translations only; a difference of frames loses digits, hence 1e-9 of the scale
    Ut = (out.X - Xn) / DT
    Uc, Us = edo.lockin_sums(Ut, cs, ok)
    for got, ref in ((out.U_c, Uc), (out.U_s, Us)):
        got = got.reshape(R, nb, 6)[:, :, :3]
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("U lock-in sums vs frame differences: %.3g" % err)
        assert err <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- 7
def test_a_trapped_shell_follows_the_explicit_recursion(orc):
    """free space, one shell_N_12 in a harmonic trap, F = F1 cos(omega t) along x: x_{n+1} = x_n + dt mu (-k (x_n - x0) + F1 cos
    (omega t_n)) with the oracle's body mobility mu (constant: an isolated shell), 1e-9 relative per step, accumulated linearly"""
    from body_shapes import dense
    cfg, a = _shell12()
    R, steps, k, F1 = 3, 40, 2.0, 1.5
    om = np.array([1.0, 6.0, 20.0])
    X0, Q0 = np.zeros((R, 1, 3)), np.tile([1.0, 0.0, 0.0, 0.0], (R, 1, 1))
    X0[:, 0, 0] = [0.3, -0.2, 0.0]
    M, K, _, _ = dense(orc, cfg, X0[0], Q0[0], a, 1.0, False)
    mu = np.linalg.inv(K.T @ np.linalg.solve(M, K))[0, 0]
    ens = _ens(X0, Q0, kBT=0.0, wall=False)
    U = ens.solve_mixed(np.zeros((R, 1), dtype=bool), np.array([1.0, 0, 0, 0, 0, 0]), max_iter=100, rtol=1e-13)[1]
    print("mu: oracle %.15g, the library's solve %.15g" % (mu, -U[0, 0]))
    assert abs(-U[0, 0] - mu) <= 1e-10 * mu             # U = -N F_body
    ens.set_traps(np.array([[k, 0.0, 0.0]]), np.zeros((1, 3)))
    amp = np.zeros(6)
    amp[0] = -F1                                        # F_body = -(the physical force)
    out = ens.run_driven(steps, F=np.zeros(6), cos=amp, omega=om, brownian=False, stride=1, lockin=True, max_iter=100, rtol=1e-13)
    ens.close()
    x, worst = X0[:, 0, 0].copy(), 0.0
    for n in range(steps):
        t = edo.clock(None, DT, np.full(R, n))
        x = x + DT * mu * (-k * x + F1 * np.cos(om * t))
        scale = np.abs(x).max() + DT * mu * F1
        worst = max(worst, np.abs(out.X[n, :, 0, 0] - x).max() / ((n + 1) * scale))
        assert np.abs(out.X[n, :, 0, 0] - x).max() <= 1e-9 * (n + 1) * scale, n
        assert np.abs(out.X[n, :, 0, 1:]).max() <= 1e-9 * (n + 1) * scale
    print("trapped shell vs the recursion: worst error per step %.3g of the scale" % worst)


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("R,nb", [(1, 1), (42, 1), (43, 1), (14, 3), (85, 1), (86, 1)])
def test_grid_edges_of_the_drive_kernel(R, nb):
    """R 6 N_bod = 6, 252, 258, 252, 510, 516: the entry counts next below and above one and two workgroups of 256 threads (a count
    is a multiple of 6, so 255, 256 and 257 themselves do not occur); amplitudes shared (amp_sets = 1), omega per replica
    (omega_sets = R), no phases and a cycle of length 1"""
    rng = np.random.default_rng(R * 100 + nb)
    X0 = np.zeros((R, nb, 3))
    X0[:, :, 0] = 3.0 * np.arange(nb)
    Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (R, nb, 1))
    A0, Cc, Ss = rng.standard_normal((R, 6 * nb)), rng.standard_normal(6 * nb), rng.standard_normal(6 * nb)
    om, n = 1.0 + np.arange(R), (np.arange(R) % 11).astype(np.int32)
    P = rng.standard_normal((1, 6 * nb))
    ens = _ens(X0, Q0, wall=False, cfg=trimer(), a=0.5)
    for sched in (None, ([1], P)):
        got, cs_sn = ens.drive_eval(A0, accepted=n, cos=Cc, sin=Ss, omega=om, schedule=sched)
        ref, _, _ = edo.drive_eval(A0, DT, n, cos=Cc, sin=Ss, phase_steps=None if sched is None else [1], phase_in=P,
                                   cycle_pos=np.zeros(R, dtype=np.int32), cs_sn=cs_sn)
        assert np.array_equal(got, ref)
        assert np.abs(cs_sn - np.stack([np.cos(om * edo.clock(None, DT, n)), np.sin(om * edo.clock(None, DT, n))], axis=1)).max() <= 4 * EPS
    ens.close()


def test_a_harmonic_run_without_phases_and_a_cycle_of_length_one():
    """R = 43 single trimers, 258 entries: the last replica sits in the second workgroup of both kernels.  n_phases = 0 and a cycle
    of one phase of zeros agree bitwise, and the last replica is its R = 1 run, lock-in sums included"""
    R, steps = 43, 3
    rng = np.random.default_rng(12)
    X0 = rng.uniform(-5.0, 5.0, (R, 1, 3))
    Q0 = np.tile([1.0, 0.0, 0.0, 0.0], (R, 1, 1))
    A0, Cc, Ss, om = rng.standard_normal((R, 6)), rng.standard_normal(6), rng.standard_normal(6), 1.0 + np.arange(R)
    kw = dict(cos=Cc, sin=Ss, brownian=False, stride=1, lockin=True, **KW)
    outs = []
    for sched in (None, ([1], np.zeros((1, 6)))):
        ens = _ens(X0, Q0, kBT=0.0, wall=False, cfg=trimer(), a=0.5)
        outs.append(ens.run_driven(steps, F=A0, omega=om, schedule=sched, **kw))
        ens.close()
    a, b = outs
    assert np.array_equal(a.X, b.X) and np.array_equal(a.U_c, b.U_c) and b.cycle_pos.tolist() == [0] * R
    assert not np.array_equal(a.X[:, 0] - X0[0], a.X[:, 1] - X0[1])   # omega per replica acts
    ens = _ens(X0[-1:], Q0[-1:], kBT=0.0, wall=False, cfg=trimer(), a=0.5)
    one = ens.run_driven(steps, F=A0[-1:], omega=om[-1:], **kw)
    ens.close()
    for name in ("X_c", "X_s", "U_c", "U_s", "norm", "t_end"):
        assert np.array_equal(getattr(one, name)[0], getattr(a, name)[-1]), name
    assert np.array_equal(one.X[:, 0], a.X[:, -1])


# ---------------------------------------------------------------------------------------------------------------- 9
def _raw(ens, d, **change):
    """rbl_ensemble_run_driven through ctypes with a valid deterministic run of 2 steps and a valid drive, the named fields of
    the drive changed -> (status, message)"""
    from rigid_body_light_amd._lib import RunDriveOut, RunOpts, RunOut, drive_opts
    R, nb = ens.R, ens.N_bodies
    L, h = ens.ctx.L, ens.ctx.h
    dd, keep = drive_opts("t", 6 * nb, cos=d["C"], sin=d["S"], omega=d["omega"], t0=d["t0"], phase_steps=PHASES, phase_in=d["P"],
                          cycle_start=d["start"], lockin=True)
    o, out, dq = RunOpts(), RunOut(), RunDriveOut()
    o.size, out.size, dq.size = C.sizeof(RunOpts), C.sizeof(RunOut), C.sizeof(RunDriveOut)
    o.n_steps, o.max_iter, o.rtol, o.F_body = 2, 50, 1e-8, d["A0"].ctypes.data
    for name, v in change.items():
        if name == "dq_size":
            dq.size = v
        elif name == "opts":
            for kk, vv in v.items():
                setattr(o, kk, vv)
        else:
            keep.append(v)
            setattr(dd, name, v.ctypes.data if isinstance(v, np.ndarray) else v)
    rc = L.rbl_ensemble_run_driven(h, C.byref(o), C.byref(dd), None, C.byref(out), C.byref(dq), None)
    return rc, L.rbl_last_error(h).decode()


def test_every_refusal_names_its_argument_and_leaves_the_ensemble_usable():
    ARG, STATE = 11, 7
    R, nb = 3, 2
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    ens = _ens(X0, Q0, kBT=0.0)
    bad = lambda a, i=0: np.where(np.arange(a.size).reshape(a.shape) == i, np.nan, a)   # noqa: E731
    cases = [
        (dict(size=8), "drive.size"), (dict(dq_size=8), "dout.size"),
        (dict(amp_sets=2), "amp_sets"), (dict(omega_sets=2), "omega_sets"), (dict(t0_sets=2), "t0_sets"),
        (dict(phase_sets=2), "phase_sets"), (dict(start_sets=2), "start_sets"), (dict(n_phases=-1), "n_phases"),
        (dict(omega=None), "omega is NULL"), (dict(t0=None), "t0 is NULL"), (dict(phase_steps=None), "phase_steps or phase_in"),
        (dict(phase_in=None), "phase_steps or phase_in"), (dict(cycle_start=None), "cycle_start is NULL"),
        (dict(cos_amp=bad(d["C"], 6 * nb + 1)), "cos_amp: set 1, entry 1"), (dict(sin_amp=bad(d["S"])), "sin_amp: set 0, entry 0"),
        (dict(omega=bad(d["omega"], 2)), "omega: set 2"), (dict(t0=np.array([0.0, np.inf, 0.0])), "t0: set 1"),
        (dict(phase_in=bad(d["P"], 6 * nb * R + 6 * nb + 3)), "phase_in: phase 1: set 1, entry 3"),
        (dict(phase_steps=np.array([1, 0, 1], dtype=np.int32)), "phase_steps[1] = 0"),
        (dict(phase_steps=np.array([2**30, 2**30, 1], dtype=np.int32)), "31 bits"),
        (dict(cycle_start=np.array([0, 4, 0], dtype=np.int32)), "cycle_start[1] = 4"),
        (dict(opts=dict(n_steps=0)), "n_steps"),                                       # the underlying run's own, unchanged
    ]
    for change, word in cases:
        rc, msg = _raw(ens, d, **change)
        assert rc == ARG and word in msg, (change, rc, msg)
        Xc, Qc = ens.get_config()
        assert np.array_equal(Xc, X0) and np.array_equal(Qc, Q0), change
    assert _raw(ens, d)[0] == 0                          # the valid call runs
    ens.close()
    # a Brownian run with prescribed_per = 6 stays refused, with the run's own message
    ens = _ens(X0, Q0, kBT=1.0)
    with pytest.raises(Exception) as e:
        ens.run_driven(2, prescribed_dof=d["dof"], body_in=d["bi_dof_A0"], cos=d["bi_dof_C"], omega=1.0)
    assert "whole-body masks only" in str(e.value)
    assert np.array_equal(ens.get_config()[0], X0)
    ens.close()
    # dt <= 0 with a harmonic part or lockin
    ens = _ens(X0, Q0, kBT=0.0, dt=0.0)
    rc, msg = _raw(ens, d)
    assert rc == ARG and "dt must be positive" in msg
    ens.close()


def test_with_joints_on_a_drive_is_refused_and_an_empty_one_runs():
    from rigid_body_light_amd._lib import RblError
    R, nb = 3, 2
    X0, Q0 = _configs(R, nb)
    d = _inputs(R, nb)
    ens = _ens(X0, Q0, kBT=0.0)
    ens.set_joint_kinds([[0, 1]], None, anchor_a=[[1.0, 0.0, 0.0]], anchor_b=[[-1.0, 0.0, 0.0]])
    with pytest.raises(RblError) as e:
        ens.run_driven(2, F=d["A0"], cos=d["C"], omega=1.0, brownian=False, **KW)
    assert "[rbl status 7]" in str(e.value) and "run_jointed" in str(e.value)
    assert np.array_equal(ens.get_config()[0], X0)
    out = ens.run_driven(2, F=d["A0"], brownian=False, **KW)        # empty: the plain run, which ignores the joints
    ref_ens = _ens(X0, Q0, kBT=0.0)
    ref = ref_ens.run(2, F=d["A0"], brownian=False, **KW)
    assert np.array_equal(ens.get_config()[0], ref_ens.get_config()[0]) and out.accepted.tolist() == ref.accepted.tolist()
    ens.close()
    ref_ens.close()


# ---------------------------------------------------------------------------------------------------------------- the example
def test_the_oscillatory_example_reproduces_the_single_relaxation_curve(capsys):
    """examples/ensemble_oscillatory.py, in this process: 64 frequencies in one run_driven, its own assertion (1e-6 F1 / k)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ensemble_oscillatory", os.path.join(ROOT, "examples", "ensemble_oscillatory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main()
    assert "single-relaxation curve" in capsys.readouterr().out
