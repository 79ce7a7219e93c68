"""The drive of a driven ensemble run (include/rbl.h section 5, rbl_ensemble_run_driven) restated in numpy, statement for statement:

    t   = t0 + dt * n                       the product rounded, then the sum
    arg = omega * t                         one rounded product
    in  = ((A0 + P[phase(p)]) + C * cos(arg)) + S * sin(arg)

with absent parts entering as zeros.  numpy evaluates each operator on float64 arrays with one rounding, so the only difference to
the device is libm's cos / sin against the device's sincos.  Used by tests/test_ensemble_driven_gpu.py and checked on its own by
tests/test_ensemble_driven_cpu.py."""
import numpy as np


def schedule_phase(phase_steps, pos):
    """the phase whose half-open range of the prefix sums holds pos (0 <= pos < the cycle's length)"""
    cum = np.concatenate([[0], np.cumsum(np.asarray(phase_steps, dtype=np.int64))])
    assert 0 <= pos < cum[-1]
    return int(np.searchsorted(cum, pos, side="right") - 1)


def schedule_next(phase_steps, pos):
    """the position after one committed step"""
    return 0 if pos + 1 == int(np.sum(np.asarray(phase_steps, dtype=np.int64))) else pos + 1


def clock(t0, dt, n):
    """t0 + dt * n per replica, two roundings.  t0: None, a number or (R,); n: (R,) integers"""
    n = np.asarray(n, dtype=np.float64)
    s = np.float64(dt) * n
    return (np.zeros_like(n) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), n.shape)) + s


def _sets(a, R, per):
    """(per,) or (R, per) -> (R, per); None -> zeros"""
    if a is None:
        return np.zeros((R, per))
    return np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, per), (R, per))


def drive_eval(A0, dt, accepted, cos=None, sin=None, omega=0.0, t0=None, phase_steps=None, phase_in=None, cycle_pos=None, cs_sn=None):
    """-> (input (R, per), cs_sn (R, 2), parts (R, per): |A0| + |P| + |C| + |S|, the scale of the rounding bound).  A0 (R, per);
    accepted (R,); cos, sin (per,) or (R, per); omega, t0 a number or (R,); phase_in (n_phases, per) or (n_phases, R, per) with
    cycle_pos (R,).  cs_sn (R, 2): these values stand for libm's cos and sin (the device's, as rbl_ensemble_drive_eval returns them)"""
    A0 = np.asarray(A0, dtype=np.float64)
    R, per = A0.shape
    if cs_sn is None:
        t = clock(t0, dt, accepted)
        arg = np.broadcast_to(np.asarray(omega, dtype=np.float64), (R,)) * t
        cs, sn = np.cos(arg), np.sin(arg)
    else:
        cs, sn = np.asarray(cs_sn)[:, 0], np.asarray(cs_sn)[:, 1]
    P = np.zeros((R, per))
    if phase_steps is not None:
        pi = np.asarray(phase_in, dtype=np.float64)
        if pi.ndim == 2:
            pi = np.broadcast_to(pi[:, None, :], (pi.shape[0], R, per))
        for r in range(R):
            P[r] = pi[schedule_phase(phase_steps, int(cycle_pos[r])), r]
    C, S = _sets(cos, R, per), _sets(sin, R, per)
    a = A0 + P
    hc = C * cs[:, None]
    hs = S * sn[:, None]
    v = (a + hc) + hs
    return v, np.stack([cs, sn], axis=1), np.abs(A0) + np.abs(P) + np.abs(C) + np.abs(S)


def lockin_sums(values, cs_sn, committed):
    """sum over the steps n, in step order, of values[n] * cs_sn[n][:, 0] and * cs_sn[n][:, 1] where committed[n] (R,) is true:
    values (steps, R, ...), cs_sn (steps, R, 2) -> (sum_c, sum_s), product and sum rounded one after the other"""
    values = np.asarray(values, dtype=np.float64)
    sc, ss = np.zeros(values.shape[1:]), np.zeros(values.shape[1:])
    for n in range(values.shape[0]):
        shape = (-1,) + (1,) * (values.ndim - 2)
        ok = np.asarray(committed[n], dtype=bool).reshape(shape)
        pc = values[n] * cs_sn[n][:, 0].reshape(shape)
        ps = values[n] * cs_sn[n][:, 1].reshape(shape)
        sc = np.where(ok, sc + pc, sc)
        ss = np.where(ok, ss + ps, ss)
    return sc, ss


def lockin_norm(cs_sn, committed):
    """norm (R, 5) = sum cs, sn, cs^2, sn^2, cs sn over the committed steps, in step order"""
    R = cs_sn[0].shape[0]
    out = np.zeros((R, 5))
    for n in range(len(cs_sn)):
        cs, sn = cs_sn[n][:, 0], cs_sn[n][:, 1]
        q = np.stack([cs, sn, cs * cs, sn * sn, cs * sn], axis=1)
        out = np.where(np.asarray(committed[n], dtype=bool)[:, None], out + q, out)
    return out
