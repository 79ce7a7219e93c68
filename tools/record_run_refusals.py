"""Record what the four run entry points (rbl_ensemble_run, _run_jointed, _run_observed, _run_driven) answer to malformed
requests: rows [entry, case, status, message] in a JSON file.  tests/test_ensemble_run_refusals_cpu.py replays the same
cases (it imports CPU_CASES / GPU_CASES and replay() from here) and compares status and message byte for byte, so the table
recorded on one commit pins the order of refusals, the status codes and the names that lead the messages for the next.

    python tools/record_run_refusals.py [--root DIR] [--gpu] [--out tests/golden/ensemble_run_refusals.json]

--root: the built checkout whose library answers (default: this one).  Without --gpu only the cases that are decided on a
context without an ensemble are run: they touch no device.  --gpu adds the cases that need R (an ensemble of R = 2 replicas of
two 12-blob shells, 2 steps) and keeps the CPU rows of an existing file.

A case: entry, what the context is (ctx), which optional structs travel (jointed, observed), the fields changed from a valid
request ("o.n_steps": 0; "@name": the address of an array of the pool), the structs passed as NULL (null), and for the GPU cases
what is switched on around the call (joints, cell).  Its name is its description."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("run", "run_jointed", "run_observed", "run_driven")


def _pool():
    bad, nan = np.arange(15.0), np.arange(15.0)
    bad[3 * 3 + 1], nan[14] = np.inf, np.nan
    return {"F": np.zeros(64), "fr": np.zeros(4096), "pts": np.arange(15.0) + 1.0, "pts3": np.arange(90.0) + 1.0, "bad": bad, "nan": nan,
            "mask": np.zeros(48, dtype=np.uint8), "bi": np.zeros(48), "omega": np.array([2.0]), "t0": np.array([0.5]),
            "nan1": np.array([np.nan]), "inf1": np.array([np.inf]), "nanF": np.full(64, np.nan),
            "ps": np.array([1, 2, 1], dtype=np.int32), "ps0": np.array([1, 0, 1], dtype=np.int32),
            "ps31": np.array([2**30, 2**30, 5], dtype=np.int32), "pin": np.zeros(192),
            "cs3": np.array([3], dtype=np.int32), "cs4": np.array([4], dtype=np.int32), "csm1": np.array([-1], dtype=np.int32),
            "cs1": np.array([1], dtype=np.int32), "cs0": np.array([0], dtype=np.int32),
            # a schedule for the two joints of the motor (a ball joint, a lock joint): 2 phases, 1 or 3 sets
            "jps": np.array([2, 3], dtype=np.int32), "jrates": np.array([0.0, 0.5, 0.0, -0.5] * 3),
            "jrates_ball": np.array([0.25, 0.5, 0.0, -0.5]), "jcs5": np.array([5, 0, 0], dtype=np.int32)}


POOL = _pool()


def case(entry, ctx=None, jointed=False, observed=False, null=(), joints=False, cell=False, **change):
    assert entry in ENTRIES
    d = dict(entry=entry, ctx=dict(ctx or {}), jointed=jointed, observed=observed, null=list(null), joints=joints, cell=cell,
             change={k.replace("__", "."): v for k, v in change.items()})
    d["name"] = json.dumps({k: v for k, v in d.items() if k != "entry" and v not in ({}, [], False)}, sort_keys=True)
    return d


def _cpu_cases():
    c = []
    masked = dict(o__F_body=None, o__prescribed="@mask", o__body_in="@bi")
    frames = dict(out__frame_X="@fr", out__frame_Q="@fr", out__frame_accepted_at="@fr")
    # ---- rbl_ensemble_run (tests/test_ensemble_run_cpu.py)
    c += [case("run", null=[n]) for n in ("o", "out", "h")]
    for ch in (dict(o__size=8), dict(out__size=0), dict(o__n_steps=0), dict(o__n_steps=-2), dict(o__stride=-1), dict(o__check_every=-1),
               dict(o__on_error=2), dict(o__on_error=-1), dict(o__F_body=None), dict(o__prescribed="@mask", o__body_in="@bi"),
               dict(o__body_in="@bi"), dict(o__F_body=None, o__prescribed="@mask"), dict(o__F_body=None, o__body_in="@bi"),
               dict(o__max_iter=0), dict(o__max_iter=-3), dict(o__rtol=-1.0), dict(o__rtol="nan"), dict(o__stride=2),
               dict(o__stride=1, out__frame_X="@fr", out__frame_Q="@fr"), dict(o__stride=1, **frames, **masked),
               dict(o__max_iter=256), dict(o__max_iter=256, **masked), dict(o__prescribed_per=3), dict(o__prescribed_per=6, **masked),
               dict(), masked, dict(o__stride=5), dict(o__brownian=0, o__on_error=1)):
        c.append(case("run", **ch))
    for ctx in (dict(params=False), dict(comm=True)):
        c += [case("run", ctx=ctx), case("run", ctx=ctx, **masked)]
    # ---- rbl_ensemble_run_jointed (tests/test_ensemble_run_joints_cpu.py)
    cold = dict(kBT=0.0, a=0.4)
    c += [case("run_jointed", ctx=cold, null=[n]) for n in ("h", "o", "jo", "out", "jout")]
    c += [case("run_jointed", ctx=cold, **{s + "__size": "+8"}) for s in ("o", "jo", "out", "jout")]
    for motor in (False, True):
        ctx = dict(cold, motor=motor)
        for ch in (dict(o__n_steps=0), dict(o__stride=-1), dict(o__check_every=-1), dict(o__on_error=2), dict(o__prescribed_per=6),
                   dict(o__max_iter=0), dict(o__max_iter=256), dict(o__rtol=-1.0), dict(o__prescribed="@mask"), dict(o__body_in="@F"),
                   dict(jo__gamma=-0.1), dict(jo__gamma=1.5), dict(jo__gamma="nan"), dict(o__F_body=None), dict(), dict(o__stride=2),
                   dict(jo__n_phases=-1), dict(jo__start_sets=1), dict(jo__n_phases=2, jo__rate_sets=1, jo__phase_steps="@jps", jo__phase_rates="@jrates")):
            c.append(case("run_jointed", ctx=ctx, **ch))
    hot = dict(kBT=0.01, a=0.4)
    c += [case("run_jointed", ctx=hot, o__brownian=1), case("run_jointed", ctx=cold, o__brownian=1),
          case("run_jointed", ctx=dict(cold, dt=0.0, motor=True)), case("run_jointed", ctx=dict(cold, dt=0.0)),
          case("run_jointed", ctx=dict(cold, motor=True, comm=True)), case("run_jointed", ctx=dict(cold, comm=True))]
    # ---- rbl_ensemble_run_observed (tests/test_ensemble_observed_cpu.py)
    for jointed in (False, True):
        c += [case("run_observed", jointed=jointed, null=[n]) for n in ("h", "obs", "oout", "o", "out")]
        for ch in (dict(obs__size=8), dict(oout__size=0), dict(obs__n_probes=-1), dict(obs__points=None), dict(obs__point_sets=0),
                   dict(obs__point_sets=-3), dict(obs__probe_body=-2), dict(obs__points="@bad"), dict(obs__points="@nan"),
                   dict(o__stride=2, oout__frame_D="@fr", **frames), dict(o__stride=2, oout__frame_u="@fr", **frames),
                   dict(o__stride=2, obs__moments=0, **frames), dict(o__stride=2, obs__n_probes=0, **frames),
                   dict(o__n_steps=0), dict(o__size=8), dict(out__size=0), dict(o__stride=-1), dict(o__on_error=2), dict(o__F_body=None),
                   dict(o__max_iter=0), dict(o__rtol=-1.0), dict(o__stride=2, oout__frame_u="@fr", oout__frame_D="@fr"),
                   dict(), dict(obs__n_probes=0, obs__moments=0), dict(obs__moments=0), dict(obs__n_probes=0), dict(o__stride=5),
                   dict(obs__n_probes=0, obs__moments=0, obs__point_sets=-7, obs__probe_body=-9, obs__points=None)):
            c.append(case("run_observed", jointed=jointed, **ch))
    c += [case("run_observed", jointed=True, null=["jout"]), case("run_observed", jointed=True, jo__size=8),
          case("run_observed", jointed=True, ctx=dict(motor=True, kBT=0.0), jo__gamma=2.0)]
    # ---- rbl_ensemble_run_driven (tests/test_ensemble_driven_cpu.py)
    for ch in (dict(d__size=8), dict(dq__size=16), dict(d__n_phases=-1), dict(d__omega=None), dict(d__t0=None), dict(d__phase_steps=None),
               dict(d__phase_in=None), dict(d__cycle_start=None), dict(d__omega="@nan1"), dict(d__t0="@inf1"), dict(d__phase_steps="@ps0"),
               dict(d__phase_steps="@ps31"), dict(d__cycle_start="@cs4"), dict(d__cycle_start="@csm1"),
               dict(d__n_phases=0, d__cycle_start="@cs1"), dict(d__cos_amp="@nanF"), dict()):
        c.append(case("run_driven", **ch))
    c += [case("run_driven", null=["d", "dq"]), case("run_driven", null=["o"]), case("run_driven", null=["h"]), case("run_driven", null=["dq"]),
          case("run_driven", null=["out"]), case("run_driven", ctx=dict(dt=0.0)), case("run_driven", ctx=dict(dt=0.0), d__cos_amp=None, d__lockin=0),
          case("run_driven", observed=True), case("run_driven", observed=True, null=["oout"]), case("run_driven", observed=True, obs__size=8),
          case("run_driven", ctx=dict(comm=True)), case("run_driven", ctx=dict(params=False))]
    empty = dict(d__cos_amp=None, d__lockin=0, d__n_phases=0, d__start_sets=0)      # nothing drives: the underlying run
    c += [case("run_driven", **empty), case("run_driven", o__n_steps=0, **empty), case("run_driven", observed=True, o__n_steps=0, **empty),
          case("run_driven", null=["dq"], **empty), case("run_driven", observed=True, obs__n_probes=-1, **empty)]
    # ---- two faults from two different layers: which one is named
    c += [case("run_observed", obs__size=8, o__n_steps=0), case("run_observed", jointed=True, obs__size=8, o__n_steps=0),
          case("run_driven", d__n_phases=-1, o__size=8), case("run_driven", d__omega=None, o__size=8),
          case("run_driven", observed=True, d__n_phases=-1, obs__size=8),
          case("run_jointed", ctx=cold, o__stride=-1, jo__gamma=2.0), case("run_jointed", ctx=dict(cold, motor=True), o__stride=-1, jo__gamma=2.0),
          case("run_observed", o__stride=2, o__size=8, oout__frame_D="@fr", **frames),
          case("run_observed", jointed=True, o__stride=2, o__size=8, oout__frame_D="@fr", **frames),
          case("run_driven", null=["dq"], o__n_steps=0), case("run_driven", observed=True, null=["dq"], o__n_steps=0),
          case("run_jointed", ctx=cold, o__prescribed="@mask", o__on_error=2), case("run_jointed", ctx=dict(cold, motor=True), o__prescribed="@mask", o__on_error=2),
          case("run_observed", jointed=True, o__prescribed="@mask", o__on_error=2),
          case("run_driven", observed=True, obs__n_probes=-1, o__n_steps=0), case("run_driven", dq__size=16, d__size=8),
          case("run_observed", obs__points="@bad", out__size=0), case("run_driven", observed=True, o__stride=2, **frames),
          case("run_observed", jointed=True, obs__n_probes=-1, jo__gamma=2.0), case("run_jointed", ctx=hot, o__brownian=1, o__max_iter=0),
          case("run", o__max_iter=256, o__rtol=-1.0), case("run", o__stride=2, o__max_iter=0), case("run", ctx=dict(params=False), o__n_steps=0)]
    return c


def _gpu_cases():
    motor = dict(joints=True)
    sched = dict(jo__n_phases=2, jo__rate_sets=1, jo__phase_steps="@jps", jo__phase_rates="@jrates")
    cold = dict(o__brownian=0)
    return [case("run_observed", obs__point_sets=3, obs__points="@pts3"), case("run_observed", obs__probe_body=2),
            case("run_observed", jointed=True, obs__point_sets=3, obs__points="@pts3", **motor),
            case("run_driven", observed=True, obs__probe_body=2),
            case("run_jointed", **motor, **dict(sched, jo__rate_sets=3)), case("run_jointed", **motor, jo__start_sets=3, jo__cycle_start="@jcs5", **sched),
            case("run_jointed", **motor, jo__start_sets=1, jo__cycle_start="@jcs5", **sched),
            case("run_jointed", **motor, jo__start_sets=1, jo__cycle_start="@cs1"),
            case("run_jointed", **motor, **dict(sched, jo__phase_rates="@jrates_ball")),
            case("run_jointed", **sched),                                        # a schedule with the joints off
            case("run_driven", **motor, **cold), case("run_driven", observed=True, **motor, **cold),
            case("run_jointed", cell=True, **motor), case("run_jointed", cell=True), case("run_observed", jointed=True, cell=True, **motor),
            case("run", o__prescribed_per=6, o__F_body=None, o__prescribed="@mask", o__body_in="@bi"),
            case("run_driven", o__prescribed_per=6, o__F_body=None, o__prescribed="@mask", o__body_in="@bi", o__brownian=1),
            case("run_driven", d__amp_sets=3, **cold), case("run_driven", d__cycle_start="@cs4", **cold)]


CPU_CASES, GPU_CASES = _cpu_cases(), _gpu_cases()


def _value(v, old=None):
    if isinstance(v, str) and v.startswith("@"):
        return POOL[v[1:]].ctypes.data
    if v == "nan":
        return float("nan")
    if v == "+8":
        return old + 8
    return v


def _request(m, cs, n_steps):
    """the structs of a valid request of the case's entry point, its changes made -> {name: struct}"""
    S = dict(o=m.RunOpts(), out=m.RunOut(), jo=m.RunJointOpts(), jout=m.RunJointOut(), obs=m.RunObsOpts(), oout=m.RunObsOut(),
             d=m.RunDriveOpts(), dq=m.RunDriveOut())
    for s in S.values():
        s.size = C.sizeof(type(s))
    o, jo, obs, d = S["o"], S["jo"], S["obs"], S["d"]
    o.n_steps, o.brownian, o.split_rand, o.max_iter, o.seed, o.delta, o.rtol = n_steps, int(cs["entry"] == "run"), 1, 10, 1, 1e-4, 1e-8
    o.F_body = POOL["F"].ctypes.data
    jo.gamma = 1.0
    obs.n_probes, obs.point_sets, obs.probe_body, obs.moments, obs.points = 5, 1, -1, 1, POOL["pts"].ctypes.data
    d.amp_sets = d.omega_sets = d.t0_sets = d.phase_sets = d.start_sets = 1
    d.n_phases, d.lockin = 3, 1
    d.cos_amp, d.omega, d.t0 = POOL["F"].ctypes.data, POOL["omega"].ctypes.data, POOL["t0"].ctypes.data
    d.phase_steps, d.phase_in, d.cycle_start = POOL["ps"].ctypes.data, POOL["pin"].ctypes.data, POOL["cs3"].ctypes.data
    for k, v in cs["change"].items():
        tag, name = k.split(".")
        setattr(S[tag], name, _value(v, getattr(S[tag], name)))
    return S


def call(L, h, m, cs, n_steps=4):
    """-> (status, message) of the case's call on context h"""
    S = _request(m, cs, n_steps)
    p = {k: (None if k in cs["null"] else C.byref(s)) for k, s in S.items()}
    hh = None if "h" in cs["null"] else h
    e = cs["entry"]
    if e == "run":
        rc = L.rbl_ensemble_run(hh, p["o"], p["out"])
    elif e == "run_jointed":
        rc = L.rbl_ensemble_run_jointed(hh, p["o"], p["jo"], p["out"], p["jout"])
    elif e == "run_observed":
        j = cs["jointed"]
        rc = L.rbl_ensemble_run_observed(hh, p["o"], p["jo"] if j else None, p["obs"], p["out"], p["jout"] if j else None, p["oout"])
    else:
        ob = cs["observed"]
        rc = L.rbl_ensemble_run_driven(hh, p["o"], p["d"], p["obs"] if ob else None, p["out"], p["dq"], p["oout"] if ob else None)
    out = S["out"]
    left = "" if "out" in cs["null"] else " [steps_done %d, stopped_at %d, stop_replica %d]" % (out.steps_done, out.stopped_at, out.stop_replica)
    return rc, ("" if hh is None else L.rbl_last_error(h).decode()) + left


_MOTOR = dict(body=np.array([[0, 1], [0, 1]], dtype=np.int32), kind=np.array([0, 1], dtype=np.int32), anchor=np.zeros((2, 6)),
              axis=np.tile([0.0, 0.0, 1.0], (2, 1)), q_rel=np.tile([1.0, 0.0, 0.0, 0.0], (2, 1)))
_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
_cb = _CB(lambda user, buf, n: 0)


def _set_motor(L, h, on=1):
    M = _MOTOR
    assert L.rbl_set_joint_kinds(h, 2, M["body"].ctypes.data, M["anchor"].ctypes.data, M["kind"].ctypes.data, M["axis"].ctypes.data,
                                 M["q_rel"].ctypes.data, on) == 0


def _context(L, pkg, params=True, kBT=1.0, dt=0.01, a=None, motor=False, comm=False):
    """parameters (or none), no ensemble: such a context never initialises a device"""
    h = L.rbl_create()
    if params:
        p, cfg = pkg.load_structure(12)
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)
        assert L.rbl_set_parameters(h, p["sep"] / 2.0 if a is None else a, dt, kBT, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    if motor:
        _set_motor(L, h)
    if comm:
        L.rbl_set_comm_ops.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.rbl_set_comm_ops(h, 0, 2, C.cast(_cb, C.c_void_p), None, None) == 0
    return h


def load(root):
    """(package, its _lib module, the library) of the built checkout at root"""
    import importlib
    sys.path.insert(0, root)
    pkg = importlib.import_module("rigid_body_light_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(root), pkg.__file__
    m = importlib.import_module("rigid_body_light_amd._lib")
    return pkg, m, m.lib()


def replay_cpu(pkg, m, L):
    rows = []
    for cs in CPU_CASES:
        h = _context(L, pkg, **cs["ctx"])
        rc, msg = call(L, h, m, cs)
        L.rbl_destroy(h)
        rows.append([cs["entry"], cs["name"], rc, msg])
    return rows


def replay_gpu(pkg, m, L):
    """R = 2 replicas of two 12-blob shells above the wall at kBT > 0; after every case a one-step call still works"""
    p, cfg = pkg.load_structure(12)
    X = np.array([[[0.0, 0.0, 4.0], [6.0, 0.0, 4.0]], [[0.1, 0.0, 4.1], [6.0, 0.2, 4.0]]])
    Q = np.tile([1.0, 0.0, 0.0, 0.0], (2, 2, 1))
    ens = pkg.Ensemble(cfg, X, Q, a=p["sep"] / 2.0, eta=1.0, dt=0.01, kBT=0.01, wall=True)
    h = ens.ctx.h
    rows = []
    for cs in GPU_CASES:
        if cs["joints"]:
            _set_motor(L, h)
        if cs["cell"]:
            ens.set_cell(40.0, 40.0)
        rc, msg = call(L, h, m, cs, n_steps=2)
        if cs["cell"]:
            ens.set_cell(40.0, 40.0, on=False)
        if cs["joints"]:
            _set_motor(L, h, on=0)
        assert rc != 0, (cs["name"], "was not refused")
        its, res = ens.step_deterministic(np.zeros((2, 12)), max_iter=50, rtol=1e-8)
        assert (its >= 0).all() and np.isfinite(res).all(), cs["name"]
        rows.append([cs["entry"], cs["name"], rc, msg])
    ens.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "ensemble_run_refusals.json"))
    args = ap.parse_args()
    pkg, m, L = load(os.path.abspath(args.root))
    table = {"cpu": [], "gpu": []}
    if os.path.exists(args.out):
        table.update(json.load(open(args.out)))
    if args.gpu:
        table["gpu"] = replay_gpu(pkg, m, L)
    else:
        table["cpu"] = replay_cpu(pkg, m, L)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:                         # one row a line
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in table[k])) for k in ("cpu", "gpu")) + "\n}\n")
    print("%d cpu rows, %d gpu rows -> %s" % (len(table["cpu"]), len(table["gpu"]), args.out))


if __name__ == "__main__":
    main()
