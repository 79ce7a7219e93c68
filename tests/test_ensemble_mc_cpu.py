"""Metropolis sampling of the force model (include/rbl.h section 5, rbl_ensemble_mc; Ensemble.metropolis): what can be checked
without a device -- the declaration and the layout of the two structs, every refusal that is decided before the library touches the
GPU, the argument rules of the Python layer, and the numpy oracle of the GPU tests (tests/mc_oracle.py) against the existing oracles."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_shapes  # noqa: E402
import bond_oracle  # noqa: E402
import mc_oracle  # noqa: E402
import table_oracle  # noqa: E402
import typed_oracle  # noqa: E402

RBL_ERR_STATE, RBL_ERR_ARG = 7, 11
_KEEP = []


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


def _args(**change):
    from rigid_body_light_amd._lib import McOpts, McOut
    o, out = McOpts(), McOut()
    o.size, out.size = C.sizeof(McOpts), C.sizeof(McOut)
    o.n_sweeps, o.step_x, o.step_theta, o.seed = 4, 0.1, 0.1, 1
    for k, v in change.items():
        if k.startswith("out_"):
            setattr(out, k[4:], v)
        else:
            setattr(o, k, v)
    return o, out


def _run(L, h, **change):
    o, out = _args(**change)
    return L.rbl_ensemble_mc(h, C.byref(o), C.byref(out)), L.rbl_last_error(h)


def test_the_entry_point_and_its_structs_are_declared_and_exported():
    from rigid_body_light_amd._lib import McOpts, McOut
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rbl_ensemble_mc\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+rbl_mc_opts\s*\*\s*opts\s*,\s*rbl_mc_out\s*\*\s*out\s*\)", code)
    assert hasattr(_lib(), "rbl_ensemble_mc")
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    for word in ("rbl_ensemble_mc", "Philox", "0x4D430000", "detailed balance", "Hastings", "wall_rejected", "replica exchange"):
        assert word in sec5, word
    for name, cls in (("rbl_mc_opts", McOpts), ("rbl_mc_out", McOut)):     # the ctypes mirror has the header's fields, in order
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(McOpts) == 4 * 8 + 2 * 8 + 6 * 4 + 2 * 8 and C.sizeof(McOut) == 8 + 9 * 8


def test_every_refusal_is_decided_before_a_device_is_touched():
    L = _lib()
    h = _ctx(L)                                          # parameters, no ensemble: this context never initialises a device
    o, out = _args()
    assert L.rbl_ensemble_mc(h, None, C.byref(out)) == RBL_ERR_ARG and b"NULL" in L.rbl_last_error(h)
    assert L.rbl_ensemble_mc(h, C.byref(o), None) == RBL_ERR_ARG and b"NULL" in L.rbl_last_error(h)
    assert L.rbl_ensemble_mc(None, C.byref(o), C.byref(out)) == RBL_ERR_ARG
    kT, bad_kT, nan_kT, fz, fr = np.array([1.0, 2.0]), np.array([1.0, 0.0]), np.array([np.nan]), np.zeros(8, dtype=np.uint8), np.zeros(64)
    _KEEP.extend([kT, bad_kT, nan_kT, fz, fr])
    for change, word in (
            (dict(size=8), b"opts.size"), (dict(out_size=0), b"out.size"),
            (dict(n_sweeps=0), b"n_sweeps"), (dict(n_sweeps=-3), b"n_sweeps"),
            (dict(step_x=-0.1), b"step_x"), (dict(step_x=float("inf")), b"step_x"), (dict(step_theta=-1.0), b"step_theta"),
            (dict(step_theta=float("nan")), b"step_theta"),
            (dict(kBT_sets=1, kBT=bad_kT[1:].ctypes.data), b"kBT[0]"), (dict(kBT_sets=1, kBT=nan_kT.ctypes.data), b"kBT[0]"),
            (dict(kBT_sets=1), b"kBT is NULL"), (dict(kBT_sets=-1), b"kBT_sets"),
            (dict(frozen_sets=-2), b"frozen_sets"), (dict(frozen_sets=1), b"frozen is NULL"),
            (dict(stride=-1), b"stride"), (dict(n_trace=-1), b"n_trace"), (dict(sweep_start=-1), b"sweep_start"),
            (dict(replica_base=-1), b"replica_base"),
            (dict(stride=2), b"frame_X"), (dict(stride=1, out_frame_X=fr.ctypes.data, out_frame_Q=fr.ctypes.data), b"frame_E"),
            (dict(n_trace=3), b"trace"),
    ):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_ARG and word in msg, (change, rc, msg)
    # nothing wrong but the state (entries of kBT beyond the first are read only once kBT_sets is known to be R: here R is unknown)
    for change in (dict(), dict(stride=9), dict(kBT_sets=2, kBT=kT.ctypes.data), dict(kBT_sets=2, kBT=bad_kT.ctypes.data)):
        rc, msg = _run(L, h, **change)
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg, (change, rc, msg)
    # hard joints and the dipole terms: RBL_ERR_STATE, the term named
    L.rbl_set_joints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    body, anchor = np.array([0, 1], dtype=np.int32), np.zeros(6)
    assert L.rbl_set_joints(h, 1, body.ctypes.data, anchor.ctypes.data, 1) == 0
    rc, msg = _run(L, h)
    assert rc == RBL_ERR_STATE and b"joints" in msg
    assert L.rbl_set_joints(h, 1, body.ctypes.data, anchor.ctypes.data, 0) == 0
    m = np.array([0.0, 0.0, 1.0])
    assert L.rbl_set_dipoles(h, m.ctypes.data, 1, 1.0, 1.0, 10.0, 1) == 0
    rc, msg = _run(L, h)
    assert rc == RBL_ERR_STATE and b"dipole pair" in msg
    assert L.rbl_set_dipoles(h, m.ctypes.data, 1, 0.0, 1.0, 10.0, 1) == 0
    B = np.array([0.0, 0.0, 1.0])
    Z = np.zeros(3)
    assert L.rbl_set_magnetic_field(h, B.ctypes.data, Z.ctypes.data, Z.ctypes.data, 0.0, 1) == 0
    rc, msg = _run(L, h)
    assert rc == RBL_ERR_STATE and b"field torque" in msg
    L.rbl_destroy(h)
    h = _ctx(L, params=False)
    assert _run(L, h)[0] == RBL_ERR_STATE
    L.rbl_destroy(h)
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = _ctx(L)
    assert L.rbl_set_comm_ops(h, 0, 2, C.cast(cb, C.c_void_p), None, None) == 0
    rc, msg = _run(L, h)
    assert rc == RBL_ERR_ARG and b"communicator" in msg
    L.rbl_destroy(h)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _ensemble(R=3, nb=4):
    """an Ensemble over a binding that knows its shape and whose library fails the test when called: DeviceContext.ensemble_mc, the
    one owner of the argument checks, raises before it gets there"""
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import DeviceContext
    ctx = DeviceContext.__new__(DeviceContext)
    ctx.L, ctx.h, ctx._borrowed = _NoLibrary(), None, True
    ctx.ensemble_info = lambda: (R, nb)
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = R, nb, 12, ctx
    return e


@pytest.mark.parametrize("kwargs", [
    dict(n_sweeps=0), dict(n_sweeps=-1),
    dict(step_x=-0.1), dict(step_x=np.nan), dict(step_theta=-0.2), dict(step_theta=np.inf),
    dict(kBT=0.0), dict(kBT=-1.0), dict(kBT=[1.0, np.nan, 1.0]), dict(kBT=[1.0, 2.0]), dict(kBT=np.ones((3, 1))),
    dict(frozen=[0, 1, 0]), dict(frozen=np.zeros((2, 4))), dict(frozen=np.zeros((3, 4, 1))),
    dict(stride=-1), dict(trace=-1), dict(sweep_start=-1), dict(replica_base=-2),
])
def test_metropolis_argument_errors_raise_before_the_library_is_called(kwargs):
    e = _ensemble()
    args = dict(n_sweeps=4, step_x=0.1, step_theta=0.1)
    args.update(kwargs)
    with pytest.raises(ValueError):
        e.metropolis(**args)
    if "n_sweeps" not in kwargs and set(kwargs) <= {"kBT", "frozen"}:
        with pytest.raises(ValueError):
            e.metropolis_tune(rounds=1, **kwargs)


def test_metropolis_tune_argument_errors():
    e = _ensemble()
    for kw in (dict(target=0.0), dict(target=1.0), dict(rounds=0)):
        with pytest.raises(ValueError):
            e.metropolis_tune(**kw)


def test_the_option_is_named_and_bounded():
    L = _lib()
    k = L.rbl_option_key(b"mc_sweeps_per_launch")
    nm, lo, hi, df = C.c_char_p(), C.c_int64(), C.c_int64(), C.c_int64()
    assert k > 0 and L.rbl_option_info(k, C.byref(nm), C.byref(lo), C.byref(hi), C.byref(df)) == 0
    assert lo.value == 1 and hi.value >= 1024 and lo.value <= df.value <= hi.value


# ---- the oracle of the GPU tests against the existing oracles ---------------------------------------------------------------------
def _case(nb, seed, wall=True):
    from rigid_body_light_amd import load_structure
    p, cfg = load_structure(12)
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    X = np.stack([np.array([2.6 * (i % 2), 2.6 * (i // 2), 2.2]) for i in range(nb)]) + rng.uniform(-0.3, 0.3, (nb, 3))
    Q = rng.standard_normal((nb, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return p["sep"] / 2.0, cfg, X, Q


def _tab(f, df, lo, hi, n):
    x = np.linspace(lo, hi, n)
    return f(x), df(x), lo, hi


def test_the_oracle_agrees_with_the_existing_oracles():
    a, cfg, X, Q = _case(4, 3)
    builtin = dict(w=0.4, eps_wall=3.0, b_wall=0.2, eps_blob=2.0, b_blob=0.3, r_cut=2.5 * a)
    pair = _tab(lambda r: 0.7 * np.cos(r), lambda r: -0.7 * np.sin(r), 0.2, 3.0 * a, 65)
    height = _tab(lambda z: 0.1 * (z - 3.0) ** 2, lambda z: 0.2 * (z - 3.0), 0.5, 4.0, 33)
    traps = (np.full((4, 3), 0.5) * [1.0, 0.0, 2.0], X + 0.2)
    types = np.tile((cfg - cfg.mean(axis=0))[:, 2] > 0.0, 4).astype(int)
    tables = {(0, 0): _tab(lambda r: 0.3 / (r + 0.5), lambda r: -0.3 / (r + 0.5) ** 2, 0.0, 2.8 * a, 33),
              (0, 1): _tab(lambda r: -0.5 * np.exp(-r), lambda r: 0.5 * np.exp(-r), 0.1, 3.2 * a, 33)}
    r = mc_oracle.positions(cfg, X, Q).reshape(-1, 3)
    m = dict(a=a, wall=True, builtin=builtin, pair=pair, height=height, traps=traps)
    Eo = table_oracle.interactions(r, X, 12, a, True, builtin=builtin, pair=pair, height=height, traps=traps)[2]
    E = mc_oracle.energy_terms(m, cfg, X, Q)
    assert E["pairs"] != 0.0 and E["traps"] != 0.0 and abs(E["total"] - Eo) <= 1e-12 * abs(Eo)
    m = dict(a=a, wall=True, builtin=builtin, pair=pair, types=types, tables=tables)
    Eo = typed_oracle.interactions(r, X, 12, a, True, types=types, tables=tables, builtin=builtin, pair=pair)[2]
    assert abs(mc_oracle.energy_terms(m, cfg, X, Q)["total"] - Eo) <= 1e-12 * abs(Eo)
    L = (9.0, 0.0)                                       # one axis periodic: the minimum image
    m["L"] = L
    Eo = typed_oracle.interactions(r, X, 12, a, True, types=types, tables=tables, builtin=builtin, pair=pair, L=L)[2]
    assert abs(mc_oracle.energy_terms(m, cfg, X, Q)["total"] - Eo) <= 1e-12 * abs(Eo)
    # bonds: a chain, a tabulated bond and a tether
    c0 = cfg - cfg.mean(axis=0)
    bonds = dict(body=[[0, 1], [1, 2], [2, 3], [0, -1]], anchor=np.concatenate([np.tile(np.concatenate([c0[0], c0[5]]), (3, 1)),
                 [np.concatenate([c0[2], [0.0, 0.0, 3.0]])]]), k=np.array([2.0, 1.5, 1.0, 0.5]), l0=np.array([1.0, 1.2, 0.0, 0.5]),
                 kind=[0, 0, 1, 0], table=_tab(lambda d: 0.5 * d * d, lambda d: d, 0.5, 2.0, 17))
    Eo = bond_oracle.bonds(X, Q, bonds["body"], bonds["anchor"], bonds["k"], bonds["l0"], kind=bonds["kind"], table=bonds["table"])[1]
    E = mc_oracle.energy_terms(dict(a=a, wall=True, bonds=bonds), cfg, X, Q)
    assert abs(E["total"] - Eo) <= 1e-12 * abs(Eo) and E["blob"] == 0.0
    # what the bodies take part in adds up: every pair and body-body bond is counted by both of its bodies
    m = dict(a=a, wall=True, builtin=builtin, pair=pair, height=height, traps=traps, types=types, tables=tables, bonds=bonds)
    T = mc_oracle.energy_terms(m, cfg, X, Q)
    parts = sum(mc_oracle.body_energy(m, cfg, X, Q, b)[0] for b in range(4))
    bb = sum(mc_oracle.bond_energy(m, X, Q, k) for k in range(3))
    assert abs(parts - (T["total"] + T["pairs"] + bb)) <= 1e-12 * (abs(T["total"]) + abs(T["pairs"]))


def test_the_oracle_s_body_update_is_the_library_s():
    """update_X_Q against the host restatement the steps integrate with (c_rigid.update_X_Q needs a device; the formula is the
    header's): a rotation by phi about the lab axes, composed from the left"""
    X, Q = np.array([0.1, 0.2, 0.3]), np.array([1.0, 0.0, 0.0, 0.0])
    Xn, Qn = mc_oracle.update_X_Q(X, Q, np.array([1.0, 2.0, 3.0, 0.0, 0.0, np.pi / 2]))
    assert np.allclose(Xn, [1.1, 2.2, 3.3]) and np.allclose(mc_oracle.rot(Qn) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    X2, Q2 = mc_oracle.update_X_Q(Xn, Qn, np.array([0.0, 0.0, 0.0, np.pi / 2, 0.0, 0.0]))
    assert np.allclose(mc_oracle.rot(Q2) @ [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]) and abs(np.linalg.norm(Q2) - 1.0) < 1e-15
    assert np.array_equal(mc_oracle.update_X_Q(X, Q, np.zeros(6))[1], Q)
