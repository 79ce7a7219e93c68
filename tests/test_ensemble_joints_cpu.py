"""Hard joints in ensembles (include/rbl.h section 5) without a GPU: the refusals of the new entry points that a context without a
device reaches, the declarations and exports, the capacity rule held against its own stated formula, the Python layer's shape
checks, and the compiler's resource figures of k_gmres_small_jt.  No device is touched.  (The refusals that need an ensemble
configuration -- sets, a rate on a joint that is no lock, a body index beyond a replica, RBL_ERR_SIZE -- are in the GPU file.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import body_shapes as bs  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
ERR_STATE, ERR_ARG = 7, 11
NAN = float("nan")
NAMES = ("rbl_ensemble_set_joint_rates", "rbl_ensemble_set_joint_angles", "rbl_ensemble_solve_jointed", "rbl_ensemble_step_jointed",
         "rbl_ensemble_joint_state")


def _lib():
    from rigid_body_light_amd._lib import lib
    L = lib()
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    return L


def _context(L, dt=0.01):
    from rigid_body_light_amd import load_structure
    cfg = np.ascontiguousarray(load_structure(12)[1])
    h = L.rbl_create()
    assert L.rbl_set_parameters(h, 0.4, dt, 0.0, 1.0, cfg.ctypes.data, 12) == 0
    return h


def _set_motor(L, h):
    """a ball joint and a lock joint between the bodies 0 and 1 (no configuration is set: the indices are checked at use)"""
    body = np.array([[0, 1], [0, 1]], dtype=np.int32)
    kind = np.array([0, 1], dtype=np.int32)
    anchor, axis, q_rel = np.zeros((2, 6)), np.tile([0.0, 0.0, 1.0], (2, 1)), np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    assert L.rbl_set_joint_kinds(h, 2, body.ctypes.data, anchor.ctypes.data, kind.ctypes.data, axis.ctypes.data, q_rel.ctypes.data, 1) == 0


def test_the_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    assert re.search(r"\bint\s+rbl_ensemble_joints_fit\s*\(", code) and hasattr(L, "rbl_ensemble_joints_fit")
    for said in ("k_gmres_small_jt", "16 n_j + 18 n_j^2", "redundant", "rbl_ensemble_run"):
        assert said in text, said


def test_the_jointed_calls_refuse_before_any_device_work():
    L = _lib()
    h = _context(L)
    F, out, it, res = np.zeros(12), np.zeros(200), np.zeros(4, dtype=np.int32), np.zeros(4)
    f, o, tail = F.ctypes.data, out.ctypes.data, (it.ctypes.data, res.ctypes.data)

    def solve(ff=f, mi=50, rt=1e-8, hh=None):
        return L.rbl_ensemble_solve_jointed(h if hh is None else hh, ff, None, None, mi, rt, o, o, o, *tail)

    def step(ff=f, gamma=1.0, mi=50, rt=1e-8, hh=None):
        return L.rbl_ensemble_step_jointed(h if hh is None else hh, ff, None, None, gamma, mi, rt, o, *tail)

    def said(hh=None):
        return L.rbl_last_error(h if hh is None else hh)

    assert L.rbl_ensemble_solve_jointed(None, f, None, None, 50, 1e-8, o, o, o, *tail) == ERR_ARG
    assert L.rbl_ensemble_step_jointed(None, f, None, None, 1.0, 50, 1e-8, o, *tail) == ERR_ARG
    for with_joints in (False, True):
        if with_joints:
            _set_motor(L, h)
        for call in (solve, step):
            assert call(ff=None) == ERR_ARG and b"F_body is NULL" in said()
            for mi in (0, -3, 256):
                assert call(mi=mi) == ERR_ARG and b"max_iter" in said()
            for rt in (-1.0, NAN):
                assert call(rt=rt) == ERR_ARG and b"rtol" in said()
            assert call() == ERR_STATE and b"no ensemble configuration" in said()
        for g in (-0.1, 1.5, NAN):
            assert step(gamma=g) == ERR_ARG and b"gamma" in said()
    # dt <= 0 with the joints on: refused as rbl_step_jointed refuses it
    h0 = _context(L, dt=0.0)
    _set_motor(L, h0)
    assert step(hh=h0) == ERR_ARG and b"dt must be positive" in said(h0)
    L.rbl_destroy(h0)
    # rates, angles and the state query need the ensemble and the joints
    v = np.zeros(2)
    for fn in (L.rbl_ensemble_set_joint_rates, L.rbl_ensemble_set_joint_angles):
        assert fn(None, v.ctypes.data, 1) == ERR_ARG
        assert fn(h, v.ctypes.data, 1) == ERR_STATE and b"no ensemble configuration" in said()
    assert L.rbl_ensemble_joint_state(None, o, o, o) == ERR_ARG
    assert L.rbl_ensemble_joint_state(h, o, o, o) == ERR_STATE and b"no ensemble configuration" in said()
    # a communicator: RBL_ERR_ARG, joints on or off
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    for with_joints in (False, True):
        h3 = _context(L)
        if with_joints:
            _set_motor(L, h3)
        assert L.rbl_set_comm_ops(h3, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
        assert solve(hh=h3) == ERR_ARG and b"communicator" in said(h3)
        assert step(hh=h3) == ERR_ARG and b"communicator" in said(h3)
        L.rbl_destroy(h3)
    L.rbl_destroy(h)


# ---- the capacity rule: include/rbl.h section 5 states it; restated here ----------------------------------------------------------
def _stated_bytes(nblb, nb, m, nj):
    """rbl_gmres_small_fits' vectors (tests/body_shapes.py restates them) with 3 n_j more in each of the three vectors, and the
    joint data: 16 n_j + 18 n_j^2 + (7 n_j + N_bod + 2) / 2 doubles"""
    extra = 0 if nj == 0 else 3 * 3 * nj + 16 * nj + 18 * nj * nj + (7 * nj + nb + 2) // 2
    return bs.small_lds_bytes(nblb, nb, m) + 8 * extra


def _fits(L, nblb, nb, m, nj):
    b = ctypes.c_int64(0)
    ok = L.rbl_ensemble_joints_fit(nblb, nb, m, nj, ctypes.byref(b))
    return bool(ok), b.value


def test_the_capacity_rule_is_the_stated_formula():
    L = _lib()
    # every shape of the GPU tests fits: (bodies, joints) of the weld and motors, the hinge, case_steps, the hub, the cfg 1 chain
    for nb, nj, m in ((2, 2, 100), (3, 4, 60), (3, 4, 100), (3, 5, 100), (9, 16, 100), (10, 11, 100), (2, 5, 100)):
        ok, b = _fits(L, 12, nb, m, nj)
        assert ok and b == _stated_bytes(12, nb, m, nj) <= bs.SMALL_LDS_MAX, (nb, nj, m, b)
    assert _fits(L, 12, 9, 100, 16)[1] > 100 * 1024             # the largest: well beyond what the unjointed vectors take (73 KB)
    # the rule against the formula over a sweep, and the first joint count beyond it for the hub's and the chain's bodies
    for nb, m in ((9, 100), (10, 100), (3, 60), (12, 50)):
        answers = [_fits(L, 12, nb, m, nj) for nj in range(0, 40)]
        for nj, (ok, b) in enumerate(answers):
            assert b == _stated_bytes(12, nb, m, nj), (nb, m, nj)
            assert ok == (bs.small_fits(12, nb, m) and b <= bs.SMALL_LDS_MAX), (nb, m, nj)
        first = next(nj for nj, (ok, _) in enumerate(answers) if not ok)
        assert first >= 1 and _stated_bytes(12, nb, m, first - 1) <= bs.SMALL_LDS_MAX < _stated_bytes(12, nb, m, first), (nb, m, first)
    # zero joints: the plain predicate's answer, where it accepts and where it refuses
    for nblb, nb, m in ((12, 10, 100), (12, 21, 50), (12, 22, 50), (4, 49, 255), (4, 50, 255), (3, 64, 38), (3, 64, 39), (12, 10, 256), (12, 10, 0)):
        assert _fits(L, nblb, nb, m, 0)[0] == bs.small_fits(nblb, nb, m), (nblb, nb, m)
    assert not _fits(L, 12, 10, 100, -1)[0]


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    """stands where the device context would: it answers the host-side query of the stored joints (nj of them, switched on) and
    any other call into the library fails the test"""
    def __init__(self, nj):
        self.nj = nj

    def joints(self):
        return dict(on=True, body=np.zeros((self.nj, 2), dtype=np.int32), anchor_a=np.zeros((self.nj, 3)), anchor_b=np.zeros((self.nj, 3)))

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _ensemble(R=3, nb=4, nj=5):
    from rigid_body_light_amd import Ensemble
    e = Ensemble.__new__(Ensemble)
    e.R, e.N_bodies, e.blobs_per_body, e.ctx = R, nb, 12, _NoLibrary(nj)
    return e


def test_set_joints_still_refuses_and_points_at_set_joint_kinds():
    from rigid_body_light_amd import Ensemble
    e = _ensemble()
    with pytest.raises(ValueError, match="not offered for ensembles") as info:
        e.set_joints([[0, 1]], np.zeros(3), np.zeros(3))
    assert "set_joint_kinds" in str(info.value) and "set_joint_kinds" in Ensemble.set_joints.__doc__
    for name in ("set_joint_kinds", "joint_kinds", "set_joint_rates", "set_joint_angles", "solve_jointed", "step_jointed", "joint_state",
                 "hinge", "weld", "motor"):
        assert callable(getattr(Ensemble, name)), name
    from rigid_body_light_amd._lib import DeviceContext
    for name in ("ensemble_set_joint_rates", "ensemble_set_joint_angles", "ensemble_solve_jointed", "ensemble_step_jointed",
                 "ensemble_joint_state"):
        assert callable(getattr(DeviceContext, name)), name


def test_shape_errors_raise_before_the_library_is_called():
    e = _ensemble(R=3, nb=4, nj=5)
    for call in (e.solve_jointed, e.step_jointed):
        for F in (np.zeros(23), np.zeros((2, 24)), np.zeros((3, 4, 6))):
            with pytest.raises(ValueError):
                call(F)
        with pytest.raises(ValueError):
            call(np.zeros(24), slip=np.zeros(7))
    for rows in (np.zeros(14), np.zeros((5, 2)), np.zeros((2, 15)), np.zeros((3, 5, 4)), np.zeros((3, 3, 5))):
        with pytest.raises(ValueError):
            e.solve_jointed(np.zeros(24), joint_rhs=rows)
        with pytest.raises(ValueError):
            e.step_jointed(np.zeros(24), joint_velocity=rows)
    for v in (np.zeros(4), np.zeros((2, 5)), np.zeros((3, 5, 1)), 0.5):
        with pytest.raises(ValueError):
            e.set_joint_rates(v)
        with pytest.raises(ValueError):
            e.set_joint_angles(v)
    with pytest.raises(ValueError, match="local to a replica"):
        e.set_joint_kinds([[0, 4]], None, np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        e.set_joint_kinds([[0, 1]], [3], np.zeros(3), np.zeros(3))        # no such kind
    with pytest.raises(ValueError, match="switches the stored joints off"):
        e.set_joint_kinds(None, None)                                     # body=None goes with on=False only
    # what the wrappers hand on: joint rows as (3 n,), (n, 3) or with a leading R
    b = np.arange(15.0)
    for given in (b, b.reshape(5, 3)):
        assert np.array_equal(e._joint_rows_in("joint_rhs", given, 5), b)
    b3 = np.arange(45.0).reshape(3, 15)
    for given in (b3, b3.reshape(3, 5, 3)):
        assert np.array_equal(e._joint_rows_in("joint_rhs", given, 5), b3)


# ---- the compiler's resource figures of the jointed kernel ----------------------------------------------------------------------------
def test_the_jointed_solver_kernels_fit_a_1024_thread_workgroup_without_scratch(tmp_path):
    """compiled as tests/test_ensemble_mixed_cpu.py compiles rbl_small.hip: four instantiations <WALL, VLDS>, no scratch, four
    waves per SIMD (a workgroup of 1024 threads on one CU), at most 128 VGPRs"""
    from rigid_body_light_amd import build as B
    src = os.path.join(B.CSRC, "rbl_small_joints.hip")
    cmd = [B.HIPCC, "-Rpass-analysis=kernel-resource-usage", "-O3", "-std=c++17", "--offload-arch=" + B.ARCH, "-x", "hip",
           "--offload-device-only", "-c", src, "-o", str(tmp_path / "rbl_small_joints.co")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-3000:]
    found, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_gmres_small_jtILb([01])ELb([01])E", m.group(1))
            name = tuple(int(g) for g in k.groups()) if k else None
            if name is not None:
                found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name is not None:
            found[name][m.group(1).split()[0]] = int(m.group(2))
    assert sorted(found) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(found)
    for (wall, vlds), r in sorted(found.items()):
        print("k_gmres_small_jt<WALL=%d, VLDS=%d>: %d VGPRs, scratch %d bytes/lane, %d waves/SIMD" % (wall, vlds, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
        assert r["ScratchSize"] == 0 and r["Occupancy"] == 4 and r["VGPRs"] <= 128, (wall, vlds, r)
