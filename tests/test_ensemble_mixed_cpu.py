"""Replica ensembles with held or driven bodies (include/rbl.h section 5, the rbl_ensemble_*_mixed entry points): what can be
checked without a device -- the declarations, every refusal that is decided before the library touches the GPU, the shape rules
of the Python layer, and the compiler's resource figures of the one-kernel solver: the masked instantiations of k_gmres_small
spill nothing, the four unmasked ones use what they used before the masked ones existed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rbl_ensemble_solve_mixed", "rbl_ensemble_step_mixed", "rbl_ensemble_step_brownian_mixed")
RBL_ERR_SIZE, RBL_ERR_STATE, RBL_ERR_ARG = 4, 7, 11


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


def _calls(L, h, mask, body_in, max_iter=10, rtol=1e-8):
    """the three entry points on one set of arguments -> their status codes (and the messages)"""
    m = None if mask is None else mask.ctypes.data
    b = None if body_in is None else body_in.ctypes.data
    U, F, lam = np.zeros(64), np.zeros(64), np.zeros(512)
    it, res = np.zeros(4, dtype=np.int32), np.zeros(4)
    out = []
    out.append((L.rbl_ensemble_solve_mixed(h, m, b, None, max_iter, rtol, lam.ctypes.data, U.ctypes.data, F.ctypes.data, it.ctypes.data,
                                           res.ctypes.data), L.rbl_last_error(h)))
    out.append((L.rbl_ensemble_step_mixed(h, m, b, None, max_iter, rtol, F.ctypes.data, it.ctypes.data, res.ctypes.data),
                L.rbl_last_error(h)))
    out.append((L.rbl_ensemble_step_brownian_mixed(h, m, b, None, None, 0, 1, 1e-4, max_iter, rtol, F.ctypes.data, it.ctypes.data,
                                                   res.ctypes.data), L.rbl_last_error(h)))
    return out


def test_the_three_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*rbl_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*prescribed\s*,\s*const\s+double\s*\*\s*body_in" % n,
                         code), n
        assert hasattr(L, n), n
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    for n in NAMES:
        assert n in sec5                                  # appended to section 5


def test_every_refusal_is_decided_before_a_device_is_touched():
    L = _lib()
    mask, bi = np.zeros(8, dtype=np.uint8), np.zeros(48)
    h = _ctx(L)                                           # parameters, no ensemble: this context never initialises a device
    for rc, msg in _calls(L, h, None, bi):
        assert rc == RBL_ERR_ARG and b"NULL" in msg
    for rc, msg in _calls(L, h, mask, None):
        assert rc == RBL_ERR_ARG and b"NULL" in msg
    for bad in (0, -3):
        for rc, msg in _calls(L, h, mask, bi, max_iter=bad):
            assert rc == RBL_ERR_ARG and b"max_iter" in msg
    for rc, msg in _calls(L, h, mask, bi, rtol=-1.0):
        assert rc == RBL_ERR_ARG
    for rc, msg in _calls(L, h, mask, bi, max_iter=256):
        assert rc == RBL_ERR_SIZE and b"max_iter <= 255" in msg and b"beyond the one-kernel solver" in msg   # the existing message
    for rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_STATE and b"no ensemble configuration" in msg
    # the solve's outputs
    it, res = np.zeros(4, dtype=np.int32), np.zeros(4)
    assert L.rbl_ensemble_solve_mixed(None, mask.ctypes.data, bi.ctypes.data, None, 10, 1e-8, None, None, None, it.ctypes.data,
                                      res.ctypes.data) == RBL_ERR_ARG
    L.rbl_destroy(h)
    h = _ctx(L, params=False)                             # no parameters at all
    for rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_STATE
    L.rbl_destroy(h)
    # a context with a communicator: RBL_ERR_ARG, as for the other ensemble calls
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
    cb = CB(lambda user, buf, n: 0)
    h = _ctx(L)
    assert L.rbl_set_comm_ops(h, 0, 2, C.cast(cb, C.c_void_p), None, None) == 0
    for rc, msg in _calls(L, h, mask, bi):
        assert rc == RBL_ERR_ARG and b"communicator" in msg
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


@pytest.mark.parametrize("prescribed", [
    np.zeros(3, dtype=bool),                              # neither (N_bod,) nor (R, N_bod)
    np.zeros((2, 4), dtype=bool),                         # replicas differ
    np.zeros((3, 4, 1), dtype=bool),
    [0.0, 1.0],                                           # floats are neither a mask nor indices
    [4],                                                  # no such body
    [-1],
    [1, 1],                                               # twice
])
def test_prescribed_shape_and_value_errors_raise_before_the_library_is_called(prescribed):
    e = _ensemble()
    for call in (e.solve_mixed, e.step_mixed, e.step_brownian_mixed):
        with pytest.raises(ValueError):
            call(prescribed, np.zeros(24))


@pytest.mark.parametrize("body_in", [np.zeros(23), np.zeros((4, 5)), np.zeros((2, 24)), np.zeros((3, 4, 5)), np.zeros((3, 6, 4))])
def test_body_in_shape_errors_raise_before_the_library_is_called(body_in):
    e = _ensemble()
    for call in (e.solve_mixed, e.step_mixed, e.step_brownian_mixed):
        with pytest.raises(ValueError):
            call([1], body_in)


def test_slip_and_noise_shape_errors_raise_before_the_library_is_called():
    e = _ensemble()
    for call in (e.solve_mixed, e.step_mixed, e.step_brownian_mixed):
        with pytest.raises(ValueError):
            call([1], np.zeros(24), slip=np.zeros(7))
    with pytest.raises(ValueError):
        e.step_brownian_mixed([1], np.zeros(24), W=np.zeros((3, 5)))


def test_prescribed_and_body_in_are_read_as_the_single_system_reads_them():
    e = _ensemble(R=3, nb=4)
    m = e._prescribed_mask([2, 0])
    assert m.dtype == np.uint8 and m.shape == (3, 4) and np.array_equal(m, np.tile([1, 0, 1, 0], (3, 1)))
    m = e._prescribed_mask(np.array([False, True, False, False]))
    assert np.array_equal(m, np.tile([0, 1, 0, 0], (3, 1)))
    per = np.zeros((3, 4), dtype=bool); per[1, 3] = True
    assert np.array_equal(e._prescribed_mask(per), per.astype(np.uint8))
    assert not e._prescribed_mask([]).any()
    b = np.arange(24.0)
    for given in (b, b.reshape(4, 6)):
        assert np.array_equal(e._body_in(given), np.tile(b, (3, 1)))
    b3 = np.arange(72.0).reshape(3, 24)
    for given in (b3, b3.reshape(3, 4, 6)):
        assert np.array_equal(e._body_in(given), b3)


# VGPRs and scratch bytes per lane of the four unmasked instantiations <WALL, VLDS> at the commit before the masked ones were added
# (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; HISTORY.md has both sets of lines)
PARENT = {(1, 1): (128, 0), (1, 0): (128, 0), (0, 1): (111, 0), (0, 0): (119, 0)}


def test_masked_solver_kernels_use_no_scratch_and_the_unmasked_ones_what_they_used(tmp_path):
    from rigid_body_light_amd import build as B
    src = os.path.join(B.CSRC, "rbl_small.hip")
    cmd = [B.HIPCC, "-Rpass-analysis=kernel-resource-usage", "-O3", "-std=c++17", "--offload-arch=" + B.ARCH, "-x", "hip",
           "--offload-device-only", "-c", src, "-o", str(tmp_path / "rbl_small.co")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-3000:]
    found = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*k_gmres_smallILb([01])ELb([01])ELb([01])E", line)
        if m:
            name = tuple(int(g) for g in m.groups())
            found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name is not None:
            found[name][m.group(1).split()[0]] = int(m.group(2))
    assert len(found) == 8, sorted(found)
    for (wall, vlds, mixed), r in sorted(found.items()):
        print("k_gmres_small<WALL=%d, VLDS=%d, MIXED=%d>: %d VGPRs, scratch %d bytes/lane, %d waves/SIMD"
              % (wall, vlds, mixed, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
    for (wall, vlds, mixed), r in found.items():
        assert r["ScratchSize"] == 0 and r["Occupancy"] == 4 and r["VGPRs"] <= 128, (wall, vlds, mixed, r)
        if not mixed:
            assert (r["VGPRs"], r["ScratchSize"]) == PARENT[(wall, vlds)], (wall, vlds, r)
