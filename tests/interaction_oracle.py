"""ctypes front-end of tests/interaction_oracle.c: the CPU all-pairs restatement of the force model of include/rbl.h section 4
(test infrastructure; the reference has no force model).  The shared library is compiled next to the source on first use
(and by __graft_entry__.build())."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "interaction_oracle.c")
_LIB_PATH = os.path.join(_HERE, "libinteraction_oracle.so")
_dp = C.POINTER(C.c_double)
_LIB = None


def build(force=False):
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(_SRC):
        subprocess.check_call([os.environ.get("CC", "cc"), "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-fopenmp",
                               "-Wall", "-Wextra", "-shared", "-o", _LIB_PATH, _SRC, "-lm"])
    return _LIB_PATH


def _lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        L.orc_interactions.restype = C.c_double
        L.orc_interactions.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_double] * 6 + [_dp, _dp]
        _LIB = L
    return _LIB


def interactions(r, X, N_blb, a, wall, w, eps_wall, b_wall, eps_blob, b_blob, r_cut):
    """-> (f_blob (N, 3), FT_body (6 N_bod,) physical force and torque about X, total energy)"""
    r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1))
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1))
    nb = X.size // 3
    assert r.size == 3 * nb * N_blb
    f = np.zeros(r.size)
    FT = np.zeros(6 * nb)
    E = _lib().orc_interactions(r.ctypes.data_as(_dp), X.ctypes.data_as(_dp), nb, int(N_blb), float(a), int(bool(wall)), float(w),
                                float(eps_wall), float(b_wall), float(eps_blob), float(b_blob), float(r_cut),
                                f.ctypes.data_as(_dp), FT.ctypes.data_as(_dp))
    return f.reshape(-1, 3), FT, E
