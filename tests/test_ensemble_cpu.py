"""Ensembles of independent replicas (include/rbl.h section 5): what can be checked without a device -- the size, state and
shape rules are decided before the library touches the GPU."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    from rigid_body_light_amd._lib import lib
    return lib()


def _ctx(L, n_blb=12, params=True):
    from rigid_body_light_amd import load_structure
    h = L.rbl_create()
    if params:
        p, cfg = load_structure(n_blb)
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)
        assert L.rbl_set_parameters(h, p["sep"] / 2.0, 0.01, 1.0, 1.0, cfg.ctypes.data, cfg.shape[0]) == 0
    return h


RBL_ERR_SIZE, RBL_ERR_STATE = 4, 7


def _set(L, h, R, nb):
    X = np.zeros((max(R, 1), nb, 3)); Q = np.tile([1.0, 0, 0, 0], (max(R, 1), nb, 1))
    return L.rbl_ensemble_set_config(h, R, nb, X.ctypes.data, Q.ctypes.data)


def test_every_ensemble_entry_point_is_declared_and_exported():
    import os
    L = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rbl.h")).read()
    for name in ("rbl_ensemble_set_config", "rbl_ensemble_get_config", "rbl_ensemble_info", "rbl_ensemble_config_dev",
                 "rbl_ensemble_step_deterministic", "rbl_ensemble_step_brownian", "rbl_ensemble_interaction_forces"):
        assert name + "(" in hdr
        assert hasattr(L, name)


@pytest.mark.parametrize("R", [0, -1, 65536])
def test_replica_count_outside_1_to_65535_is_a_size_error(R):
    L = _lib()
    h = _ctx(L)
    assert _set(L, h, R, 2) == RBL_ERR_SIZE
    assert b"R must be" in L.rbl_last_error(h)
    L.rbl_destroy(h)


@pytest.mark.parametrize("n_blb,nb", [(12, 22), (1, 65), (642, 1)])
def test_systems_beyond_the_one_kernel_solver_are_a_size_error(n_blb, nb):
    from rigid_body_light_amd import load_structure
    L = _lib()
    if n_blb == 1:
        h = L.rbl_create()
        cfg = np.zeros((1, 3))
        assert L.rbl_set_parameters(h, 0.5, 0.01, 1.0, 1.0, cfg.ctypes.data, 1) == 0
    else:
        load_structure(n_blb)
        h = _ctx(L, n_blb)
    assert _set(L, h, 4, nb) == RBL_ERR_SIZE
    L.rbl_destroy(h)


def test_calls_before_parameters_or_ensemble_config_are_state_errors():
    L = _lib()
    h = _ctx(L, params=False)
    assert _set(L, h, 4, 1) == RBL_ERR_STATE                     # no parameters
    L.rbl_destroy(h)
    h = _ctx(L)
    r, nb = C.c_int(-1), C.c_int(-1)
    assert L.rbl_ensemble_info(h, C.byref(r), C.byref(nb)) == RBL_ERR_STATE and (r.value, nb.value) == (0, 0)
    F = np.zeros(6)
    it, res = np.zeros(1, dtype=np.int32), np.zeros(1)
    assert L.rbl_ensemble_step_deterministic(h, F.ctypes.data, None, 10, 1e-8, it.ctypes.data, res.ctypes.data) == RBL_ERR_STATE
    assert L.rbl_ensemble_step_brownian(h, F.ctypes.data, None, None, 0, 1, 1e-4, 10, 1e-8, it.ctypes.data,
                                        res.ctypes.data) == RBL_ERR_STATE
    X, Q = np.zeros(3), np.zeros(4)
    assert L.rbl_ensemble_get_config(h, X.ctypes.data, Q.ctypes.data) == RBL_ERR_STATE
    assert L.rbl_ensemble_interaction_forces(h, None, None) == RBL_ERR_STATE
    p, q = C.c_void_p(), C.c_void_p()
    assert L.rbl_ensemble_config_dev(h, C.byref(p), C.byref(q)) == RBL_ERR_STATE
    L.rbl_destroy(h)


@pytest.mark.parametrize("X,Q", [
    (np.zeros((4, 3)), np.zeros((4, 4))),                 # no replica axis
    (np.zeros((2, 3, 2)), np.zeros((2, 3, 4))),           # positions are not 3-vectors
    (np.zeros((2, 3, 3)), np.zeros((2, 2, 4))),           # bodies differ
    (np.zeros((2, 3, 3)), np.zeros((3, 3, 4))),           # replicas differ
])
def test_ensemble_shape_errors_raise_before_the_library_is_called(X, Q):
    from rigid_body_light_amd import Ensemble, load_structure
    p, cfg = load_structure(12)
    with pytest.raises(ValueError):
        Ensemble(cfg, X, Q, a=p["sep"] / 2.0, eta=1.0, dt=0.01)


def test_ensemble_is_exported_from_the_package():
    import rigid_body_light_amd
    assert "Ensemble" in rigid_body_light_amd.__all__
    assert rigid_body_light_amd.Ensemble.__module__ == "rigid_body_light_amd.ensemble"
