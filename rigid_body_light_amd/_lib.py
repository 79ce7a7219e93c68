"""ctypes binding of librbl.so (include/rbl.h): `DeviceContext` is the ONE Python binding of everything the library has beyond
the reference's surface -- the force model, tables, traps, dipoles, bonds, joints, the imposed flow and moments, the velocity
field, prescribed kinematics, ensembles -- in host-array methods, and of the device-pointer API (section 3) for callers that keep
data resident on the GPU (bench.py, dist.py).  It owns its rbl_ctx, or borrows the one of a `c_rigid.CManyBodies`
(`DeviceContext.borrow`: how `RigidBody` reaches these methods).  torch is used only as the owner of device memory and
streams; the pointers handed over are raw HIP pointers."""
import ctypes as C
import os

try:  # one HIP runtime per process: torch's bundled copy must be loaded first (see __init__.py)
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
IN_PACKAGE_LIB = os.path.join(_HERE, "librbl.so")   # the file c_rigid is linked against (rpath $ORIGIN)
_LIBS = {}                                          # path -> loaded library


def lib(path=None):
    """the library at `path` with its argument types declared, loaded once per path.  None: RBL_LIBRARY (A/B kernel builds),
    else the in-package file"""
    if path is None:
        path = os.environ.get("RBL_LIBRARY") or IN_PACKAGE_LIB
    L = _LIBS.get(path)
    if L is None:
        if not os.path.exists(path):
            raise ImportError("librbl.so not built; run `python rigid_body_light_amd/build.py`")
        L = C.CDLL(path)
        vp, i64, dbl = C.c_void_p, C.c_int64, C.c_double
        L.rbl_create.restype = vp
        L.rbl_destroy.argtypes = [vp]
        L.rbl_last_error.restype = C.c_char_p
        L.rbl_last_error.argtypes = [vp]
        L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, C.c_int]
        L.rbl_set_wall_pc.argtypes = [vp, C.c_int]
        L.rbl_set_config.argtypes = [vp, vp, vp, C.c_int]
        L.rbl_set_stream.argtypes = [vp, vp]
        L.rbl_apply_M_dev.argtypes = [vp, vp, vp, i64, i64, i64, vp]
        L.rbl_sync_bodies_dev.argtypes = [vp]
        L.rbl_prepare_dev.argtypes = [vp]
        L.rbl_positions_dev.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(i64)]
        L.rbl_K_x_U_dev.argtypes = [vp, vp, vp]
        L.rbl_KT_x_Lam_dev.argtypes = [vp, vp, vp]
        L.rbl_apply_PC_dev.argtypes = [vp, vp, vp]
        L.rbl_apply_saddle_dev.argtypes = [vp, vp, vp]
        L.rbl_evolve_X_Q.argtypes = [vp, vp]
        L.rbl_get_config.argtypes = [vp, vp, vp]
        L.rbl_set_blk_pc.argtypes = [vp, C.c_int]
        L.rbl_apply_M_multi_dev.argtypes = [vp, vp, vp, i64, C.c_int, vp]
        L.rbl_apply_M_sym_dev.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, vp]
        L.rbl_apply_M_sym_multi_dev.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, C.c_int, vp]
        L.rbl_apply_M_sym_info.argtypes = [vp, i64, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)]
        L.rbl_apply_M_sym_kernel.argtypes = [vp, i64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.rbl_blob_positions_dev.argtypes = [vp, C.c_int, C.c_int, vp]
        L.rbl_rotne_prager_tensor_dev.argtypes = [vp, vp, i64, C.c_int, vp]
        L.rbl_cholesky_lower_dev.argtypes = [vp, vp, i64, C.c_int]
        L.rbl_trmv_lower_dev.argtypes = [vp, vp, i64, vp, vp]
        L.rbl_M_half_W_dev.argtypes = [vp, vp, i64, vp, C.c_int, vp]
        L.rbl_sync_check.argtypes = [vp]
        L.rbl_set_lanczos.argtypes = [vp, C.c_int, dbl]
        L.rbl_get_lanczos_report.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_update_X_Q.argtypes = [vp, vp, vp, vp]
        L.rbl_step_deterministic.argtypes = [vp, vp, vp, C.c_int, dbl, C.c_int, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_step_brownian.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, dbl, C.c_int, dbl, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_block_solve_dev.argtypes = [vp, vp, vp, C.c_int]
        L.rbl_block_solve_range_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int]
        L.rbl_set_no_damp.argtypes = [vp, C.c_int]
        L.rbl_set_block_refresh.argtypes = [vp, C.c_int]
        L.rbl_gmres_saddle_dev.argtypes = [vp, vp, C.c_int, dbl, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_gmres_saddle_multi_dev.argtypes = [vp, vp, C.c_int, C.c_int, dbl, vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_Kinv_x_V.argtypes = [vp, vp, vp]
        L.rbl_set_comm.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        L.rbl_set_comm_ops.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
        L.rbl_comm_unique_id.argtypes = [vp]
        L.rbl_comm_init_rccl.argtypes = [vp, vp, C.c_int, C.c_int]
        L.rbl_comm_finalize.argtypes = [vp]
        L.rbl_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_comm_allreduce_dev.argtypes = [vp, vp, i64]
        L.rbl_comm_allgatherv_dev.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i64)]
        L.rbl_set_option.argtypes = [vp, C.c_int, i64]
        L.rbl_get_option.argtypes = [vp, C.c_int, C.POINTER(i64)]
        L.rbl_option_info.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.rbl_option_key.argtypes = [C.c_char_p]
        L.rbl_apply_saddle.argtypes = [vp, vp, vp]
        L.rbl_multi_body_pos_dev.argtypes = [vp, vp]
        L.rbl_RHS_and_Midpoint_dev.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, dbl, vp, vp, vp]
        L.rbl_set_timing.argtypes = [vp, C.c_int]
        L.rbl_reset_timings.argtypes = [vp]
        L.rbl_get_timings.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
        L.rbl_set_interactions.argtypes = [vp, dbl, dbl, dbl, dbl, dbl, dbl, C.c_int]
        L.rbl_get_interactions.argtypes = [vp, C.POINTER(dbl), C.POINTER(C.c_int)]
        L.rbl_set_pair_table.argtypes = L.rbl_set_height_table.argtypes = [vp, vp, vp, C.c_int, dbl, dbl, C.c_int]
        L.rbl_get_pair_table.argtypes = L.rbl_get_height_table.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(dbl), C.POINTER(dbl),
                                                                           C.POINTER(C.c_int), vp]
        L.rbl_set_traps.argtypes = [vp, vp, vp, C.c_int, C.c_int]
        L.rbl_get_traps.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp]
        L.rbl_interactions_active.argtypes = [vp, C.POINTER(C.c_int)]
        L.rbl_set_blob_types.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
        L.rbl_get_blob_types.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
        L.rbl_set_type_table.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, dbl, dbl, C.c_int]
        L.rbl_get_type_table.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int), vp]
        L.rbl_clear_type_tables.argtypes = [vp]
        L.rbl_set_dipoles.argtypes = [vp, vp, C.c_int, dbl, dbl, dbl, C.c_int]
        L.rbl_get_dipoles.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int), vp]
        L.rbl_set_magnetic_field.argtypes = [vp, vp, vp, vp, dbl, C.c_int]
        L.rbl_get_magnetic_field.argtypes = [vp, vp, C.POINTER(dbl), C.POINTER(C.c_int)]
        L.rbl_set_field_time.argtypes = [vp, vp, C.c_int]
        L.rbl_get_field_time.argtypes = [vp, C.POINTER(C.c_int), vp]
        L.rbl_set_bonds.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int]
        L.rbl_get_bonds.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, vp, vp]
        L.rbl_set_bond_table.argtypes = L.rbl_set_pair_table.argtypes
        L.rbl_get_bond_table.argtypes = L.rbl_get_pair_table.argtypes
        L.rbl_bond_state.argtypes = L.rbl_ensemble_bond_state.argtypes = [vp, vp, vp, vp]
        L.rbl_set_joints.argtypes = [vp, C.c_int, vp, vp, C.c_int]
        L.rbl_get_joints.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp]
        L.rbl_solve_jointed.argtypes = L.rbl_solve_jointed_dev.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp, C.POINTER(C.c_int),
                                                                         C.POINTER(dbl)]
        L.rbl_step_jointed.argtypes = [vp, vp, vp, vp, dbl, C.c_int, dbl, vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_joint_state.argtypes = [vp, vp, vp]
        L.rbl_set_joint_kinds.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int]
        L.rbl_get_joint_kinds.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, vp, vp, vp, vp, vp]
        L.rbl_set_joint_rates.argtypes = [vp, vp]
        L.rbl_joint_state_kinds.argtypes = [vp, vp, vp, vp]
        L.rbl_set_periodic.argtypes = [vp, dbl, dbl, C.c_int, C.c_int, C.c_int]
        L.rbl_get_periodic.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_ensemble_set_periodic.argtypes = L.rbl_set_periodic.argtypes
        L.rbl_ensemble_get_periodic.argtypes = L.rbl_get_periodic.argtypes
        L.rbl_ensemble_set_cells.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int]
        L.rbl_ensemble_get_cells.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_interaction_forces_dev.argtypes = [vp, vp, vp, C.POINTER(dbl)]
        L.rbl_interaction_forces.argtypes = [vp, vp, vp, C.POINTER(dbl)]
        L.rbl_interaction_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.rbl_get_sizes.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_ensemble_set_config.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        L.rbl_ensemble_get_config.argtypes = [vp, vp, vp]
        L.rbl_ensemble_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_ensemble_config_dev.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.rbl_ensemble_step_deterministic.argtypes = [vp, vp, vp, C.c_int, dbl, vp, vp]
        L.rbl_ensemble_step_brownian.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_int, dbl, C.c_int, dbl, vp, vp]
        L.rbl_ensemble_interaction_forces.argtypes = [vp, vp, vp]
        L.rbl_ensemble_solve_mixed.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp, vp, vp]
        L.rbl_ensemble_step_mixed.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp]
        L.rbl_ensemble_solve_mixed_dof.argtypes = L.rbl_ensemble_solve_mixed.argtypes
        L.rbl_ensemble_step_mixed_dof.argtypes = L.rbl_ensemble_step_mixed.argtypes
        L.rbl_ensemble_step_brownian_mixed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, dbl, C.c_int, dbl, vp, vp, vp]
        L.rbl_ensemble_run.argtypes = [vp, C.POINTER(RunOpts), C.POINTER(RunOut)]
        L.rbl_ensemble_mc.argtypes = [vp, C.POINTER(McOpts), C.POINTER(McOut)]
        L.rbl_ensemble_run_jointed.argtypes = [vp, C.POINTER(RunOpts), C.POINTER(RunJointOpts), C.POINTER(RunOut), C.POINTER(RunJointOut)]
        L.rbl_run_schedule_phase.argtypes = [vp, C.c_int, i64]
        L.rbl_ensemble_set_joint_rates.argtypes = L.rbl_ensemble_set_joint_angles.argtypes = [vp, vp, C.c_int]
        L.rbl_ensemble_solve_jointed.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp, vp, vp]
        L.rbl_ensemble_step_jointed.argtypes = [vp, vp, vp, vp, dbl, C.c_int, dbl, vp, vp, vp]
        L.rbl_ensemble_joint_state.argtypes = [vp, vp, vp, vp]
        L.rbl_ensemble_joints_fit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i64)]
        L.rbl_ensemble_run_observed.argtypes = [vp, C.POINTER(RunOpts), C.POINTER(RunJointOpts), C.POINTER(RunObsOpts), C.POINTER(RunOut),
                                                C.POINTER(RunJointOut), C.POINTER(RunObsOut)]
        L.rbl_ensemble_run_driven.argtypes = [vp, C.POINTER(RunOpts), C.POINTER(RunDriveOpts), C.POINTER(RunObsOpts), C.POINTER(RunOut),
                                              C.POINTER(RunDriveOut), C.POINTER(RunObsOut)]
        L.rbl_ensemble_drive_eval.argtypes = [vp, C.POINTER(RunDriveOpts), vp, vp, vp, vp, vp]
        L.rbl_ensemble_velocity_field.argtypes = L.rbl_ensemble_velocity_field_dev.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, vp]
        L.rbl_ensemble_probe_info.argtypes = [vp, i64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)]
        L.rbl_velocity_field.argtypes = [vp, vp, i64, vp, vp, i64, vp]
        L.rbl_velocity_field_dev.argtypes = [vp, vp, i64, vp, vp, i64, vp]
        L.rbl_velocity_field_info.argtypes = [vp, i64, i64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)]
        L.rbl_solve_mixed.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_solve_mixed_dev.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_step_mixed.argtypes = [vp, vp, vp, vp, C.c_int, dbl, vp, C.POINTER(C.c_int), C.POINTER(dbl)]
        L.rbl_solve_mixed_dof.argtypes = L.rbl_solve_mixed_dof_dev.argtypes = L.rbl_solve_mixed.argtypes
        L.rbl_step_mixed_dof.argtypes = L.rbl_step_mixed.argtypes
        L.rbl_solve_mixed_multi.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, dbl, vp, vp, vp, vp, vp]
        L.rbl_solve_mixed_multi_dev.argtypes = L.rbl_solve_mixed_dof_multi.argtypes = L.rbl_solve_mixed_multi.argtypes
        L.rbl_solve_mixed_dof_multi_dev.argtypes = L.rbl_solve_mixed_multi.argtypes
        L.rbl_RHS_and_Midpoint_mixed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, dbl, vp, vp, vp]
        L.rbl_RHS_and_Midpoint_mixed_dev.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, dbl, vp, vp, vp]
        L.rbl_step_brownian_mixed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, dbl, C.c_int, dbl, vp, C.POINTER(C.c_int),
                                              C.POINTER(dbl)]
        L.rbl_RHS_and_Midpoint_mixed_dof.argtypes = L.rbl_RHS_and_Midpoint_mixed_dof_dev.argtypes = L.rbl_RHS_and_Midpoint_mixed.argtypes
        L.rbl_step_brownian_mixed_dof.argtypes = L.rbl_step_brownian_mixed.argtypes
        L.rbl_ensemble_step_brownian_mixed_dof.argtypes = L.rbl_ensemble_step_brownian_mixed.argtypes
        L.rbl_set_background_flow.argtypes = [vp, vp, vp, C.c_int]
        L.rbl_set_body_slip.argtypes = [vp, vp, vp, C.c_int, C.c_int]
        L.rbl_get_flow_model.argtypes = [vp, C.POINTER(dbl), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rbl_flow_slip_dev.argtypes = L.rbl_flow_slip.argtypes = L.rbl_ensemble_flow_slip.argtypes = [vp, vp]
        L.rbl_first_moments_dev.argtypes = L.rbl_first_moments.argtypes = [vp, vp, vp]
        L.rbl_step_moments.argtypes = L.rbl_ensemble_step_moments.argtypes = [vp, vp]
        _LIBS[path] = L
    return L


class RblError(RuntimeError):
    pass


def _ptr(a):
    """address of a numpy array, None for None (an argument left out)"""
    return None if a is None else a.ctypes.data


MHALF_METHODS = {"cholesky": 0, "lanczos": 1, "lanczos_pc": 2}   # RBL_MHALF_* of include/rbl.h


def mhalf_code(method):
    """the root method's code from its name; an integer passes through"""
    if not isinstance(method, str):
        return int(method)
    if method not in MHALF_METHODS:
        raise RuntimeError("M_half_W: method must be 'cholesky', 'lanczos' or 'lanczos_pc'")
    return MHALF_METHODS[method]


def tabulate(U, dU, lo, hi, n):
    """values of the callables U(x) and dU(x) = dU/dx on the uniform grid lo + k (hi - lo) / (n - 1), k = 0 .. n - 1: the two
    arrays set_pair_table / set_height_table take"""
    import numpy as np
    x = np.linspace(float(lo), float(hi), int(n))
    return (np.ascontiguousarray(np.broadcast_to(np.asarray(U(x), dtype=np.float64), x.shape)),
            np.ascontiguousarray(np.broadcast_to(np.asarray(dU(x), dtype=np.float64), x.shape)))


def dipole_args(who, m_body, c_dd, r_core):
    """the checks set_dipoles can make before the library is called -> contiguous float64 m_body (n, 3), r_core as a float.
    r_core=None is accepted only without the pair term (c_dd == 0), where no core is needed"""
    import numpy as np
    m = np.ascontiguousarray(m_body, dtype=np.float64)
    if m.shape == (3,):
        m = m.reshape(1, 3)
    if m.ndim != 2 or m.shape[1] != 3 or not m.shape[0]:
        raise ValueError("%s: m_body must have shape (3,) or (n, 3); got %s" % (who, m.shape))
    if r_core is None:
        if float(c_dd) != 0.0:
            raise ValueError("%s: r_core is needed with c_dd != 0 (below it the pair energy is a quadratic form)" % who)
        r_core = 0.0
    return m, float(r_core)


def bond_args(who, body, anchor_a, anchor_b, k, l0, kind, sets=(1,)):
    """the checks set_bonds can make before the library is called -> contiguous body int32 (n, 2), anchor float64 (n, 6), kind
    int32 (n,) or None, param float64 (n_sets, n, 2).  body: (n, 2) integers (or (2,) for one bond), the second -1 for a lab
    point; anchor_a, anchor_b: (3,) -- every bond alike -- or (n, 3); k, l0: a number, (n,) or (n_sets, n) with n_sets in `sets`
    (None: any count); kind: None (all harmonic) or (n,) integers"""
    import numpy as np
    b = np.asarray(body)
    if b.shape == (2,):
        b = b.reshape(1, 2)
    if b.ndim != 2 or b.shape[1] != 2 or not b.shape[0] or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("%s: body must be an integer array of shape (n, 2); got %s of dtype %s" % (who, b.shape, b.dtype))
    n = b.shape[0]
    anchors = []
    for name, v in (("anchor_a", anchor_a), ("anchor_b", anchor_b)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape == (3,):
            v = np.broadcast_to(v, (n, 3))
        if v.shape != (n, 3):
            raise ValueError("%s: %s must have shape (3,) or (%d, 3); got %s" % (who, name, n, v.shape))
        anchors.append(v)
    par = []
    for name, v in (("k", k), ("l0", l0)):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            v = np.broadcast_to(v, (n,))
        if v.ndim == 1 and v.shape == (n,):
            v = v.reshape(1, n)
        if v.ndim != 2 or v.shape[1] != n or not v.shape[0] or (sets is not None and v.shape[0] not in sets):
            want = "(n_sets, %d)" % n if sets is None else " or ".join("(%d, %d)" % (q, n) for q in sets if q != 1)
            raise ValueError("%s: %s must be a number or have shape (%d,)%s; got %s" % (who, name, n, " or " + want if want else "", v.shape))
        par.append(v)
    n_sets = max(par[0].shape[0], par[1].shape[0])
    if any(v.shape[0] not in (1, n_sets) for v in par):
        raise ValueError("%s: k and l0 hold different numbers of sets; got %s and %s" % (who, par[0].shape, par[1].shape))
    param = np.ascontiguousarray(np.stack([np.broadcast_to(v, (n_sets, n)) for v in par], axis=2))
    if kind is not None:
        kind = np.asarray(kind)
        if kind.shape != (n,) or not np.issubdtype(kind.dtype, np.integer):
            raise ValueError("%s: kind must be None or an integer array of shape (%d,); got %s of dtype %s" % (who, n, kind.shape, kind.dtype))
        kind = np.ascontiguousarray(kind, dtype=np.int32)
    return (np.ascontiguousarray(b, dtype=np.int32), np.ascontiguousarray(np.concatenate(anchors, axis=1)), kind, param)


def joint_args(who, body, anchor_a, anchor_b):
    """the checks set_joints can make before the library is called -> contiguous body int32 (n, 2), anchor float64 (n, 6).
    body: (n, 2) integers (or (2,) for one joint), the second -1 for a lab point; anchor_a, anchor_b: (3,) -- every joint alike --
    or (n, 3)"""
    b, anchor, _, _ = bond_args(who, body, anchor_a, anchor_b, 0.0, 0.0, None)
    return b, anchor


JOINT_BALL, JOINT_LOCK, JOINT_AXIS = 0, 1, 2          # RBL_JOINT_* of include/rbl.h section 9


def quat_mul(p, q):
    """Hamilton product of two quaternions (w, x, y, z): R(p q) = R(p) R(q)"""
    import numpy as np
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return np.concatenate([[p[0] * q[0] - p[1:] @ q[1:]], p[0] * q[1:] + q[0] * p[1:] + np.cross(p[1:], q[1:])])


def quat_matrix(q):
    """rotation matrix of a quaternion (w, x, y, z), normalised here: lab = R body"""
    import numpy as np
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def relative_quat(Q, a, b):
    """Q_A^-1 Q_B of the bodies a and b of the configuration's quaternions Q (N_bod, 4); b = -1, the lab: Q_B is the identity"""
    import numpy as np
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    qa = Q[a] / np.linalg.norm(Q[a])
    qb = np.array([1.0, 0.0, 0.0, 0.0]) if b < 0 else Q[b] / np.linalg.norm(Q[b])
    return quat_mul(qa * [1.0, -1.0, -1.0, -1.0], qb)


def joint_kind_args(who, body, kind, anchor_a=None, anchor_b=None, axis=None, q_rel=None):
    """the checks set_joint_kinds can make before the library is called -> contiguous body int32 (n, 2), kind int32 (n,), anchor
    float64 (n, 6), axis float64 (n, 3), q_rel float64 (n, 4).  kind: (n,) integers, JOINT_BALL, JOINT_LOCK or JOINT_AXIS;
    anchors as set_joints takes them, needed when there is a ball joint; axis (3,) or (n, 3), in body A's frame, needed when
    there is a lock or axis joint, finite and of norm >= 1e-12 on their rows; q_rel (4,) or (n, 4), of non-zero norm on those rows,
    or None: the identity here, which the caller replaces by that of the configuration (default_q_rel) once every check has passed"""
    import numpy as np
    b = np.asarray(body)
    if b.shape == (2,):
        b = b.reshape(1, 2)
    if b.ndim != 2 or b.shape[1] != 2 or not b.shape[0] or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("%s: body must be an integer array of shape (n, 2); got %s of dtype %s" % (who, b.shape, b.dtype))
    n = b.shape[0]
    k = np.asarray(kind)
    if k.ndim == 0 and np.issubdtype(k.dtype, np.integer):
        k = np.broadcast_to(k, (n,))
    if k.shape != (n,) or not np.issubdtype(k.dtype, np.integer):
        raise ValueError("%s: kind must be an integer array of shape (%d,); got %s of dtype %s" % (who, n, k.shape, k.dtype))
    for j in range(n):
        if k[j] not in (JOINT_BALL, JOINT_LOCK, JOINT_AXIS):
            raise ValueError("%s: joint %d: unknown kind %d (JOINT_BALL 0, JOINT_LOCK 1, JOINT_AXIS 2)" % (who, j, k[j]))
    ball, ang = k == JOINT_BALL, k != JOINT_BALL
    if ball.any() and (anchor_a is None or anchor_b is None):
        raise ValueError("%s: joint %d is a ball joint: anchor_a and anchor_b are needed" % (who, int(np.argmax(ball))))
    if ang.any() and axis is None:
        raise ValueError("%s: joint %d is a lock or axis joint: axis is needed" % (who, int(np.argmax(ang))))
    out = []
    for name, v, w in (("anchor_a", anchor_a, 3), ("anchor_b", anchor_b, 3), ("axis", axis, 3), ("q_rel", q_rel, 4)):
        if v is None:
            v = np.zeros((n, w))
            if name == "q_rel":
                v[:, 0] = 1.0
        v = np.asarray(v, dtype=np.float64)
        if v.shape == (w,):
            v = np.broadcast_to(v, (n, w))
        if v.shape != (n, w):
            raise ValueError("%s: %s must have shape (%d,) or (%d, %d); got %s" % (who, name, w, n, w, v.shape))
        out.append(np.array(v))
    anchor = np.concatenate(out[:2], axis=1)
    anchor[ang] = 0.0                                     # not read for an angular joint
    for j in np.flatnonzero(ball):
        if not np.isfinite(anchor[j]).all():
            raise ValueError("%s: joint %d: every value of the anchors must be finite" % (who, j))
    for j in np.flatnonzero(ang):
        na = np.linalg.norm(out[2][j])
        if not np.isfinite(na) or na < 1e-12:
            raise ValueError("%s: joint %d: axis must be finite and of norm >= 1e-12" % (who, j))
        nq = np.linalg.norm(out[3][j])
        if not np.isfinite(nq) or not nq > 0.0:
            raise ValueError("%s: joint %d: q_rel must be finite and of non-zero norm" % (who, j))
    return (np.ascontiguousarray(b, dtype=np.int32), np.ascontiguousarray(k, dtype=np.int32), np.ascontiguousarray(anchor),
            np.ascontiguousarray(out[2]), np.ascontiguousarray(out[3]))


def default_q_rel(who, body, kind, q_rel, Q):
    """q_rel = Q_A^-1 Q_B of the configuration's quaternions Q on the rows of the lock and axis joints, in place"""
    import numpy as np
    nb = np.asarray(Q).reshape(-1, 4).shape[0]
    for j in np.flatnonzero(kind != JOINT_BALL):
        if not 0 <= body[j, 0] < nb or not -1 <= body[j, 1] < nb:
            raise ValueError("%s: joint %d: body index out of range of the %d bodies of the configuration" % (who, j, nb))
        q_rel[j] = relative_quat(Q, body[j, 0], body[j, 1])


def _joint_rows(X, Q, a, b, point, axis, kinds):
    """the rows of a composed joint between the bodies a and b (b = -1: the lab) of the configuration X, Q: a ball joint at the
    lab-frame point `point` first, then one angular joint per further entry of kinds about the lab-frame direction `axis`"""
    import numpy as np
    X, Q = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    a, b = int(a), int(b)
    if not 0 <= a < X.shape[0] or not -1 <= b < X.shape[0] or a == b:
        raise ValueError("joint builder: bodies (%d, %d): the first must be a body of the configuration, the second another or -1" % (a, b))
    point, axis = np.asarray(point, dtype=np.float64), np.asarray(axis, dtype=np.float64)
    if point.shape != (3,) or axis.shape != (3,) or not np.isfinite(point).all() or not np.isfinite(axis).all() or np.linalg.norm(axis) < 1e-12:
        raise ValueError("joint builder: point and axis must be finite vectors of 3, the axis of norm >= 1e-12")
    n = len(kinds)
    RA = quat_matrix(Q[a])
    rows = dict(body=np.tile([a, b], (n, 1)), kind=np.array(kinds, dtype=np.int32), anchor_a=np.zeros((n, 3)), anchor_b=np.zeros((n, 3)),
                axis=np.tile(RA.T @ (axis / np.linalg.norm(axis)), (n, 1)), q_rel=np.tile(relative_quat(Q, a, b), (n, 1)))
    rows["anchor_a"][0] = RA.T @ (point - X[a])
    rows["anchor_b"][0] = point if b < 0 else quat_matrix(Q[b]).T @ (point - X[b])
    return rows


def hinge(X, Q, a, b, point, axis):
    """a five-row hinge between the bodies a and b (b = -1: the lab) at the configuration X, Q: a ball joint at the lab-frame
    point and an axis joint about the lab-frame direction axis -> rows for joint_rows / set_joint_kinds"""
    return _joint_rows(X, Q, a, b, point, axis, [JOINT_BALL, JOINT_AXIS])


def weld(X, Q, a, b, point):
    """the two bodies move as one: a ball joint at the lab-frame point and a lock joint (its rate stays 0)"""
    return _joint_rows(X, Q, a, b, point, [0.0, 0.0, 1.0], [JOINT_BALL, JOINT_LOCK])


def motor(X, Q, a, b, point, axis):
    """a driven hinge: a ball joint at the lab-frame point and a lock joint whose rate (set_joint_rates) turns body b relative
    to body a about the lab-frame direction axis, fixed in body a"""
    return _joint_rows(X, Q, a, b, point, axis, [JOINT_BALL, JOINT_LOCK])


def joint_rows(*rows):
    """the rows of several builders (hinge, weld, motor, or dicts of the same keys) concatenated -> the keyword arguments of
    set_joint_kinds"""
    import numpy as np
    keys = ("body", "kind", "anchor_a", "anchor_b", "axis", "q_rel")
    return {k: np.concatenate([np.atleast_2d(r[k]) if k != "kind" else np.atleast_1d(r[k]) for r in rows]) for k in keys}


def blob_anchor(cfg, k):
    """body-frame position of blob k of the structure cfg (N_blb, 3) with the structure's mean removed, as the library removes
    it: the anchor of a bond that ends on that blob"""
    import numpy as np
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 3)
    mean = np.zeros(3)
    for row in cfg:                                    # the library's own order of summation
        mean = mean + row
    return cfg[int(k)] - mean / float(cfg.shape[0])


def field_args(who, B0, B1, B2):
    """-> three contiguous float64 vectors of 3 (None: zeros)"""
    import numpy as np
    out = []
    for name, B in (("B0", B0), ("B1", B1), ("B2", B2)):
        B = np.zeros(3) if B is None else np.ascontiguousarray(B, dtype=np.float64)
        if B.shape != (3,):
            raise ValueError("%s: %s must have shape (3,); got %s" % (who, name, B.shape))
        out.append(B)
    return out


def table_arrays(who, U, dU):
    """the checks a table's arrays can fail before the library is called -> contiguous float64 U, dU"""
    import numpy as np
    U, dU = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(dU, dtype=np.float64)
    if U.ndim != 1 or U.shape != dU.shape:
        raise ValueError("%s: U and dU must be one-dimensional and of one length; got %s and %s" % (who, U.shape, dU.shape))
    return U, dU


MAX_BLOB_TYPES = 8   # include/rbl.h section 4: the descriptors of the 36 type pairs sit in LDS


def blob_type_args(who, types, n_types):
    """the checks set_blob_types can make before the library is called -> contiguous int32 types (flattened), n_types.
    types: integers of shape (N_blb,) -- every body alike -- or (N_bod, N_blb); n_types None: the largest type + 1"""
    import numpy as np
    t = np.asarray(types)
    if t.ndim not in (1, 2) or not t.size:
        raise ValueError("%s: types must have shape (N_blb,) or (N_bod, N_blb); got %s" % (who, t.shape))
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError("%s: types must be integers; got dtype %s" % (who, t.dtype))
    if n_types is None:
        n_types = int(t.max()) + 1
    return np.ascontiguousarray(t.reshape(-1), dtype=np.int32), int(n_types)


def type_pair_args(who, ta, tb):
    """two type indices as Python integers (a float or a bool is a ValueError, the range is the library's to refuse)"""
    import numpy as np
    for name, v in (("ta", ta), ("tb", tb)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: %s must be an integer; got %r" % (who, name, v))
    return int(ta), int(tb)


def patch_types(ref_config, axis, cos_half_angle=0.0):
    """blob types of a patchy particle: type 1 for the blobs of the structure `ref_config` (N_blb, 3) whose direction from the
    structure's mean lies within the cap about the body-frame `axis`, n . axis >= cos_half_angle |n| |axis|, else type 0.
    cos_half_angle = 0: a hemisphere, a Janus particle.  A blob at the mean itself is type 0.  -> int32 (N_blb,)"""
    import numpy as np
    cfg = np.asarray(ref_config, dtype=np.float64)
    ax = np.asarray(axis, dtype=np.float64)
    if cfg.ndim != 2 or cfg.shape[1] != 3 or not cfg.shape[0]:
        raise ValueError("patch_types: ref_config must have shape (N_blb, 3); got %s" % (cfg.shape,))
    if ax.shape != (3,) or not np.isfinite(ax).all() or not np.linalg.norm(ax) > 0.0:
        raise ValueError("patch_types: axis must be a finite non-zero vector of 3; got %r" % (axis,))
    if not -1.0 <= float(cos_half_angle) <= 1.0:
        raise ValueError("patch_types: cos_half_angle must lie in [-1, 1]; got %r" % (cos_half_angle,))
    n = cfg - cfg.mean(axis=0)
    ln = np.linalg.norm(n, axis=1)
    inside = (ln > 0.0) & (n @ (ax / np.linalg.norm(ax)) >= float(cos_half_angle) * ln)
    return inside.astype(np.int32)


def check_brownian_mask6(who, mask6, n_bod, replicas=1):
    """The masks per velocity component that the Brownian midpoint step takes (include/rbl.h section 7): in every body's row the
    three rotation entries (3..5) are all 0 or all 1 -- only then are the free components a subset of the coordinates.  The
    library's own refusal, worded as it words it, raised as ValueError before the library is called.  mask6: replicas * n_bod
    rows of six entries, in any shape"""
    import numpy as np
    rot = (np.asarray(mask6).reshape(-1, 6)[:, 3:] != 0).sum(axis=1)
    bad = np.flatnonzero((rot != 0) & (rot != 3))
    if bad.size:
        g = int(bad[0])
        where = "replica %d, body %d" % (g // n_bod, g % n_bod) if replicas > 1 else "body %d" % g
        raise ValueError("%s: %s: the rotation is partly prescribed (entries 3..5 of a body's row of prescribed6 must be all 0 or all "
                         "1 in the Brownian step: the drift of a partly prescribed rotation has not been derived)" % (who, where))


class RunOpts(C.Structure):
    """rbl_run_opts (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("n_steps", C.c_int32), ("brownian", C.c_int32), ("split_rand", C.c_int32),
                ("max_iter", C.c_int32), ("stride", C.c_int32), ("on_error", C.c_int32), ("check_every", C.c_int32),
                ("prescribed_per", C.c_int32), ("seed", C.c_uint64), ("delta", C.c_double), ("rtol", C.c_double),
                ("F_body", C.c_void_p), ("prescribed", C.c_void_p), ("body_in", C.c_void_p), ("slip", C.c_void_p)]


class RunOut(C.Structure):
    """rbl_run_out (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("accepted", C.c_void_p), ("rejected", C.c_void_p), ("first_flags", C.c_void_p),
                ("first_status", C.c_void_p), ("iters_sum", C.c_void_p), ("resid_max", C.c_void_p), ("F_sum", C.c_void_p),
                ("frame_X", C.c_void_p), ("frame_Q", C.c_void_p), ("frame_accepted_at", C.c_void_p), ("frame_F", C.c_void_p),
                ("steps_done", C.c_int32), ("stopped_at", C.c_int32), ("stop_replica", C.c_int32), ("reserved", C.c_int32)]


class McOpts(C.Structure):
    """rbl_mc_opts (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("n_sweeps", C.c_int64), ("sweep_start", C.c_int64), ("seed", C.c_uint64), ("step_x", C.c_double),
                ("step_theta", C.c_double), ("replica_base", C.c_int32), ("kBT_sets", C.c_int32), ("frozen_sets", C.c_int32),
                ("stride", C.c_int32), ("n_trace", C.c_int32), ("reserved", C.c_int32), ("kBT", C.c_void_p), ("frozen", C.c_void_p)]


class McOut(C.Structure):
    """rbl_mc_out (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("tried", C.c_void_p), ("accepted", C.c_void_p), ("wall_rejected", C.c_void_p),
                ("energy_start", C.c_void_p), ("energy_end", C.c_void_p), ("frame_X", C.c_void_p), ("frame_Q", C.c_void_p),
                ("frame_E", C.c_void_p), ("trace", C.c_void_p)]


class McResult:
    """what a Metropolis chain returns (DeviceContext.ensemble_mc, Ensemble.metropolis): tried, accepted, wall_rejected (R,) int64;
    acceptance = accepted / tried (nan where nothing was tried); energy_start, energy_end (R,); with stride > 0 the frames X
    (n_frames, R, N_bod, 3), Q (n_frames, R, N_bod, 4), E (n_frames, R), else None; with trace > 0 the first trials of every replica,
    trace (R, n_trace, 10): body, dX (3), phi (3), dE, u_6, verdict (0 rejected, 1 accepted, 2 rejected at the wall), else None"""

    def __init__(self, tried, accepted, wall_rejected, energy_start, energy_end, X=None, Q=None, E=None, trace=None):
        import numpy as np
        self.tried, self.accepted, self.wall_rejected = tried, accepted, wall_rejected
        self.energy_start, self.energy_end = energy_start, energy_end
        self.X, self.Q, self.E, self.trace = X, Q, E, trace
        with np.errstate(divide="ignore", invalid="ignore"):
            self.acceptance = accepted / tried.astype(np.float64)


def mc_args(who, R, n_bod, n_sweeps, step_x, step_theta, kBT, frozen, stride, trace, sweep_start, replica_base):
    """the argument checks of a Metropolis chain, before the library is called (ValueError) -> (n_sweeps, kBT array or None,
    frozen (sets, N_bod) uint8 or None, stride, trace, sweep_start, replica_base)"""
    import numpy as np
    n_sweeps, stride, trace, sweep_start, replica_base = int(n_sweeps), int(stride), int(trace), int(sweep_start), int(replica_base)
    if n_sweeps < 1:
        raise ValueError("%s: n_sweeps must be >= 1; got %d" % (who, n_sweeps))
    for name, v in (("step_x", step_x), ("step_theta", step_theta)):
        if not np.isfinite(v) or v < 0.0:
            raise ValueError("%s: %s must be finite and >= 0; got %r" % (who, name, v))
    if stride < 0 or trace < 0 or sweep_start < 0 or replica_base < 0:
        raise ValueError("%s: stride, trace, sweep_start and replica_base must be >= 0; got %d, %d, %d, %d"
                         % (who, stride, trace, sweep_start, replica_base))
    if kBT is not None:
        kBT = np.ascontiguousarray(np.atleast_1d(np.asarray(kBT, dtype=np.float64)))
        if kBT.ndim != 1 or kBT.size not in (1, R):
            raise ValueError("%s: kBT must be one value or one per replica (%d); got shape %s" % (who, R, kBT.shape))
        if not np.all(np.isfinite(kBT)) or not np.all(kBT > 0.0):
            raise ValueError("%s: every kBT must be finite and > 0" % who)
    if frozen is not None:
        frozen = np.asarray(frozen)
        if frozen.shape == (n_bod,):
            frozen = frozen.reshape(1, n_bod)
        if frozen.shape not in ((1, n_bod), (R, n_bod)):
            raise ValueError("%s: frozen must have shape (%d,) or (%d, %d); got %s" % (who, n_bod, R, n_bod, frozen.shape))
        frozen = np.ascontiguousarray(frozen != 0, dtype=np.uint8)
    return n_sweeps, kBT, frozen, stride, trace, sweep_start, replica_base


class RunJointOpts(C.Structure):
    """rbl_run_joint_opts (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("gamma", C.c_double), ("joint_velocity", C.c_void_p), ("n_phases", C.c_int32),
                ("rate_sets", C.c_int32), ("start_sets", C.c_int32), ("reserved", C.c_int32), ("phase_steps", C.c_void_p),
                ("phase_rates", C.c_void_p), ("cycle_start", C.c_void_p)]


class RunJointOut(C.Structure):
    """rbl_run_joint_out (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("theta", C.c_void_p), ("cycle_pos", C.c_void_p), ("phi_sum", C.c_void_p),
                ("frame_theta", C.c_void_p), ("frame_phi", C.c_void_p), ("frame_gap", C.c_void_p)]


class RunObsOpts(C.Structure):
    """rbl_run_obs_opts (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("n_probes", C.c_int32), ("point_sets", C.c_int32), ("probe_body", C.c_int32),
                ("moments", C.c_int32), ("points", C.c_void_p)]


class RunObsOut(C.Structure):
    """rbl_run_obs_out (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("u_sum", C.c_void_p), ("D_sum", C.c_void_p), ("frame_u", C.c_void_p), ("frame_D", C.c_void_p)]


class RunDriveOpts(C.Structure):
    """rbl_run_drive_opts (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("amp_sets", C.c_int32), ("omega_sets", C.c_int32), ("t0_sets", C.c_int32), ("n_phases", C.c_int32),
                ("phase_sets", C.c_int32), ("start_sets", C.c_int32), ("lockin", C.c_int32), ("reserved", C.c_int32),
                ("cos_amp", C.c_void_p), ("sin_amp", C.c_void_p), ("omega", C.c_void_p), ("t0", C.c_void_p), ("phase_steps", C.c_void_p),
                ("phase_in", C.c_void_p), ("cycle_start", C.c_void_p)]


class RunDriveOut(C.Structure):
    """rbl_run_drive_out (include/rbl.h section 5)"""
    _fields_ = [("size", C.c_int64), ("X_c", C.c_void_p), ("X_s", C.c_void_p), ("U_c", C.c_void_p), ("U_s", C.c_void_p),
                ("F_c", C.c_void_p), ("F_s", C.c_void_p), ("norm", C.c_void_p), ("cycle_pos", C.c_void_p), ("t_end", C.c_void_p)]


RUN_STOP, RUN_REJECT, RUN_CHECK_DEFAULT = 0, 1, 64


def drive_opts(who, nb6, cos=None, sin=None, omega=None, t0=None, phase_steps=None, phase_in=None, cycle_start=None, lockin=False):
    """rbl_run_drive_opts from arrays -> (RunDriveOpts, the arrays it points into: keep them alive over the call).  cos, sin:
    (6 N_bod,) or (sets, 6 N_bod); omega, t0: a number or (sets,); phase_steps (n_phases,) with phase_in (n_phases, 6 N_bod) or
    (n_phases, sets, 6 N_bod); cycle_start: an integer or (sets,).  The set counts go to the library as they are (it refuses
    what is neither 1 nor R); only what cannot be laid out raises ValueError here"""
    import numpy as np
    d = RunDriveOpts()
    d.size = C.sizeof(RunDriveOpts)
    keep = []

    def amp(name, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != nb6:
            raise ValueError("%s: %s must have shape (%d,) or (sets, %d); got %s" % (who, name, nb6, nb6, a.shape))
        return a
    c_, s_ = amp("cos", cos), amp("sin", sin)
    if c_ is not None and s_ is not None and c_.shape[0] != s_.shape[0]:
        if 1 not in (c_.shape[0], s_.shape[0]):
            raise ValueError("%s: cos and sin must hold the same number of sets, or one of them a single set; got %d and %d"
                             % (who, c_.shape[0], s_.shape[0]))
        sets = max(c_.shape[0], s_.shape[0])
        c_, s_ = (np.ascontiguousarray(np.broadcast_to(a, (sets, nb6))) for a in (c_, s_))
    for a in (c_, s_):
        if a is not None:
            d.amp_sets = a.shape[0]
            keep.append(a)
    d.cos_amp = None if c_ is None else c_.ctypes.data
    d.sin_amp = None if s_ is None else s_.ctypes.data
    if omega is not None:
        om = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
        d.omega, d.omega_sets = om.ctypes.data, om.size
        keep.append(om)
    if t0 is not None:
        t = np.ascontiguousarray(t0, dtype=np.float64).reshape(-1)
        d.t0, d.t0_sets = t.ctypes.data, t.size
        keep.append(t)
    if phase_steps is not None:
        ps = np.ascontiguousarray(phase_steps, dtype=np.int32).reshape(-1)
        pi = np.ascontiguousarray(phase_in, dtype=np.float64)
        if pi.ndim == 2:
            pi = pi.reshape(pi.shape[0], 1, pi.shape[1])
        if pi.ndim != 3 or pi.shape[0] != ps.size or pi.shape[2] != nb6:
            raise ValueError("%s: phase_in must have shape (%d, %d) or (%d, sets, %d); got %s" % (who, ps.size, nb6, ps.size, nb6, pi.shape))
        d.n_phases, d.phase_sets, d.phase_steps, d.phase_in = ps.size, pi.shape[1], ps.ctypes.data, pi.ctypes.data
        keep += [ps, pi]
    if cycle_start is not None:
        cs = np.ascontiguousarray(cycle_start, dtype=np.int32).reshape(-1)
        d.cycle_start, d.start_sets = cs.ctypes.data, cs.size
        keep.append(cs)
    d.lockin = int(bool(lockin))
    return d, keep


class RunResult:
    """what a run of ensemble steps leaves (DeviceContext.ensemble_run, Ensemble.run): per replica accepted, rejected,
    first_flags / first_status (the error word / the status code of the first rejected step, 0: none), iters_sum and resid_max over
    the accepted steps; F_sum and F_mean (R, 6 N_bod) for runs with prescribed bodies (F_mean = F_sum / accepted, NaN where nothing
    was accepted), else None; steps_done, stopped_at (-1: never), stop_replica; the frames X (n_frames, R, N_bod, 3), Q (n_frames,
    R, N_bod, 4), accepted_at (n_frames, R) and, with prescribed bodies, F (n_frames, R, 6 N_bod); status and error: the call's
    status code and message (0, None for a run that did not stop).
    A run with hard joints (DeviceContext.ensemble_run_jointed, Ensemble.run_jointed) adds theta (R, n_joints), the angles it
    leaves, cycle_pos (R,), the positions in the motor schedule at its end, phi_sum and phi_mean (R, n_joints, 3) over the accepted
    steps (phi_mean NaN where nothing was accepted) and the frames theta (n_frames, R, n_joints), phi and gap (n_frames, R,
    n_joints, 3), here as frame_theta, frame_phi and frame_gap; all of them None for other runs.
    A run with observers (DeviceContext.ensemble_run_observed; Ensemble.run / run_jointed with probes or moments) adds, for P probe
    points, u_sum (R, P, 3), the field summed over the replica's accepted steps in step order, u_mean = u_sum / accepted (zeros,
    not NaN, where nothing was accepted) and the frames frame_u (n_frames, R, P, 3); with moments D_sum, D_mean (R, N_bod, 3, 3),
    stresslet_mean (the symmetric traceless part of D_mean) and frame_D (n_frames, R, N_bod, 3, 3).  A frame holds its step's value,
    or the replica's last accepted one where it was rejected in that step (zeros before any).  None for runs without them.
    A driven run (DeviceContext.ensemble_run_driven, Ensemble.run_driven) adds cycle_pos (R,) and t_end (R,), the drive's cycle
    positions and clocks at its end, and with lockin the sums over the replica's accepted steps, in step order, of the step's
    value times cs = cos(omega t) / sn = sin(omega t): X_c, X_s (R, N_bod, 3) of the body centres the step started from, U_c,
    U_s (R, 6 N_bod) of the step's body velocities, F_c, F_s (R, 6 N_bod) of the loads (masked runs) and norm (R, 5) = sum cs,
    sn, cs^2, sn^2, cs sn"""
    theta = cycle_pos = phi_sum = phi_mean = frame_theta = frame_phi = frame_gap = None
    u_sum = u_mean = frame_u = D_sum = D_mean = stresslet_mean = frame_D = None
    X_c = X_s = U_c = U_s = F_c = F_s = norm = t_end = None

    def __repr__(self):
        return "RunResult(steps_done=%d, stopped_at=%d, accepted=%d..%d, rejected=%d)" % (
            self.steps_done, self.stopped_at, int(self.accepted.min()), int(self.accepted.max()), int(self.rejected.sum()))


def np_contig(a):
    import numpy as np
    return np.ascontiguousarray(a)


def periodic_args(who, Lx, Ly, images):
    """the checks set_periodic can make before the library is called -> (Lx, Ly, nx, ny)"""
    import numbers
    for name, v in (("Lx", Lx), ("Ly", Ly)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise TypeError("%s: %s must be a real number, got %r" % (who, name, v))
    try:
        n = tuple(images)
    except TypeError:
        raise TypeError("%s: images must be a pair of integers (nx, ny), got %r" % (who, images)) from None
    if len(n) != 2:
        raise ValueError("%s: images must be a pair (nx, ny), got %d entries" % (who, len(n)))
    for v in n:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError("%s: images must be integers, got %r" % (who, v))
    return float(Lx), float(Ly), int(n[0]), int(n[1])


def cells_args(who, Lx, Ly, images, R=None):
    """the checks set_cells can make before the library is called: Lx, Ly real scalars or (R,), images (nx, ny) or (R, 2) of
    integers, scalars broadcast -> (Lx (R,), Ly (R,), n (R, 2) int32).  R=None: the arrays' own common length (1 when all are
    scalars), for the caller to compare with the ensemble's"""
    import numbers
    import numpy as np
    sizes = {}
    out = {}
    for name, v in (("Lx", Lx), ("Ly", Ly)):
        if isinstance(v, bool) or isinstance(v, (str, bytes)) or v is None:
            raise TypeError("%s: %s must be a real number or an array of R real numbers, got %r" % (who, name, v))
        if isinstance(v, numbers.Real):
            out[name] = float(v)
            continue
        try:
            arr = np.asarray(v)
        except Exception:
            raise TypeError("%s: %s must be a real number or an array of R real numbers, got %r" % (who, name, v)) from None
        if arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
            raise TypeError("%s: %s must hold real numbers, got dtype %s" % (who, name, arr.dtype))
        if arr.ndim != 1 or arr.size < 1:
            raise ValueError("%s: %s must be a real number or have shape (R,), got shape %s" % (who, name, arr.shape))
        out[name] = arr.astype(np.float64)
        sizes[name] = arr.size
    try:
        narr = np.asarray(images)
    except Exception:
        raise TypeError("%s: images must be a pair of integers (nx, ny) or an (R, 2) array of integers, got %r" % (who, images)) from None
    if narr.dtype == np.bool_ or not np.issubdtype(narr.dtype, np.integer):
        raise TypeError("%s: images must be integers, got %r" % (who, images))
    if narr.shape == (2,):
        pass
    elif narr.ndim == 2 and narr.shape[1] == 2 and narr.shape[0] >= 1:
        sizes["images"] = narr.shape[0]
    else:
        raise ValueError("%s: images must be a pair (nx, ny) or have shape (R, 2), got shape %s" % (who, narr.shape))
    if R is None:
        R = max(sizes.values()) if sizes else 1
    for name, n in sizes.items():
        if n != R:
            raise ValueError("%s: %s has %d entries, the ensemble has R = %d replicas" % (who, name, n, R))
    L = [np.ascontiguousarray(np.broadcast_to(out[name], (R,)), dtype=np.float64) for name in ("Lx", "Ly")]
    return L[0], L[1], np.ascontiguousarray(np.broadcast_to(narr, (R, 2)), dtype=np.int32)


class DeviceContext:
    """One rbl_ctx bound to the current HIP device and a stream: its own, or (`borrow`) somebody else's."""

    _owner = None       # a borrowed view: whoever owns the rbl_ctx, kept alive; the view never destroys the context
    _borrowed = False

    def __init__(self, a, eta, wall, cfg=None, dt=0.0, kBT=1.0, stream_ptr=None):
        import numpy as np
        self.L = lib()
        self.h = self.L.rbl_create()
        if not self.h:
            raise RblError("rbl_create failed")
        cfg = np.ascontiguousarray(np.zeros((1, 3)) if cfg is None else cfg, dtype=np.float64)
        self._chk(self.L.rbl_set_parameters(self.h, a, dt, kBT, eta, cfg.ctypes.data, cfg.shape[0]))
        self._a = float(a)
        self._cfg = cfg.reshape(-1, 3).copy()
        self._chk(self.L.rbl_set_wall_pc(self.h, int(bool(wall))))
        self._chk(self.L.rbl_set_stream(self.h, stream_ptr))
        self._stream_ptr = int(stream_ptr or 0)

    @classmethod
    def borrow(cls, handle, a, cfg, owner=None):
        """A view of an existing rbl_ctx (handle: its address, `c_rigid.CManyBodies.handle()`) that calls nothing on it: the
        owner's parameters, wall flag and stream stand, and the owner destroys it.  a, cfg: the blob radius and the structure the
        owner was given (the default cutoff, blob_anchor).  owner: kept referenced, so the context outlives the view.  The view
        calls into the in-package library, the one c_rigid is linked against, whatever RBL_LIBRARY says."""
        import numpy as np
        self = cls.__new__(cls)
        self.L = lib(IN_PACKAGE_LIB)
        self.h = int(handle)
        self._owner, self._borrowed = owner, True
        self._a = float(a)
        self._cfg = np.array(cfg, dtype=np.float64).reshape(-1, 3)
        self._stream_ptr = 0
        return self

    def _chk(self, rc):
        if rc != 0:
            raise RblError("%s [rbl status %d]" % (self.L.rbl_last_error(self.h).decode(), rc))

    def set_config(self, X, Q):
        import numpy as np
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1)
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1)
        self._chk(self.L.rbl_set_config(self.h, X.ctypes.data, Q.ctypes.data, X.size // 3))

    def set_comm(self, sharded, native=None):
        """multi-GPU inside the library's solvers: `sharded` is a dist.ShardedMobility (rank, world, process group).  Every
        full mobility product of librbl's own GMRES / Lanczos / step drivers becomes this rank's share + one collective.
        native (default: whenever the process group moves device buffers, i.e. backend nccl): RCCL INSIDE librbl --
        rank 0's rbl_comm_unique_id is broadcast through the process group once, then rbl_comm_init_rccl; no Python runs
        between two products of a solve.  Otherwise (gloo rehearsals, several ranks sharing one GPU) the collectives are
        callbacks into torch.distributed, host-staged.  None switches it off.  A group of one rank keeps it on only when
        `sharded` was built with force_collectives (the world-1 RCCL test)."""
        import torch
        import torch.distributed as dist
        if sharded is None or not sharded.collectives:
            self._comm_cb = self._comm_cb2 = None
            self._chk(self.L.rbl_set_comm(self.h, 0, 1, None, None))
            return
        if native is None:
            native = not sharded.stage_cpu and sharded.device.type == "cuda"
        if native:
            ident = [None]
            if sharded.rank == 0:
                buf = C.create_string_buffer(128)
                if self.L.rbl_comm_unique_id(buf) != 0:
                    raise RblError("rbl_comm_unique_id failed (librccl not loadable?)")
                ident[0] = buf.raw
            dist.broadcast_object_list(ident, src=dist.get_global_rank(sharded.group, 0) if sharded.group is not None else 0,
                                       group=sharded.group)
            self._comm_cb = self._comm_cb2 = None
            self._chk(self.L.rbl_comm_init_rccl(self.h, ident[0], sharded.rank, sharded.world))
            return

        class _View:   # a raw device pointer as a torch tensor (no copy)
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        views = {}     # (pointer, count) -> tensor view: librbl works on the same few buffers over and over

        def _view(ptr, count):
            t = views.get((ptr, count))
            if t is None:
                t = views[(ptr, count)] = torch.as_tensor(_View(ptr, int(count)), device=sharded.device)
            return t

        def _on_ctx_stream(fn):
            # rbl.h: a collective must be ordered on the CONTEXT's stream (the library enqueues producer and consumer
            # kernels there); torch issues collectives on its current stream, so make the context's stream current
            if sharded.device.type == "cuda" and torch.cuda.current_stream(sharded.device).cuda_stream != self._stream_ptr:
                with torch.cuda.stream(torch.cuda.ExternalStream(self._stream_ptr, device=sharded.device)):
                    fn()
            else:
                fn()

        def _allreduce(user, ptr, count):
            try:
                _on_ctx_stream(lambda: sharded.all_reduce_sum(_view(ptr, count)))
                return 0
            except Exception as e:      # never unwind through the C caller
                import sys
                print("rbl all-reduce callback failed: %r" % (e,), file=sys.stderr)
                return 1

        def _allgatherv(user, ptr, offs, cnts):
            try:
                W = sharded.world
                o = [int(offs[r]) for r in range(W)]
                n = [int(cnts[r]) for r in range(W)]
                _on_ctx_stream(lambda: sharded.all_gather_segments(lambda a, k: _view(ptr + 8 * a, k), o, n))
                return 0
            except Exception as e:
                import sys
                print("rbl all-gather callback failed: %r" % (e,), file=sys.stderr)
                return 1

        self._comm_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)(_allreduce)
        self._comm_cb2 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64))(_allgatherv)
        self._chk(self.L.rbl_set_comm_ops(self.h, sharded.rank, sharded.world, C.cast(self._comm_cb, C.c_void_p),
                                          C.cast(self._comm_cb2, C.c_void_p), None))

    def comm_info(self):
        """(rank, world, kind) of the context's communicator; kind 0 none, 1 callbacks, 2 RCCL inside librbl"""
        r, w, k = C.c_int(0), C.c_int(1), C.c_int(0)
        self._chk(self.L.rbl_comm_info(self.h, C.byref(r), C.byref(w), C.byref(k)))
        return r.value, w.value, k.value

    def comm_finalize(self):
        self._chk(self.L.rbl_comm_finalize(self.h))
        self._comm_cb = self._comm_cb2 = None

    # -- named options (include/rbl.h RBL_OPT_*) -----------------------------------------
    def _opt_key(self, name):
        key = name if isinstance(name, int) else self.L.rbl_option_key(str(name).encode())
        if not key:
            raise RblError("unknown option %r" % (name,))
        return key

    def set_option(self, name, value):
        self._chk(self.L.rbl_set_option(self.h, self._opt_key(name), int(value)))

    def get_option(self, name):
        v = C.c_int64(0)
        self._chk(self.L.rbl_get_option(self.h, self._opt_key(name), C.byref(v)))
        return v.value

    def set_stream(self, stream_ptr):
        self._chk(self.L.rbl_set_stream(self.h, stream_ptr))
        self._stream_ptr = int(stream_ptr or 0)

    TIMING_PHASES = ("product", "per_body", "factor", "collective", "dense", "total", "forces")   # RBL_T_* of include/rbl.h

    def set_timing(self, on=True):
        """hipEvent brackets around the phases of librbl's own solvers (rbl_set_timing)"""
        self._chk(self.L.rbl_set_timing(self.h, int(bool(on))))

    def reset_timings(self):
        self._chk(self.L.rbl_reset_timings(self.h))

    def timings(self):
        """{phase: (milliseconds, brackets)} accumulated since the last reset (synchronises the stream)"""
        n = len(self.TIMING_PHASES)
        ms, calls = (C.c_double * n)(), (C.c_int64 * n)()
        self._chk(self.L.rbl_get_timings(self.h, ms, calls))
        return {k: (ms[i], calls[i]) for i, k in enumerate(self.TIMING_PHASES)}

    # -- configuration-dependent forces (include/rbl.h section 4) ----------------------
    def set_interactions(self, w=0.0, eps_wall=0.0, b_wall=1.0, eps_blob=0.0, b_blob=1.0, r_cut=None, on=True):
        """weight w per blob, wall repulsion eps_wall exp(-(h - a)/b_wall), blob-blob repulsion eps_blob (2a/r) exp(-(r - 2a)/b_blob)
        between bodies, truncated at r_cut (default 2a + 20 b_blob); the whole-step entry points and the krylov.py steppers add
        these forces at q^n.  on=False switches the model off."""
        if r_cut is None:
            r_cut = 2.0 * self._a + 20.0 * b_blob
        self._chk(self.L.rbl_set_interactions(self.h, float(w), float(eps_wall), float(b_wall), float(eps_blob), float(b_blob),
                                              float(r_cut), int(bool(on))))

    def interaction_params(self):
        """{w, eps_wall, b_wall, eps_blob, b_blob, r_cut, on, a} of the context's force model"""
        v, on = (C.c_double * 6)(), C.c_int(0)
        self._chk(self.L.rbl_get_interactions(self.h, v, C.byref(on)))
        return dict(zip(("w", "eps_wall", "b_wall", "eps_blob", "b_blob", "r_cut"), list(v)), on=bool(on.value), a=self._a)

    def interactions_on(self):
        """any term of the model is on: the built-in one, a pair table, a height table, the traps, dipole pairs, the field torque,
        bonds"""
        return self.interactions_active() != 0

    def interactions_active(self):
        """bit 0 built-in terms, bit 1 pair table, bit 2 height table, bit 3 traps, bit 4 dipole pairs, bit 5 field torque,
        bit 6 bonds, bit 7 typed pair tables (types on and a usable type table on)"""
        m = C.c_int(0)
        self._chk(self.L.rbl_interactions_active(self.h, C.byref(m)))
        return m.value

    def set_pair_table(self, U, dU, r_min, r_cut, on=True):
        """a radial potential between blobs of different bodies from its values U and derivatives dU = dU/dr on the uniform grid
        r_min .. r_cut (see `tabulate`): cubic Hermite inside, the tangent at r_min below it, nothing beyond r_cut (the table is
        not shifted: U(r_cut) != 0 is a jump in the energy).  Adds to the built-in steric term.  on=False stores it switched off; U = dU = None
        with on=False only switches the stored table off."""
        if U is None and dU is None and not on:       # only the switch: the stored table stays
            return self._chk(self.L.rbl_set_pair_table(self.h, None, None, 0, 0.0, 0.0, 0))
        U, dU = table_arrays("set_pair_table", U, dU)
        self._chk(self.L.rbl_set_pair_table(self.h, U.ctypes.data, dU.ctypes.data, U.size, float(r_min), float(r_cut), int(bool(on))))

    def set_height_table(self, U, dU, h_min, h_cut, on=True):
        """the same construction in the blob height z over h_min .. h_cut, with or without the wall"""
        if U is None and dU is None and not on:
            return self._chk(self.L.rbl_set_height_table(self.h, None, None, 0, 0.0, 0.0, 0))
        U, dU = table_arrays("set_height_table", U, dU)
        self._chk(self.L.rbl_set_height_table(self.h, U.ctypes.data, dU.ctypes.data, U.size, float(h_min), float(h_cut), int(bool(on))))

    def _get_table(self, fn):
        import numpy as np
        n, lo, hi, on = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        self._chk(fn(self.h, C.byref(n), C.byref(lo), C.byref(hi), C.byref(on), None))
        coef = np.zeros((max(n.value - 1, 0), 4))
        if n.value:
            self._chk(fn(self.h, None, None, None, None, coef.ctypes.data))
        return dict(n=n.value, lo=lo.value, hi=hi.value, on=bool(on.value), coef=coef)

    def pair_table(self):
        """{n, lo, hi, on, coef (n - 1, 4)} of the pair table (n = 0: never set)"""
        return self._get_table(self.L.rbl_get_pair_table)

    def set_blob_types(self, types, n_types=None, on=True):
        """a type per blob, integers in [0, n_types), n_types <= 8 (None: the largest type + 1): shape (N_blb,) -- every body
        alike -- or (N_bod, N_blb), one row per body of the system (of ONE replica of an ensemble, shared by all).  With
        set_type_table a pair of blobs of different bodies gets the table of its two types on top of the steric term and the
        untyped pair table: a patch of another type makes the pair potential depend on orientation (`patch_types`).
        types=None with on=False only switches the stored types off."""
        if types is None and not on:
            return self._chk(self.L.rbl_set_blob_types(self.h, None, 0, 0, 0))
        t, n_types = blob_type_args("set_blob_types", types, n_types)
        self._chk(self.L.rbl_set_blob_types(self.h, t.ctypes.data, t.size, n_types, int(bool(on))))

    def blob_types(self):
        """{on, n_types, types (n,) int32} (n = 0: never set)"""
        import numpy as np
        n, nt, on = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_blob_types(self.h, C.byref(n), C.byref(nt), C.byref(on), None))
        t = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._chk(self.L.rbl_get_blob_types(self.h, None, None, None, t.ctypes.data))
        return dict(on=bool(on.value), n_types=nt.value, types=t)

    def set_type_table(self, ta, tb, U, dU, r_min, r_cut, on=True):
        """the pair table of set_pair_table for blobs of the types ta and tb (one table per unordered pair: (tb, ta) names the
        same one).  U = dU = None with on=False only switches the stored table off."""
        ta, tb = type_pair_args("set_type_table", ta, tb)
        if U is None and dU is None and not on:
            return self._chk(self.L.rbl_set_type_table(self.h, ta, tb, None, None, 0, 0.0, 0.0, 0))
        U, dU = table_arrays("set_type_table", U, dU)
        self._chk(self.L.rbl_set_type_table(self.h, ta, tb, U.ctypes.data, dU.ctypes.data, U.size, float(r_min), float(r_cut), int(bool(on))))

    def type_table(self, ta, tb):
        """{n, lo, hi, on, coef (n - 1, 4)} of the table of the type pair (ta, tb) (n = 0: never set)"""
        ta, tb = type_pair_args("type_table", ta, tb)
        return self._get_table(lambda h, *a: self.L.rbl_get_type_table(h, ta, tb, *a))

    def clear_type_tables(self):
        """forget every type table; the types stay"""
        self._chk(self.L.rbl_clear_type_tables(self.h))

    def height_table(self):
        return self._get_table(self.L.rbl_get_height_table)

    def set_traps(self, k, X0, on=True):
        """harmonic traps on the body centres: stiffness k and centre X0, (n, 3) each (a component of k that is 0: no trap along
        that axis); force -k (X - X0) on the body, no torque.  n: the bodies -- of an ensemble: those of one replica (shared by
        all) or R N_bod entries, replica-major"""
        import numpy as np
        if k is None and X0 is None and not on:
            return self._chk(self.L.rbl_set_traps(self.h, None, None, 0, 0))
        k, X0 = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(X0, dtype=np.float64)
        if k.ndim != 2 or k.shape[1] != 3 or k.shape != X0.shape:
            raise ValueError("set_traps: k and X0 must both have shape (n, 3); got %s and %s" % (k.shape, X0.shape))
        self._chk(self.L.rbl_set_traps(self.h, k.ctypes.data, X0.ctypes.data, k.shape[0], int(bool(on))))

    def traps(self):
        """{on, k (n, 3), X0 (n, 3)}"""
        import numpy as np
        n, on = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_traps(self.h, C.byref(n), C.byref(on), None, None))
        k, X0 = np.zeros((n.value, 3)), np.zeros((n.value, 3))
        if n.value:
            self._chk(self.L.rbl_get_traps(self.h, None, None, k.ctypes.data, X0.ctypes.data))
        return dict(on=bool(on.value), k=k, X0=X0)

    def set_dipoles(self, m_body, c_dd=0.0, r_core=None, r_cut=float("inf"), on=True):
        """permanent magnetic moments fixed in the bodies: m_body (3,) -- every body alike -- or (n, 3), body frame, n the bodies
        as set_traps counts them.  c_dd > 0 switches the dipole pairs between body centres on (c_dd: mu_0 / 4 pi in the caller's
        units; r_core: below it the pair energy is a quadratic form, the force bounded; pairs beyond r_cut are skipped, the
        energy is not shifted); the torque of set_magnetic_field needs the moments too.  m_body=None with on=False only switches
        the dipoles off."""
        if m_body is None and not on:
            return self._chk(self.L.rbl_set_dipoles(self.h, None, 0, 0.0, 0.0, 0.0, 0))
        m, r_core = dipole_args("set_dipoles", m_body, c_dd, r_core)
        self._chk(self.L.rbl_set_dipoles(self.h, m.ctypes.data, m.shape[0], float(c_dd), r_core, float(r_cut), int(bool(on))))

    def dipoles(self):
        """{on, c_dd, r_core, r_cut, m_body (n, 3)} (n = 0: never set)"""
        import numpy as np
        n, on = C.c_int(0), C.c_int(0)
        c_dd, r_core, r_cut = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self._chk(self.L.rbl_get_dipoles(self.h, C.byref(n), C.byref(c_dd), C.byref(r_core), C.byref(r_cut), C.byref(on), None))
        m = np.zeros((n.value, 3))
        if n.value:
            self._chk(self.L.rbl_get_dipoles(self.h, None, None, None, None, None, m.ctypes.data))
        return dict(on=bool(on.value), c_dd=c_dd.value, r_core=r_core.value, r_cut=r_cut.value, m_body=m)

    def set_magnetic_field(self, B0=None, B1=None, B2=None, omega=0.0, on=True):
        """the uniform field B(t) = B0 + B1 cos(omega t) + B2 sin(omega t), lab frame (None: zeros), t the field time of
        set_field_time: torque m x B on every body that carries a moment (set_dipoles), no force.  B0 = B1 = B2 = None with
        on=False only switches the field off."""
        if B0 is None and B1 is None and B2 is None and not on:
            return self._chk(self.L.rbl_set_magnetic_field(self.h, None, None, None, 0.0, 0))
        B0, B1, B2 = field_args("set_magnetic_field", B0, B1, B2)
        self._chk(self.L.rbl_set_magnetic_field(self.h, B0.ctypes.data, B1.ctypes.data, B2.ctypes.data, float(omega), int(bool(on))))

    def magnetic_field(self):
        """{on, omega, B0, B1, B2}"""
        import numpy as np
        B, om, on = np.zeros((3, 3)), C.c_double(0.0), C.c_int(0)
        self._chk(self.L.rbl_get_magnetic_field(self.h, B.ctypes.data, C.byref(om), C.byref(on)))
        return dict(on=bool(on.value), omega=om.value, B0=B[0].copy(), B1=B[1].copy(), B2=B[2].copy())

    def set_field_time(self, t):
        """the time the field is evaluated at: a number, or one per replica of an ensemble.  No step advances it; inside
        ensemble_run replica r's clock runs as t[r] + dt * (its accepted steps) and the value set here stays"""
        import numpy as np
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=np.float64)))
        if t.ndim != 1:
            raise ValueError("set_field_time: t must be a number or one-dimensional; got shape %s" % (t.shape,))
        self._chk(self.L.rbl_set_field_time(self.h, t.ctypes.data, t.size))

    def field_time(self):
        """the field time(s) as set, (n,)"""
        import numpy as np
        n = C.c_int(0)
        self._chk(self.L.rbl_get_field_time(self.h, C.byref(n), None))
        t = np.zeros(n.value)
        self._chk(self.L.rbl_get_field_time(self.h, None, t.ctypes.data))
        return t

    def set_bonds(self, body, anchor_a, anchor_b, k, l0=0.0, kind=None, on=True):
        """bonds and tethers between anchor points fixed in the bodies (include/rbl.h section 4): bond b joins the point
        X_i + R(Q_i) anchor_a[b] of body i = body[b, 0] to the same kind of point of body j = body[b, 1] != i, or, with j = -1, to
        the lab point anchor_b[b].  kind 0 (the default): U = k (d - l0)^2 / 2; kind 1: U = k T(d), T the bond table of
        set_bond_table.  k, l0: a number, (n,) or (n_sets, n), n_sets = 1 or the replicas of an ensemble.  body=None with
        on=False only switches the bonds off."""
        if body is None and not on:
            return self._chk(self.L.rbl_set_bonds(self.h, 0, None, None, None, None, 0, 0))
        b, anchor, kind, param = bond_args("set_bonds", body, anchor_a, anchor_b, k, l0, kind, sets=None)
        self._chk(self.L.rbl_set_bonds(self.h, b.shape[0], b.ctypes.data, anchor.ctypes.data, None if kind is None else kind.ctypes.data,
                                       param.ctypes.data, param.shape[0], int(bool(on))))

    def bonds(self):
        """{on, body (n, 2), anchor_a (n, 3), anchor_b (n, 3), kind (n,), k (n_sets, n), l0 (n_sets, n)} (n = 0: never set)"""
        import numpy as np
        n, ns, on = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_bonds(self.h, C.byref(n), C.byref(ns), C.byref(on), None, None, None, None))
        body, anchor = np.zeros((n.value, 2), dtype=np.int32), np.zeros((n.value, 6))
        kind, param = np.zeros(n.value, dtype=np.int32), np.zeros((ns.value, n.value, 2))
        if n.value:
            self._chk(self.L.rbl_get_bonds(self.h, None, None, None, body.ctypes.data, anchor.ctypes.data, kind.ctypes.data, param.ctypes.data))
        return dict(on=bool(on.value), body=body, anchor_a=anchor[:, :3].copy(), anchor_b=anchor[:, 3:].copy(), kind=kind,
                    k=param[:, :, 0].copy(), l0=param[:, :, 1].copy())

    # -- hard joints (include/rbl.h section 9) ---------------------------------------------------------------------------------
    def set_joints(self, body, anchor_a, anchor_b, on=True):
        """ball joints between the point X_i + R(Q_i) anchor_a[j] of body i = body[j, 0] and the same kind of point of body
        body[j, 1] != i, or, with body[j, 1] = -1, the lab point anchor_b[j] (a pivot): constraints of solve_jointed /
        step_jointed, ignored by every other call.  body=None with on=False only switches them off."""
        if body is None and not on:
            return self._chk(self.L.rbl_set_joints(self.h, 0, None, None, 0))
        b, anchor = joint_args("set_joints", body, anchor_a, anchor_b)
        self._chk(self.L.rbl_set_joints(self.h, b.shape[0], b.ctypes.data, anchor.ctypes.data, int(bool(on))))

    def joints(self):
        """{on, body (n, 2), anchor_a (n, 3), anchor_b (n, 3)} (n = 0: never set)"""
        import numpy as np
        n, on = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_joints(self.h, C.byref(n), C.byref(on), None, None))
        body, anchor = np.zeros((n.value, 2), dtype=np.int32), np.zeros((n.value, 6))
        if n.value:
            self._chk(self.L.rbl_get_joints(self.h, None, None, body.ctypes.data, anchor.ctypes.data))
        return dict(on=bool(on.value), body=body, anchor_a=anchor[:, :3].copy(), anchor_b=anchor[:, 3:].copy())

    def _joints_active(self):
        n, on = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_joints(self.h, C.byref(n), C.byref(on), None, None))
        return n.value if on.value else 0

    def _jointed_args(self, who, F_body, slip, jv, jname):
        import numpy as np
        nb, nl = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), C.byref(nl)))
        nj = self._joints_active()
        F = np.ascontiguousarray(F_body, dtype=np.float64).reshape(-1)
        sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64).reshape(-1)
        jr = None if jv is None else np.ascontiguousarray(jv, dtype=np.float64).reshape(-1)
        if F.size != 6 * nb.value or (sl is not None and sl.size != 3 * nb.value * nl.value) or (jr is not None and jr.size != 3 * nj):
            raise ValueError("%s: F_body (6 N_bod), slip (3 N_blobs) or %s (3 n_joints) has the wrong size" % (who, jname))
        return nb.value, nl.value, nj, F, sl, jr

    def solve_jointed(self, F_body, slip=None, joint_rhs=None, max_iter=100, rtol=1.0e-8):
        """the saddle solve with the joints as constraints J U = joint_rhs (None: zero); host arrays -> (lambda, U, phi, iterations,
        residual estimate), phi (3 n_joints) in the convention of F_body: F_body + J^T phi in the plain solve gives the same
        lambda and U.  Joints off or never set: the plain solve, phi empty."""
        import numpy as np
        nb, nl, nj, F, sl, jr = self._jointed_args("solve_jointed", F_body, slip, joint_rhs, "joint_rhs")
        lam, U, phi = np.empty(3 * nb * nl), np.empty(6 * nb), np.empty(3 * nj)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_solve_jointed(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                           None if jr is None or not nj else jr.ctypes.data, int(max_iter), float(rtol), lam.ctypes.data,
                                           U.ctypes.data, phi.ctypes.data if nj else None, C.byref(it), C.byref(res)))
        return lam, U, phi, it.value, res.value

    def solve_jointed_dev(self, d_F_body, d_slip, d_joint_rhs, max_iter, rtol, d_lam, d_U, d_phi):
        """the same on device addresses (d_slip, d_joint_rhs, d_lam may be None / 0) -> (iterations, residual estimate)"""
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_solve_jointed_dev(self.h, d_F_body, d_slip or None, d_joint_rhs or None, int(max_iter), float(rtol),
                                               d_lam or None, d_U, d_phi or None, C.byref(it), C.byref(res)))
        return it.value, res.value

    def step_jointed(self, F_body, slip=None, joint_velocity=None, gamma=1.0, max_iter=50, rtol=1.0e-8):
        """one deterministic time step with the joints: J U = -(gamma / dt) gap + joint_velocity -> (phi, iterations, residual
        estimate)"""
        import numpy as np
        nb, nl, nj, F, sl, jr = self._jointed_args("step_jointed", F_body, slip, joint_velocity, "joint_velocity")
        phi = np.empty(3 * nj)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_step_jointed(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                          None if jr is None or not nj else jr.ctypes.data, float(gamma), int(max_iter), float(rtol),
                                          phi.ctypes.data if nj else None, C.byref(it), C.byref(res)))
        return phi, it.value, res.value

    def joint_state(self):
        """-> (gaps p_A - p_B at the context's configuration (n_joints, 3), phi of the last jointed solve or step (n_joints, 3));
        for a set given through set_joint_kinds -> (gap, phi, theta (n_joints,)), the gap rows of a lock or axis joint its angular
        gap e"""
        import numpy as np
        n, kinds = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_joint_kinds(self.h, C.byref(n), None, C.byref(kinds), None, None, None, None, None, None, None))
        gap, phi = np.zeros((max(n.value, 1), 3)), np.zeros((max(n.value, 1), 3))
        if not kinds.value:
            self._chk(self.L.rbl_joint_state(self.h, gap.ctypes.data, phi.ctypes.data))
            return gap[:n.value], phi[:n.value]
        theta = np.zeros(max(n.value, 1))
        self._chk(self.L.rbl_joint_state_kinds(self.h, gap.ctypes.data, phi.ctypes.data, theta.ctypes.data))
        return gap[:n.value], phi[:n.value], theta[:n.value]

    def set_joint_kinds(self, body, kind, anchor_a=None, anchor_b=None, axis=None, q_rel=None, on=True):
        """joints of every kind (include/rbl.h section 9): kind[j] JOINT_BALL (anchors as set_joints), JOINT_LOCK (w_A = w_B; with
        a rate, a motor about axis) or JOINT_AXIS (relative rotation free about axis only); axis in body A's frame; q_rel the
        target Q_A^-1 Q_B, None: that of the current configuration.  body=None with on=False only switches the joints off."""
        if body is None and not on:
            return self._chk(self.L.rbl_set_joint_kinds(self.h, 0, None, None, None, None, None, 0))
        b, k, anchor, ax, qr = joint_kind_args("set_joint_kinds", body, kind, anchor_a, anchor_b, axis, q_rel)
        if q_rel is None and (k != JOINT_BALL).any():
            default_q_rel("set_joint_kinds", b, k, qr, self._config()[1])
        self._chk(self.L.rbl_set_joint_kinds(self.h, b.shape[0], b.ctypes.data, anchor.ctypes.data, k.ctypes.data, ax.ctypes.data,
                                             qr.ctypes.data, int(bool(on))))

    def joint_kinds(self):
        """{on, by_kinds, body, anchor_a, anchor_b, kind, axis, q_rel, theta, rate} of the stored joints (n = 0: never set); a set
        given through set_joints reads back as ball joints throughout"""
        import numpy as np
        n, on, kinds = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_joint_kinds(self.h, C.byref(n), C.byref(on), C.byref(kinds), None, None, None, None, None, None, None))
        m = n.value
        body, anchor, kind = np.zeros((m, 2), dtype=np.int32), np.zeros((m, 6)), np.zeros(m, dtype=np.int32)
        axis, q_rel, theta, rate = np.zeros((m, 3)), np.zeros((m, 4)), np.zeros(m), np.zeros(m)
        if m:
            self._chk(self.L.rbl_get_joint_kinds(self.h, None, None, None, body.ctypes.data, anchor.ctypes.data, kind.ctypes.data,
                                                 axis.ctypes.data, q_rel.ctypes.data, theta.ctypes.data, rate.ctypes.data))
        return dict(on=bool(on.value), by_kinds=bool(kinds.value), body=body, anchor_a=anchor[:, :3].copy(), anchor_b=anchor[:, 3:].copy(),
                    kind=kind, axis=axis, q_rel=q_rel, theta=theta, rate=rate)

    def set_joint_rates(self, rates):
        """the motors' rates, one per stored joint (a number: every lock joint alike is NOT assumed -- give (n_joints,)): body B of
        a lock joint turns relative to body A at +rate about the joint's axis; 0 for every other kind"""
        import numpy as np
        n = C.c_int(0)
        self._chk(self.L.rbl_get_joints(self.h, C.byref(n), None, None, None))
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.size != n.value or not n.value:
            raise ValueError("set_joint_rates: rates must have one value per stored joint (%d); got %d" % (n.value, r.size))
        if not np.isfinite(r).all():
            raise ValueError("set_joint_rates: joint %d: the rate must be finite" % int(np.argmin(np.isfinite(r))))
        self._chk(self.L.rbl_set_joint_rates(self.h, r.ctypes.data))

    def _config(self):
        nb, nl = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), C.byref(nl)))
        return self.get_config(nb.value)

    def hinge(self, a, b, point, axis):
        """rows of a five-row hinge (ball + axis joint) at the current configuration; point and axis in the lab frame"""
        return hinge(*self._config(), a, b, point, axis)

    def weld(self, a, b, point):
        """rows of a weld (ball + lock joint) at the current configuration; point in the lab frame"""
        return weld(*self._config(), a, b, point)

    def motor(self, a, b, point, axis):
        """rows of a motor (ball + lock joint, driven by set_joint_rates) at the current configuration"""
        return motor(*self._config(), a, b, point, axis)

    # -- periodic cell in x and y (include/rbl.h section 10) ---------------------------------------------------------------------
    def set_periodic(self, Lx, Ly, images=(1, 1), on=True):
        """the periodic cell: lengths Lx, Ly (0: that axis is open) and the image counts (nx, ny) of the truncated lattice sum,
        |p| <= nx and |q| <= ny images about the nearest one of every pair (1 ... 16 on a periodic axis).  With the cell on every
        mobility product of the library is the periodic one and the pair forces use the minimum image; coordinates stay unwrapped."""
        Lx, Ly, nx, ny = periodic_args("set_periodic", Lx, Ly, images)
        self._chk(self.L.rbl_set_periodic(self.h, Lx, Ly, nx, ny, int(bool(on))))

    def periodic(self):
        """{on, Lx, Ly, images (nx, ny)} (both lengths 0: never set)"""
        Lx, Ly, nx, ny, on = C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_periodic(self.h, C.byref(Lx), C.byref(Ly), C.byref(nx), C.byref(ny), C.byref(on)))
        return dict(on=bool(on.value), Lx=Lx.value, Ly=Ly.value, images=(nx.value, ny.value))

    # -- the cell of an ensemble (include/rbl.h section 5): state of its own beside the one above --------------------------------------
    def ensemble_set_periodic(self, Lx, Ly, images=(1, 1), on=True):
        """one periodic cell shared by the replicas of the context's ensemble (Lx, Ly, images as set_periodic takes them): the
        one-kernel solver, the drift and the dense Brownian root sum over the images, the pair forces use the minimum image"""
        Lx, Ly, nx, ny = periodic_args("ensemble_set_periodic", Lx, Ly, images)
        self._chk(self.L.rbl_ensemble_set_periodic(self.h, Lx, Ly, nx, ny, int(bool(on))))

    def ensemble_periodic(self):
        """{on, Lx, Ly, images (nx, ny)} of the ensemble's cell (both lengths 0: never set)"""
        Lx, Ly, nx, ny, on = C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_ensemble_get_periodic(self.h, C.byref(Lx), C.byref(Ly), C.byref(nx), C.byref(ny), C.byref(on)))
        return dict(on=bool(on.value), Lx=Lx.value, Ly=Ly.value, images=(nx.value, ny.value))

    def ensemble_set_cells(self, Lx, Ly, images=(1, 1), on=True):
        """a periodic cell PER REPLICA of the context's ensemble: Lx, Ly real scalars or (R,), images (nx, ny) or (R, 2); scalars
        broadcast.  Replica r sums over its own images in the solver, the drift, the dense Brownian root and the probes, and its pair
        forces use its own minimum image.  Replaces a shared cell (ensemble_set_periodic), as that replaces this"""
        args = cells_args("ensemble_set_cells", Lx, Ly, images)       # types and shapes, before the library is called
        R = self.ensemble_info()[0]
        if R:                                                # (no ensemble: the library's refusal, behind its argument checks)
            args = cells_args("ensemble_set_cells", Lx, Ly, images, R)
        Lx, Ly, n = args
        nx, ny = np_contig(n[:, 0]), np_contig(n[:, 1])
        self._chk(self.L.rbl_ensemble_set_cells(self.h, Lx.size, Lx.ctypes.data, Ly.ctypes.data, nx.ctypes.data, ny.ctypes.data,
                                                int(bool(on))))

    def ensemble_cells(self):
        """{on, per_replica, Lx (R,), Ly (R,), images (R, 2)} of the ensemble's cell, shared (R equal rows) or per replica"""
        import numpy as np
        R = self.ensemble_info()[0]
        Lx, Ly = np.zeros(R), np.zeros(R)
        nx, ny = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        on, per = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_ensemble_get_cells(self.h, Lx.ctypes.data, Ly.ctypes.data, nx.ctypes.data, ny.ctypes.data, C.byref(on),
                                                C.byref(per)))
        return dict(on=bool(on.value), per_replica=bool(per.value), Lx=Lx, Ly=Ly, images=np.stack([nx, ny], axis=1))

    def set_bond_table(self, U, dU, r_min, r_cut, on=True):
        """the potential T(d) of the kind-1 bonds from its values U and derivatives dU = dU/dd on the uniform grid r_min .. r_cut
        (see `tabulate`): cubic Hermite inside, continued along its tangent at BOTH ends (a bond never breaks).  U = dU = None with
        on=False only switches the stored table off."""
        if U is None and dU is None and not on:
            return self._chk(self.L.rbl_set_bond_table(self.h, None, None, 0, 0.0, 0.0, 0))
        U, dU = table_arrays("set_bond_table", U, dU)
        self._chk(self.L.rbl_set_bond_table(self.h, U.ctypes.data, dU.ctypes.data, U.size, float(r_min), float(r_cut), int(bool(on))))

    def bond_table(self):
        return self._get_table(self.L.rbl_get_bond_table)

    def blob_anchor(self, k):
        """body-frame position of blob k with the structure's mean removed: the anchor of a bond that ends on that blob"""
        return blob_anchor(self._cfg, k)

    def bond_state(self):
        """-> (length, tension dU/dd, energy) of every bond at the context's configuration, (n_bonds,) each"""
        import numpy as np
        n = C.c_int(0)
        self._chk(self.L.rbl_get_bonds(self.h, C.byref(n), None, None, None, None, None, None))
        out = np.zeros((3, max(n.value, 1)))
        self._chk(self.L.rbl_bond_state(self.h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return out[0, :n.value], out[1, :n.value], out[2, :n.value]

    def ensemble_bond_state(self):
        """-> (length, tension, energy) of every bond of every replica, (R, n_bonds) each"""
        import numpy as np
        n = C.c_int(0)
        self._chk(self.L.rbl_get_bonds(self.h, C.byref(n), None, None, None, None, None, None))
        R = self.ensemble_info()[0]
        out = np.zeros((3, max(R * n.value, 1)))
        self._chk(self.L.rbl_ensemble_bond_state(self.h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return tuple(out[q, :R * n.value].reshape(R, n.value) for q in range(3))

    def interaction_forces_dev(self, d_f_blob, d_FT_body, energy=False):
        """PHYSICAL forces at the current configuration into device buffers (addresses or None); energy=True also returns the
        total potential energy (synchronises the stream)"""
        E = C.c_double(0.0)
        self._chk(self.L.rbl_interaction_forces_dev(self.h, d_f_blob, d_FT_body, C.byref(E) if energy else None))
        return E.value if energy else None

    def interaction_forces(self):
        """-> (f_blob (N, 3), FT_body (6 N_bod,)): PHYSICAL blob forces and body force / torque about the centre (U = +N FT)"""
        import numpy as np
        nb, nblb = self._sizes()
        f = np.zeros(3 * nb * nblb); FT = np.zeros(6 * nb)
        self._chk(self.L.rbl_interaction_forces(self.h, f.ctypes.data, FT.ctypes.data, None))
        return f.reshape(-1, 3), FT

    def interaction_energy(self):
        E = C.c_double(0.0)
        self._chk(self.L.rbl_interaction_forces(self.h, None, None, C.byref(E)))
        return E.value

    def interaction_stats(self):
        """(candidate body pairs, ordered blob pairs inside r_cut) of the last evaluation"""
        bp, pp = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.rbl_interaction_stats(self.h, C.byref(bp), C.byref(pp)))
        return bp.value, pp.value

    # -- imposed flow, active slip, first moments (include/rbl.h section 8) --------------
    def set_background_flow(self, u0=None, G=None, on=True):
        """u_inf(r) = u0 + G r, G[i, j] = d u_i / d x_j (None: zeros); the whole-step entry points and the krylov.py steppers add
        -u_inf at the blobs of q^n to their slip.  on=False switches the flow off."""
        import numpy as np
        u0 = np.zeros(3) if u0 is None else np.asarray(u0, dtype=np.float64)
        G = np.zeros((3, 3)) if G is None else np.asarray(G, dtype=np.float64)
        if u0.shape != (3,) or G.shape != (3, 3):
            raise ValueError("set_background_flow: u0 must have shape (3,) and G (3, 3); got %s and %s" % (u0.shape, G.shape))
        u0, G = np.ascontiguousarray(u0), np.ascontiguousarray(G)
        self._chk(self.L.rbl_set_background_flow(self.h, u0.ctypes.data, G.ctypes.data, int(bool(on))))

    def set_body_slip(self, slip_body, scale=None, on=True):
        """slip_body: the body-frame pattern, 3 N_blb numbers; scale: a factor per body (None: 1), one per body of the context's
        configuration or of an ensemble's replica"""
        import numpy as np
        sb = np.ascontiguousarray(np.asarray(slip_body, dtype=np.float64).reshape(-1))
        if sb.size != 3 * self._sizes()[1]:
            raise ValueError("set_body_slip: slip_body must have 3 N_blb = %d entries; got shape %s" % (3 * self._sizes()[1], np.shape(slip_body)))
        sc = None if scale is None else np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        self._chk(self.L.rbl_set_body_slip(self.h, sb.ctypes.data, None if sc is None else sc.ctypes.data, 0 if sc is None else sc.size,
                                           int(bool(on))))

    def flow_model(self):
        """{u0 (3,), G (3, 3), flow_on, body_slip_on}"""
        import numpy as np
        v, f, b = (C.c_double * 12)(), C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_flow_model(self.h, v, C.byref(f), C.byref(b)))
        return {"u0": np.array(v[:3]), "G": np.array(v[3:]).reshape(3, 3), "flow_on": bool(f.value), "body_slip_on": bool(b.value)}

    def flow_model_on(self):
        f, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_flow_model(self.h, None, C.byref(f), C.byref(b)))
        return bool(f.value or b.value)

    def flow_slip_dev(self, d_out):
        """the model's term at the current configuration into a device buffer of 3 N_blobs doubles (enqueued)"""
        self._chk(self.L.rbl_flow_slip_dev(self.h, d_out))

    def flow_slip(self):
        import numpy as np
        nb, nblb = self._sizes()
        out = np.zeros(3 * nb * nblb)
        self._chk(self.L.rbl_flow_slip(self.h, out.ctypes.data))
        return out

    def first_moments_dev(self, d_lambda, d_D):
        """D_b = sum (r_i - X_b) lambda_i^T per body: device buffers of 3 N_blobs and 9 N_bod doubles (enqueued)"""
        self._chk(self.L.rbl_first_moments_dev(self.h, d_lambda, d_D))

    def first_moments(self, lam):
        import numpy as np
        nb, nblb = self._sizes()
        lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64).reshape(-1))
        if lam.size != 3 * nb * nblb:
            raise ValueError("first_moments: lam must have 3 N_blobs = %d entries; got %d" % (3 * nb * nblb, lam.size))
        D = np.zeros((nb, 3, 3))
        self._chk(self.L.rbl_first_moments(self.h, lam.ctypes.data, D.ctypes.data))
        return D

    def record_moments(self, on=True):
        self.set_option("record_moments", int(bool(on)))

    def step_moments(self):
        import numpy as np
        D = np.zeros((self._sizes()[0], 3, 3))
        self._chk(self.L.rbl_step_moments(self.h, D.ctypes.data))
        return D

    def ensemble_flow_slip(self):
        """-> (R, n3): the model's term at every replica's configuration"""
        import numpy as np
        R, nb = self.ensemble_info()
        out = np.zeros((R, 3 * nb * self._sizes()[1]))
        self._chk(self.L.rbl_ensemble_flow_slip(self.h, out.ctypes.data))
        return out

    def ensemble_step_moments(self):
        """-> (R, N_bod, 3, 3): first moments recorded by the last ensemble step"""
        import numpy as np
        R, nb = self.ensemble_info()
        D = np.zeros((R, nb, 3, 3))
        self._chk(self.L.rbl_ensemble_step_moments(self.h, D.ctypes.data))
        return D

    # -- ensembles of independent replicas (include/rbl.h section 5) ---------------------
    def ensemble_set_config(self, X, Q):
        """X (R, N_bod, 3), Q (R, N_bod, 4): R independent replicas of the context's structure"""
        import numpy as np
        X = np.ascontiguousarray(X, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        self._chk(self.L.rbl_ensemble_set_config(self.h, X.shape[0], X.shape[1], X.ctypes.data, Q.ctypes.data))

    def ensemble_info(self):
        """(R, N_bod) of the ensemble, (0, 0) when none is set"""
        r, nb = C.c_int(0), C.c_int(0)
        self.L.rbl_ensemble_info(self.h, C.byref(r), C.byref(nb))
        return r.value, nb.value

    def ensemble_get_config(self):
        """-> X (R, N_bod, 3), Q (R, N_bod, 4)"""
        import numpy as np
        R, nb = self.ensemble_info()
        X = np.zeros((R, nb, 3)); Q = np.zeros((R, nb, 4))
        self._chk(self.L.rbl_ensemble_get_config(self.h, X.ctypes.data, Q.ctypes.data))
        return X, Q

    def ensemble_config_dev(self):
        """device addresses of the resident X and Q (valid until the next ensemble call)"""
        x, q = C.c_void_p(), C.c_void_p()
        self._chk(self.L.rbl_ensemble_config_dev(self.h, C.byref(x), C.byref(q)))
        return x.value, q.value

    def _ens_vec(self, v, per, what):
        import numpy as np
        R = self.ensemble_info()[0]
        v = np.asarray(v, dtype=np.float64)
        if v.size == per:
            v = np.broadcast_to(v.reshape(1, per), (R, per))
        if v.size != R * per:
            raise ValueError("%s must have %d entries per replica (shape (%d,) or (%d, %d)); got shape %s" % (what, per, per, R, per, v.shape))
        return np.ascontiguousarray(v.reshape(R, per))

    def ensemble_step_deterministic(self, F_body, max_iter=50, rtol=None, slip=None):
        """one deterministic step of every replica -> (iterations[R], residual estimates[R]); F_body (6 N_bod,) or (R, 6 N_bod)"""
        import numpy as np
        R, nb = self.ensemble_info()
        F = self._ens_vec(F_body, 6 * nb, "F_body")
        sl = None if slip is None else self._ens_vec(slip, 3 * nb * self._sizes()[1], "slip")
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(self.L.rbl_ensemble_step_deterministic(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data, int(max_iter),
                                                         float(rtol or 0.0), it.ctypes.data, res.ctypes.data))
        return it, res

    @staticmethod
    def _ens_noise(W, R, n3):
        """W (R, 3 n3) as a contiguous array, or None"""
        import numpy as np
        if W is None:
            return None
        Wh = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
        if Wh.size != R * 3 * n3:
            raise ValueError("W must have shape (%d, %d); got %s" % (R, 3 * n3, Wh.shape))
        return Wh

    def ensemble_step_brownian(self, F_body, W=None, seed=0, split_rand=True, delta=1.0e-4, max_iter=50, rtol=1e-8, slip=None):
        """one stochastic midpoint step of every replica (dense Cholesky root) -> (iterations[R], residual estimates[R]);
        W: (R, 3 n3) standard normals [W1 | W2 | W_rfd] per replica, or None to draw them from `seed`"""
        import numpy as np
        R, nb = self.ensemble_info()
        n3 = 3 * nb * self._sizes()[1]
        F = self._ens_vec(F_body, 6 * nb, "F_body")
        sl = None if slip is None else self._ens_vec(slip, n3, "slip")
        Wh = self._ens_noise(W, R, n3)
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(self.L.rbl_ensemble_step_brownian(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                                    None if Wh is None else Wh.ctypes.data, int(seed), int(bool(split_rand)),
                                                    float(delta), int(max_iter), float(rtol or 0.0), it.ctypes.data, res.ctypes.data))
        return it, res

    def ensemble_interaction_forces(self):
        """-> (FT (R, 6 N_bod) in the reference convention -K^T f_phys, energy (R,))"""
        import numpy as np
        R, nb = self.ensemble_info()
        FT, E = np.zeros((R, 6 * nb)), np.zeros(R)
        self._chk(self.L.rbl_ensemble_interaction_forces(self.h, FT.ctypes.data, E.ctypes.data))
        return FT, E

    def ensemble_mc(self, n_sweeps, step_x, step_theta, seed=0, kBT=None, frozen=None, stride=0, trace=0, sweep_start=0, replica_base=0):
        """n_sweeps Metropolis sweeps of every replica on the force model (include/rbl.h section 5, rbl_ensemble_mc) -> McResult;
        the result is the ensemble's configuration.  kBT: None (the context's), one value or (R,); frozen: None, (N_bod,) or
        (R, N_bod), bodies that are never tried.  Shape and value errors raise ValueError before the library is called"""
        import numpy as np
        R, nb = self.ensemble_info()
        n_sweeps, kBT, frozen, stride, trace, sweep_start, replica_base = mc_args(
            "ensemble_mc", R, nb, n_sweeps, step_x, step_theta, kBT, frozen, stride, trace, sweep_start, replica_base)
        o, out = McOpts(), McOut()
        o.size, out.size = C.sizeof(McOpts), C.sizeof(McOut)
        o.n_sweeps, o.sweep_start, o.seed, o.step_x, o.step_theta = n_sweeps, sweep_start, int(seed), float(step_x), float(step_theta)
        o.replica_base, o.stride, o.n_trace = replica_base, stride, trace
        o.kBT_sets, o.kBT = (0, None) if kBT is None else (kBT.size, kBT.ctypes.data)
        o.frozen_sets, o.frozen = (0, None) if frozen is None else (frozen.shape[0], frozen.ctypes.data)
        tried, acc, wr = (np.zeros(R, dtype=np.int64) for _ in range(3))
        E0, E1 = np.zeros(R), np.zeros(R)
        out.tried, out.accepted, out.wall_rejected = tried.ctypes.data, acc.ctypes.data, wr.ctypes.data
        out.energy_start, out.energy_end = E0.ctypes.data, E1.ctypes.data
        nf = n_sweeps // stride if stride > 0 else 0
        fX = fQ = fE = tr = None
        if nf:
            fX, fQ, fE = np.zeros((nf, R, nb, 3)), np.zeros((nf, R, nb, 4)), np.zeros((nf, R))
            out.frame_X, out.frame_Q, out.frame_E = fX.ctypes.data, fQ.ctypes.data, fE.ctypes.data
        if trace:
            tr = np.zeros((R, trace, 10))
            out.trace = tr.ctypes.data
        self._chk(self.L.rbl_ensemble_mc(self.h, C.byref(o), C.byref(out)))
        return McResult(tried, acc, wr, E0, E1, fX, fQ, fE, tr)

    def _ens_mixed_args(self, who, prescribed, body_in, slip, per=1):
        """mask (R, N_bod) uint8 -- (N_bod,) is broadcast over the replicas --, body_in (R, 6 N_bod), slip (R, n3) or None.
        per=6: a mask per velocity component, (R, 6 N_bod) from (N_bod, 6) or (R, N_bod, 6)"""
        import numpy as np
        R, nb = self.ensemble_info()
        m = np.asarray(prescribed)
        if per == 6:
            if m.shape == (nb, 6):
                m = np.broadcast_to(m.reshape(1, nb, 6), (R, nb, 6))
            if m.shape != (R, nb, 6):
                raise ValueError("%s: prescribed6 must have shape (%d, 6) or (%d, %d, 6); got %s" % (who, nb, R, nb, m.shape))
            m = np.ascontiguousarray(m.reshape(R, 6 * nb), dtype=np.uint8)
        else:
            if m.size == nb:
                m = np.broadcast_to(m.reshape(1, nb), (R, nb))
            if m.size != R * nb:
                raise ValueError("%s: prescribed must have shape (%d,) or (%d, %d); got %s" % (who, nb, R, nb, m.shape))
            m = np.ascontiguousarray(m.reshape(R, nb), dtype=np.uint8)
        bi = self._ens_vec(body_in, 6 * nb, "body_in")
        sl = None if slip is None else self._ens_vec(slip, 3 * nb * self._sizes()[1], "slip")
        return R, nb, m, bi, sl

    def _ens_solve_mixed(self, who, per, prescribed, body_in, max_iter, rtol, slip):
        import numpy as np
        R, nb, m, bi, sl = self._ens_mixed_args(who, prescribed, body_in, slip, per=per)
        n3 = 3 * nb * self._sizes()[1]
        lam, U, F = np.zeros((R, n3)), np.zeros((R, 6 * nb)), np.zeros((R, 6 * nb))
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, None if sl is None else sl.ctypes.data,
                                                int(max_iter), float(rtol or 0.0), lam.ctypes.data, U.ctypes.data, F.ctypes.data,
                                                it.ctypes.data, res.ctypes.data))
        return lam, U, F, it, res

    def _ens_step_mixed(self, who, per, prescribed, body_in, max_iter, rtol, slip):
        import numpy as np
        R, nb, m, bi, sl = self._ens_mixed_args(who, prescribed, body_in, slip, per=per)
        F = np.zeros((R, 6 * nb))
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, None if sl is None else sl.ctypes.data,
                                                int(max_iter), float(rtol or 0.0), F.ctypes.data, it.ctypes.data, res.ctypes.data))
        return F, it, res

    def _ens_step_brownian_mixed(self, who, per, prescribed, body_in, W, seed, split_rand, delta, max_iter, rtol, slip):
        import numpy as np
        R, nb, m, bi, sl = self._ens_mixed_args(who, prescribed, body_in, slip, per=per)
        if per == 6:
            check_brownian_mask6(who, m, nb, R)
        Wh = self._ens_noise(W, R, 3 * nb * self._sizes()[1])
        F = np.zeros((R, 6 * nb))
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, None if sl is None else sl.ctypes.data,
                                                None if Wh is None else Wh.ctypes.data, int(seed), int(bool(split_rand)), float(delta),
                                                int(max_iter), float(rtol or 0.0), F.ctypes.data, it.ctypes.data, res.ctypes.data))
        return F, it, res

    def ensemble_solve_mixed(self, prescribed, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        """solve_mixed at every replica's configuration (nothing moves) -> (lambda (R, n3), U (R, 6 N_bod), F (R, 6 N_bod),
        iterations[R], residual estimates[R]); prescribed: 0/1 per body, (N_bod,) or (R, N_bod)"""
        return self._ens_solve_mixed("ensemble_solve_mixed", 1, prescribed, body_in, max_iter, rtol, slip)

    def ensemble_step_mixed(self, prescribed, body_in, max_iter=50, rtol=1.0e-8, slip=None):
        """one deterministic step of every replica with prescribed bodies -> (F (R, 6 N_bod), iterations[R], residual estimates[R])"""
        return self._ens_step_mixed("ensemble_step_mixed", 1, prescribed, body_in, max_iter, rtol, slip)

    def ensemble_solve_mixed_dof(self, prescribed6, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        """solve_mixed_dof at every replica's configuration (nothing moves) -> (lambda (R, n3), U (R, 6 N_bod), F (R, 6 N_bod),
        iterations[R], residual estimates[R]); prescribed6: 0/1 per velocity component, (N_bod, 6) or (R, N_bod, 6)"""
        return self._ens_solve_mixed("ensemble_solve_mixed_dof", 6, prescribed6, body_in, max_iter, rtol, slip)

    def ensemble_step_mixed_dof(self, prescribed6, body_in, max_iter=50, rtol=1.0e-8, slip=None):
        """one deterministic step of every replica with prescribed velocity components -> (F (R, 6 N_bod), iterations[R],
        residual estimates[R])"""
        return self._ens_step_mixed("ensemble_step_mixed_dof", 6, prescribed6, body_in, max_iter, rtol, slip)

    def ensemble_step_brownian_mixed(self, prescribed, body_in, W=None, seed=0, split_rand=True, delta=1.0e-4, max_iter=50, rtol=1.0e-8,
                                     slip=None):
        """one stochastic midpoint step of every replica with prescribed bodies (dense Cholesky root) -> (F (R, 6 N_bod),
        iterations[R], residual estimates[R]); W as ensemble_step_brownian"""
        return self._ens_step_brownian_mixed("ensemble_step_brownian_mixed", 1, prescribed, body_in, W, seed, split_rand, delta, max_iter,
                                             rtol, slip)

    def ensemble_step_brownian_mixed_dof(self, prescribed6, body_in, W=None, seed=0, split_rand=True, delta=1.0e-4, max_iter=50,
                                         rtol=1.0e-8, slip=None):
        """one stochastic midpoint step of every replica with prescribed velocity components (dense Cholesky root); prescribed6:
        (N_bod, 6) or (R, N_bod, 6), every body's rotation entries all 0 or all 1 (check_brownian_mask6) -> (F (R, 6 N_bod),
        iterations[R], residual estimates[R]); W as ensemble_step_brownian"""
        return self._ens_step_brownian_mixed("ensemble_step_brownian_mixed_dof", 6, prescribed6, body_in, W, seed, split_rand, delta,
                                             max_iter, rtol, slip)

    # -- hard joints of an ensemble (include/rbl.h section 5; the set is set_joints' / set_joint_kinds') ------------------------
    def _ens_joint_count(self):
        n = C.c_int(0)
        self._chk(self.L.rbl_get_joints(self.h, C.byref(n), None, None, None))
        return n.value

    def _ens_joint_values(self, who, v):
        """(n_joints,) -- every replica alike -- or (R, n_joints) -> (contiguous array, sets)"""
        import numpy as np
        R, n = self.ensemble_info()[0], self._ens_joint_count()
        v = np.ascontiguousarray(v, dtype=np.float64)
        if not n or v.shape not in ((n,), (R, n)):
            raise ValueError("%s: one value per stored joint, shape (%d,) or (%d, %d); got %s" % (who, n, R, n, v.shape))
        return v, (1 if v.ndim == 1 else R)

    def ensemble_set_joint_rates(self, rates):
        """the motors' rates: (n_joints,) for every replica, or (R, n_joints); non-zero on lock joints only"""
        r, sets = self._ens_joint_values("ensemble_set_joint_rates", rates)
        self._chk(self.L.rbl_ensemble_set_joint_rates(self.h, r.ctypes.data, sets))

    def ensemble_set_joint_angles(self, theta):
        """the motors' angles: (n_joints,) for every replica, or (R, n_joints) -- a sweep of stroke phases, or a restart"""
        t, sets = self._ens_joint_values("ensemble_set_joint_angles", theta)
        self._chk(self.L.rbl_ensemble_set_joint_angles(self.h, t.ctypes.data, sets))

    def _ens_jointed_args(self, F_body, slip, jv, jname):
        R, nb = self.ensemble_info()
        nj = self._joints_active()
        F = self._ens_vec(F_body, 6 * nb, "F_body")
        sl = None if slip is None else self._ens_vec(slip, 3 * nb * self._sizes()[1], "slip")
        jr = None if jv is None or not nj else self._ens_vec(jv, 3 * nj, jname)
        return R, nb, nj, F, sl, jr

    def ensemble_solve_jointed(self, F_body, slip=None, joint_rhs=None, max_iter=100, rtol=1.0e-8):
        """solve_jointed at every replica's configuration (nothing moves) -> (lambda (R, n3), U (R, 6 N_bod), phi (R, 3 n_joints),
        iterations[R], residual estimates[R]).  Joints off or never set: the unjointed solve, phi empty"""
        import numpy as np
        R, nb, nj, F, sl, jr = self._ens_jointed_args(F_body, slip, joint_rhs, "joint_rhs")
        lam, U, phi = np.zeros((R, 3 * nb * self._sizes()[1])), np.zeros((R, 6 * nb)), np.zeros((R, 3 * nj))
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(self.L.rbl_ensemble_solve_jointed(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                                    None if jr is None else jr.ctypes.data, int(max_iter), float(rtol or 0.0),
                                                    lam.ctypes.data, U.ctypes.data, phi.ctypes.data if nj else None, it.ctypes.data,
                                                    res.ctypes.data))
        return lam, U, phi, it, res

    def ensemble_step_jointed(self, F_body, slip=None, joint_velocity=None, gamma=1.0, max_iter=50, rtol=1.0e-8):
        """one deterministic step of every replica with the joints: J U = -(gamma / dt) gap + joint_velocity -> (phi (R, 3 n_joints),
        iterations[R], residual estimates[R])"""
        import numpy as np
        R, nb, nj, F, sl, jr = self._ens_jointed_args(F_body, slip, joint_velocity, "joint_velocity")
        phi = np.zeros((R, 3 * nj))
        it, res = np.zeros(R, dtype=np.int32), np.zeros(R)
        self._chk(self.L.rbl_ensemble_step_jointed(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                                   None if jr is None else jr.ctypes.data, float(gamma), int(max_iter), float(rtol or 0.0),
                                                   phi.ctypes.data if nj else None, it.ctypes.data, res.ctypes.data))
        return phi, it, res

    def ensemble_joint_state(self, phi=True):
        """-> (gap (R, n_joints, 3) at the replicas' configurations, phi (R, n_joints, 3) of the last jointed ensemble solve or
        step, theta (R, n_joints)).  phi=False: before any jointed solve has succeeded with this set -> (gap, None, theta)"""
        import numpy as np
        R, n = self.ensemble_info()[0], self._ens_joint_count()
        gap, ph, theta = np.zeros((R, max(n, 1), 3)), np.zeros((R, max(n, 1), 3)), np.zeros((R, max(n, 1)))
        self._chk(self.L.rbl_ensemble_joint_state(self.h, gap.ctypes.data, ph.ctypes.data if phi else None, theta.ctypes.data))
        return gap[:, :n], (ph[:, :n] if phi else None), theta[:, :n]

    def ensemble_run(self, n_steps, F_body=None, prescribed=None, body_in=None, brownian=True, seed=0, stride=0, on_error=RUN_STOP,
                     check_every=RUN_CHECK_DEFAULT, slip=None, split_rand=True, delta=1.0e-4, max_iter=50, rtol=1.0e-8, per=1):
        """n_steps steps of every replica in one call (rbl_ensemble_run): the inputs are uploaded once, the verdict, the commit
        and the records are kept per replica on the device -> (RunResult, status): the result is filled for a stopped run too,
        whose status and message it carries; nothing is raised here for such a run (Ensemble.run does).  F_body (6 N_bod,) or
        (R, 6 N_bod) for free bodies, or prescribed (N_bod,) / (R, N_bod) with body_in -- per=6: a mask per velocity component,
        (N_bod, 6) / (R, N_bod, 6), deterministic runs only --; on_error: RUN_STOP or RUN_REJECT"""
        return self._ensemble_run(None, n_steps, F_body=F_body, prescribed=prescribed, body_in=body_in, brownian=brownian, seed=seed, stride=stride,
                                  on_error=on_error, check_every=check_every, slip=slip, split_rand=split_rand, delta=delta, max_iter=max_iter,
                                  rtol=rtol, per=per)

    def _ensemble_run(self, obs, n_steps, F_body=None, prescribed=None, body_in=None, brownian=True, seed=0, stride=0, on_error=RUN_STOP,
                      check_every=RUN_CHECK_DEFAULT, slip=None, split_rand=True, delta=1.0e-4, max_iter=50, rtol=1.0e-8, per=1, drive=None):
        """ensemble_run's arguments, checked and laid out for _run; obs (ensemble_run_observed) and drive (ensemble_run_driven) pass through"""
        import numpy as np
        R, nb = self.ensemble_info()
        if R == 0:
            self._chk(self.L.rbl_ensemble_get_config(self.h, None, None))       # the state error, as every ensemble call gives it
        if (F_body is None) == (prescribed is None and body_in is None):
            raise ValueError("ensemble_run: give either F_body or prescribed with body_in")
        if F_body is None and (prescribed is None or body_in is None):
            raise ValueError("ensemble_run: prescribed and body_in go together")
        n_steps, stride = int(n_steps), int(stride)
        if n_steps < 1 or stride < 0:
            raise ValueError("ensemble_run: need n_steps >= 1 and stride >= 0; got %d and %d" % (n_steps, stride))
        masked = F_body is None
        sl = None
        if masked:
            _, _, m, bi, sl = self._ens_mixed_args("ensemble_run", prescribed, body_in, slip, per=per)
        else:
            F = self._ens_vec(F_body, 6 * nb, "F_body")
            sl = None if slip is None else self._ens_vec(slip, 3 * nb * self._sizes()[1], "slip")
        return self._run(masked, dict(n_steps=n_steps, brownian=int(bool(brownian)), split_rand=int(bool(split_rand)), max_iter=int(max_iter),
                                      stride=stride, on_error=int(on_error), check_every=int(check_every), seed=int(seed), delta=float(delta),
                                      rtol=float(rtol or 0.0), prescribed_per=int(per), F_body=None if masked else F,
                                      prescribed=m if masked else None, body_in=bi if masked else None, slip=sl), obs=obs, drive=drive)

    def _run(self, masked, opts, joints=None, obs=None, drive=None):
        """the one body of a run, and the one place a run enters the library.  opts: the fields of rbl_run_opts (arrays for the
        pointers); masked: prescribed bodies, so F_sum, F, F_mean.  The optional parts, each with its structs and its records on the
        result: joints (RunJointOpts, the arrays behind its pointers, the active joints' count), obs (ensemble_run_observed's
        (points, probe_body, moments)), drive (drive_opts' keywords); they choose the entry point.  -> (RunResult, status)"""
        import numpy as np
        R, nb = self.ensemble_info()
        o = RunOpts()
        o.size = C.sizeof(RunOpts)
        for k, v in opts.items():
            setattr(o, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        nf = o.n_steps // o.stride if o.stride > 0 else 0
        res = RunResult()
        res.accepted, res.rejected = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        res.first_flags, res.first_status = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.int32)
        res.iters_sum, res.resid_max = np.zeros(R, dtype=np.int64), np.zeros(R)
        res.F_sum = np.zeros((R, 6 * nb)) if masked else None
        res.X, res.Q = np.zeros((nf, R, nb, 3)), np.zeros((nf, R, nb, 4))
        res.accepted_at = np.zeros((nf, R), dtype=np.int32)
        res.F = np.zeros((nf, R, 6 * nb)) if masked else None
        res.F_mean = None
        out = RunOut()
        out.size = C.sizeof(RunOut)
        out.accepted, out.rejected = res.accepted.ctypes.data, res.rejected.ctypes.data
        out.first_flags, out.first_status = res.first_flags.ctypes.data, res.first_status.ctypes.data
        out.iters_sum, out.resid_max = res.iters_sum.ctypes.data, res.resid_max.ctypes.data
        out.F_sum = res.F_sum.ctypes.data if masked else None
        out.frame_X, out.frame_Q, out.frame_accepted_at = res.X.ctypes.data, res.Q.ctypes.data, res.accepted_at.ctypes.data
        out.frame_F = res.F.ctypes.data if masked else None
        out.stopped_at = out.stop_replica = -1       # a refused call leaves them so
        jo = jout = dd = dq = oo = oq = None
        if joints is not None:
            jo, keep, nj = joints
            res.theta, res.cycle_pos, res.phi_sum = np.zeros((R, nj)), np.zeros(R, dtype=np.int32), np.zeros((R, nj, 3))
            res.frame_theta, res.frame_phi, res.frame_gap = np.zeros((nf, R, nj)), np.zeros((nf, R, nj, 3)), np.zeros((nf, R, nj, 3))
            jout = RunJointOut()
            jout.size = C.sizeof(RunJointOut)
            jout.theta, jout.cycle_pos, jout.phi_sum = res.theta.ctypes.data, res.cycle_pos.ctypes.data, res.phi_sum.ctypes.data
            jout.frame_theta, jout.frame_phi, jout.frame_gap = res.frame_theta.ctypes.data, res.frame_phi.ctypes.data, res.frame_gap.ctypes.data
        if drive is not None:
            dd, keep = drive_opts("ensemble_run_driven", 6 * nb, **drive)
            dq = RunDriveOut()
            dq.size = C.sizeof(RunDriveOut)
            res.cycle_pos, res.t_end = np.zeros(R, dtype=np.int32), np.zeros(R)
            dq.cycle_pos, dq.t_end = res.cycle_pos.ctypes.data, res.t_end.ctypes.data
            if dd.lockin:
                res.X_c, res.X_s, res.norm = np.zeros((R, nb, 3)), np.zeros((R, nb, 3)), np.zeros((R, 5))
                res.U_c, res.U_s = np.zeros((R, 6 * nb)), np.zeros((R, 6 * nb))
                dq.X_c, dq.X_s, dq.norm = res.X_c.ctypes.data, res.X_s.ctypes.data, res.norm.ctypes.data
                dq.U_c, dq.U_s = res.U_c.ctypes.data, res.U_s.ctypes.data
                if o.prescribed:
                    res.F_c, res.F_s = np.zeros((R, 6 * nb)), np.zeros((R, 6 * nb))
                    dq.F_c, dq.F_s = res.F_c.ctypes.data, res.F_s.ctypes.data
        if obs is not None:
            pts, body, moments = obs
            oo, oq = RunObsOpts(), RunObsOut()
            oo.size, oq.size = C.sizeof(RunObsOpts), C.sizeof(RunObsOut)
            oo.probe_body, oo.moments = int(body), int(bool(moments))
            if pts is not None:
                P = pts.shape[-2]
                oo.n_probes, oo.point_sets, oo.points = P, (1 if pts.ndim == 2 else pts.shape[0]), pts.ctypes.data
                if P:
                    res.u_sum, res.frame_u = np.zeros((R, P, 3)), np.zeros((nf, R, P, 3))
                    oq.u_sum, oq.frame_u = res.u_sum.ctypes.data, res.frame_u.ctypes.data
            if moments:
                res.D_sum, res.frame_D = np.zeros((R, nb, 3, 3)), np.zeros((nf, R, nb, 3, 3))
                oq.D_sum, oq.frame_D = res.D_sum.ctypes.data, res.frame_D.ctypes.data

        def ref(s):
            return None if s is None else C.byref(s)
        if dd is not None:
            rc = self.L.rbl_ensemble_run_driven(self.h, C.byref(o), C.byref(dd), ref(oo), C.byref(out), C.byref(dq), ref(oq))
        elif oo is not None:
            rc = self.L.rbl_ensemble_run_observed(self.h, C.byref(o), ref(jo), C.byref(oo), C.byref(out), ref(jout), C.byref(oq))
        elif jo is not None:
            rc = self.L.rbl_ensemble_run_jointed(self.h, C.byref(o), C.byref(jo), C.byref(out), C.byref(jout))
        else:
            rc = self.L.rbl_ensemble_run(self.h, C.byref(o), C.byref(out))
        res.steps_done, res.stopped_at, res.stop_replica = out.steps_done, out.stopped_at, out.stop_replica
        res.status, res.error = rc, None
        if rc != 0:
            res.error = "%s [rbl status %d]" % (self.L.rbl_last_error(self.h).decode(), rc)
            if out.stopped_at < 0:                    # refused, or failed outside the steps: there is no result
                raise RblError(res.error)
        with np.errstate(divide="ignore", invalid="ignore"):
            if masked:
                res.F_mean = np.where(res.accepted[:, None] > 0, res.F_sum / res.accepted[:, None], np.nan)
            if joints is not None:
                res.phi_mean = np.where(res.accepted[:, None, None] > 0, res.phi_sum / res.accepted[:, None, None], np.nan)
                res.phi, res.gap = res.frame_phi, res.frame_gap
        return res, rc

    def ensemble_run_driven(self, n_steps, cos=None, sin=None, omega=None, t0=None, phase_steps=None, phase_in=None, cycle_start=None,
                            lockin=False, probes=None, probe_body=None, moments=False, **run_args):
        """a run whose body input follows a drive (rbl_ensemble_run_driven) -> (RunResult, status) as ensemble_run returns them:
        run_args are ensemble_run's keywords, F_body or body_in standing for the constant part A0.  Before every step replica r
        steps with ((A0 + P[phase]) + cos * cs) + sin * sn, cs, sn = cos, sin(omega_r t_r), t_r = t0_r + dt * accepted_r; the
        arrays as drive_opts lays them out.  lockin: the sums X_c ... norm on the result; cycle_pos and t_end always.  probes,
        probe_body, moments: ensemble_run_observed's.  Nothing given: the underlying run"""
        drive = dict(cos=cos, sin=sin, omega=omega, t0=t0, phase_steps=phase_steps, phase_in=phase_in, cycle_start=cycle_start, lockin=lockin)
        if probes is not None or moments:
            return self.ensemble_run_observed(n_steps, probes=probes, probe_body=probe_body, moments=moments, drive=drive, **run_args)
        return self._ensemble_run(None, n_steps, drive=drive, **run_args)

    def ensemble_drive_eval(self, base, accepted=None, cycle_pos=None, **drive):
        """the body input a driven run's step would take (rbl_ensemble_drive_eval: the run's own kernel, one launch) -> (input
        (R, 6 N_bod), cs_sn (R, 2)).  base (6 N_bod,) or (R, 6 N_bod): A0; accepted (R,) the replicas' step counters (None: 0);
        cycle_pos (R,) their cycle positions (None: cycle_start); drive: drive_opts' keywords"""
        import numpy as np
        R, nb = self.ensemble_info()
        if R == 0:
            self._chk(self.L.rbl_ensemble_get_config(self.h, None, None))       # the state error, as every ensemble call gives it
        A0 = self._ens_vec(base, 6 * nb, "base")
        dd, keep = drive_opts("ensemble_drive_eval", 6 * nb, **drive)
        ints = []
        for name, a in (("accepted", accepted), ("cycle_pos", cycle_pos)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.int32)
                if a.shape != (R,):
                    raise ValueError("ensemble_drive_eval: %s must have shape (%d,); got %s" % (name, R, a.shape))
            ints.append(a)
        out, cs_sn = np.zeros((R, 6 * nb)), np.zeros((R, 2))
        self._chk(self.L.rbl_ensemble_drive_eval(self.h, C.byref(dd), A0.ctypes.data, None if ints[0] is None else ints[0].ctypes.data,
                                                 None if ints[1] is None else ints[1].ctypes.data, out.ctypes.data, cs_sn.ctypes.data))
        return out, cs_sn

    def ensemble_run_observed(self, n_steps, probes=None, probe_body=None, moments=False, jointed=False, **run_args):
        """a run with observers (rbl_ensemble_run_observed) -> (RunResult, status) as ensemble_run returns them: run_args are
        ensemble_run's keywords, or with jointed=True ensemble_run_jointed's.  probes: (P, 3), one set of points for every replica,
        or (R, P, 3); probe_body=None: lab points, b: offsets fixed in body b that follow it.  The result gains u_sum, u_mean,
        frame_u and, with moments, D_sum, D_mean, stresslet_mean, frame_D (RunResult).  Nothing asked for: the underlying run"""
        import numpy as np
        pts = None
        if probes is not None:
            pts = np.ascontiguousarray(probes, dtype=np.float64)
            if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
                raise ValueError("ensemble_run_observed: probes must have shape (P, 3) or (R, P, 3); got %s" % (pts.shape,))
        obs = (pts, -1 if probe_body is None else int(probe_body), bool(moments))
        run = self._ensemble_run_jointed if jointed else self._ensemble_run
        res, rc = run(obs, n_steps, **run_args)
        acc = res.accepted.astype(np.float64)
        div = np.where(acc > 0, acc, 1.0)                  # a replica that accepted nothing has zero sums: its means are zeros
        if res.u_sum is not None:
            res.u_mean = res.u_sum / div[:, None, None]
        if res.D_sum is not None:
            res.D_mean = res.D_sum / div[:, None, None, None]
            sym = 0.5 * (res.D_mean + np.swapaxes(res.D_mean, -1, -2))
            res.stresslet_mean = sym - np.trace(sym, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
        return res, rc

    def ensemble_velocity_field(self, points, lam, body=None):
        """the flow every replica's blob forces lam (R, 3 N) drive at points (P, 3) -- one set for every replica -- or (R, P, 3), at
        the ensemble's current configuration and in its cell (rbl_ensemble_velocity_field) -> (R, P, 3).  body=b: the points are
        offsets fixed in body b of each replica"""
        import numpy as np
        R, nb = self.ensemble_info()
        if R == 0:
            self._chk(self.L.rbl_ensemble_get_config(self.h, None, None))       # the state error, as every ensemble call gives it
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
            raise ValueError("ensemble_velocity_field: points must have shape (P, 3) or (R, P, 3); got %s" % (pts.shape,))
        n3 = 3 * nb * self._sizes()[1]
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if lam.size != R * n3:
            raise ValueError("ensemble_velocity_field: lam must hold R * 3 N = %d values; got shape %s" % (R * n3, lam.shape))
        P = pts.shape[-2]
        u = np.empty((R, P, 3))
        self._chk(self.L.rbl_ensemble_velocity_field(self.h, pts.ctypes.data, P, 1 if pts.ndim == 2 else pts.shape[0],
                                                     -1 if body is None else int(body), lam.ctypes.data, u.ctypes.data))
        return u

    def ensemble_velocity_field_dev(self, d_points, n_points, point_sets, d_lam, d_out, body=None):
        """the same on device addresses; returns once the replicas' error words have been read"""
        self._chk(self.L.rbl_ensemble_velocity_field_dev(self.h, d_points, n_points, point_sets, -1 if body is None else int(body), d_lam, d_out))

    def ensemble_probe_info(self, n_points):
        """(points per lane NI, waves per workgroup, point tiles) of the probe kernel's launch for n_points points per replica"""
        ni, wv, tl = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self.L.rbl_ensemble_probe_info(self.h, n_points, C.byref(ni), C.byref(wv), C.byref(tl)))
        return ni.value, wv.value, tl.value

    def ensemble_run_jointed(self, n_steps, F_body, slip=None, joint_velocity=None, gamma=1.0, phase_steps=None, phase_rates=None,
                             cycle_start=None, stride=0, on_error=RUN_STOP, check_every=RUN_CHECK_DEFAULT, max_iter=50, rtol=1.0e-8,
                             brownian=False, prescribed=None, per=0):
        """n_steps jointed steps of every replica in one call (rbl_ensemble_run_jointed) -> (RunResult, status), as ensemble_run
        returns them, with the joints' records (theta, cycle_pos, phi_sum, phi_mean, frame_theta / frame_phi / frame_gap).
        The motor schedule: phase_steps (n_phases,) integers and phase_rates (n_phases, n_joints) or (n_phases, R, n_joints), both
        None for the stored rates; cycle_start None, an integer or (R,) integers.  brownian, prescribed and per exist so that the
        library's refusals can be reached; nothing else is offered through them"""
        return self._ensemble_run_jointed(None, n_steps, F_body, slip=slip, joint_velocity=joint_velocity, gamma=gamma, phase_steps=phase_steps,
                                          phase_rates=phase_rates, cycle_start=cycle_start, stride=stride, on_error=on_error,
                                          check_every=check_every, max_iter=max_iter, rtol=rtol, brownian=brownian, prescribed=prescribed, per=per)

    def _ensemble_run_jointed(self, obs, n_steps, F_body, slip=None, joint_velocity=None, gamma=1.0, phase_steps=None, phase_rates=None,
                              cycle_start=None, stride=0, on_error=RUN_STOP, check_every=RUN_CHECK_DEFAULT, max_iter=50, rtol=1.0e-8,
                              brownian=False, prescribed=None, per=0):
        """ensemble_run_jointed's arguments, checked and laid out for _run; obs (ensemble_run_observed) passes through"""
        import numpy as np
        R, nb = self.ensemble_info()
        if R == 0:
            self._chk(self.L.rbl_ensemble_get_config(self.h, None, None))       # the state error, as every ensemble call gives it
        n_steps, stride = int(n_steps), int(stride)
        if n_steps < 1 or stride < 0:
            raise ValueError("ensemble_run_jointed: need n_steps >= 1 and stride >= 0; got %d and %d" % (n_steps, stride))
        if (phase_steps is None) != (phase_rates is None):
            raise ValueError("ensemble_run_jointed: phase_steps and phase_rates go together")
        _, _, nj, F, sl, jv = self._ens_jointed_args(F_body, slip, joint_velocity, "joint_velocity")
        nst = self._ens_joint_count()                     # the stored joints, on or off: what a schedule is measured against
        jo = RunJointOpts()
        jo.size, jo.gamma = C.sizeof(RunJointOpts), float(gamma)
        jo.joint_velocity = None if jv is None else jv.ctypes.data
        ps = pr = cs = None
        if phase_steps is not None:
            ps = np.ascontiguousarray(phase_steps, dtype=np.int32).reshape(-1)
            pr = np.ascontiguousarray(phase_rates, dtype=np.float64)
            if pr.shape not in ((ps.size, nst), (ps.size, R, nst)):
                raise ValueError("ensemble_run_jointed: phase_rates must have shape (%d, %d) or (%d, %d, %d); got %s"
                                 % (ps.size, nst, ps.size, R, nst, pr.shape))
            jo.n_phases, jo.rate_sets = ps.size, (1 if pr.ndim == 2 else R)
            jo.phase_steps, jo.phase_rates = ps.ctypes.data, pr.ctypes.data
        if cycle_start is not None:
            cs = np.ascontiguousarray(cycle_start, dtype=np.int32).reshape(-1)
            if cs.size not in (1, R):
                raise ValueError("ensemble_run_jointed: cycle_start must be one integer or %d; got %d" % (R, cs.size))
            jo.start_sets, jo.cycle_start = cs.size, cs.ctypes.data
        pm = None if prescribed is None else np.ascontiguousarray(prescribed, dtype=np.uint8)
        return self._run(False, dict(n_steps=n_steps, brownian=int(bool(brownian)), max_iter=int(max_iter), stride=stride, on_error=int(on_error),
                                     check_every=int(check_every), rtol=float(rtol or 0.0), prescribed_per=int(per), F_body=F, slip=sl,
                                     prescribed=pm), joints=(jo, (jv, ps, pr, cs), nj), obs=obs)

    def _sizes(self):
        nb, nblb = C.c_int(0), C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), C.byref(nblb)))
        return nb.value, nblb.value

    def apply_M(self, dF, dr, n_blobs, row_begin, row_end, dout):
        """dF, dr, dout: integer device addresses (tensor.data_ptr())."""
        self._chk(self.L.rbl_apply_M_dev(self.h, dF, dr, n_blobs, row_begin, row_end, dout))

    # -- device-resident rigid-body operators (own configuration) ----------------------
    def positions_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.rbl_positions_dev(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def prepare(self):
        """uploads, workspace growth and PC build now -> later operator calls are launch-only"""
        self._chk(self.L.rbl_prepare_dev(self.h))

    def K_x_U(self, dU, dout):
        self._chk(self.L.rbl_K_x_U_dev(self.h, dU, dout))

    def KT_x_Lam(self, dlam, dout):
        self._chk(self.L.rbl_KT_x_Lam_dev(self.h, dlam, dout))

    def apply_PC(self, din, dout):
        self._chk(self.L.rbl_apply_PC_dev(self.h, din, dout))

    def apply_saddle(self, dx, dout):
        self._chk(self.L.rbl_apply_saddle_dev(self.h, dx, dout))

    def evolve(self, U_host):
        import numpy as np
        U = np.ascontiguousarray(U_host, dtype=np.float64).reshape(-1)
        self._chk(self.L.rbl_evolve_X_Q(self.h, U.ctypes.data))

    def block_solve(self, din, dout, mode, body_begin=0, body_end=-1):
        """per-body Cholesky factors L L^T = M_body: mode 0 (L L^T)^-1, 1 L^-1, 2 L^-T, 3 L x; full-length blob
        vectors, only the bodies [body_begin, body_end) are factored, read and written (default: all)"""
        self._chk(self.L.rbl_block_solve_range_dev(self.h, din, dout, mode, int(body_begin), int(body_end)))

    def set_block_refresh(self, every):
        """keep the per-body Cholesky factors for `every` configuration changes (1 = rebuild after each)"""
        self._chk(self.L.rbl_set_block_refresh(self.h, int(every)))

    def set_no_damp(self, on):
        self._chk(self.L.rbl_set_no_damp(self.h, int(bool(on))))

    def step_deterministic(self, F_body, max_iter=20, rtol=None, slip=None, warm_start=False):
        """one deterministic time step inside librbl (solve + evolve) -> (iterations, residual estimate);
        warm_start 0..3: cold / previous solution / linear / quadratic extrapolation of the last solutions"""
        import numpy as np
        F = np.ascontiguousarray(F_body, dtype=np.float64).reshape(-1)
        sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64).reshape(-1)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_step_deterministic(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data, int(max_iter),
                                                float(rtol or 0.0), int(warm_start), C.byref(it), C.byref(res)))
        return it.value, res.value

    def step_brownian(self, F_body, max_iter=20, rtol=None, slip=None, W=None, seed=0, method=2, split_rand=True,
                      delta=1.0e-4):
        """one stochastic midpoint step inside librbl -> (iterations, residual estimate)"""
        import numpy as np
        F = np.ascontiguousarray(F_body, dtype=np.float64).reshape(-1)
        sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64).reshape(-1)
        Wh = None if W is None else np.ascontiguousarray(W, dtype=np.float64).reshape(-1)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_step_brownian(self.h, F.ctypes.data, None if sl is None else sl.ctypes.data,
                                           None if Wh is None else Wh.ctypes.data, int(seed), mhalf_code(method), int(bool(split_rand)),
                                           float(delta), int(max_iter), float(rtol or 0.0), C.byref(it), C.byref(res)))
        return it.value, res.value

    def gmres_saddle(self, d_rhs, max_iter, rtol, d_x, use_x0=False):
        """native right-preconditioned GMRES on the saddle operator -> (iterations, residual estimate);
        use_x0: d_x holds an initial guess (warm start from the previous time step)"""
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_gmres_saddle_dev(self.h, d_rhs, int(max_iter), float(rtol or 0.0), d_x, int(bool(use_x0)),
                                              C.byref(it), C.byref(res)))
        return it.value, res.value

    def gmres_saddle_multi(self, d_rhs, nrhs, max_iter, rtol, d_x):
        """nrhs right-hand sides in lock step (device vectors, one after the other) -> (iterations[nrhs], residuals[nrhs])"""
        it, res = (C.c_int * nrhs)(), (C.c_double * nrhs)()
        self._chk(self.L.rbl_gmres_saddle_multi_dev(self.h, d_rhs, int(nrhs), int(max_iter), float(rtol or 0.0), d_x, it, res))
        return list(it), list(res)

    def update_X_Q(self, U_host, n_bodies):
        """configuration displaced by U (displacement units), not committed -> (X, Q)"""
        import numpy as np
        U = np.ascontiguousarray(U_host, dtype=np.float64).reshape(-1)
        X = np.zeros(3 * n_bodies); Q = np.zeros(4 * n_bodies)
        self._chk(self.L.rbl_update_X_Q(self.h, U.ctypes.data, X.ctypes.data, Q.ctypes.data))
        return X.reshape(-1, 3), Q.reshape(-1, 4)

    def Kinv_x_V(self, V_host, n_bodies):
        """K^-1 V (reference :406): V[3 N_blobs] host -> [6 N_bodies] host (O(N) host work)"""
        import numpy as np
        V = np.ascontiguousarray(V_host, dtype=np.float64).reshape(-1)
        out = np.zeros(6 * n_bodies)
        self._chk(self.L.rbl_Kinv_x_V(self.h, V.ctypes.data, out.ctypes.data))
        return out

    def RHS_and_Midpoint(self, dSlip, dForce, dW, seed, method, split_rand, delta, dRHS, n_bodies):
        """device-vector form of the reference's RHS_and_Midpoint -> (X_half, Q_half) on the host"""
        import numpy as np
        X = np.zeros(3 * n_bodies); Q = np.zeros(4 * n_bodies)
        self._chk(self.L.rbl_RHS_and_Midpoint_dev(self.h, dSlip, dForce, dW, seed, mhalf_code(method), int(split_rand), delta,
                                                  dRHS, X.ctypes.data, Q.ctypes.data))
        return X.reshape(-1, 3), Q.reshape(-1, 4)

    def get_config(self, n_bodies):
        import numpy as np
        X = np.zeros(3 * n_bodies); Q = np.zeros(4 * n_bodies)
        self._chk(self.L.rbl_get_config(self.h, X.ctypes.data, Q.ctypes.data))
        return X.reshape(-1, 3), Q.reshape(-1, 4)

    def apply_M_multi(self, dF, dr, n_blobs, nrhs, dout):
        """nrhs vectors, column-major (3 n_blobs) x nrhs; >= 4 go through the fp64-MFMA kernel."""
        self._chk(self.L.rbl_apply_M_multi_dev(self.h, dF, dr, n_blobs, nrhs, dout))

    def apply_M_sym(self, dF, dr, n_blobs, i_first, i_step, dout):
        """partial product over share i_first of i_step of the tile rows (sum over the shares = full U)."""
        self._chk(self.L.rbl_apply_M_sym_dev(self.h, dF, dr, n_blobs, i_first, i_step, dout))

    def apply_M_sym_multi(self, dF, dr, n_blobs, nrhs, i_first, i_step, dout):
        """the same for nrhs = 1 or 2 vectors ([nrhs][3 n_blobs]); two vectors share the pair coefficients"""
        self._chk(self.L.rbl_apply_M_sym_multi_dev(self.h, dF, dr, n_blobs, nrhs, i_first, i_step, dout))

    def apply_M_sym_info(self, n_blobs, i_step=1, nrhs=1):
        """(rows per lane NI, column tiles per work unit, slab workspace bytes) of the symmetric kernel launch"""
        ni, ch, wb = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self.L.rbl_apply_M_sym_info(self.h, n_blobs, i_step, nrhs, C.byref(ni), C.byref(ch), C.byref(wb)))
        return ni.value, ch.value, wb.value

    def apply_M_sym_units(self, n_blobs, n_cu=256, i_step=1, nrhs=1):
        """work units of the symmetric product of that size on a GPU of n_cu compute units under this context's options, in the
        order they are handed out (needs no device): (units, info, workspace bytes) with units an (n, 9) int64 array -- index, row
        group, chunk, first column tile, column tiles, row-sum (offset, length), column-sum (offset, length) in doubles -- and info a
        dict (include/rbl.h rbl_apply_M_sym_units)"""
        import numpy as np
        f = self.L.rbl_apply_M_sym_units
        f.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        n, wb, info = C.c_int64(0), C.c_int64(0), (C.c_int * 8)()
        self._chk(f(self.h, n_blobs, n_cu, i_step, nrhs, None, 0, C.byref(n), info, C.byref(wb)))
        units = np.zeros((n.value, 9), dtype=np.int64)
        self._chk(f(self.h, n_blobs, n_cu, i_step, nrhs, units.ctypes.data, n.value, C.byref(n), info, C.byref(wb)))
        keys = ("rows_per_lane", "waves", "chunk", "tail_chunk", "tail_chunks", "chunks", "work_queue", "live_only")
        return units, dict(zip(keys, list(info))), wb.value

    def apply_M_sym_kernel(self, n_blobs, wall, i_step=1, nrhs=1):
        """name of the kernel instantiation a symmetric product of that size launches under this context's options"""
        buf = C.create_string_buffer(64)
        self._chk(self.L.rbl_apply_M_sym_kernel(self.h, n_blobs, i_step, nrhs, 1 if wall else 0, buf, 64))
        return buf.value.decode()

    # -- fluid velocity at arbitrary points (include/rbl.h section 6) --------------------------------------------------------
    def velocity_field(self, points, lam, positions=None):
        """u at points (P, 3) or flat 3P from blob forces lam on blobs `positions` (None: the context's own blobs at its
        configuration); host arrays in, a flat (3P,) array out"""
        import numpy as np
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
        r = None if positions is None else np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        u = np.empty_like(pts)
        self._chk(self.L.rbl_velocity_field(self.h, pts.ctypes.data, pts.size // 3, lam.ctypes.data,
                                            None if r is None else r.ctypes.data, lam.size // 3, u.ctypes.data))
        return u

    def velocity_field_dev(self, d_points, n_points, d_lam, d_r, n_src, d_out):
        """the same on device addresses (d_r = None / 0: the context's own blobs); enqueued on the context's stream"""
        self._chk(self.L.rbl_velocity_field_dev(self.h, d_points, n_points, d_lam, d_r or None, n_src, d_out))

    def velocity_field_info(self, n_points, n_src):
        """(points per lane NI, source chunks, workspace bytes) of the product of that size on this context"""
        ni, ch, wb = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self.L.rbl_velocity_field_info(self.h, n_points, n_src, C.byref(ni), C.byref(ch), C.byref(wb)))
        return ni.value, ch.value, wb.value

    # -- prescribed kinematics (include/rbl.h section 7) ---------------------------------------------------------------------
    # The host-array methods: each whole-body / _dof pair is one body that takes `who`, the entry point's name without rbl_, and
    # `per`, the mask entries per body -- 1, or 6 for a mask per velocity component.
    def _mixed_host_args(self, who, per, prescribed, body_in, slip, W=None, brownian=False):
        """-> (mask, N_bod, N_blb, body_in, slip or None, W or None), flat and contiguous"""
        import numpy as np
        m, nb, nl = self._mixed_sizes(who, per, prescribed, brownian)
        bi = np.ascontiguousarray(body_in, dtype=np.float64).reshape(-1)
        sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64).reshape(-1)
        Wh = None if W is None else np.ascontiguousarray(W, dtype=np.float64).reshape(-1)
        if bi.size != 6 * nb or (sl is not None and sl.size != 3 * nb * nl) or (Wh is not None and Wh.size != 9 * nb * nl):
            raise ValueError(who + ": body_in (6 N_bod), slip (3 N_blobs) or W (9 N_blobs) has the wrong size")
        return m, nb, nl, bi, sl, Wh

    def _solve_mixed(self, who, per, prescribed, body_in, max_iter, rtol, slip):
        import numpy as np
        m, nb, nl, bi, sl, _ = self._mixed_host_args(who, per, prescribed, body_in, slip)
        lam, U, F = np.empty(3 * nb * nl), np.empty(6 * nb), np.empty(6 * nb)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, _ptr(sl), int(max_iter), float(rtol),
                                                lam.ctypes.data, U.ctypes.data, F.ctypes.data, C.byref(it), C.byref(res)))
        return lam, U, F, it.value, res.value

    def _step_mixed(self, who, per, prescribed, body_in, max_iter, rtol, slip):
        import numpy as np
        m, nb, _, bi, sl, _ = self._mixed_host_args(who, per, prescribed, body_in, slip)
        F = np.empty(6 * nb)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, _ptr(sl), int(max_iter), float(rtol),
                                                F.ctypes.data, C.byref(it), C.byref(res)))
        return F, it.value, res.value

    def _solve_mixed_multi(self, who, per, prescribed, body_in, max_iter, rtol, slip):
        import numpy as np
        m, nb, nl = self._mixed_sizes(who, per, prescribed, brownian=False)
        bi = np.ascontiguousarray(body_in, dtype=np.float64)
        if bi.ndim != 2 or bi.shape[0] < 1 or bi.shape[1] != 6 * nb:
            raise ValueError("%s: body_in must have shape (k, 6 N_bod), k >= 1; got %s" % (who, bi.shape))
        k = bi.shape[0]
        sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64)
        if sl is not None and sl.shape != (k, 3 * nb * nl):
            raise ValueError("%s: slip must have shape (k, 3 N_blobs) = (%d, %d); got %s" % (who, k, 3 * nb * nl, sl.shape))
        lam, U, F = np.empty((k, 3 * nb * nl)), np.empty((k, 6 * nb)), np.empty((k, 6 * nb))
        it, res = np.zeros(k, dtype=np.int32), np.zeros(k)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, k, bi.ctypes.data, _ptr(sl), int(max_iter), float(rtol),
                                                lam.ctypes.data, U.ctypes.data, F.ctypes.data, it.ctypes.data, res.ctypes.data))
        return lam, U, F, it, res

    def _rhs_and_midpoint_mixed(self, who, per, prescribed, body_in, slip, W, seed, method, split_rand, delta):
        import numpy as np
        m, nb, nl, bi, sl, Wh = self._mixed_host_args(who, per, prescribed, body_in, slip, W, brownian=True)
        s, X, Q = np.empty(3 * nb * nl), np.empty(3 * nb), np.empty(4 * nb)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, _ptr(sl), _ptr(Wh), int(seed), mhalf_code(method),
                                                int(bool(split_rand)), float(delta), s.ctypes.data, X.ctypes.data, Q.ctypes.data))
        return s, X, Q

    def solve_mixed(self, prescribed, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        """bodies with prescribed[b] = 1 move with body_in[b] (a velocity), the others carry body_in[b] as their load; host arrays
        -> (lambda, U, F, iterations, residual estimate)"""
        return self._solve_mixed("solve_mixed", 1, prescribed, body_in, max_iter, rtol, slip)

    def solve_mixed_dof(self, prescribed6, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        """solve_mixed with a mask per velocity component (prescribed6: 6 N_bod entries, in body_in's order)"""
        return self._solve_mixed("solve_mixed_dof", 6, prescribed6, body_in, max_iter, rtol, slip)

    def step_mixed(self, prescribed, body_in, max_iter=50, rtol=1.0e-8, slip=None):
        """the solve, then evolve_X_Q(U) -> (F, iterations, residual estimate)"""
        return self._step_mixed("step_mixed", 1, prescribed, body_in, max_iter, rtol, slip)

    def step_mixed_dof(self, prescribed6, body_in, max_iter=50, rtol=1.0e-8, slip=None):
        return self._step_mixed("step_mixed_dof", 6, prescribed6, body_in, max_iter, rtol, slip)

    def solve_mixed_multi(self, prescribed, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        """k right-hand sides under ONE mask in lock step: body_in (k, 6 N_bod), slip None or (k, 3 N_blobs); host arrays
        -> (lambda (k, 3 N_blobs), U (k, 6 N_bod), F (k, 6 N_bod), iterations (k,), residual estimates (k,))"""
        return self._solve_mixed_multi("solve_mixed_multi", 1, prescribed, body_in, max_iter, rtol, slip)

    def solve_mixed_dof_multi(self, prescribed6, body_in, max_iter=100, rtol=1.0e-8, slip=None):
        return self._solve_mixed_multi("solve_mixed_dof_multi", 6, prescribed6, body_in, max_iter, rtol, slip)

    def RHS_and_Midpoint_mixed(self, prescribed, body_in, slip=None, W=None, seed=0, method="cholesky", split_rand=True, delta=1.0e-4):
        """right-hand side and predictor of the Brownian step with prescribed bodies at q^n, nothing committed; host arrays, W
        (9 N_blobs: W1 | W2 | W_rfd) or None for seeded device noise -> (s (3 N_blobs), X_half (3 N_bod), Q_half (4 N_bod))"""
        return self._rhs_and_midpoint_mixed("RHS_and_Midpoint_mixed", 1, prescribed, body_in, slip, W, seed, method, split_rand, delta)

    def RHS_and_Midpoint_mixed_dof(self, prescribed6, body_in, slip=None, W=None, seed=0, method="cholesky", split_rand=True, delta=1.0e-4):
        """the same with a mask per velocity component, every body's rotation entries all 0 or all 1"""
        return self._rhs_and_midpoint_mixed("RHS_and_Midpoint_mixed_dof", 6, prescribed6, body_in, slip, W, seed, method, split_rand,
                                            delta)

    def solve_mixed_dev(self, prescribed, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F):
        """the same on device addresses (prescribed: a host array; d_slip, d_lam may be None / 0) -> (iterations, residual estimate)"""
        import numpy as np
        m = np.ascontiguousarray(prescribed, dtype=np.uint8).reshape(-1)
        nb = C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), None))
        if m.size != nb.value:
            raise ValueError("solve_mixed_dev: prescribed must have N_bod entries")
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_solve_mixed_dev(self.h, m.ctypes.data, d_body_in, d_slip or None, int(max_iter), float(rtol), d_lam or None,
                                             d_U, d_F, C.byref(it), C.byref(res)))
        return it.value, res.value

    def solve_mixed_dof_dev(self, prescribed6, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F):
        """solve_mixed_dev with a mask per velocity component (prescribed6: a host array of 6 N_bod entries) -> (iterations,
        residual estimate)"""
        import numpy as np
        m = np.ascontiguousarray(prescribed6, dtype=np.uint8).reshape(-1)
        nb = C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), None))
        if m.size != 6 * nb.value:
            raise ValueError("solve_mixed_dof_dev: prescribed6 must have 6 N_bod entries")
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(self.L.rbl_solve_mixed_dof_dev(self.h, m.ctypes.data, d_body_in, d_slip or None, int(max_iter), float(rtol),
                                                 d_lam or None, d_U, d_F, C.byref(it), C.byref(res)))
        return it.value, res.value

    def _mixed_multi_dev(self, who, per, prescribed, nrhs, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F):
        import numpy as np
        m = np.ascontiguousarray(prescribed, dtype=np.uint8).reshape(-1)
        nb = C.c_int(0)
        self._chk(self.L.rbl_get_sizes(self.h, C.byref(nb), None))
        if m.size != per * nb.value:
            raise ValueError("%s: prescribed must have %sN_bod entries" % (who, "6 " if per == 6 else ""))
        if int(nrhs) < 1:
            raise ValueError("%s: need nrhs >= 1" % who)
        it, res = np.zeros(int(nrhs), dtype=np.int32), np.zeros(int(nrhs))
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, int(nrhs), d_body_in, d_slip or None, int(max_iter), float(rtol),
                                                d_lam or None, d_U, d_F, it.ctypes.data, res.ctypes.data))
        return it, res

    def solve_mixed_multi_dev(self, prescribed, nrhs, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F):
        """nrhs right-hand sides under ONE mask in lock step, on device addresses: d_body_in nrhs vectors of 6 N_bod, d_slip (None / 0
        or nrhs vectors of 3 N_blobs), d_lam (may be None / 0), d_U, d_F likewise, one vector after the other; prescribed: a host array
        of N_bod entries -> (iterations (nrhs,), residual estimates (nrhs,))"""
        return self._mixed_multi_dev("solve_mixed_multi_dev", 1, prescribed, nrhs, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F)

    def solve_mixed_dof_multi_dev(self, prescribed6, nrhs, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F):
        """solve_mixed_multi_dev with a mask per velocity component (prescribed6: a host array of 6 N_bod entries)"""
        return self._mixed_multi_dev("solve_mixed_dof_multi_dev", 6, prescribed6, nrhs, d_body_in, d_slip, max_iter, rtol, d_lam, d_U, d_F)

    def _mixed_sizes(self, who, per, prescribed, brownian=True):
        """the mask of a call -> (mask, N_bod, N_blb).  per = 6: a mask per velocity component, 6 N_bod entries, in a Brownian
        call every body's rotation entries all 0 or all 1"""
        import numpy as np
        m = np.ascontiguousarray(prescribed, dtype=np.uint8).reshape(-1)
        nb, nl = self._sizes()
        if m.size != per * nb:
            raise ValueError(who + (": prescribed6 must have 6 N_bod entries" if per == 6 else ": prescribed must have N_bod entries"))
        if per == 6 and brownian:
            check_brownian_mask6(who, m, nb)
        return m, nb, nl

    def _rhs_and_midpoint_mixed_dev(self, who, per, prescribed, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s):
        import numpy as np
        m, nb, _ = self._mixed_sizes(who, per, prescribed)
        X = np.zeros(3 * nb); Q = np.zeros(4 * nb)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, d_body_in, d_slip or None, d_W or None, int(seed), mhalf_code(method),
                                                int(bool(split_rand)), float(delta), d_s, X.ctypes.data, Q.ctypes.data))
        return X.reshape(-1, 3), Q.reshape(-1, 4)

    def _step_brownian_mixed(self, who, per, prescribed, body_in, max_iter, rtol, slip, W, seed, method, split_rand, delta):
        import numpy as np
        m, nb, _, bi, sl, Wh = self._mixed_host_args(who, per, prescribed, body_in, slip, W, brownian=True)
        F = np.empty(6 * nb)
        it, res = C.c_int(0), C.c_double(0.0)
        self._chk(getattr(self.L, "rbl_" + who)(self.h, m.ctypes.data, bi.ctypes.data, _ptr(sl), _ptr(Wh), int(seed), mhalf_code(method),
                                                int(bool(split_rand)), float(delta), int(max_iter), float(rtol), F.ctypes.data,
                                                C.byref(it), C.byref(res)))
        return F, it.value, res.value

    def RHS_and_Midpoint_mixed_dev(self, prescribed, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s):
        """right-hand side and predictor of the Brownian step with prescribed bodies on device addresses (prescribed: a host
        array; d_slip, d_W may be None / 0; d_s: 3 N_blobs) -> (X_half, Q_half) on the host"""
        return self._rhs_and_midpoint_mixed_dev("RHS_and_Midpoint_mixed_dev", 1, prescribed, d_body_in, d_slip, d_W, seed, method,
                                                split_rand, delta, d_s)

    def step_brownian_mixed(self, prescribed, body_in, max_iter=50, rtol=1.0e-8, slip=None, W=None, seed=0, method=2, split_rand=True,
                            delta=1.0e-4):
        """one stochastic midpoint step with prescribed bodies inside librbl; host arrays -> (F, iterations, residual estimate)"""
        return self._step_brownian_mixed("step_brownian_mixed", 1, prescribed, body_in, max_iter, rtol, slip, W, seed, method, split_rand,
                                         delta)

    def RHS_and_Midpoint_mixed_dof_dev(self, prescribed6, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s):
        """RHS_and_Midpoint_mixed_dev with a mask per velocity component (prescribed6: a host array of 6 N_bod entries, every
        body's rotation entries all 0 or all 1) -> (X_half, Q_half) on the host"""
        return self._rhs_and_midpoint_mixed_dev("RHS_and_Midpoint_mixed_dof_dev", 6, prescribed6, d_body_in, d_slip, d_W, seed, method,
                                                split_rand, delta, d_s)

    def step_brownian_mixed_dof(self, prescribed6, body_in, max_iter=50, rtol=1.0e-8, slip=None, W=None, seed=0, method=2, split_rand=True,
                                delta=1.0e-4):
        """one stochastic midpoint step with prescribed velocity components inside librbl; host arrays -> (F, iterations, residual
        estimate)"""
        return self._step_brownian_mixed("step_brownian_mixed_dof", 6, prescribed6, body_in, max_iter, rtol, slip, W, seed, method,
                                         split_rand, delta)

    def blob_positions(self, body_begin, body_end, dout):
        self._chk(self.L.rbl_blob_positions_dev(self.h, body_begin, body_end, dout))

    def multi_body_pos(self, dout):
        """all blob positions into a device vector; on a row-split multi-GPU context: own bodies + one all-gather"""
        self._chk(self.L.rbl_multi_body_pos_dev(self.h, dout))

    def build_M(self, dr, n_blobs, scale_damp, dout):
        self._chk(self.L.rbl_rotne_prager_tensor_dev(self.h, dr, n_blobs, int(scale_damp), dout))

    def cholesky(self, dM, n, zero_upper=False):
        self._chk(self.L.rbl_cholesky_lower_dev(self.h, dM, n, int(zero_upper)))

    def trmv_lower(self, dL, n, dW, dout):
        self._chk(self.L.rbl_trmv_lower_dev(self.h, dL, n, dW, dout))

    def M_half_W(self, dr, n_blobs, dW, method, dout):
        self._chk(self.L.rbl_M_half_W_dev(self.h, dr, n_blobs, dW, mhalf_code(method), dout))

    def set_lanczos(self, max_iter, tol):
        self._chk(self.L.rbl_set_lanczos(self.h, max_iter, tol))

    def lanczos_report(self):
        it, res = C.c_int(0), C.c_double(0.0)
        self.L.rbl_get_lanczos_report(self.h, C.byref(it), C.byref(res))
        return it.value, res.value

    def sync_check(self):
        self._chk(self.L.rbl_sync_check(self.h))

    def close(self):
        if self.h and not self._borrowed:
            self.L.rbl_destroy(self.h)
        self.h = self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
