"""One Python binding for everything beyond the reference's surface (no GPU): `RigidBody.ctx` is a `DeviceContext` that borrows
the rbl_ctx of `RigidBody.cb`, the pybind11 class keeps the reference's methods and the solver and stepping methods only, and
the setters reach the library through the view."""
import os
import shutil
import subprocess
import sys

import numpy as np

from conftest import ROOT, create_solver, random_positions

# what left c_rigid.CManyBodies: bound once, by DeviceContext (and presented by RigidBody)
MOVED = ("velocity_field", "solve_mixed", "step_mixed", "solve_mixed_dof", "step_mixed_dof", "solve_mixed_multi", "solve_mixed_dof_multi",
         "RHS_and_Midpoint_mixed", "step_brownian_mixed", "RHS_and_Midpoint_mixed_dof", "step_brownian_mixed_dof",
         "set_interactions", "set_pair_table", "set_height_table", "set_traps", "set_dipoles", "dipoles", "set_magnetic_field",
         "magnetic_field", "set_field_time", "field_time", "set_bonds", "set_bond_table", "bond_state", "set_joints", "joints",
         "solve_jointed", "step_jointed", "joint_state", "interactions_active", "interaction_forces", "interaction_energy",
         "set_background_flow", "set_body_slip", "flow_model", "flow_slip", "first_moments", "step_moments")
HELPERS = ("bad_mixed_arg", "mixed_args", "noise_arg", "joints_active", "jointed_args")        # C++ helpers of those methods
KEPT = ("apply_M_multi", "M_half_W", "M_half_W_r", "M_RFD", "KTinv_RFD", "update_X_Q", "step_deterministic", "step_brownian",
        "RHS_and_Midpoint", "lanczos_report", "set_lanczos", "rotne_prager_tensor", "cholesky_lower", "pair_blocks", "apply_saddle",
        "solve_saddle", "solve_saddle_multi", "evolve_X_Q_RFD", "set_option", "get_option", "handle")


def _three(wall=False, seed=5):
    X, Q = random_positions(3, wall=wall, seed=seed, min_dist=4.5)
    return create_solver(X, Q, wall_PC=wall, block_PC=True, dt=0.01)


def test_view_borrows_the_owners_context():
    rb = _three()
    assert rb.ctx.h == rb.cb.handle() and rb.ctx._owner is rb.cb
    assert np.array_equal(rb.ctx.blob_anchor(4), rb.blob_anchor(4))


def test_closing_the_view_leaves_the_owner_alive():
    rb = _three()
    X0, Q0 = rb.get_config()
    rb.ctx.close()
    assert rb.ctx.h is None
    del rb.ctx
    X, Q = rb.get_config()
    assert np.array_equal(X, X0) and np.array_equal(Q, Q0)
    assert rb.cb.get_option("record_moments") == 0
    other = _three(seed=7)
    del rb                                                # of two objects the older one goes first ...
    assert other.get_config()[0].shape == (3, 3)
    third = _three(seed=8)
    del third                                             # ... or the younger one does
    assert other.get_config()[0].shape == (3, 3)
    view = other.ctx
    del other
    assert view._owner.get_option("record_moments") == 0  # a view alone keeps its owner's context alive


_CHILD = """
from rigid_body_light_amd import RigidBody, load_structure
from rigid_body_light_amd import _lib
rb = RigidBody(load_structure(12)[1], [[0.0, 0.0, 5.0]], [[1.0, 0.0, 0.0, 0.0]], 1.0, 1.0, 0.01)
print("VIEW", rb.ctx.L._name)
print("OWNING", _lib.lib()._name)    # what DeviceContext.__init__ takes (it then binds a stream, which needs a device)
"""


def test_view_loads_the_in_package_library_whatever_RBL_LIBRARY_says(tmp_path):
    from rigid_body_light_amd import _lib
    copy = str(tmp_path / "librbl_copy.so")
    shutil.copy(_lib.IN_PACKAGE_LIB, copy)
    env = dict(os.environ, RBL_LIBRARY=copy)
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    names = dict(line.split(" ", 1) for line in out.splitlines() if line.startswith(("VIEW ", "OWNING ")))
    assert names["VIEW"] == _lib.IN_PACKAGE_LIB
    assert names["OWNING"] == copy


def test_one_binding():
    from rigid_body_light_amd import RigidBody, c_rigid
    from rigid_body_light_amd._lib import DeviceContext
    for name in MOVED + HELPERS:
        assert not hasattr(c_rigid.CManyBodies, name), name
    for name in MOVED:
        assert hasattr(DeviceContext, name), name
        assert hasattr(RigidBody, name) or name == "interactions_active", name
    for name in KEPT:
        assert hasattr(c_rigid.CManyBodies, name), name


def test_root_method_names_live_in_one_table():
    import pytest
    from rigid_body_light_amd._lib import MHALF_METHODS, mhalf_code
    assert MHALF_METHODS == {"cholesky": 0, "lanczos": 1, "lanczos_pc": 2}
    assert [mhalf_code(m) for m in ("cholesky", "lanczos", "lanczos_pc", 1, np.int64(2))] == [0, 1, 2, 1, 2]
    with pytest.raises(RuntimeError, match="M_half_W: method must be 'cholesky', 'lanczos' or 'lanczos_pc'"):
        mhalf_code("qr")


def test_setters_round_trip_through_the_view():
    rb = _three()
    rb.set_bonds([[0, 1], [2, -1]], rb.blob_anchor(3), [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]], k=[2.0, 3.0], l0=0.5, kind=[0, 0])
    b = rb.ctx.bonds()
    assert b["on"] and np.array_equal(b["body"], [[0, 1], [2, -1]]) and b["body"].dtype == np.int32
    assert np.array_equal(b["anchor_a"], np.tile(rb.blob_anchor(3), (2, 1))) and np.array_equal(b["anchor_b"], [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    assert np.array_equal(b["kind"], [0, 0]) and np.array_equal(b["k"], [[2.0, 3.0]]) and np.array_equal(b["l0"], [[0.5, 0.5]])
    assert rb.ctx.interactions_active() == 64
    rb.set_bonds(None, None, None, None, on=False)
    assert not rb.ctx.bonds()["on"] and rb.ctx.bonds()["body"].shape == (2, 2) and rb.ctx.interactions_active() == 0

    rb.set_joints([[0, 1], [1, -1]], [0.0, 0.0, 1.5], [[0.0, 0.0, -1.5], [4.0, 5.0, 6.0]])
    j = rb.joints()
    assert j["on"] and np.array_equal(j["body"], [[0, 1], [1, -1]])
    assert np.array_equal(j["anchor_a"], [[0.0, 0.0, 1.5]] * 2) and np.array_equal(j["anchor_b"], [[0.0, 0.0, -1.5], [4.0, 5.0, 6.0]])
    rb.set_joints(None, None, None, on=False)
    assert not rb.joints()["on"] and rb.joints()["body"].shape == (2, 2)

    m = np.arange(9.0).reshape(3, 3)
    rb.set_dipoles(m, c_dd=0.25, r_core=2.0, r_cut=30.0)
    d = rb.dipoles()
    assert d["on"] and (d["c_dd"], d["r_core"], d["r_cut"]) == (0.25, 2.0, 30.0) and np.array_equal(d["m_body"], m)
    rb.set_dipoles(None, on=False)
    assert not rb.dipoles()["on"] and np.array_equal(rb.dipoles()["m_body"], m)

    rb.set_magnetic_field(B0=[0.0, 0.0, 1.0], B2=[0.5, 0.0, 0.0], omega=3.0)
    f = rb.magnetic_field()
    assert set(f) == {"B0", "B1", "B2", "on", "omega"} and f["on"] and f["omega"] == 3.0
    assert np.array_equal(f["B0"], [0.0, 0.0, 1.0]) and np.array_equal(f["B1"], np.zeros(3)) and np.array_equal(f["B2"], [0.5, 0.0, 0.0])
    rb.set_magnetic_field(on=False)
    assert not rb.magnetic_field()["on"] and rb.magnetic_field()["omega"] == 3.0

    assert rb.field_time() == 0.0
    rb.set_field_time(0.375)
    assert rb.field_time() == 0.375 and np.array_equal(rb.ctx.field_time(), [0.375])
