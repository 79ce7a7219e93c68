"""Host-side operator surface of the MI355X-native blob-mobility library.

`RigidBody` presents the constructor, attributes, methods, output shapes and RuntimeError
behaviour of the reference's Python wrapper (reference src/Rigid.py:5-135) so that user code written
against `from Rigid import RigidBody` runs unchanged, but every call lands in librbl.so: the reference's
surface and the solver and stepping methods through the pybind11 class `c_rigid.CManyBodies` (`self.cb`), everything
newer through `self.ctx`, a `_lib.DeviceContext` that borrows the same rbl_ctx.  Size rules are kept in one table (`_expected_size`) instead
of per-method checks; shapes follow the shape X was given in (2-D in -> (-1, 3) out, flat in -> flat out,
reference src/Rigid.py:54,60,66).

Beyond the reference surface (its C++ has these, its Python does not): `solve_saddle`, `solve_saddle_multi`,
`body_mobility_matrix`, `M_half_W`, `M_RFD`,
`KTinv_RFD`, `M_RFD_cfgs`, `M_RFD_from_U`, `KT_RFD_from_U`, `evolve_rigid_bodies_RFD`, `apply_M_multi`,
`dense_mobility`, `velocity_field` (the flow at arbitrary points), prescribed kinematics (`solve_mixed`, `step_mixed`,
`body_resistance_matrix`: bodies that are held or driven, and the loads that takes; `solve_mixed_dof`, `step_mixed_dof`: the same for
single velocity components; `solve_mixed_multi`, `solve_mixed_dof_multi`: many right-hand sides under one mask in lock step; `step_brownian_mixed`,
`RHS_and_Midpoint_mixed`: the same among Brownian bodies; `step_brownian_mixed_dof`, `RHS_and_Midpoint_mixed_dof`: Brownian steps with single
velocity components prescribed, a body's rotation wholly or not at all), a force model the reference does not have (`set_interactions`, `interaction_forces`),
and an imposed flow, a body-frame slip and stresslets (`set_background_flow`, `set_body_slip`, `flow_slip`, `first_moments`, `stresslets`,
`record_moments`, `step_moments`).
"""
import numpy as np

from . import c_rigid as _ext
from ._lib import JOINT_AXIS, JOINT_BALL, JOINT_LOCK, DeviceContext, default_q_rel, hinge, joint_kind_args, joint_rows, motor, weld, blob_anchor, bond_args, check_brownian_mask6, blob_type_args, dipole_args, field_args, joint_args, patch_types, periodic_args, table_arrays, tabulate  # noqa: F401

_KBT_IN_WRAPPER = 1.0   # the reference wrapper passes kBT = 1 whatever the caller wants (src/Rigid.py:23)


def _fail(message):
    raise RuntimeError(message)


class RigidBody:
    X_shape = None
    Q_shape = None

    # ------------------------------------------------------------------ construction
    def __init__(self, rigid_config, X, Q, a, eta, dt, wall_PC=False, block_PC=False):
        template = np.asarray(rigid_config)
        if template.size % 3:
            _fail(f"Rigid config must have length 3N. Rigid config shape: {template.shape}")
        self.cb = _ext.CManyBodies()
        self.precision = self.cb.precision
        self.blobs_per_body = template.size // 3
        self._cfg = np.array(template, dtype=np.float64).reshape(-1, 3)
        self._a = a                          # (the force model's default cutoff)
        self._wall = bool(wall_PC)
        self.cb.setParameters(a, dt, _KBT_IN_WRAPPER, eta, template.reshape(self.blobs_per_body, 3))
        self.ctx = DeviceContext.borrow(self.cb.handle(), a, template.reshape(self.blobs_per_body, 3), owner=self.cb)
        self.cb.setWallPC(bool(wall_PC))
        self.cb.setBlkPC(bool(block_PC))
        self.set_config(X, Q)

    # ------------------------------------------------------------------ size / shape rules
    def _expected_size(self, kind):
        n_blob3 = 3 * self.total_blobs
        return {"blob": n_blob3, "body": 6 * self.N_bodies, "system": n_blob3 + 6 * self.N_bodies}[kind]

    def _require(self, vec, kind):
        vec = np.asarray(vec)
        want = self._expected_size(kind)
        if vec.size != want:
            label = {"blob": "lambda must have total size 3*N_blobs",
                     "body": "U must have total size 6*N_bodies",
                     "system": "Rigid system input vector must have total size 3*N_blobs + 6*N_bodies"}[kind]
            _fail(f"{label} = {want}. Got shape: {vec.shape}")
        return vec.reshape(-1)

    def _like_X(self, flat):
        return np.asarray(flat).reshape((-1, 3) if len(self.X_shape) == 2 else (-1,))

    # ------------------------------------------------------------------ configuration
    def set_config(self, X, Q):
        X, Q = np.asarray(X), np.asarray(Q)
        if X.size % 3:
            _fail("X must have total length 3N")
        if Q.size % 4:
            _fail("Q must have total length 4N")
        if X.size // 3 != Q.size // 4:
            _fail("X and Q must have the same number of bodies")
        self.N_bodies = X.size // 3
        self.total_blobs = self.N_bodies * self.blobs_per_body
        self.X_shape, self.Q_shape = X.shape, Q.shape
        self.cb.setConfig(X.reshape(-1), Q.reshape(-1))       # Q is normalised inside (c_rigid_obj.cpp:216)
        self.cb.set_K_mats()

    def get_config(self):
        X, Q = self.cb.getConfig()
        return X.reshape(self.X_shape), Q.reshape(self.Q_shape)

    def get_blob_positions(self):
        return self._like_X(self.cb.multi_body_pos())          # GPU: r_k = R(Q_b) c_k + X_b (:257-300)

    def evolve_rigid_bodies(self, U):
        self.cb.evolve_X_Q(self._require(U, "body"))           # multiplies by dt inside (:869)

    # ------------------------------------------------------------------ geometric operators
    def K_dot(self, U):
        return self._like_X(self.cb.K_x_U(self._require(U, "body")))

    def KT_dot(self, lambda_vec):
        return self._like_X(self.cb.KT_x_Lam(self._require(lambda_vec, "blob")))

    def get_K(self):
        return self.cb.get_K()

    def get_Kinv(self):
        return self.cb.get_Kinv()

    # ------------------------------------------------------------------ mobility
    def apply_M(self, forces, positions):
        """U = M F (or B M B F with the wall term when wall_PC), GPU, matrix-free.  The blob count is
        whatever `positions` holds, not necessarily the object's own (reference tests/test_interface.py:171)."""
        forces, positions = np.asarray(forces), np.asarray(positions)
        if forces.size != positions.size:
            _fail("Positions and forces must be of the same size")
        if forces.size % 3:
            _fail("Positions and forces must have total length 3N, where N is the number of blobs")
        return self.cb.apply_M(forces.reshape(-1), positions.reshape(-1))

    def apply_saddle(self, x):
        """[M lambda - K U ; K^T lambda]  (reference src/Rigid.py:73-80)."""
        return self.cb.apply_saddle(self._require(x, "system"))    # one boundary crossing (rbl_apply_saddle); the reference
                                                                    # composes it from four calls through its extension

    def apply_PC(self, b):
        return self.cb.apply_PC(self._require(b, "system"))

    def solve_saddle(self, rhs, max_iter=100, rtol=1.0e-8, x0=None):
        """Solve [M -K; K^T 0] x = rhs by the library's own right-preconditioned GMRES (apply_PC as preconditioner), all
        iterations on the GPU: what a user of the reference loops over apply_saddle / apply_PC for from outside
        (src/Rigid.py:69-80).  -> (x, iterations, residual estimate)"""
        return self.cb.solve_saddle(self._require(rhs, "system"), int(max_iter), float(rtol),
                                    None if x0 is None else self._require(x0, "system"))

    def solve_saddle_multi(self, rhs, max_iter=100, rtol=1.0e-8):
        """The same solve for SEVERAL right-hand sides of this configuration at once, rhs (k, 3 N_blobs + 6 N_bodies): k GMRES
        recurrences in lock step, each column the iterates `solve_saddle` would give it, the k mobility products of an iteration
        ONE launch on the fp64 matrix cores (16 columns per pass).  -> (x (k, size), iterations (k,), residual estimates (k,))"""
        rhs = np.ascontiguousarray(np.atleast_2d(np.asarray(rhs, dtype=np.float64)))
        if rhs.shape[1] != 3 * self.total_blobs + 6 * self.N_bodies:
            _fail("solve_saddle_multi: rhs must have shape (k, 3*total_blobs + 6*N_bodies)")
        return self.cb.solve_saddle_multi(rhs, int(max_iter), float(rtol))

    def body_mobility_matrix(self, max_iter=100, rtol=1.0e-8, columns=None):
        """The (6 N_bodies) x (6 N_bodies) body mobility matrix N = (K^T M^-1 K)^-1 of the current configuration, U = N F: one
        saddle solve [M -K; K^T 0][lambda; U] = [0; e_c] per unit load e_c (force / torque component c of one body), the 6 N_bodies
        solves through `solve_saddle_multi`.  columns: only these unit loads (default all).  -> (N[:, columns], iterations)"""
        nb6, n3 = 6 * self.N_bodies, 3 * self.total_blobs
        cols = np.arange(nb6) if columns is None else np.asarray(columns, dtype=int).reshape(-1)
        rhs = np.zeros((cols.size, n3 + nb6))
        rhs[np.arange(cols.size), n3 + cols] = 1.0          # K^T lambda = e_c, M lambda = K U  =>  U = (K^T M^-1 K)^-1 e_c
        x, its, _ = self.solve_saddle_multi(rhs, max_iter, rtol)
        return np.ascontiguousarray(x[:, n3:].T), its

    # ------------------------------------------------------------------ beyond the reference's Python surface
    def M_half_W(self, W=None, seed=0, method="cholesky"):
        """Brownian increment M^{1/2} W (reference c_rigid_obj.cpp:661-675, C++ only).
        W=None draws reproducible N(0,1) noise from `seed` on the device."""
        return self.cb.M_half_W(None if W is None else self._require(W, "blob"), seed, method)

    def M_RFD(self, W=None, seed=0, delta=1.0e-4):
        """(1/delta)[M(q + delta/2 Kinv W) - M(q - delta/2 Kinv W)] W  (reference :769-796, C++ only)."""
        return self.cb.M_RFD(None if W is None else self._require(W, "blob"), seed, delta)

    def KTinv_RFD(self, W, delta=1.0e-4):
        """reference c_rigid_obj.cpp:743-767 (C++ only); W has length 6*N_bodies."""
        return self.cb.KTinv_RFD(self._require(W, "body"), delta)

    def M_RFD_cfgs(self, U, delta=1.0e-4):
        """blob positions of the configurations displaced by +-(delta/2) U (reference :798-818, C++ only) -> (r_plus, r_minus)."""
        return self.cb.M_RFD_cfgs(self._require(U, "body"), delta)

    def M_RFD_from_U(self, U, W, delta=1.0e-3):
        """(1/delta)[M(q + delta/2 U) - M(q - delta/2 U)] W for the caller's displacement U (reference :820-842, C++ only)."""
        return self.cb.M_RFD_from_U(self._require(U, "body"), self._require(W, "blob"), delta)

    def KT_RFD_from_U(self, U, W, delta=1.0e-3):
        """(1/delta)[K(q + delta/2 U)^T - K(q - delta/2 U)^T] W (reference :844-863, C++ only); W has length 3*N_blobs."""
        return self.cb.KT_RFD_from_U(self._require(U, "body"), self._require(W, "blob"), delta)

    def evolve_rigid_bodies_RFD(self, U):
        """commit the configuration displaced by U (displacement units, no dt) and keep the preconditioner
        (reference evolve_X_Q_RFD :880-893, C++ only)."""
        self.cb.evolve_X_Q_RFD(self._require(U, "body"))

    def update_X_Q(self, U):
        """configuration displaced by U (translation + rotation vector per body), NOT committed
        (reference c_rigid_obj.cpp:798-863, C++ only) -> (X, Q) flat arrays."""
        return self.cb.update_X_Q(self._require(U, "body"))

    def RHS_and_Midpoint(self, slip, force, W=None, seed=0, method="cholesky", split_rand=True, delta=1.0e-4):
        """Right-hand side and predictor configuration of the stochastic midpoint step (reference
        c_rigid_obj.cpp:917-976, C++ only): ([slip - (kBT M_RFD + BI) ; -force], X_half, Q_half).
        W = [W1 | W2 | W_rfd] (9*N_blobs numbers) or None for seeded device noise."""
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1))
        return self.cb.RHS_and_Midpoint(self._require(slip, "blob"), self._require(force, "body"), W, seed,
                                        method, split_rand, delta)

    def step_deterministic(self, F_body, slip=None, max_iter=50, rtol=1.0e-8, warm_start=False):
        """One deterministic time step inside the library: GMRES on the saddle system with rhs [slip ; -F_body]
        (apply_PC as preconditioner), then evolve_rigid_bodies(U).  warm_start: False/0 cold, True/1 start from the previous
        step's solution, 2 / 3 from the linear / quadratic extrapolation of the last solutions (smooth forcing: far fewer
        iterations).  Returns (iterations, residual estimate)."""
        return self.cb.step_deterministic(self._require(F_body, "body"), None if slip is None else self._require(slip, "blob"),
                                          max_iter, rtol, int(warm_start))

    def step_brownian(self, F_body, slip=None, W=None, seed=0, method="lanczos_pc", split_rand=True, delta=1.0e-4,
                      max_iter=50, rtol=1.0e-8):
        """One stochastic midpoint step inside the library (RHS_and_Midpoint at q^n, solve at q^{n+1/2}, update from q^n).
        Note the reference wrapper fixes kBT = 1 (src/Rigid.py:23); scale dt / forces accordingly."""
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1))
        return self.cb.step_brownian(self._require(F_body, "body"), None if slip is None else self._require(slip, "blob"),
                                     W, seed, method, split_rand, delta, max_iter, rtol)

    def set_interactions(self, w=0.0, eps_wall=0.0, b_wall=1.0, eps_blob=0.0, b_blob=1.0, r_cut=None, on=True):
        """Configuration-dependent forces on the blobs (include/rbl.h section 4): weight w per blob (-w z^), wall repulsion
        eps_wall exp(-(h - a)/b_wall) (with wall_PC), steric repulsion eps_blob (2a/r) exp(-(r - 2a)/b_blob) between blobs of
        different bodies, cut off at r_cut (default 2a + 20 b_blob).  step_deterministic / step_brownian then add these forces
        at the configuration the step starts from; on=False switches the model off."""
        if r_cut is None:
            r_cut = 2.0 * self._a + 20.0 * b_blob
        self.ctx.set_interactions(w, eps_wall, b_wall, eps_blob, b_blob, r_cut, on)

    def set_pair_table(self, U, dU, r_min, r_cut, on=True):
        """A tabulated radial potential between blobs of different bodies (include/rbl.h section 4): values U and derivatives
        dU = dU/dr on the uniform grid r_min .. r_cut (`tabulate(U, dU, r_min, r_cut, n)` makes them from callables).  Cubic
        Hermite inside the grid, the tangent at r_min below it, nothing beyond r_cut; the table is not shifted, so
        U(r_cut) != 0 is a jump in the energy.  Adds to the steric term of set_interactions."""
        U, dU = table_arrays("set_pair_table", U, dU)
        self.ctx.set_pair_table(U, dU, r_min, r_cut, on)

    def set_height_table(self, U, dU, h_min, h_cut, on=True):
        """The same construction in the blob height z over h_min .. h_cut, with or without the wall."""
        U, dU = table_arrays("set_height_table", U, dU)
        self.ctx.set_height_table(U, dU, h_min, h_cut, on)

    def set_blob_types(self, types, n_types=None, on=True):
        """A type per blob (include/rbl.h section 4): integers in [0, n_types), n_types <= 8, of shape (N_blobs_per_body,) --
        every body alike -- or (N_bodies, N_blobs_per_body).  With set_type_table a pair of blobs of different bodies gets the
        table of its two types on top of the steric term and the pair table; `patch_types` types a cap of the structure."""
        if types is None and not on:
            return self.ctx.set_blob_types(None, on=False)
        t, n_types = blob_type_args("set_blob_types", types, n_types)
        if t.size not in (self.blobs_per_body, self.N_bodies * self.blobs_per_body):
            raise ValueError(f"set_blob_types: types must have shape ({self.blobs_per_body},) or ({self.N_bodies}, {self.blobs_per_body}). "
                             f"Got shape: {np.shape(types)}")
        self.ctx.set_blob_types(t, n_types, on)

    def blob_types(self):
        """{on, n_types, types}"""
        return self.ctx.blob_types()

    def set_type_table(self, ta, tb, U, dU, r_min, r_cut, on=True):
        """The pair table of set_pair_table for blobs of the types ta and tb; (tb, ta) names the same table."""
        self.ctx.set_type_table(ta, tb, U, dU, r_min, r_cut, on)

    def type_table(self, ta, tb):
        """{n, lo, hi, on, coef (n - 1, 4)}"""
        return self.ctx.type_table(ta, tb)

    def clear_type_tables(self):
        self.ctx.clear_type_tables()

    def set_traps(self, k, X0, on=True):
        """Harmonic traps on the body centres: k and X0 of shape (N_bodies, 3), lab frame; a component of k that is 0 leaves
        that axis free.  The body feels -k (X - X0) and no torque."""
        k, X0 = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(X0, dtype=np.float64)
        if k.ndim != 2 or k.shape[1] != 3 or k.shape != X0.shape:
            raise ValueError(f"set_traps: k and X0 must both have shape (N_bodies, 3). Got shapes: {k.shape} and {X0.shape}")
        self.ctx.set_traps(k, X0, on)

    def set_dipoles(self, m_body, c_dd=0.0, r_core=None, r_cut=np.inf, on=True):
        """Permanent magnetic moments fixed in the bodies (include/rbl.h section 4): m_body of shape (3,) -- every body alike --
        or (N_bodies, 3), body frame; the lab-frame moment is R(Q) m_body.  c_dd > 0 adds the dipole pairs between the body
        centres, U = c_dd [m_i.m_j / s^3 - 3 (m_i.r)(m_j.r) / s^5], s = max(|r|, r_core), skipped beyond r_cut (not shifted);
        set_magnetic_field adds the torque m x B(t).  Both enter the body forces and torques of every step at q^n."""
        if m_body is None and not on:
            return self.ctx.set_dipoles(None, on=False)
        m, r_core = dipole_args("set_dipoles", m_body, c_dd, r_core)
        if m.shape[0] not in (1, self.N_bodies):
            raise ValueError(f"set_dipoles: m_body must have shape (3,) or (N_bodies, 3). Got shape: {m.shape}")
        self.ctx.set_dipoles(m, c_dd, r_core, r_cut, on)

    def dipoles(self):
        """{on, c_dd, r_core, r_cut, m_body (n, 3)}"""
        return self.ctx.dipoles()

    def set_magnetic_field(self, B0=None, B1=None, B2=None, omega=0.0, on=True):
        """The uniform field B(t) = B0 + B1 cos(omega t) + B2 sin(omega t), lab frame (None: zeros), evaluated at the field
        time of set_field_time -- no step advances that clock.  Torque m x B on every body with a moment, no force."""
        if B0 is None and B1 is None and B2 is None and not on:
            return self.ctx.set_magnetic_field(on=False)
        B0, B1, B2 = field_args("set_magnetic_field", B0, B1, B2)
        self.ctx.set_magnetic_field(B0, B1, B2, float(omega), bool(on))

    def magnetic_field(self):
        """{on, omega, B0, B1, B2}"""
        return self.ctx.magnetic_field()

    def set_field_time(self, t):
        """The time the field is evaluated at by the next steps and queries (default 0); the caller advances it."""
        self.ctx.set_field_time(t)

    def field_time(self):
        return float(self.ctx.field_time()[0])

    def set_bonds(self, body, anchor_a, anchor_b, k, l0=0.0, kind=None, on=True):
        """Bonds and tethers between anchor points fixed in the bodies (include/rbl.h section 4).  body: (n_bonds, 2) integers;
        bond b joins the point X_i + R(Q_i) anchor_a[b] of body i = body[b, 0] to the same kind of point of body j = body[b, 1]
        != i or, with j = -1, to the lab-frame point anchor_b[b] (a tether).  Anchors are body-frame vectors from the body's
        centre ((3,): every bond alike, or (n_bonds, 3); `blob_anchor(k)` ends a bond on blob k).  kind 0 (default): harmonic,
        U = k (d - l0)^2 / 2; kind 1: U = k T(d) with the table of set_bond_table.  k, l0: a number or (n_bonds,).  One bond is a
        ball joint, two a hinge, three non-collinear ones a stiff joint.  The bonds enter the body forces and torques of every
        step at q^n.  body=None with on=False only switches them off."""
        if body is None and not on:
            return self.ctx.set_bonds(None, None, None, None, on=False)
        b, anchor, kind, param = bond_args("set_bonds", body, anchor_a, anchor_b, k, l0, kind, sets=(1,))
        self.ctx.set_bonds(b, anchor[:, :3], anchor[:, 3:], param[0, :, 0], param[0, :, 1], kind, bool(on))

    def set_bond_table(self, U, dU, r_min, r_cut, on=True):
        """The potential T(d) of the kind-1 bonds: values U and derivatives dU = dU/dd on the uniform grid r_min .. r_cut
        (`tabulate` makes them from callables).  Cubic Hermite inside the grid, continued along its tangent at BOTH ends: a bond
        never breaks.  FENE, worm-like chain, Morse, ..."""
        U, dU = table_arrays("set_bond_table", U, dU)
        self.ctx.set_bond_table(U, dU, r_min, r_cut, on)

    def bond_state(self):
        """-> (length, tension dU/dd, energy) of every bond at the current configuration, (n_bonds,) each"""
        return self.ctx.bond_state()

    def blob_anchor(self, k):
        """Body-frame position of blob k with the structure's mean removed: the anchor of a bond that ends on that blob."""
        return blob_anchor(self._cfg, k)

    # -- hard joints (include/rbl.h section 9) -----------------------------------------------------------------------------------
    def set_joints(self, body, anchor_a, anchor_b, on=True):
        """Hard joints: ball joints between anchor points fixed in the bodies, imposed as constraints of the saddle solve (the
        bonds of set_bonds are springs).  The description is set_bonds': body (n_joints, 2) integers; joint j joins the point
        X_i + R(Q_i) anchor_a[j] of body i = body[j, 0] to the same kind of point of body body[j, 1] != i or, with body[j, 1] = -1,
        to the lab-frame point anchor_b[j] (a pivot).  Anchors: (3,) -- every joint alike -- or (n_joints, 3); zeros are the body
        centre, `blob_anchor(k)` is blob k.  One joint leaves the relative rotation free, two between the same bodies are a hinge.
        Refused (RuntimeError naming the joint): a body index out of range, both ends on one body, a pivot in the first slot,
        non-finite anchors, a third joint between one pair of bodies or a third pivot on one body.  Only solve_jointed and
        step_jointed use the joints; every other method ignores them.  body=None with on=False only switches them off."""
        if body is None and not on:
            return self.ctx.set_joints(None, None, None, on=False)
        b, anchor = joint_args("set_joints", body, anchor_a, anchor_b)
        self.ctx.set_joints(b, anchor[:, :3], anchor[:, 3:], bool(on))

    def joints(self):
        """-> {on, body (n_joints, 2), anchor_a (n_joints, 3), anchor_b (n_joints, 3)} (n_joints = 0: never set)"""
        return self.ctx.joints()

    def set_joint_kinds(self, body, kind, anchor_a=None, anchor_b=None, axis=None, q_rel=None, on=True):
        """Hard joints of every kind, a superset of set_joints: kind[j] is JOINT_BALL (0; three translational rows, anchors as in
        set_joints), JOINT_LOCK (1; w_A = w_B) or JOINT_AXIS (2; w_A - w_B free about axis only).  axis (3,) or (n_joints, 3) is
        fixed in body A's frame; q_rel (4,) or (n_joints, 4), scalar first, is the target Q_A^-1 Q_B, None: that of the current
        configuration.  Body B = -1 is the lab.  Compose them: ball + axis on one pair is a five-row hinge, ball + lock a weld,
        ball + lock with a rate (set_joint_rates) a motor -- `hinge`, `weld`, `motor` build the rows, `joint_rows` concatenates
        them.  Refused with the joint named: an unknown kind, a bad axis or q_rel, a second angular joint on a pair, an angular
        joint next to two ball joints on a pair, and what set_joints refuses."""
        if body is None and not on:
            return self.ctx.set_joint_kinds(None, None, on=False)
        b, k, anchor, ax, qr = joint_kind_args("set_joint_kinds", body, kind, anchor_a, anchor_b, axis, q_rel)
        if q_rel is None and (k != JOINT_BALL).any():
            default_q_rel("set_joint_kinds", b, k, qr, self.cb.getConfig()[1])
        self.ctx.set_joint_kinds(b, k, anchor[:, :3], anchor[:, 3:], ax, qr, bool(on))

    def set_joint_rates(self, rates):
        """The motors' rates (n_joints,): body B of a lock joint turns relative to body A at +rate about the joint's axis (fixed
        in A); 0 for every other kind.  Read by step_jointed; the motor angle theta advances by rate dt per accepted step."""
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if not np.isfinite(r).all():
            _fail("set_joint_rates: joint %d: the rate must be finite" % int(np.argmin(np.isfinite(r))))
        self.ctx.set_joint_rates(r)

    def joint_kinds(self):
        """-> {on, by_kinds, body, anchor_a, anchor_b, kind, axis, q_rel, theta, rate} of the stored joints"""
        return self.ctx.joint_kinds()

    def hinge(self, a, b, point, axis):
        """Rows of a five-row hinge between the bodies a and b (b = -1: the lab) at the current configuration: a ball joint at
        the lab-frame point and an axis joint about the lab-frame direction axis."""
        return hinge(*self.cb.getConfig(), a, b, point, axis)

    def weld(self, a, b, point):
        """Rows of a weld: a ball joint at the lab-frame point and a lock joint; the two bodies move as one."""
        return weld(*self.cb.getConfig(), a, b, point)

    def motor(self, a, b, point, axis):
        """Rows of a motor or driven hinge: a ball joint at the lab-frame point and a lock joint about axis, driven by
        set_joint_rates."""
        return motor(*self.cb.getConfig(), a, b, point, axis)

    # -- periodic cell in x and y (include/rbl.h section 10) -----------------------------------------------------------------------
    def set_periodic(self, Lx, Ly, images=(1, 1), on=True):
        """A periodic cell of lengths Lx, Ly along x and y above the wall (0: that axis stays open): every mobility product --
        apply_M, the solves, the Brownian roots and drift, every step -- sums the wall-corrected pair mobility over
        images = (nx, ny) periodic images on either side of every pair's nearest one, and the pair forces (steric, pair table,
        dipole pairs) use the minimum image.  Positions stay unwrapped.  The sum is truncated: its remainder falls like 1 / n, and
        the nearest image alone (n = 0) is not positive definite, so a periodic axis takes 1 <= n <= 16.  Needs the wall; L must
        exceed 4a; the force model needs 2 R_body + r_cut <= L / 2.  Bonds and joints join bodies at their unwrapped positions.
        Not offered with the cell on (RuntimeError, "periodic"): the dense mobility and the dense Cholesky root, the velocity
        field, ensembles, several GPUs."""
        Lx, Ly, nx, ny = periodic_args("set_periodic", Lx, Ly, images)
        self.ctx.set_periodic(Lx, Ly, images=(nx, ny), on=bool(on))

    def periodic(self):
        """-> {on, Lx, Ly, images (nx, ny)} (both lengths 0: never set)"""
        return self.ctx.periodic()

    def _jointed_args(self, who, F_body, slip, jv, name):
        F, sl = self._body_in_and_slip(F_body, slip)
        if jv is not None:
            jv = np.ascontiguousarray(jv, dtype=np.float64).reshape(-1)
            if jv.size != 3 * self.ctx._joints_active():
                _fail(f"{who}: {name} must have length 3*n_joints (of the joints that are on)")
        return F, sl, jv

    def solve_jointed(self, F_body, slip=None, joint_rhs=None, max_iter=100, rtol=1.0e-8):
        """The saddle solve with the joints as constraints:  M lambda - K U = slip,  K^T lambda + J^T phi = -F_body,  J U = joint_rhs
        (None: zero; (n_joints, 3) or flat), (J U)_j the velocity of joint j's point on body A minus that of its point on body B.
        ONE GMRES solve on the GPU, longer by 3 n_joints unknowns, whose preconditioner inverts the jointed system exactly for
        the context's block or diagonal M.  -> (lambda, U, phi, iterations, residual estimate).  phi (3 n_joints) is in the
        convention of F_body: the joints load the bodies with J^T phi, and solve_saddle with F_body + J^T phi returns the same
        lambda and U.  A joint set whose constraints are redundant raises RuntimeError ("redundant").  With the joints off or
        never set this is the plain solve and phi is empty."""
        F, sl, jr = self._jointed_args("solve_jointed", F_body, slip, joint_rhs, "joint_rhs")
        return self.ctx.solve_jointed(F, slip=sl, joint_rhs=jr, max_iter=int(max_iter), rtol=float(rtol))

    def step_jointed(self, F_body, slip=None, joint_velocity=None, gamma=1.0, max_iter=50, rtol=1.0e-8):
        """One deterministic time step with the joints: the force model (bonds included) and the flow model at q^n as in
        step_deterministic, solve_jointed with joint_rhs = -(gamma / dt) gap(q^n) + joint_velocity, then evolve_rigid_bodies(U).
        gamma in [0, 1]: 1 (default) takes the O(dt^2) gap of the explicit rotation update out in the next step, 0 constrains the
        velocities only.  joint_velocity (n_joints, 3) or None: the rate of change asked of p_A - p_B (a pivot moving with v: -v).
        -> (phi, iterations, residual estimate)."""
        F, sl, jv = self._jointed_args("step_jointed", F_body, slip, joint_velocity, "joint_velocity")
        return self.ctx.step_jointed(F, slip=sl, joint_velocity=jv, gamma=float(gamma), max_iter=int(max_iter), rtol=float(rtol))

    def joint_state(self):
        """-> (gaps p_A - p_B of every stored joint at the current configuration (n_joints, 3), phi of the last solve_jointed /
        step_jointed (n_joints, 3); RuntimeError if there has been none with this joint set).  A set given through
        set_joint_kinds -> (gap, phi, theta (n_joints,)): the gap rows of a lock or axis joint hold its angular gap e."""
        return self.ctx.joint_state()

    def interaction_forces(self):
        """The model's body forces and torques at the current configuration, 6 * N_bodies, in the reference convention
        (-K^T f_phys): add them to F in rhs = [0 ; -F] of a solve over apply_saddle."""
        return -self.ctx.interaction_forces()[1]      # the library's are the physical ones, +K^T f

    def interaction_energy(self):
        return self.ctx.interaction_energy()

    def velocity_field(self, points, blob_forces, positions=None, with_flow=False):
        """Fluid velocity at arbitrary points from blob forces (include/rbl.h section 6): the velocity `apply_M` would give an
        extra force-free blob of radius a at each point -- e.g. the flow around the bodies after `solve_saddle`, whose first
        3 * total_blobs entries are the blob forces.  points: (P, 3) or flat 3P; blob_forces: flat or (N, 3); positions: the
        blobs' positions (default: this object's blobs at the current configuration, then blob_forces must have 3 * total_blobs
        entries).  With the wall, points at z <= 0 get u = 0.  with_flow=True adds the background flow u0 + G p of set_background_flow
        (while it is on; with the wall only at points above it), on the host.  Returns (P, 3) or flat, following the shape of `points`."""
        pts = np.asarray(points, dtype=np.float64)
        lam = np.asarray(blob_forces, dtype=np.float64)
        if not (pts.ndim == 2 and pts.shape[1] == 3) and not (pts.ndim == 1 and pts.size % 3 == 0):
            raise ValueError(f"velocity_field: points must have shape (P, 3) or (3P,). Got shape: {pts.shape}")
        if not (lam.ndim == 2 and lam.shape[1] == 3) and not (lam.ndim == 1 and lam.size % 3 == 0):
            raise ValueError(f"velocity_field: blob_forces must have shape (N, 3) or (3N,). Got shape: {lam.shape}")
        if positions is None:
            if lam.size != 3 * self.total_blobs:
                raise ValueError(f"velocity_field: blob_forces must have total size 3*N_blobs = {3 * self.total_blobs}. Got shape: {lam.shape}")
            r = None
        else:
            r = np.asarray(positions, dtype=np.float64)
            if r.size != lam.size:
                raise ValueError(f"velocity_field: positions and blob_forces must be of the same size. Got {r.shape} and {lam.shape}")
            r = r.reshape(-1)
        u = self.ctx.velocity_field(pts.reshape(-1), lam.reshape(-1), r)
        if with_flow:
            m = self.flow_model()
            if m["flow_on"]:
                p = pts.reshape(-1, 3)
                uinf = m["u0"] + p @ m["G"].T
                if self._wall:
                    uinf[p[:, 2] <= 0.0] = 0.0
                u = u + uinf.reshape(-1)
        return u.reshape(pts.shape)

    # ------------------------------------------------------------------ imposed flow, active slip, stresslets (include/rbl.h section 8)
    def set_background_flow(self, u0=None, G=None, on=True):
        """Background flow u_inf(r) = u0 + G r, G[i, j] = d u_i / d x_j (None: zeros).  Every step entry point (step_deterministic,
        step_brownian, step_mixed, step_mixed_dof, step_brownian_mixed) then adds -u_inf at the blobs of q^n to its slip; the bare
        solves do not: pass them slip=flow_slip().  With wall_PC only u = (G[0, 2] z, G[1, 2] z, 0) is accepted -- at the use, not
        here.  on=False switches the flow off."""
        u0 = np.zeros(3) if u0 is None else np.asarray(u0, dtype=np.float64)
        G = np.zeros((3, 3)) if G is None else np.asarray(G, dtype=np.float64)
        if u0.shape != (3,):
            raise ValueError(f"set_background_flow: u0 must have shape (3,). Got shape: {u0.shape}")
        if G.shape != (3, 3):
            raise ValueError(f"set_background_flow: G must have shape (3, 3). Got shape: {G.shape}")
        self.ctx.set_background_flow(u0, np.ascontiguousarray(G), bool(on))

    def set_body_slip(self, slip_body, scale=None, on=True):
        """Active slip carried by the bodies: slip_body (blobs_per_body, 3) or flat, a pattern in the BODY frame in the units and
        sign of the `slip` argument; scale: a factor per body, (N_bodies,) (None: 1; 0: a passive body).  The steps add
        scale_b R(q_b) slip_body to their slip at q^n.  on=False switches it off."""
        sb = np.asarray(slip_body, dtype=np.float64)
        if sb.size != 3 * self.blobs_per_body or not (sb.ndim == 1 or (sb.ndim == 2 and sb.shape[1] == 3)):
            raise ValueError(f"set_body_slip: slip_body must have shape ({self.blobs_per_body}, 3) or ({3 * self.blobs_per_body},). Got shape: {sb.shape}")
        sc = None
        if scale is not None:
            sc = np.asarray(scale, dtype=np.float64)
            if sc.shape != (self.N_bodies,):
                raise ValueError(f"set_body_slip: scale must have shape (N_bodies,) = ({self.N_bodies},). Got shape: {sc.shape}")
            sc = np.ascontiguousarray(sc)
        self.ctx.set_body_slip(np.ascontiguousarray(sb).reshape(-1), sc, bool(on))

    def flow_model(self):
        """{u0 (3,), G (3, 3), flow_on, body_slip_on} of the context's flow model"""
        return self.ctx.flow_model()

    def flow_slip(self):
        """The flow model's term at the current configuration, t_i = scale_b R(q_b) slip_body_i - (u0 + G r_i): what the steps add
        to their slip, and what a bare solve takes as slip=.  Zeros with both parts off.  Shaped like the blob positions."""
        return self._like_X(self.ctx.flow_slip())

    def first_moments(self, lam):
        """D_b = sum_i (r_i - X_b) lambda_i^T over the blobs of each body -> (N_bodies, 3, 3).  lam: any blob vector -- the lambda
        of a solve, or the model's blob forces for the interparticle contribution."""
        lam = np.asarray(lam, dtype=np.float64)
        if lam.size != 3 * self.total_blobs:
            raise ValueError(f"first_moments: lam must have total size 3*N_blobs = {3 * self.total_blobs}. Got shape: {lam.shape}")
        return self.ctx.first_moments(np.ascontiguousarray(lam).reshape(-1)).reshape(self.N_bodies, 3, 3)

    def stresslets(self, lam):
        """The symmetric traceless part of first_moments(lam) -> (N_bodies, 3, 3)"""
        D = self.first_moments(lam)
        S = 0.5 * (D + D.transpose(0, 2, 1))
        return S - np.trace(S, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3.0

    def record_moments(self, on=True):
        """Every step from now on also leaves the first moments of its solve's lambda on the device (one small launch): read them
        with step_moments().  Switching discards what was recorded."""
        self.cb.set_option("record_moments", int(bool(on)))

    def step_moments(self):
        """first moments recorded by the last step, (N_bodies, 3, 3), with the lever arms of the configuration it solved at (q^n
        for the deterministic steps, q^{n+1/2} for the midpoint steps).  The Brownian drift's share of the stress is not in it."""
        return self.ctx.step_moments().reshape(self.N_bodies, 3, 3)

    # ------------------------------------------------------------------ prescribed kinematics (include/rbl.h section 7)
    def _prescribed_mask(self, prescribed):
        """boolean array of N_bodies (dtype bool: the only form read as a mask), or a list of body indices (any integer array,
        0/1 values included) -> uint8 mask; ValueError before the library is called"""
        p = np.asarray(prescribed)
        nb = self.N_bodies
        if p.dtype == np.bool_:
            if p.size != nb:
                raise ValueError(f"prescribed: a boolean array must have N_bodies = {nb} entries. Got shape: {p.shape}")
            return np.ascontiguousarray(p.reshape(-1), dtype=np.uint8)
        if p.size and not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"prescribed must be a boolean array of N_bodies or a list of body indices. Got dtype: {p.dtype}")
        idx = p.reshape(-1).astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= nb):
            raise ValueError(f"prescribed: body indices must lie in [0, {nb})")
        if np.unique(idx).size != idx.size:
            raise ValueError("prescribed: a body index appears twice (integers are body indices; a 0/1 mask must have dtype bool)")
        mask = np.zeros(nb, dtype=np.uint8)
        mask[idx] = 1
        return mask

    def _prescribed_mask6(self, prescribed):
        p = np.asarray(prescribed)
        if p.dtype != np.bool_ or p.shape != (self.N_bodies, 6):
            raise ValueError(f"prescribed must be a boolean array of shape (N_bodies, 6) = ({self.N_bodies}, 6): one entry per velocity "
                             f"component (translation x, y, z, rotation x, y, z). Got dtype {p.dtype}, shape {p.shape}")
        return np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)

    def _mixed_args(self, prescribed, body_in, slip, per=1):
        """per: mask entries per body, 1 (bodies) or 6 (velocity components, the _dof methods)"""
        mask = self._prescribed_mask6(prescribed) if per == 6 else self._prescribed_mask(prescribed)
        return (mask,) + self._body_in_and_slip(body_in, slip)

    def _body_in_and_slip(self, body_in, slip):
        bi = np.asarray(body_in, dtype=np.float64)
        if bi.size != 6 * self.N_bodies:
            raise ValueError(f"body_in must have total size 6*N_bodies = {6 * self.N_bodies}. Got shape: {bi.shape}")
        sl = None
        if slip is not None:
            sl = np.asarray(slip, dtype=np.float64)
            if sl.size != 3 * self.total_blobs:
                raise ValueError(f"slip must have total size 3*N_blobs = {3 * self.total_blobs}. Got shape: {sl.shape}")
            sl = sl.reshape(-1)
        return bi.reshape(-1), sl

    def solve_mixed(self, prescribed, body_in, slip=None, max_iter=100, rtol=1.0e-8):
        """Prescribed kinematics: the bodies in `prescribed` (boolean array of N_bodies, or a list of body indices) move with the
        velocity given in their six slots of body_in (translation, rotation; zeros hold a body), the others are free and carry their
        load F_b there (the convention of step_deterministic's F_body, rhs [slip ; -F]).  ONE GMRES solve on the GPU of the size and
        per-iteration cost of a mobility solve; it takes 2-3.5 times the iterations when a quarter to all of the bodies are
        prescribed.  Only an array of dtype bool is read as a mask: integers are ALWAYS body indices ([0, 1] prescribes bodies 0
        and 1), so convert a 0/1 integer mask with .astype(bool).  -> (lambda, U, F, iterations, residual estimate): blob forces (what velocity_field takes), all
        body velocities (prescribed ones echoed), all body loads (free ones echoed, prescribed ones -K_b^T lambda: the load it takes
        to move them as told)."""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip)
        return self.ctx.solve_mixed(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def step_mixed(self, prescribed, body_in, slip=None, max_iter=50, rtol=1.0e-8):
        """One deterministic time step with prescribed bodies: solve_mixed at the current configuration, then
        evolve_rigid_bodies(U) -- a prescribed body advances by its own velocity, a held one stays.  With the force model on its
        loads are added to the FREE bodies only; the F returned for a prescribed body is the total load everything other than the
        fluid supplies (the model's share included).  -> (F, iterations, residual estimate)"""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip)
        return self.ctx.step_mixed(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def solve_mixed_dof(self, prescribed, body_in, slip=None, max_iter=100, rtol=1.0e-8):
        """Prescribed kinematics per velocity component: `prescribed` is a boolean array of shape (N_bodies, 6) over each body's
        lab-frame components (translation x, y, z, then rotation x, y, z, the order of body_in).  A prescribed component moves with
        the velocity in its slot of body_in (zero holds it), a free one carries its load there: a microroller has its rotation
        prescribed and its translation free, a trapped particle the reverse, a quasi-2D suspension only U_z = 0.  The solver is
        solve_mixed's (1.00-1.05 of its time per iteration at cfg 2 and cfg 3: profiles/prescribed_dof.jsonl), and with whole rows set the results are solve_mixed's.  -> (lambda, U, F, iterations, residual estimate): U
        with the prescribed components echoed, F with the free components echoed and -K^T lambda on the prescribed ones (the force
        or torque along that component that it takes)."""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip, per=6)
        return self.ctx.solve_mixed_dof(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def step_mixed_dof(self, prescribed, body_in, slip=None, max_iter=50, rtol=1.0e-8):
        """One deterministic time step with a mask per velocity component: solve_mixed_dof at the current configuration, then
        evolve_rigid_bodies(U).  With the force model on its loads are added to the FREE components only; the F of a prescribed
        component is the total load along it that everything other than the fluid supplies.  -> (F, iterations, residual estimate)"""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip, per=6)
        return self.ctx.step_mixed_dof(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def _multi_body_in_and_slip(self, body_in, slip):
        bi = np.asarray(body_in)
        if bi.dtype.kind not in "fiu" or bi.ndim != 2 or bi.shape[0] < 1 or bi.shape[1] != 6 * self.N_bodies:
            raise ValueError(f"body_in must be a real array of shape (k, 6*N_bodies) = (k, {6 * self.N_bodies}) with k >= 1: one row per "
                             f"right-hand side. Got dtype {bi.dtype}, shape {bi.shape}")
        sl = None
        if slip is not None:
            sl = np.asarray(slip)
            if sl.dtype.kind not in "fiu" or sl.shape != (bi.shape[0], 3 * self.total_blobs):
                raise ValueError(f"slip must be a real array of shape (k, 3*N_blobs) = ({bi.shape[0]}, {3 * self.total_blobs}). "
                                 f"Got dtype {sl.dtype}, shape {sl.shape}")
            sl = np.ascontiguousarray(sl, dtype=np.float64)
        return np.ascontiguousarray(bi, dtype=np.float64), sl

    def solve_mixed_multi(self, prescribed, body_in, slip=None, max_iter=100, rtol=1.0e-8):
        """solve_mixed for k right-hand sides under ONE mask, in lock step: body_in has shape (k, 6 N_bodies), slip is None or
        (k, 3 N_blobs), `prescribed` is read exactly as solve_mixed reads it.  The k GMRES recurrences advance together (16 a batch):
        one multi-vector mobility product per iteration on the fp64 matrix cores, shared passes over the per-body factors, one launch
        of each masked kernel for all columns; a column stops when it has converged, and each column's iterates are those of
        solve_mixed on it alone up to the rounding of the product (16 columns at cfg 3: a third of the sequential loop's time).
        -> (lambda (k, 3 N_blobs), U (k, 6 N_bodies), F (k, 6 N_bodies), iterations (k,), residual estimates (k,))"""
        mask = self._prescribed_mask(prescribed)
        bi, sl = self._multi_body_in_and_slip(body_in, slip)
        return self.ctx.solve_mixed_multi(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def solve_mixed_dof_multi(self, prescribed, body_in, slip=None, max_iter=100, rtol=1.0e-8):
        """solve_mixed_dof for k right-hand sides under ONE mask per velocity component (a boolean array of shape (N_bodies, 6)), in
        lock step as solve_mixed_multi: body_in (k, 6 N_bodies), slip None or (k, 3 N_blobs).
        -> (lambda (k, 3 N_blobs), U (k, 6 N_bodies), F (k, 6 N_bodies), iterations (k,), residual estimates (k,))"""
        mask = self._prescribed_mask6(prescribed)
        bi, sl = self._multi_body_in_and_slip(body_in, slip)
        return self.ctx.solve_mixed_dof_multi(mask, bi, slip=sl, max_iter=int(max_iter), rtol=float(rtol))

    def _noise_arg(self, W):
        if W is None:
            return None
        W = np.asarray(W, dtype=np.float64)
        if W.size != 9 * self.total_blobs:
            raise ValueError(f"W must have total size 9*N_blobs = {9 * self.total_blobs} (W1 | W2 | W_rfd). Got shape: {W.shape}")
        return np.ascontiguousarray(W.reshape(-1))

    def RHS_and_Midpoint_mixed(self, prescribed, body_in, slip=None, W=None, seed=0, method="cholesky", split_rand=True, delta=1.0e-4):
        """Right-hand side and predictor of the Brownian midpoint step with prescribed bodies (include/rbl.h section 7):
        s = slip - kBT M_RFD - BI with the RFD direction masked to the free bodies, and q^{n+1/2}: a free body displaced by
        (dt/2) c1 Kinv M^{1/2}W1, a prescribed one by (dt/2) U_p.  Of body_in only the prescribed bodies' velocities are read.
        Nothing is committed.  -> (s, X_half, Q_half)"""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip)
        W = self._noise_arg(W)
        return self.ctx.RHS_and_Midpoint_mixed(mask, bi, slip=sl, W=W, seed=int(seed), method=method, split_rand=bool(split_rand), delta=float(delta))

    def step_brownian_mixed(self, prescribed, body_in, slip=None, W=None, seed=0, method="lanczos_pc", split_rand=True, delta=1.0e-4,
                            max_iter=50, rtol=1.0e-8):
        """One stochastic midpoint step with prescribed bodies: the bodies in `prescribed` (as solve_mixed reads it) are held or
        driven with the velocity in their slots of body_in, the others are Brownian under their loads: RHS_and_Midpoint_mixed at
        q^n, solve_mixed at q^{n+1/2}, update from q^n -- a prescribed body advances by exactly dt U_p.  The free bodies' velocity
        has the covariance (2 kBT/dt) (K_f^T M^-1 K_f)^-1 and the drift kBT div of it.  The force model enters the free bodies
        only, at q^n.  The F returned for a prescribed body is its instantaneous load, thermal part included: average it over
        steps for a microrheology measurement.  kBT = 1 as in step_brownian.  -> (F, iterations, residual estimate)"""
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip)
        W = self._noise_arg(W)
        return self.ctx.step_brownian_mixed(mask, bi, slip=sl, W=W, seed=int(seed), method=method, split_rand=bool(split_rand),
                                            delta=float(delta), max_iter=int(max_iter), rtol=float(rtol))

    def _brownian_dof_args(self, who, prescribed, body_in, slip):
        mask, bi, sl = self._mixed_args(prescribed, body_in, slip, per=6)
        check_brownian_mask6(who, mask, self.N_bodies)
        return mask, bi, sl

    def RHS_and_Midpoint_mixed_dof(self, prescribed, body_in, slip=None, W=None, seed=0, method="cholesky", split_rand=True, delta=1.0e-4):
        """RHS_and_Midpoint_mixed with a mask per velocity component (boolean, shape (N_bodies, 6), as solve_mixed_dof takes it) in
        which every body's three rotation entries are all False or all True: s = slip - kBT M_RFD - BI with the RFD direction
        D_f Kinv W_rfd, and q^{n+1/2} = q^n displaced by D_f (dt/2) c1 Kinv M^{1/2}W1 + D_p (dt/2) U_p, component by component.
        Nothing is committed.  -> (s, X_half, Q_half)"""
        mask, bi, sl = self._brownian_dof_args("RHS_and_Midpoint_mixed_dof", prescribed, body_in, slip)
        W = self._noise_arg(W)
        return self.ctx.RHS_and_Midpoint_mixed_dof(mask, bi, slip=sl, W=W, seed=int(seed), method=method, split_rand=bool(split_rand), delta=float(delta))

    def step_brownian_mixed_dof(self, prescribed, body_in, slip=None, W=None, seed=0, method="lanczos_pc", split_rand=True, delta=1.0e-4,
                                max_iter=50, rtol=1.0e-8):
        """One stochastic midpoint step with prescribed velocity components: a quasi-2D Brownian layer (U_z = 0 for every body), a
        trapped probe held in place and free to turn, a microroller with Omega imposed whose translation diffuses.  `prescribed` is
        a boolean array of shape (N_bodies, 6) as step_mixed_dof takes it, with ONE restriction: a body's three rotation entries
        are all False or all True.  Then the free components are a subset of the coordinates (translations are Cartesian, a whole
        rotation is treated as the all-free step treats it, and K^T K has no translation-rotation coupling), and the argument of
        step_brownian_mixed carries over: the free components' velocity has the covariance (2 kBT/dt) Ntilde with
        Ntilde = ((K D_f)^T M^-1 K D_f)^-1 and the drift kBT div Ntilde over the free coordinates.  A partly prescribed rotation
        is a ValueError naming the body: nobody has derived its drift.  RHS_and_Midpoint_mixed_dof at q^n, solve_mixed_dof at
        q^{n+1/2}, update from q^n -- a prescribed component advances by exactly dt U_p.  The force model loads the free components
        only, at q^n.  With whole rows the results are step_brownian_mixed's, bit for bit.  -> (F, iterations, residual estimate)"""
        mask, bi, sl = self._brownian_dof_args("step_brownian_mixed_dof", prescribed, body_in, slip)
        W = self._noise_arg(W)
        return self.ctx.step_brownian_mixed_dof(mask, bi, slip=sl, W=W, seed=int(seed), method=method, split_rand=bool(split_rand),
                                                delta=float(delta), max_iter=int(max_iter), rtol=float(rtol))

    def body_resistance_matrix(self, max_iter=100, rtol=1.0e-8, columns=None, lock_step=False):
        """The (6 N_bodies) x (6 N_bodies) body resistance matrix R = N^-1 of the current configuration, the inverse of
        `body_mobility_matrix` (symmetric positive definite): the PHYSICAL loads that move the bodies with velocities U are R U.
        Every body prescribed, one solve_mixed per unit velocity (one after the other).  The F of solve_mixed follows the reference
        convention of step_deterministic's F_body (rhs [slip ; -F], U = -N F), so a column here is -F.  columns: only these
        unit velocities (default all).  lock_step=True: the unit velocities go through solve_mixed_multi, 16 columns advancing
        together; the columns agree with the default's to the solves' tolerance, not bit for bit.  -> (R[:, columns], iterations)"""
        nb6 = 6 * self.N_bodies
        cols = np.arange(nb6) if columns is None else np.asarray(columns, dtype=int).reshape(-1)
        everyone = np.ones(self.N_bodies, dtype=bool)
        if lock_step:
            if cols.size == 0:
                return np.zeros((nb6, 0)), np.zeros(0, dtype=int)
            U = np.zeros((cols.size, nb6))
            U[np.arange(cols.size), cols] = 1.0
            _, _, F, its, _ = self.solve_mixed_multi(everyone, U, max_iter=max_iter, rtol=rtol)
            return -np.ascontiguousarray(F.T), np.asarray(its, dtype=int)
        R, its = np.zeros((nb6, cols.size)), np.zeros(cols.size, dtype=int)
        for j, c in enumerate(cols):
            U = np.zeros(nb6)
            U[c] = 1.0
            _, _, F, its[j], _ = self.solve_mixed(everyone, U, max_iter=max_iter, rtol=rtol)
            R[:, j] = -F
        return R, its

    def apply_M_multi(self, forces, positions):
        """k right-hand sides at once, forces (k, 3N); k >= 4 runs on the fp64 matrix cores."""
        return self.cb.apply_M_multi(np.atleast_2d(np.asarray(forces)), np.asarray(positions).reshape(-1))

    def dense_mobility(self, positions, scale_damp=False):
        """rotne_prager_tensor (reference :413-459) as a dense (3N, 3N) array."""
        return self.cb.rotne_prager_tensor(np.asarray(positions).reshape(-1), scale_damp)
