"""The periodic cell of include/rbl.h section 10 on the GPU, against tests/periodic_oracle.py (the definition restated in numpy on
the CPU oracle's pair block): the product, lattice translations, "off is off", the solves against dense numpy solves with M_per,
the Lanczos root and the drift term, the minimum-image force model, and every refusal with its message.

Tolerances are the project's own for the same comparison in the open system: relative L2 <= 1e-12 for a product against the
oracle (tests/test_gpu_parity.py), 1e-7 for a solve to rtol 1e-10 against the dense solve (tests/test_prescribed_gpu.py,
tests/test_joints_gpu.py), the Lanczos tolerance's 1e-7 for the root and 1e-7 for the difference quotient M_RFD
(tests/test_gpu_parity.py).  Iteration counts are printed (run with -s) and asserted only as "converged within max_iter"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_oracle as jo  # noqa: E402
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ETA = 1.0


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _body(c, block=False, dt=0.01):
    from rigid_body_light_amd import RigidBody
    return RigidBody(c["cfg"], c["X"], c["Q"], c["a"], ETA, dt, wall_PC=True, block_PC=block)


@pytest.fixture(scope="module")
def ten(orc):
    """10 x shell_N_12 in a cell of three lattice spacings by three plus 0.7, and its dense B M_per B for images (1, 1) and (2, 1)
    and, with y open, (1, 0): computed once, shared, never written to"""
    c = pc.layer10()
    B = orc.damp(c["r"].reshape(-1), c["a"])
    T = po.image_terms(orc, c["r"], c["a"], ETA, c["L"], (2, 1))
    Lx0 = (c["L"][0], 0.0)
    c["M"] = {(c["L"], (1, 1)): po.truncated(T, (1, 1), B), (c["L"], (2, 1)): po.truncated(T, (2, 1), B),
              (Lx0, (1, 0)): po.dense_M(orc, c["r"], c["a"], ETA, Lx0, (1, 0))}
    from oracle import oracle as O
    c["K"] = O.K_matrix(c["X"], O.normalize_quats(c["Q"]), O.remove_mean(c["cfg"]))
    for m in c["M"].values():
        m.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------ 1: the product
def _products(rb, F, r):
    """the product with the column split left to the heuristic, at 1 and forced above 1 (the option is a request: a system of one
    column tile has nothing to split)"""
    out = []
    for js in (0, 1, 3):
        rb.cb.set_option("ordered_jsplit", js)
        out.append(rb.apply_M(F, r))
    rb.cb.set_option("ordered_jsplit", 0)
    return out


def test_product_against_M_per_one_ragged_tile(ten):
    rb = _body(ten)
    r = rb.get_blob_positions().reshape(-1)
    assert np.abs(r - ten["r"].reshape(-1)).max() <= 1e-14
    F = np.random.default_rng(2).standard_normal(r.size)
    for (L, n), M in ten["M"].items():
        rb.set_periodic(L[0], L[1], images=n)
        ref = M @ F
        for U in _products(rb, F, r):
            print("10 x 12, cell %.3f x %.3f, images %s: rel. error %.2e" % (L[0], L[1], n, _rel(U, ref)))
            assert _rel(U, ref) <= 1e-12
        assert np.array_equal(rb.apply_M(F, r), rb.apply_M(F, r))              # one summation order
    open_U = _body(ten).apply_M(F, r)
    assert _rel(open_U, ten["M"][(ten["L"], (1, 1))] @ F) > 1e-2               # the neighbours across the boundary do count


def test_row_range_of_the_device_entry_point(ten):
    import torch
    rb = _body(ten)
    rb.set_periodic(*ten["L"], images=(1, 1))
    N = 120
    dev = torch.device("cuda:0")
    F = np.random.default_rng(4).standard_normal(3 * N)
    dF, dr = torch.from_numpy(F).to(dev), torch.from_numpy(ten["r"].reshape(-1).copy()).to(dev)
    ref = ten["M"][(ten["L"], (1, 1))] @ F
    for b, e in ((0, N), (37, 101), (119, 120)):
        out = torch.full((3 * N,), -7.0, dtype=torch.float64, device=dev)
        rb.ctx.apply_M(dF.data_ptr(), dr.data_ptr(), N, b, e, out.data_ptr())
        rb.ctx.sync_check()
        got = out.cpu().numpy()
        assert _rel(got[:3 * (e - b)], ref[3 * b:3 * e]) <= 1e-12 and np.all(got[3 * (e - b):] == -7.0)


def test_product_two_column_tiles_sampled_rows(orc):
    """3 x shell_N_162: 486 blobs, two column tiles, the second ragged (230 of 256); 16 sampled rows, the tile boundary among them;
    the column split at 1 and at 2; a row range across the tile boundary"""
    import torch
    from rigid_body_light_amd import make_config
    c = make_config(3, 162, True)
    s = pc.spacing(c["a"])
    L = (2.0 * s, 2.0 * s + 0.7)
    rb = _body(c)
    rb.set_periodic(L[0], L[1], images=(1, 1))
    r = rb.get_blob_positions().reshape(-1)
    N = r.size // 3
    assert N == 486
    F = np.random.default_rng(6).standard_normal(r.size)
    which = [0, 1, 100, 161, 162, 254, 255, 256, 257, 300, 323, 324, 400, 470, 484, 485]
    ref = po.rows(orc, r, which, c["a"], ETA, L, (1, 1)) @ F
    idx = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in which])
    for U in _products(rb, F, r):
        print("3 x 162, 16 sampled rows: rel. error %.2e" % _rel(U[idx], ref))
        assert _rel(U[idx], ref) <= 1e-12
    dev = torch.device("cuda:0")
    dF, dr = torch.from_numpy(F).to(dev), torch.from_numpy(r.copy()).to(dev)
    b, e = 250, 301
    out = torch.empty(3 * (e - b), dtype=torch.float64, device=dev)
    rb.ctx.apply_M(dF.data_ptr(), dr.data_ptr(), N, b, e, out.data_ptr())
    rb.ctx.sync_check()
    inside = [k for k, i in enumerate(which) if b <= i < e]
    got = out.cpu().numpy().reshape(-1, 3)[[which[k] - b for k in inside]].reshape(-1)
    assert len(inside) == 5 and _rel(got, ref.reshape(-1, 3)[inside].reshape(-1)) <= 1e-12


def test_one_body_alone_sees_its_own_images(orc):
    from rigid_body_light_amd import make_config
    c = make_config(1, 12, True)
    s = pc.spacing(c["a"])
    r = pc.blob_positions(c["cfg"], c["X"], c["Q"])
    F = np.random.default_rng(7).standard_normal(r.size)
    rb = _body(c)
    U_open = rb.apply_M(F, r.reshape(-1))
    for L, n in (((s, s + 0.7), (1, 1)), ((s, s + 0.7), (2, 3)), ((0.0, s), (0, 2))):
        rb.set_periodic(L[0], L[1], images=(max(n[0], 1), n[1]))
        ref = po.dense_M(orc, r, c["a"], ETA, L, n) @ F
        for U in _products(rb, F, r.reshape(-1)):
            print("one body, cell %.2f x %.2f, images %s: rel. error %.2e, against the open system %.2e" % (L[0], L[1], n, _rel(U, ref), _rel(U, U_open)))
            assert _rel(U, ref) <= 1e-12 and _rel(U, U_open) > 1e-2


def test_overlap_only_through_the_boundary(orc):
    """two bodies whose blobs come closer than 2a only through the boundary: the overlap branch of the pair arithmetic is taken for
    the nearest image and for nothing else"""
    from rigid_body_light_amd import make_config
    c = make_config(2, 12, True)
    a = c["a"]
    L = (10.0, 9.0)
    c["X"][0] = [1.0, 0.5, 2.0]
    sep = 2.6
    while True:                                                   # approach through the x boundary until two blobs overlap
        c["X"][1] = [1.0 + L[0] - sep, 0.5 + 2.0 * L[1], 2.1]     # (and two cells away in y)
        r = pc.blob_positions(c["cfg"], c["X"], c["Q"])
        d = np.linalg.norm(po.nearest(r[:12, None, :] - r[None, 12:, :], L), axis=2)
        if d.min() < 1.6 * a:
            break
        sep -= 0.02
    direct = np.linalg.norm(r[:12, None, :] - r[None, 12:, :], axis=2)
    print("closest pair through the boundary %.3f a, directly %.1f a" % (d.min() / a, direct.min() / a))
    assert 0.3 * a < d.min() < 2.0 * a and direct.min() > 10.0 * a
    rb = _body(c)
    rb.set_periodic(L[0], L[1], images=(1, 2))
    F = np.random.default_rng(8).standard_normal(r.size)
    ref = po.dense_M(orc, r, a, ETA, L, (1, 2)) @ F
    for U in _products(rb, F, r.reshape(-1)):
        assert _rel(U, ref) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 2: translations
def _shifts(L, nb):
    """whole cell vectors, different for different bodies, both signs; at most 2 cells: |shift| <= 2 x 10.7 < 100 a = 41.6"""
    k = np.array([[0, 0], [1, 0], [-1, 2], [0, -2], [2, 1], [-2, -1], [1, -1], [0, 1], [-1, 0], [2, -2]])[:nb]
    return np.concatenate([k * np.array(L), np.zeros((nb, 1))], axis=1)


def test_lattice_translations_leave_the_product_and_the_forces_alone(ten):
    """bodies moved by whole cell vectors: the product changes by the rounding of the larger coordinates only (DESIGN.md 5a:
    4.5e-14 at 100 a for the coordinate scaling), the force model's output likewise"""
    L = ten["L"]
    rb = _body(ten)
    rb.set_periodic(L[0], L[1], images=(1, 1))
    rb.set_interactions(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)   # 2 R_body + r_cut = 3.6 <= L / 2
    F = np.random.default_rng(9).standard_normal(360)
    U0 = rb.apply_M(F, ten["r"].reshape(-1))
    f0, FT0 = rb.ctx.interaction_forces()
    sh = _shifts(L, 10)
    assert np.abs(sh).max() <= 100.0 * ten["a"] and (sh > 0).any() and (sh < 0).any()
    X1 = ten["X"] + sh
    r1 = pc.blob_positions(ten["cfg"], X1, ten["Q"])
    U1 = rb.apply_M(F, r1.reshape(-1))
    print("product after lattice translations: rel. change %.2e" % _rel(U1, U0))
    assert _rel(U1, U0) <= 1e-12
    rb.set_config(X1, ten["Q"])
    f1, FT1 = rb.ctx.interaction_forces()
    print("forces after lattice translations: rel. change %.2e (blobs) %.2e (bodies)" % (_rel(f1, f0), _rel(FT1, FT0)))
    assert np.abs(f0).max() > 0.1 and _rel(f1, f0) <= 1e-12 and _rel(FT1, FT0) <= 1e-12
    X, _ = rb.get_config()
    assert np.array_equal(np.asarray(X).reshape(-1, 3), X1)       # coordinates are never wrapped


# ------------------------------------------------------------------------------------------------------------ 3: off is off
@pytest.mark.parametrize("block", [False, True])
def test_a_cell_that_is_off_changes_no_bit(ten, block):
    rng = np.random.default_rng(10)
    F, Fb, slip = rng.standard_normal(360), rng.standard_normal(60), 0.1 * rng.standard_normal(360)
    out = []
    for with_cell in (False, True):
        rb = _body(ten, block)
        rb.set_interactions(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)
        if with_cell:
            rb.set_periodic(ten["L"][0], ten["L"][1], images=(2, 1), on=False)
            assert rb.periodic() == dict(on=False, Lx=ten["L"][0], Ly=ten["L"][1], images=(2, 1))
        U = rb.apply_M(F, ten["r"].reshape(-1))
        x, its, res = rb.solve_saddle(np.concatenate([slip, -Fb]), max_iter=200, rtol=1e-10)
        f, FT = rb.ctx.interaction_forces()
        its_s, res_s = rb.step_deterministic(Fb, slip=slip, max_iter=200, rtol=1e-10)
        X, Q = rb.get_config()
        out.append((U, x, its, res, f, FT, its_s, res_s, np.array(X), np.array(Q)))
    for p, q in zip(*out):
        assert np.array_equal(p, q)


# ------------------------------------------------------------------------------------------------------------ 4: the solves
@pytest.mark.parametrize("block", [False, True])
def test_solves_against_the_dense_solve_with_M_per(orc, ten, block):
    from oracle import oracle as O
    L, n = ten["L"], (1, 1)
    M, K = ten["M"][(L, n)], ten["K"]
    n3, nb6 = 360, 60
    rng = np.random.default_rng(11)
    Fb, slip = rng.standard_normal(nb6), 0.1 * rng.standard_normal(n3)
    A = np.block([[M, -K], [K.T, np.zeros((nb6, nb6))]])
    rb = _body(ten, block)
    rb.set_periodic(L[0], L[1], images=n)
    # solve_saddle
    xd = np.linalg.solve(A, np.concatenate([slip, -Fb]))
    x, its, res = rb.solve_saddle(np.concatenate([slip, -Fb]), max_iter=200, rtol=1e-10)
    print("solve_saddle block=%s: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e" % (block, its, res, _rel(x[:n3], xd[:n3]), _rel(x[n3:], xd[n3:])))
    assert 0 < its < 200 and res < 1e-10 and _rel(x[:n3], xd[:n3]) <= 1e-7 and _rel(x[n3:], xd[n3:]) <= 1e-7
    # one mask per velocity component
    P = np.zeros((10, 6), dtype=bool)
    P[:, 3:] = rng.random((10, 1)) < 0.5
    P[[1, 4], :3] = True
    Up = rng.standard_normal((10, 6))
    free = ~P.reshape(-1)
    Kf, Kp = K[:, free], K[:, ~free]
    nf = Kf.shape[1]
    xm = np.linalg.solve(np.block([[M, -Kf], [Kf.T, np.zeros((nf, nf))]]),
                         np.concatenate([slip + Kp @ Up.reshape(-1)[~free], -Fb[free]]))
    U_d = Up.reshape(-1).copy(); U_d[free] = xm[n3:]
    F_d = Fb.copy(); F_d[~free] = -(Kp.T @ xm[:n3])
    lam, U, Fo, its, res = rb.solve_mixed_dof(P, np.where(P, Up, Fb.reshape(10, 6)).reshape(-1), slip=slip, max_iter=200, rtol=1e-10)
    print("solve_mixed_dof block=%s: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e F %.2e"
          % (block, its, res, _rel(lam, xm[:n3]), _rel(U, U_d), _rel(Fo, F_d)))
    assert 0 < its < 200 and res < 1e-10 and _rel(lam, xm[:n3]) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(Fo, F_d) <= 1e-7
    # one joint set
    body, anchor = jo.chain_set(10, ten["X"], seed=12)
    rb.set_joints(body, anchor[:, :3], anchor[:, 3:])
    crhs = rng.standard_normal(3 * body.shape[0])
    J = jo.J_matrix(ten["X"], ten["Q"], body, anchor)
    lam_d, U_d, phi_d = jo.dense_jointed(M, K, J, Fb, slip, crhs)
    lam, U, phi, its, res = rb.solve_jointed(Fb, slip=slip, joint_rhs=crhs, max_iter=200, rtol=1e-10)
    print("solve_jointed block=%s: %d iterations, residual %.2e, rel. diff lambda %.2e U %.2e phi %.2e"
          % (block, its, res, _rel(lam, lam_d), _rel(U, U_d), _rel(phi, phi_d)))
    assert 0 < its < 200 and res < 1e-10 and _rel(lam, lam_d) <= 1e-7 and _rel(U, U_d) <= 1e-7 and _rel(phi, phi_d) <= 1e-7
    rb.set_joints(None, None, None, on=False)
    # step_deterministic moves the bodies with the dense solution
    Xo, Qo = O.evolve(ten["X"], O.normalize_quats(ten["Q"]), xd[n3:], 0.01)
    its, res = rb.step_deterministic(Fb, slip=slip, max_iter=200, rtol=1e-10)
    X1, Q1 = rb.get_config()
    print("step_deterministic block=%s: %d iterations, residual %.2e" % (block, its, res))
    assert 0 < its < 200 and res < 1e-10
    assert np.abs(np.asarray(X1).reshape(-1, 3) - Xo).max() <= 1e-7 and np.abs(np.asarray(Q1).reshape(-1, 4) - Qo).max() <= 1e-7


# ------------------------------------------------------------------------------------------------------------ 5: roots and drift
def test_lanczos_root_against_the_eigh_root_of_M_per(ten):
    L, n = ten["L"], (1, 1)
    M = ten["M"][(L, n)]
    rb = _body(ten)
    rb.set_periodic(L[0], L[1], images=n)
    rb.cb.set_lanczos(200, 1e-9)
    W = np.random.default_rng(3).standard_normal(360)
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    assert lam.min() > 0.0                                        # (tests/test_periodic_cpu.py records the value)
    ref = V @ (np.sqrt(lam) * (V.T @ W))
    out = rb.M_half_W(W, method="lanczos")
    it, res = rb.cb.lanczos_report()
    print("Lanczos root: %d iterations, estimate %.2e, rel. error %.2e" % (it, res, _rel(out, ref)))
    assert 2 <= it <= 200 and res < 1e-9 and _rel(out, ref) < 1e-7
    out_pc = rb.M_half_W(W, method="lanczos_pc")                  # a different, equally exact root: its square is M W
    again = rb.M_half_W(W, method="lanczos_pc")
    assert np.array_equal(out_pc, again) and np.isfinite(out_pc).all()


def test_M_RFD_against_its_formula_on_M_per(orc):
    """(1 / delta) [M_per(q + delta / 2 Kinv W) - M_per(q - delta / 2 Kinv W)] W; the quotient amplifies the product's 1e-15 by
    1 / delta = 1e4, the bound is that of the open-system test"""
    from oracle import oracle as O
    from rigid_body_light_amd import make_config
    c = make_config(4, 12, True)
    L, n, delta = (7.0, 7.5), (1, 1), 1e-4
    rb = _body(c)
    rb.set_periodic(L[0], L[1], images=n)
    W = np.random.default_rng(13).standard_normal(144)
    cfg, Qn = O.remove_mean(c["cfg"]), O.normalize_quats(c["Q"])
    uom = O.Kinv_matrix(c["X"], Qn, cfg) @ W
    side = []
    for s in (0.5, -0.5):
        Xs, Qs = O.update_X_Q(c["X"], Qn, s * delta * uom)
        side.append(po.dense_M(orc, orc.multi_body_pos(Xs, Qs, cfg), c["a"], ETA, L, n) @ W)
    ref = (side[0] - side[1]) / delta
    out = rb.M_RFD(W, delta=delta)
    print("M_RFD: rel. error %.2e" % _rel(out, ref))
    assert _rel(out, ref) < 1e-7
    X1, _ = rb.get_config()
    assert np.allclose(np.asarray(X1).reshape(-1, 3), c["X"])


def test_two_brownian_steps_with_one_seed_give_the_same_bits(ten):
    rng = np.random.default_rng(14)
    Fb = rng.standard_normal(60)
    ends = []
    for _ in range(2):
        rb = _body(ten, block=True, dt=1e-3)
        rb.set_periodic(ten["L"][0], ten["L"][1], images=(1, 1))
        got = rb.step_brownian(Fb, seed=77, method="lanczos_pc", max_iter=200, rtol=1e-8)
        X, Q = rb.get_config()
        ends.append((np.array(X), np.array(Q)))
        print("step_brownian:", got)
    assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1])
    assert np.abs(ends[0][0].reshape(-1, 3) - ten["X"]).max() > 0.0 and np.isfinite(ends[0][0]).all()


# ------------------------------------------------------------------------------------------------------------ 6: the force model
FORCE_CELL = (12.0, 11.0)


def _across():
    """three bodies further apart than every cutoff in the open system and neighbours through the boundaries of a 12 x 11 cell"""
    from rigid_body_light_amd import make_config
    c = make_config(3, 12, True)
    c["X"] = np.array([[0.5, 0.3, 2.0], [FORCE_CELL[0] - 2.3, 0.1, 2.2], [0.7, FORCE_CELL[1] - 2.5, 2.4]])
    return c


def test_pair_forces_by_minimum_image(orc):
    from oracle import oracle as O
    c = _across()
    a, L = c["a"], FORCE_CELL
    r = pc.blob_positions(c["cfg"], c["X"], c["Q"])
    lever = (r.reshape(3, 12, 3) - c["X"][:, None, :])
    grid = np.linspace(0.5, 2.5, 41)
    tabU, tabdU = 0.4 * np.exp(-grid) * np.cos(3.0 * grid), 0.4 * np.exp(-grid) * (-np.cos(3.0 * grid) - 3.0 * np.sin(3.0 * grid))
    steric = (1.5, 0.1, 2.0 * a + 2.0)
    m_body = np.array([[0.3, -0.2, 1.0], [1.0, 0.1, 0.2], [-0.4, 0.9, 0.3]])
    m_lab = np.array([O.rot_matrix(q) @ m for q, m in zip(O.normalize_quats(c["Q"]), m_body)])

    def model(rb, which):
        rb.set_interactions(eps_blob=steric[0], b_blob=steric[1], r_cut=steric[2], on=which == "steric")
        if which == "table":
            rb.set_pair_table(tabU, tabdU, 0.5, 2.5)
        if which == "dipoles":
            rb.set_dipoles(m_body, c_dd=0.8, r_core=1.0, r_cut=5.0)

    for which in ("steric", "table", "dipoles"):
        rb = _body(c)
        model(rb, which)
        f_open, FT_open = rb.ctx.interaction_forces()
        assert not f_open.any() and not FT_open.any()             # the open system: exactly zero
        rb.set_periodic(L[0], L[1], images=(1, 1))
        f, FT = rb.ctx.interaction_forces()
        E = rb.ctx.interaction_energy()
        if which == "dipoles":
            FT_ref, E_ref = po.dipole_pairs(c["X"], m_lab, 0.8, 1.0, 5.0, L)
            assert not f.any()
        else:
            f_ref, E_ref = po.pair_forces(r, 12, a, L, steric=steric if which == "steric" else None,
                                          table=(tabU, tabdU, 0.5, 2.5) if which == "table" else None)
            FT_ref = po.KT(f_ref.reshape(3, 12, 3), lever)
            assert _rel(f, f_ref) <= 1e-12
        print("%s through the boundary: |FT| %.3e, rel. error %.2e, energy %.6e against %.6e" % (which, np.abs(FT_ref).max(), _rel(FT, FT_ref), E, E_ref))
        assert np.abs(FT_ref).max() > 1e-3 and _rel(FT, FT_ref) <= 1e-12 and abs(E - E_ref) <= 1e-12 * abs(E_ref)
        f2, FT2 = rb.ctx.interaction_forces()
        assert np.array_equal(f, f2) and np.array_equal(FT, FT2)  # bitwise reproducible
        # a cell too small for a unique minimum image: refused, naming the length and the bound; the context stays usable
        rb.set_periodic(8.0, L[1], images=(1, 1))
        with pytest.raises(RuntimeError, match=r"periodic cell too small: Lx = 8\.0.*<= L / 2 = 4\.0"):
            rb.ctx.interaction_forces()
        rb.set_periodic(L[0], L[1], images=(1, 1))
        assert np.array_equal(rb.ctx.interaction_forces()[1], FT)


# ------------------------------------------------------------------------------------------------------------ 7: the refusals
def _abi():
    L = C.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))   # its own function objects: argtypes set here stay here
    vp, dbl, i32, i64, u64 = C.c_void_p, C.c_double, C.c_int, C.c_int64, C.c_uint64
    L.rbl_last_error.restype = C.c_char_p
    L.rbl_last_error.argtypes = [vp]
    sig = dict(rbl_rotne_prager_tensor=[vp, vp, i64, i32, vp], rbl_rotne_prager_tensor_dev=[vp, vp, i64, i32, vp],
               rbl_M_half_W=[vp, vp, u64, i32, vp], rbl_M_half_W_r=[vp, vp, i64, vp, u64, i32, vp], rbl_M_half_W_dev=[vp, vp, i64, vp, i32, vp],
               rbl_apply_M_sym_dev=[vp, vp, vp, i64, i32, i32, vp], rbl_apply_M_sym_multi_dev=[vp, vp, vp, i64, i32, i32, i32, vp],
               rbl_velocity_field=[vp, vp, i64, vp, vp, i64, vp], rbl_velocity_field_dev=[vp, vp, i64, vp, vp, i64, vp],
               rbl_ensemble_set_config=[vp, i32, i32, vp, vp], rbl_ensemble_get_config=[vp, vp, vp], rbl_ensemble_config_dev=[vp, vp, vp],
               rbl_ensemble_step_deterministic=[vp, vp, vp, i32, dbl, vp, vp],
               rbl_ensemble_step_brownian=[vp, vp, vp, vp, u64, i32, dbl, i32, dbl, vp, vp],
               rbl_ensemble_interaction_forces=[vp, vp, vp], rbl_ensemble_flow_slip=[vp, vp], rbl_ensemble_step_moments=[vp, vp],
               rbl_ensemble_bond_state=[vp, vp, vp, vp], rbl_ensemble_run=[vp, vp, vp],
               rbl_ensemble_solve_mixed=[vp, vp, vp, vp, i32, dbl, vp, vp, vp, vp, vp],
               rbl_ensemble_solve_mixed_dof=[vp, vp, vp, vp, i32, dbl, vp, vp, vp, vp, vp],
               rbl_ensemble_step_mixed=[vp, vp, vp, vp, i32, dbl, vp, vp, vp], rbl_ensemble_step_mixed_dof=[vp, vp, vp, vp, i32, dbl, vp, vp, vp],
               rbl_ensemble_step_brownian_mixed=[vp, vp, vp, vp, vp, u64, i32, dbl, i32, dbl, vp, vp, vp],
               rbl_ensemble_step_brownian_mixed_dof=[vp, vp, vp, vp, vp, u64, i32, dbl, i32, dbl, vp, vp, vp])
    for name, args in sig.items():
        getattr(L, name).argtypes = args
    return L


def test_every_refusal_has_its_message_and_leaves_the_context_usable(ten):
    import torch
    from rigid_body_light_amd._lib import RunOpts, RunOut
    ERR_STATE = 7
    Lc, n = ten["L"], (1, 1)
    rb = _body(ten)
    rb.set_periodic(Lc[0], Lc[1], images=n)
    F = np.random.default_rng(15).standard_normal(360)
    ref = ten["M"][(Lc, n)] @ F
    r = ten["r"].reshape(-1).copy()
    h, L = rb.ctx.h, _abi()
    N = 120
    big = np.zeros(360 * 360)
    hp = big.ctypes.data                                          # room enough for any host output, should a call not refuse
    dev = torch.device("cuda:0")
    dbuf = torch.zeros(360 * 360, dtype=torch.float64, device=dev)
    dptr = dbuf.data_ptr()
    o, out = RunOpts(), RunOut()
    o.size, out.size = C.sizeof(RunOpts), C.sizeof(RunOut)
    calls = [("rbl_rotne_prager_tensor", (r.ctypes.data, 360, 1, hp)), ("rbl_rotne_prager_tensor_dev", (dptr, N, 1, dptr)),
             ("rbl_M_half_W", (hp, 0, 0, hp)), ("rbl_M_half_W_r", (r.ctypes.data, 360, hp, 0, 0, hp)), ("rbl_M_half_W_dev", (dptr, N, dptr, 0, dptr)),
             ("rbl_apply_M_sym_dev", (dptr, dptr, N, 0, 1, dptr)), ("rbl_apply_M_sym_multi_dev", (dptr, dptr, N, 1, 0, 1, dptr)),
             ("rbl_velocity_field", (hp, 4, hp, None, N, hp)), ("rbl_velocity_field_dev", (dptr, 4, dptr, None, N, dptr)),
             ("rbl_ensemble_set_config", (2, 5, hp, hp)), ("rbl_ensemble_get_config", (hp, hp)), ("rbl_ensemble_config_dev", (hp, hp)),
             ("rbl_ensemble_step_deterministic", (hp, None, 50, 1e-8, None, None)),
             ("rbl_ensemble_step_brownian", (hp, None, None, 1, 1, 1e-4, 50, 1e-8, None, None)),
             ("rbl_ensemble_interaction_forces", (hp, hp)), ("rbl_ensemble_flow_slip", (hp,)), ("rbl_ensemble_step_moments", (hp,)),
             ("rbl_ensemble_bond_state", (hp, hp, hp)), ("rbl_ensemble_run", (C.addressof(o), C.addressof(out))),
             ("rbl_ensemble_solve_mixed", (hp, hp, None, 50, 1e-8, hp, hp, hp, None, None)),
             ("rbl_ensemble_solve_mixed_dof", (hp, hp, None, 50, 1e-8, hp, hp, hp, None, None)),
             ("rbl_ensemble_step_mixed", (hp, hp, None, 50, 1e-8, hp, None, None)), ("rbl_ensemble_step_mixed_dof", (hp, hp, None, 50, 1e-8, hp, None, None)),
             ("rbl_ensemble_step_brownian_mixed", (hp, hp, None, None, 1, 1, 1e-4, 50, 1e-8, hp, None, None)),
             ("rbl_ensemble_step_brownian_mixed_dof", (hp, hp, None, None, 1, 1, 1e-4, 50, 1e-8, hp, None, None))]
    for name, args in calls:
        rc = getattr(L, name)(h, *args)
        msg = L.rbl_last_error(h).decode()
        assert rc == ERR_STATE and "periodic" in msg, (name, rc, msg)
        assert _rel(rb.apply_M(F, r), ref) <= 1e-12, name           # the context serves the next call
    assert not big.any() and not bool(dbuf.any())                 # refused before any work: nothing was written
    # the Lanczos roots are offered; the dense method is what is refused, also inside a Brownian step
    with pytest.raises(RuntimeError, match="periodic"):
        rb.M_half_W(F, method="cholesky")
    with pytest.raises(RuntimeError, match="periodic"):
        rb.step_brownian(np.zeros(60), seed=1, method="cholesky")
    X, _ = rb.get_config()
    assert np.array_equal(np.asarray(X).reshape(-1, 3), ten["X"])  # the refused step did not move anything
    # at use: the free-space lattice sum diverges
    from rigid_body_light_amd import RigidBody
    free = RigidBody(ten["cfg"], ten["X"], ten["Q"], ten["a"], ETA, 0.01, wall_PC=False)
    free.set_periodic(Lc[0], Lc[1], images=n)
    with pytest.raises(RuntimeError, match="periodic.*wall"):
        free.apply_M(F, r)
    free.set_periodic(Lc[0], Lc[1], images=n, on=False)
    assert np.isfinite(free.apply_M(F, r)).all()
    # ... and a cell that the parameters have outgrown (set before them): L <= 4a at use
    with pytest.raises(RuntimeError, match="4a"):
        rb.set_periodic(4.0 * ten["a"], Lc[1], images=n)
    assert rb.periodic()["Lx"] == Lc[0]
    assert _rel(rb.apply_M(F, r), ref) <= 1e-12


def test_a_context_with_an_ensemble_refuses_the_cell_and_a_short_cell_is_found_at_use(ten):
    import torch
    from rigid_body_light_amd._lib import DeviceContext, RblError
    ctx = DeviceContext(ten["a"], ETA, True, cfg=ten["cfg"], dt=0.01, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.ensemble_set_config(np.stack([ten["X"][:4], ten["X"][4:8]]), np.stack([ten["Q"][:4], ten["Q"][4:8]]))
    with pytest.raises(RblError, match=r"set_periodic: not offered for ensembles.*status 7"):
        ctx.set_periodic(ten["L"][0], ten["L"][1])
    assert ctx.periodic() == dict(on=False, Lx=0.0, Ly=0.0, images=(0, 0)) and ctx.ensemble_info() == (2, 4)
    # a cell set for small blobs, then larger blobs: L <= 4a is found at use, RBL_ERR_STATE, and the next cell is served
    ctx2 = DeviceContext(0.1, ETA, True, cfg=ten["cfg"], dt=0.01, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx2.set_periodic(1.0, 0.0, images=(1, 0))
    cfg = np.ascontiguousarray(ten["cfg"], dtype=np.float64)
    ctx2._chk(ctx2.L.rbl_set_parameters(ctx2.h, ten["a"], 0.01, 1.0, ETA, cfg.ctypes.data, cfg.shape[0]))
    ctx2._chk(ctx2.L.rbl_set_wall_pc(ctx2.h, 1))
    dev = torch.device("cuda:0")
    dr = torch.from_numpy(ten["r"].reshape(-1).copy()).to(dev)
    dF, out = torch.ones_like(dr), torch.zeros_like(dr)
    with pytest.raises(RblError, match=r"periodic cell: Lx = 1\.0.*4a.*status 7"):
        ctx2.apply_M(dF.data_ptr(), dr.data_ptr(), 120, 0, 120, out.data_ptr())
    ctx2.set_periodic(ten["L"][0], ten["L"][1], images=(1, 1))
    ctx2.apply_M(dF.data_ptr(), dr.data_ptr(), 120, 0, 120, out.data_ptr())
    ctx2.sync_check()
    assert _rel(out.cpu().numpy(), ten["M"][(ten["L"], (1, 1))] @ np.ones(360)) <= 1e-12
