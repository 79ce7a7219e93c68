"""A periodic cell per replica of an ensemble (include/rbl.h section 5: rbl_ensemble_set_cells; Ensemble.set_cells) on the GPU: the
image sum of every replica's own cell against dense numpy solves on tests/periodic_oracle.py's matrices, the table indexed by
replica (a lattice translation of a replica's own cell leaves its solution alone, another replica's does not), replica r of R
bitwise the R = 1 ensemble in the shared cell r, R equal rows bitwise the shared cell, runs bitwise the loop of one-step calls with
the probes against tests/ensemble_probe_oracle.py, the Brownian step against the numpy restatement of the scheme, the minimum-image
forces per replica, and the errors, which name their replica.

Tolerances are the project's own for the same comparisons (head of tests/test_ensemble_periodic_gpu.py): 1e-7 relative for a
solve to rtol 1e-10 against the dense solve and for what contains the difference quotient, 1e-12 for forces and for probes against
their oracles, 1e-12 for the lattice translation (rounding of the larger coordinates).

The shapes and cells are those of tests/test_ensemble_cells_cpu.py, which establishes the positivity of the oracle's matrix at
every cell where a Brownian step is taken here: A 4 tetrahedra (16 blobs, one row block of the pair sweep) in four cells, the
last with y open; B 3 trimers (9: odd N); C one body of 7 blobs (own-image terms only); D 10 x shell_N_12 (120: two row blocks and
the half offset) in three cells."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_probe_oracle as epo  # noqa: E402
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402
import test_ensemble_cells_cpu as cc  # noqa: E402  (the cases, shared with the positivity test)
from test_ensemble_periodic_gpu import _dense_saddle, _np_brownian_step  # noqa: E402  (the restatements of the shared cell's tests)

pytestmark = pytest.mark.gpu
ETA = 1.0
SOLVE = dict(max_iter=200, rtol=1e-10)
KW = dict(max_iter=200, rtol=1e-8)
MODEL = dict(w=0.3, eps_wall=0.5, b_wall=0.2, eps_blob=1.0, b_blob=0.2, r_cut=2.0)    # 2 R_body + r_cut = 3.6 <= L / 2 of every D cell


def _rel(x, y):
    return np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(np.asarray(y).reshape(-1))


def _ens(cfg, a, X, Q, dt=0.01, kBT=1.0, wall=True):
    from rigid_body_light_amd import Ensemble
    return Ensemble(cfg, np.asarray(X), np.asarray(Q), a, ETA, dt, kBT=kBT, wall=wall)


def _stack(cases):
    return np.stack([c["X"] for c in cases]), np.stack([c["Q"] for c in cases])


def _inputs(R, nb, n3, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, 6 * nb)), 0.1 * rng.standard_normal((R, n3))


def _free_solve(ens, F, slip, **kw):
    kw = kw or SOLVE
    lam, U, _, its, res = ens.solve_mixed(np.zeros(ens.N_bodies, dtype=bool), F, slip=slip, **kw)
    assert (its > 0).all() and (its < kw["max_iter"]).all(), (its, res)
    return lam, U, its


def _cells(L, scales):
    """(Lx (R,), Ly (R,)) of the cell L scaled replica by replica; a zero factor leaves that axis open"""
    return np.array([L[0] * s[0] for s in scales]), np.array([L[1] * s[1] for s in scales])


def _eff(L, n):
    """the images as stored: 0 on an open axis"""
    return (n[0] if L[0] > 0.0 else 0, n[1] if L[1] > 0.0 else 0)


# ------------------------------------------------------------------------------------------------------ 1: the operator, by the solve
@pytest.mark.parametrize("images", ["shared", "own"])
def test_A_in_four_cells_against_the_dense_solve_in_each(orc, images):
    cases = [cc.case_A(r) for r in range(4)]
    c = cases[0]
    Lx, Ly = _cells(c["L"], cc.A_SCALES)
    n = np.array([(1, 1)] * 4 if images == "shared" else cc.A_IMAGES)
    X, Q = _stack(cases)
    F, slip = _inputs(4, 4, 48, 161)
    ens = _ens(c["cfg"], c["a"], X, Q)
    lam_open, U_open, _ = _free_solve(ens, F, slip)
    ens.set_cells(Lx, Ly, images=(1, 1) if images == "shared" else n)
    got = ens.cells()
    assert got["on"] and got["per_replica"] and np.array_equal(got["Lx"], Lx) and np.array_equal(got["Ly"], Ly)
    assert np.array_equal(got["images"], [_eff((Lx[r], Ly[r]), n[r]) for r in range(4)])     # the open axis' n is stored as 0
    lam, U, its = _free_solve(ens, F, slip)
    lam2, U2, _ = _free_solve(ens, F, slip)
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2)    # one summation order
    ens.close()
    for r in range(4):
        L = (Lx[r], Ly[r])
        M, K, _ = po.dense_matrices(orc, c["cfg"], X[r], Q[r], c["a"], ETA, L, _eff(L, n[r]))
        lam_d, U_d = _dense_saddle(M, K, F[r], slip[r])
        print("A seed %d, cell %.3f x %.3f, images %s: %d iterations, rel. diff lambda %.2e U %.2e, against the open system %.2e"
              % (r, L[0], L[1], tuple(int(v) for v in n[r]), its[r], _rel(lam[r], lam_d), _rel(U[r], U_d), _rel(U[r], U_open[r])))
        assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7
        assert _rel(U[r], U_open[r]) > 1e-5                       # the cell counts at this tolerance


@pytest.mark.parametrize("name", ["B", "C"])
def test_an_odd_N_and_a_body_alone_in_two_cells_against_the_dense_solve(orc, name):
    build = {"B": lambda s: pc.layers("trimer", 3, 3, 1, seed=s), "C": lambda s: pc.layers("fib7", 1, 1, 1, seed=s, extra=(1, 1))}[name]
    cases = [build(s) for s in (0, 1)]
    c = cases[0]
    Lx, Ly = _cells(c["L"], [(1.0, 1.0), (1.3, 1.2)])
    n = [(2, 1), (1, 1)]
    X, Q = _stack(cases)
    nb, n3 = X.shape[1], 3 * X.shape[1] * c["nblb"]
    F, slip = _inputs(2, nb, n3, 162)
    ens = _ens(c["cfg"], c["a"], X, Q)
    ens.set_cells(Lx, Ly, images=n)
    lam, U, its = _free_solve(ens, F, slip)
    ens.close()
    for r in range(2):
        M, K, _ = po.dense_matrices(orc, c["cfg"], X[r], Q[r], c["a"], ETA, (Lx[r], Ly[r]), n[r])
        lam_d, U_d = _dense_saddle(M, K, F[r], slip[r])
        print("%s seed %d, cell %.3f x %.3f, images %s: %d iterations, rel. diff lambda %.2e U %.2e"
              % (name, r, Lx[r], Ly[r], n[r], its[r], _rel(lam[r], lam_d), _rel(U[r], U_d)))
        assert _rel(lam[r], lam_d) <= 1e-7 and _rel(U[r], U_d) <= 1e-7


# ------------------------------------------------------------------------------------------------------ 2: the table is indexed by replica
def test_a_translation_by_the_replicas_own_Lx_leaves_it_alone_and_by_anothers_does_not():
    """body 1 of every replica of A moved by (Lx, 0, 0): with the replica's own Lx the solution changes by no more than the bound of
    the lattice-translation tests (1e-12: the rounding of the larger coordinates), with the next replica's Lx it is another problem"""
    cases = [cc.case_A(r) for r in range(3)]
    c = cases[0]
    Lx, Ly = _cells(c["L"], cc.A_SCALES[:3])
    assert len(set(Lx)) == 3
    X, Q = _stack(cases)
    F, slip = _inputs(3, 4, 48, 163)
    U = []
    for shift in (None, Lx, np.roll(Lx, -1)):
        Xc = X.copy()
        if shift is not None:
            Xc[:, 1, 0] += shift
        ens = _ens(c["cfg"], c["a"], Xc, Q)
        ens.set_cells(Lx, Ly, images=(1, 1))
        U.append(ens.solve_mixed(np.zeros(4, dtype=bool), F, slip=slip, max_iter=200, rtol=1e-13)[1])
        assert np.array_equal(ens.get_config()[0], Xc)            # coordinates stay unwrapped
        ens.close()
    for r in range(3):
        own, other = _rel(U[1][r], U[0][r]), _rel(U[2][r], U[0][r])
        print("replica %d, Lx %.3f: U changes by %.2e after a translation by its own Lx, by %.2e after one by %.3f"
              % (r, Lx[r], own, other, np.roll(Lx, -1)[r]))
        assert own <= 1e-12 and other > 1e-3


# ------------------------------------------------------------------------------------------------------ 3, 4: bitwise on D
def _D_points():
    """8 lab points over and beside D's first cell, above the wall"""
    c = pc.layer10()
    rng = np.random.default_rng(164)
    return np.stack([rng.uniform(-0.2, 1.3, 8) * c["L"][0], rng.uniform(-0.2, 1.3, 8) * c["L"][1], rng.uniform(0.3, 5.0, 8)], axis=1)


def _D_ens(X, Q, dt=0.01, model=True):
    c = pc.layer10()
    ens = _ens(c["cfg"], c["a"], X, Q, dt=dt)
    if model:
        ens.set_interactions(**MODEL)
    return ens


def _sequence(ens, F, slip, W, run=False):
    """forces, a solve, the field of its lambda, a deterministic, a Brownian and a masked Brownian step (body 2 held) and, with
    run, five Brownian steps in one call -> every result, replica-major"""
    R, nb = ens.R, ens.N_bodies
    out = [ens.interaction_forces(), ens.interaction_energy()]
    lam, U, Fo, its, res = ens.solve_mixed(np.zeros(nb, dtype=bool), F, slip=slip, **KW)
    assert (its < 200).all()
    out += [lam, U, its, res, ens.velocity_field(_D_points(), lam)]
    its, res = ens.step_deterministic(F, slip=slip, **KW)
    assert (its < 200).all()
    out += [its, res] + list(ens.get_config())
    its, res = ens.step_brownian(F, W=W, slip=slip, **KW)
    assert (its < 200).all()
    out += [its, res] + list(ens.get_config())
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 2] = True
    body_in = F.copy().reshape(R, nb, 6)
    body_in[:, 2] = 0.0
    Fo, its, res = ens.step_brownian_mixed(mask, body_in.reshape(R, 6 * nb), W=W, slip=slip, **KW)
    assert (its < 200).all()
    out += [Fo, its, res] + list(ens.get_config())
    if run:
        r = ens.run(5, F=F, brownian=True, seed=90, stride=1, slip=slip, **KW)
        out += [r.X, r.Q, r.iters_sum, r.accepted]
        out[-4], out[-3] = np.swapaxes(r.X, 0, 1), np.swapaxes(r.Q, 0, 1)      # replica-major
    return out


def _D_inputs():
    F, slip = _inputs(3, 10, 360, 165)
    return 0.3 * F, slip, np.random.default_rng(166).standard_normal((3, 1080))


def test_replica_r_of_R_is_the_R_1_ensemble_in_the_shared_cell_r_bitwise():
    c, X, Q = cc.D_replicas()
    Lx, Ly = _cells(c["L"], cc.D_SCALES)
    F, slip, W = _D_inputs()
    ens = _D_ens(X, Q)
    ens.set_cells(Lx, Ly, images=cc.D_IMAGES)
    all3 = _sequence(ens, F, slip, W)
    ens.close()
    assert np.abs(all3[-2] - X).max() > 1e-4 and np.abs(all3[0]).max() > 1e-3    # the replicas moved, the model pushes
    for r in range(3):
        ens = _D_ens(X[r:r + 1], Q[r:r + 1])
        ens.set_cell(Lx[r], Ly[r], images=cc.D_IMAGES[r])
        one = _sequence(ens, F[r:r + 1], slip[r:r + 1], W[r:r + 1])
        ens.close()
        for k, (p, q) in enumerate(zip(all3, one)):
            assert np.array_equal(p[r], q[0]), (r, k)
    # ... and the cells differ where it counts: replica 1 in replica 0's cell is another answer
    ens = _D_ens(X[1:2], Q[1:2])
    ens.set_cell(Lx[0], Ly[0], images=cc.D_IMAGES[0])
    wrong = _sequence(ens, F[1:2], slip[1:2], W[1:2])
    ens.close()
    assert not np.array_equal(all3[3][1], wrong[3][0]) and not np.array_equal(all3[6][1], wrong[6][0])


def test_equal_rows_are_the_shared_cell_and_the_later_call_replaces_the_earlier_bitwise():
    c, X, Q = cc.D_replicas()
    L = c["L"]
    F, slip, W = _D_inputs()

    def go(setup):
        ens = _D_ens(X, Q)
        setup(ens)
        out = _sequence(ens, F, slip, W, run=True)
        ens.close()
        return out

    shared = go(lambda e: e.set_cell(L[0], L[1], images=(1, 1)))
    rows = go(lambda e: e.set_cells(np.full(3, L[0]), np.full(3, L[1]), images=(1, 1)))
    scalars = go(lambda e: e.set_cells(L[0], L[1], images=(1, 1)))

    def after(e):                                                 # a shared cell after a per-replica one
        e.set_cells(*_cells(L, cc.D_SCALES), images=cc.D_IMAGES)
        e.set_cell(L[0], L[1], images=(1, 1))
        assert e.cell() == dict(on=True, Lx=L[0], Ly=L[1], images=(1, 1)) and not e.cells()["per_replica"]
    replaced = go(after)
    for k, (p, q, s, t) in enumerate(zip(shared, rows, scalars, replaced)):
        assert np.array_equal(p, q) and np.array_equal(p, s) and np.array_equal(p, t), k
    never = go(lambda e: None)

    def off(e):
        e.set_cells(*_cells(L, cc.D_SCALES), images=cc.D_IMAGES, on=False)
        got = e.cells()
        assert not got["on"] and got["per_replica"] and np.array_equal(got["images"], cc.D_IMAGES)
    switched_off = go(off)
    for k, (p, q) in enumerate(zip(never, switched_off)):
        assert np.array_equal(p, q), k
    assert not np.array_equal(never[3], shared[3])


# ------------------------------------------------------------------------------------------------------ 5: a run is the loop
@pytest.mark.parametrize("on_error", ["stop", "reject"])
@pytest.mark.parametrize("family", ["deterministic", "brownian", "masked deterministic", "masked brownian"])
def test_a_run_of_five_steps_in_three_cells_is_five_one_step_calls_bitwise(family, on_error):
    c, X, Q = cc.D_replicas()
    Lx, Ly = _cells(c["L"], cc.D_SCALES)
    R, nb, steps = 3, 10, 5
    F, slip, _ = _D_inputs()
    mask = np.zeros((R, nb), dtype=bool)
    mask[:, 2] = True
    body_in = F.copy().reshape(R, nb, 6)
    body_in[mask] = [0.02, 0.0, 0.01, 0.0, 0.03, 0.0]
    body_in = body_in.reshape(R, 6 * nb)
    brownian, masked = "brownian" in family, "masked" in family

    def make():
        e = _D_ens(X, Q)
        e.set_cells(Lx, Ly, images=cc.D_IMAGES)
        return e
    ens = make()
    cfgs, its = [], []
    for n in range(steps):
        if masked and brownian:
            it = ens.step_brownian_mixed(mask, body_in, seed=40 + n, slip=slip, **KW)[1]
        elif masked:
            it = ens.step_mixed(mask, body_in, slip=slip, **KW)[1]
        elif brownian:
            it = ens.step_brownian(F, seed=40 + n, slip=slip, **KW)[0]
        else:
            it = ens.step_deterministic(F, slip=slip, **KW)[0]
        assert (it < 200).all()
        its.append(it); cfgs.append(ens.get_config())
    ens.close()
    ens = make()
    if masked:
        out = ens.run(steps, prescribed=mask, body_in=body_in, brownian=brownian, seed=40, stride=1, slip=slip, on_error=on_error, **KW)
    else:
        out = ens.run(steps, F=F, brownian=brownian, seed=40, stride=1, slip=slip, on_error=on_error, **KW)
    Xr, Qr = ens.get_config()
    ens.close()
    print("%s run (%s) in three cells: %s iterations over %d steps" % (family, on_error, out.iters_sum, steps))
    assert np.array_equal(Xr, cfgs[-1][0]) and np.array_equal(Qr, cfgs[-1][1])
    for k in range(steps):                                        # a frame per step
        assert np.array_equal(out.X[k], cfgs[k][0]) and np.array_equal(out.Q[k], cfgs[k][1]), k
    assert np.array_equal(out.iters_sum, np.sum(its, axis=0)) and np.array_equal(out.accepted, np.full(R, steps))
    assert np.abs(Xr - X).max() > 1e-4


def test_a_driven_run_in_three_cells_is_the_loop_of_drive_eval_and_the_step_bitwise():
    c, X, Q = cc.D_replicas()
    Lx, Ly = _cells(c["L"], cc.D_SCALES)
    F, slip, _ = _D_inputs()
    rng = np.random.default_rng(167)
    drive = dict(cos=0.2 * rng.standard_normal((3, 60)), sin=0.2 * rng.standard_normal((3, 60)), omega=np.array([2.0, 5.0, 9.0]),
                 t0=np.array([0.1, 0.2, 0.3]))

    def make():
        e = _D_ens(X, Q)
        e.set_cells(Lx, Ly, images=cc.D_IMAGES)
        return e
    ens = make()
    cfgs = []
    for n in range(5):
        inp, _ = ens.drive_eval(F, accepted=np.full(3, n, dtype=np.int32), **drive)
        ens.step_deterministic(inp, slip=slip, **KW)
        cfgs.append(ens.get_config())
    ens.close()
    ens = make()
    out = ens.run_driven(5, F=F, brownian=False, stride=1, slip=slip, **drive, **KW)
    ens.close()
    for k in range(5):
        assert np.array_equal(out.X[k], cfgs[k][0]) and np.array_equal(out.Q[k], cfgs[k][1]), k
    assert np.array_equal(out.accepted, [5, 5, 5])


@pytest.mark.parametrize("body", [None, 0])
def test_an_observed_run_in_three_cells_is_the_loop_and_the_probes_follow_each_replicas_cell(orc, body):
    """run(5, stride=1, probes, moments) against the loop solve -> velocity_field -> step; 8 lab probes, or 4 fixed in body 0.
    Replica r's field of step 0 against the restatement in cell r (1e-12)"""
    from oracle import oracle as O
    c, X, Q = cc.D_replicas()
    Lx, Ly = _cells(c["L"], cc.D_SCALES)
    F, _, _ = _D_inputs()
    pts = _D_points() if body is None else np.random.default_rng(168).uniform(1.4, 2.5, (4, 3)) * [1, -1, 1]
    free = np.zeros(10, dtype=bool)

    def make():
        e = _D_ens(X, Q, model=False)
        e.set_cells(Lx, Ly, images=cc.D_IMAGES)
        return e
    ens = make()
    res = ens.run(5, prescribed=free, body_in=F, brownian=False, stride=1, probes=pts, probe_body=body, moments=True, **KW)
    ens.close()
    assert res.accepted.tolist() == [5, 5, 5] and res.frame_u.shape == (5, 3, pts.shape[0], 3) and res.frame_D.shape == (5, 3, 10, 3, 3)
    ens = make()
    ens.record_moments(True)
    usum, Dsum, lam0 = np.zeros_like(res.u_sum), np.zeros_like(res.D_sum), None
    for n in range(5):
        lam = ens.solve_mixed(free, F, **KW)[0]
        lam0 = lam if lam0 is None else lam0
        u = ens.velocity_field(pts, lam, body=body)
        assert np.array_equal(res.frame_u[n], u), n
        ens.step_mixed(free, F, **KW)
        D = ens.step_moments()
        assert np.array_equal(res.frame_D[n], D), n
        usum += u
        Dsum += D
    ens.close()
    assert np.array_equal(res.u_sum, usum) and np.array_equal(res.D_sum, Dsum)
    cfg = O.remove_mean(c["cfg"])
    for r in range(3):
        rk = orc.multi_body_pos(X[r], O.normalize_quats(Q[r]), cfg).reshape(-1, 3)
        ref = epo.field_cell(orc, rk, lam0[r], epo.place(pts, X[r], Q[r], body), c["a"], ETA, (Lx[r], Ly[r]), cc.D_IMAGES[r])
        print("replica %d, cell %.3f x %.3f, images %s: %d probes (body %s), rel. error %.2e"
              % (r, Lx[r], Ly[r], cc.D_IMAGES[r], pts.shape[0], body, _rel(res.frame_u[0, r], ref)))
        assert np.abs(ref).max() > 1e-4 and _rel(res.frame_u[0, r], ref) <= 1e-12


# ------------------------------------------------------------------------------------------------------ 6: the Brownian step
@pytest.mark.parametrize("split_rand", [True, False])
def test_brownian_step_with_injected_noise_against_the_numpy_restatement_in_each_replicas_cell(orc, split_rand):
    from oracle import oracle as O
    cases = [cc.case_A(r) for r in range(4)]
    c = cases[0]
    Lx, Ly = _cells(c["L"], cc.A_SCALES)
    dt, kBT = 0.01, 1.0
    X, Q = _stack(cases)
    R, nb, n3 = 4, 4, 48
    rng = np.random.default_rng(169)
    F, slip, W = rng.standard_normal((R, 6 * nb)), 0.1 * rng.standard_normal((R, n3)), rng.standard_normal((R, 3 * n3))
    ens = _ens(c["cfg"], c["a"], X, Q, dt=dt, kBT=kBT)
    ens.set_cells(Lx, Ly, images=cc.A_IMAGES)
    its, res = ens.step_brownian(F, W=W, split_rand=split_rand, slip=slip, **SOLVE)
    assert (its > 0).all() and (its < 200).all() and (res < 1e-10).all()
    Xe, Qe = ens.get_config()
    ens.close()
    cfg = O.remove_mean(c["cfg"])
    P6 = np.zeros((nb, 6), dtype=bool)
    for r in range(R):
        Qn = O.normalize_quats(Q[r])
        L = (Lx[r], Ly[r])
        Xn, Qn1, _ = _np_brownian_step(orc, cfg, X[r], Qn, c["a"], L, _eff(L, cc.A_IMAGES[r]), dt, kBT, P6, F[r], slip[r], W[r], split_rand)
        moved_X, moved_Q = np.abs(Xn - X[r]).max(), np.abs(Qn1 - Qn).max()
        print("A split_rand=%s replica %d, cell %.3f x %.3f, images %s: %d iterations, X differs by %.2e of a displacement of %.2e, Q by %.2e of %.2e"
              % (split_rand, r, L[0], L[1], cc.A_IMAGES[r], its[r], np.abs(Xe[r] - Xn).max() / moved_X, moved_X,
                 np.abs(Qe[r] - Qn1).max() / moved_Q, moved_Q))
        assert np.abs(Xe[r] - Xn).max() <= 1e-7 * moved_X and np.abs(Qe[r] - Qn1).max() <= 1e-7 * moved_Q


# ------------------------------------------------------------------------------------------------------ 7: forces
def _force_replicas():
    """pc.force_case("12xshell_pair") -- 12 x shell_N_12 in layer10()'s cell, pairs across both boundaries -- and two displaced
    copies, in three cells: its own, a larger one (no pair reaches through it), and its own with y open"""
    c = pc.force_case("12xshell_pair")
    rng = np.random.default_rng(170)
    X = np.stack([c["X"], c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape), c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape)])
    Q = np.stack([c["Q"]] * 3)
    Lx, Ly = _cells(c["L"], [(1.0, 1.0), (1.2, 1.1), (1.0, 0.0)])
    return c, X, Q, Lx, Ly


@pytest.mark.parametrize("which", ["steric", "table", "dipoles"])
def test_forces_by_minimum_image_in_each_replicas_cell(which):
    from oracle import oracle as O
    c, X, Q, Lx, Ly = _force_replicas()
    a = c["a"]
    ens = _ens(c["cfg"], a, X, Q)
    m_body = np.random.default_rng(171).standard_normal((12, 3))
    dip = dict(c_dd=0.8, r_core=1.0, r_cut=4.5)                   # r_cut <= L / 2 of every periodic axis
    if which == "steric":
        ens.set_interactions(eps_blob=c["steric"][0], b_blob=c["steric"][1], r_cut=c["steric"][2], **pc.BUILTIN)
    elif which == "table":
        ens.set_pair_table(*c["table"])
    else:
        ens.set_dipoles(m_body, **dip)
    ens.set_cells(Lx, Ly)
    FT, E = ens.interaction_forces(), ens.interaction_energy()
    assert np.array_equal(FT, ens.interaction_forces())
    ens.close()
    through = []
    for r in range(3):
        L = (Lx[r], Ly[r])
        if which == "dipoles":
            m_lab = np.array([O.rot_matrix(q) @ m for q, m in zip(O.normalize_quats(Q[r]), m_body)])
            FT_ref, E_ref = po.dipole_pairs(X[r], m_lab, dip["c_dd"], dip["r_core"], dip["r_cut"], L)
            FT_shared = po.dipole_pairs(X[r], m_lab, dip["c_dd"], dip["r_core"], dip["r_cut"], (Lx[0], Ly[0]))[0]
        else:
            pos = pc.blob_positions(c["cfg"], X[r], Q[r])
            kw = dict(builtin=pc.BUILTIN, steric=c["steric"]) if which == "steric" else dict(table=c["table"])
            ref = po.force_model(pos, X[r], 12, a, L, **kw)
            FT_ref, E_ref = ref["FT"], ref["E"]
            FT_shared = po.force_model(pos, X[r], 12, a, (Lx[0], Ly[0]), **kw)["FT"]
            through.append(ref["through"])
        print("%s, replica %d, cell %.3f x %.3f: body forces / torques rel. error %.2e, energy %.2e; in replica 0's cell they differ by %.2e"
              % (which, r, L[0], L[1], _rel(-FT[r], FT_ref), abs(E[r] - E_ref) / abs(E_ref), _rel(FT_shared, FT_ref)))
        assert np.abs(FT_ref).max() > 1e-3
        assert _rel(-FT[r], FT_ref) <= 1e-12 and abs(E[r] - E_ref) <= 1e-12 * abs(E_ref)
        if r:
            assert _rel(FT_shared, FT_ref) > 1e-9                 # the replica's own cell is seen: replica 0's is a thousand bounds off
    if through:
        assert through[0] > 0 and through[1] == 0 and through[2] > 0    # (pairs through a boundary: both axes, none, x alone)


# ------------------------------------------------------------------------------------------------------ 8: errors
def test_an_overlap_through_the_boundary_of_replica_1s_smaller_cell_names_it_and_moves_nobody():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = cc.overlap_case()                                   # every replica: body 1 one SMALL cell length from body 0, blob on blob
    Lx, Ly = _cells(c["L"], cc.OVERLAP_SCALES)                    # through replica 1's boundary, 0.4 / 0.5 of it away in the larger cells
    F = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], 4)
    ens = _ens(c["cfg"], c["a"], X, Q)
    ens.set_cells(Lx, Ly, on=False)
    its, _ = ens.step_deterministic(F, max_iter=100, rtol=1e-8)   # the open system steps
    assert (its < 100).all()
    ens.set_config(X, Q)
    ens.set_cells(Lx, Ly)
    for step in ("det", "brown"):
        with pytest.raises(RblError) as e:
            if step == "det":
                ens.step_deterministic(F, max_iter=100, rtol=1e-8)
            else:
                ens.step_brownian(F, seed=1, max_iter=100, rtol=1e-8)
        assert "[rbl status 1]" in str(e.value) and "replica 1" in str(e.value), str(e.value)
        Xc, Qc = ens.get_config()
        assert np.array_equal(Xc, X) and np.array_equal(Qc, Q)    # no replica moved
    out = ens.run(3, F=F, brownian=False, on_error="reject", max_iter=100, rtol=1e-8)
    assert np.array_equal(out.rejected, [0, 3, 0]) and np.array_equal(out.accepted, [3, 0, 3]) and np.array_equal(out.first_status, [0, 1, 0])
    Xc, _ = ens.get_config()
    assert np.array_equal(Xc[1], X[1]) and np.abs(Xc[0] - X[0]).max() > 0.0
    ens.close()


def test_refusals_name_their_replica_and_the_states_read_back():
    from rigid_body_light_amd._lib import RblError
    c, X, Q = cc.D_replicas()
    L = c["L"]
    F = np.zeros(60)
    ens = _D_ens(X, Q)
    # a cell too small for the force cutoff in replica 2 only: RBL_ERR_ARG before any device work; the ensemble stays usable
    ens.set_cells([L[0], L[0], 7.0], L[1])
    for call in (ens.interaction_forces, lambda: ens.step_deterministic(F, **KW), lambda: ens.run(2, F=F, **KW)):
        with pytest.raises(RblError, match=r"replica 2: periodic cell too small: Lx = 7\.0.*status 11"):
            call()
    assert np.array_equal(ens.get_config()[0], X)
    Lx, Ly = _cells(L, cc.D_SCALES)
    ens.set_cells(Lx, Ly, images=cc.D_IMAGES)
    FT = ens.interaction_forces()
    # cell() has no one cell to report and says where to go; cells() reads the table back
    with pytest.raises(RblError, match=r"cells\(\)"):
        ens.cell()
    got = ens.cells()
    assert got["on"] and got["per_replica"] and np.array_equal(got["Lx"], Lx) and np.array_equal(got["Ly"], Ly)
    assert np.array_equal(got["images"], cc.D_IMAGES) and got["images"].shape == (3, 2)
    assert np.allclose(ens.area_fraction(2.0), 10 * 2.0 / (Lx * Ly), rtol=1e-15)
    # the jointed calls stay refused, with the shared cell's status and word
    for call in (lambda: ens.solve_jointed(F), lambda: ens.step_jointed(F), lambda: ens.joint_state(phi=False)):
        with pytest.raises(RblError, match=r"periodic.*status 7"):
            call()
    # another R: refused, nothing changed; the same R keeps the cells
    with pytest.raises(RblError, match=r"rbl_ensemble_set_cells.*status 7"):
        ens.set_config(X[:2], Q[:2])
    assert ens.R == 3 and ens.ctx.ensemble_info() == (3, 10) and np.array_equal(ens.get_config()[0], X)
    ens.set_config(X[::-1].copy(), Q)
    assert ens.cells()["per_replica"] and np.array_equal(ens.cells()["Lx"], Lx)
    ens.set_config(X, Q)
    assert np.array_equal(ens.interaction_forces(), FT)
    # a wrong R and the wrapper: the library is told the ensemble's R
    Lc = np.ascontiguousarray(Lx[:2])
    n1 = np.ones(2, dtype=np.int32)
    h = ens.ctx
    assert h.L.rbl_ensemble_set_cells(h.h, 2, Lc.ctypes.data, Lc.ctypes.data, n1.ctypes.data, n1.ctypes.data, 1) == 11
    assert b"R = 2" in h.L.rbl_last_error(h.h) and np.array_equal(ens.cells()["Lx"], Lx)
    # a shared cell lets the ensemble take another R again, and cell() answers
    ens.set_cell(L[0], L[1])
    ens.set_config(X[:2], Q[:2])
    assert ens.R == 2 and ens.cell() == dict(on=True, Lx=L[0], Ly=L[1], images=(1, 1))
    got = ens.cells()
    assert not got["per_replica"] and got["Lx"].tolist() == [L[0]] * 2 and got["images"].tolist() == [[1, 1]] * 2
    ens.close()
    # the wall off with the cells on: found at use
    cA = cc.case_A(0)
    XA, QA = _stack([cA, cc.case_A(1)])
    free = _ens(cA["cfg"], cA["a"], XA, QA, wall=False)
    free.set_cells(*_cells(cA["L"], cc.A_SCALES[:2]))
    with pytest.raises(RblError, match=r"periodic.*wall.*status 7"):
        free.step_deterministic(np.zeros(24))
    free.close()


def test_parameters_that_outgrow_replica_0s_Lx_are_found_at_use_and_a_new_radius_reaches_the_table():
    """the table holds the cells in units of the blob radius: after rbl_set_parameters with another a the next use uploads it again --
    the solve is bitwise that of an ensemble created with that radius -- and a radius with 4a beyond replica 0's Lx is RBL_ERR_STATE
    naming replica 0"""
    from rigid_body_light_amd._lib import RblError
    cases = [cc.case_A(r) for r in range(3)]
    c = cases[0]
    Lx, Ly = _cells(c["L"], cc.A_SCALES[:3])
    X, Q = _stack(cases)
    X[:, :, 2] += 1.0                                             # room above the wall for the larger blobs
    F, slip = _inputs(3, 4, 48, 172)
    cfg = np.ascontiguousarray(c["cfg"], dtype=np.float64)

    def set_radius(e, a):
        e.ctx._chk(e.ctx.L.rbl_set_parameters(e.ctx.h, a, 0.01, 1.0, ETA, cfg.ctypes.data, cfg.shape[0]))
        e.ctx._chk(e.ctx.L.rbl_set_wall_pc(e.ctx.h, 1))
    ens = _ens(c["cfg"], c["a"], X, Q)
    ens.set_cells(Lx, Ly, images=cc.A_IMAGES[:3])
    U0 = _free_solve(ens, F, slip)[1]
    a1 = 1.1 * c["a"]
    set_radius(ens, a1)
    U1 = _free_solve(ens, F, slip)[1]
    fresh = _ens(c["cfg"], a1, X, Q)
    fresh.set_cells(Lx, Ly, images=cc.A_IMAGES[:3])
    U1_fresh = _free_solve(fresh, F, slip)[1]
    fresh.close()
    assert np.array_equal(U1, U1_fresh) and not np.array_equal(U1, U0)
    a2 = 0.5 * (Lx[0] + Lx[1]) / 4.0                              # Lx[0] < 4 a2 < Lx[1]
    set_radius(ens, a2)
    for call in (lambda: _free_solve(ens, F, slip), lambda: ens.step_brownian(F, seed=1), lambda: ens.velocity_field(np.ones((1, 3)), np.zeros((3, 48)))):
        with pytest.raises(RblError, match=r"replica 0: Lx.*no longer exceeds 4a.*rbl_ensemble_set_cells.*status 7"):
            call()
    assert np.array_equal(ens.get_config()[0], X)
    ens.close()


# ------------------------------------------------------------------------------------------------------ 9: the example
def test_example_ensemble_area_fraction_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ensemble_area_fraction.py"), "--replicas", "2", "--steps", "10"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "area fraction" in out.stdout and len([l for l in out.stdout.splitlines() if l.startswith("   0.")]) == 8
