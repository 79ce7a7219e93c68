"""Replica ensembles with prescribed velocity components on the GPU (include/rbl.h section 5, rbl_ensemble_solve_mixed_dof /
rbl_ensemble_step_mixed_dof, runs with prescribed_per = 6): every replica solves and steps as a single context at its configuration
does (rbl_solve_mixed_dof, rbl_step_mixed_dof), with the Krylov basis in LDS and in global memory; masks whose rows are all-or-none
are bitwise the whole-body calls and with nobody prescribed the unmasked step; a body with its translations held keeps X bitwise
while it turns; a run is the loop of one-step calls; the force model loads the free components only; results are reproducible and
read no unwritten memory; errors leave everything where it was; the example runs.

Tolerances are those of test_ensemble_mixed_gpu.py and test_prescribed_dof_gpu.py: both sides solved to rtol 1e-12 (1e-10 where
noted), two solvers of one system within 1e-7, the true residual <= 1e-9, F_p = -K^T lambda to 1e-12.  Figures are printed before
they are asserted (run with -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_ensemble_gpu import _configs, _ensemble, _model, _packed, _shell12, _single  # noqa: E402
from test_ensemble_mixed_gpu import _masks as _body_masks, _rel  # noqa: E402

IT, RTOL = 250, 1e-12
NBLB = 12


def _masks6(R, nb, seed):
    """(R, nb, 6), another kind in every replica: none, all, whole rows only, all rotations, z only, one body with a single free
    component, a random half"""
    assert R == 7
    rng = np.random.default_rng(seed)
    P = np.zeros((R, nb, 6), dtype=bool)
    P[1] = True
    P[2, rng.permutation(nb)[:max(nb // 3, 1)]] = True
    P[3, :, 3:] = True
    P[4, :, 2] = True
    b = int(rng.integers(nb))
    P[5, b] = True
    P[5, b, 4] = False
    P[6] = rng.random((nb, 6)) < 0.5
    assert not P[0].any() and P[1].all() and P[6].any() and not P[6].all()
    rows = P[2].sum(axis=1)
    assert set(rows.tolist()) == {0, 6}
    assert len({m.tobytes() for m in P}) == R
    return P


def _inputs6(P, seed, speed=1.0):
    """loads on the free components, velocities of size <= speed / sqrt 3 on the prescribed ones (every third prescribed body row
    entry held at zero), slip"""
    R, nb = P.shape[:2]
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, nb, 6))
    Up = speed * rng.uniform(-1.0, 1.0, (R, nb, 6)) / np.sqrt(3.0)
    Up[:, ::3] = np.where(rng.random((R, Up[:, ::3].shape[1], 6)) < 0.5, 0.0, Up[:, ::3])   # some components held
    bi = np.where(P, Up, F)
    slip = 0.1 * rng.standard_normal((R, 3 * NBLB * nb))
    return bi.reshape(R, 6 * nb), slip


def _single_dof(s, which, P, body_in, slip, max_iter, rtol, nb):
    """rbl_solve_mixed_dof / rbl_step_mixed_dof on a DeviceContext -> (lambda, U, F, iterations, residual) / (F, iterations, residual)"""
    m = np.ascontiguousarray(P, dtype=np.uint8).reshape(-1)
    b = np.ascontiguousarray(body_in, dtype=np.float64).reshape(-1)
    sl = None if slip is None else np.ascontiguousarray(slip, dtype=np.float64)
    slp = None if sl is None else sl.ctypes.data
    F = np.zeros(6 * nb)
    it, res = C.c_int(0), C.c_double(0.0)
    if which == "solve":
        lam, U = np.zeros(3 * NBLB * nb), np.zeros(6 * nb)
        s._chk(s.L.rbl_solve_mixed_dof(s.h, m.ctypes.data, b.ctypes.data, slp, int(max_iter), float(rtol), lam.ctypes.data, U.ctypes.data,
                                       F.ctypes.data, C.byref(it), C.byref(res)))
        return lam, U, F, it.value, res.value
    s._chk(s.L.rbl_step_mixed_dof(s.h, m.ctypes.data, b.ctypes.data, slp, int(max_iter), float(rtol), F.ctypes.data, C.byref(it),
                                  C.byref(res)))
    return F, it.value, res.value


# ---- the solver's placement rule, restated (small_launch, small_lds_base_bytes of rbl_small_solve.hpp) --------------------------
def _basis_in_lds(nb, max_iter, nbl=NBLB):
    """the masked solve keeps the Krylov basis in LDS when its vectors, the mask's flags and (max_iter + 1) basis vectors fit in
    150 KB: the launcher's own rule"""
    N, m = nb * nbl, max_iter
    n3, nb6 = 3 * N, 6 * nb
    nsys = n3 + nb6
    base = 8 * (2 * n3 + 2 * N + N + 36 * nb + 3 * nsys + nb6 + 3 * (m + 2) + 2 * m + 8 + 16 * n3 + n3 + 6 * N
                + (m * (m + 1) // 2 if m <= 64 else 0) + nb6)
    assert base <= 150 * 1024                               # the solve fits at all
    return base + 8 * (m + 1) * nsys <= 150 * 1024


# ---- 1, 2. the solve against the single context ------------------------------------------------------------------------------------
def _compare_solve(wall, nb, max_iter):
    from rigid_body_light_amd import RigidBody
    from test_prescribed_dof_gpu import _operator_residual
    c = _shell12()
    R = 7
    X0, Q0 = _configs(R, nb, wall)
    P = _masks6(R, nb, 31)
    bi, slip = _inputs6(P, 32)
    ens = _ensemble(c, X0, Q0, wall)
    lam, U, F, its, res = ens.ensemble_solve_mixed_dof(P, bi, max_iter=max_iter, rtol=RTOL, slip=slip)
    Xa, Qa = ens.ensemble_get_config()
    ens.close()
    assert np.array_equal(Xa, X0)                                                     # nothing moves
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall)
        lam1, U1, F1, it1, res1 = _single_dof(s, "solve", P[r], bi[r], slip[r], IT, RTOL, nb)
        s.close()
        rb = RigidBody(c["cfg"], X0[r], Q0[r], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=False)
        true_res, ferr = _operator_residual(rb, P[r], bi[r], slip[r], lam[r], U[r], F[r])
        print("solve_mixed_dof wall=%s N_bod=%d max_iter=%d replica %d, %d of %d components prescribed: %d iterations (single context "
              "%d), estimate %.2e, true residual %.2e, F_p error %.2e; rel. diff lambda %.2e U %.2e F %.2e"
              % (wall, nb, max_iter, r, int(P[r].sum()), P[r].size, its[r], it1, res[r], true_res, ferr, _rel(lam[r], lam1),
                 _rel(U[r], U1), _rel(F[r], F1)))
        assert 0 < its[r] < max_iter and res[r] < RTOL and res1 < RTOL
        assert _rel(lam[r], lam1) <= 1e-7 and _rel(U[r], U1) <= 1e-7 and _rel(F[r], F1) <= 1e-7
        assert true_res <= 1e-9 and ferr <= 1e-12
        p = P[r].reshape(-1)
        assert np.array_equal(U[r][p], bi[r][p]) and np.array_equal(F[r][~p], bi[r][~p])   # echoed, component by component


@pytest.mark.parametrize("wall", [False, True])
def test_solve_equals_the_single_context_solve_per_replica(wall):
    _compare_solve(wall, 10, IT)


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("nb,max_iter,in_lds", [(4, 80, True), (10, 250, False)])
def test_solve_with_the_basis_in_lds_and_in_global_memory(nb, max_iter, in_lds, wall):
    """The side of the launcher's rule is computed from the rule itself (_basis_in_lds above restates small_lds_base_bytes and
    small_basis_bytes): 4 bodies with 80 iterations need 34 224 + 108 864 bytes <= 153 600, the basis stays in LDS (the VLDS
    instantiations); 10 bodies with 250 iterations need 87 392 + 843 360 bytes, the basis goes to global memory.

    What this cannot see: the "in LDS" case asks for 143 088 bytes of dynamic LDS, more than the 64 KB a kernel gets without
    hipFuncAttributeMaxDynamicSharedMemorySize; where the runtime refuses that attribute the launcher falls back to the basis in
    global memory without a word, and this case would then run the other instantiation and still pass.  The rule says which side
    is ASKED for; the library has no query for the side taken."""
    assert _basis_in_lds(nb, max_iter) == in_lds
    _compare_solve(wall, nb, max_iter)


# ---- 3. reduction to whole bodies --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wall", [False, True])
def test_all_or_none_rows_are_bitwise_the_whole_body_calls(wall):
    c = _shell12()
    R, nb = 7, 10
    X0, Q0 = _configs(R, nb, wall)
    mask = _body_masks(R, nb, 41)
    P = np.repeat(mask[:, :, None], 6, axis=2)
    bi, slip = _inputs6(P, 42, speed=0.3)
    a, b = _ensemble(c, X0, Q0, wall), _ensemble(c, X0, Q0, wall)
    got = a.ensemble_solve_mixed_dof(P, bi, max_iter=IT, rtol=RTOL, slip=slip)
    want = b.ensemble_solve_mixed(mask, bi, max_iter=IT, rtol=RTOL, slip=slip)
    print("reduction wall=%s, solve: iterations %s (whole bodies %s)" % (wall, got[3], want[3]))
    assert np.all(got[3] > 0) and np.all(got[3] < IT)
    for x, y in zip(got, want):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for n in range(3):
        Fa, ita, resa = a.ensemble_step_mixed_dof(P, bi, max_iter=IT, rtol=RTOL, slip=slip)
        Fb, itb, resb = b.ensemble_step_mixed(mask, bi, max_iter=IT, rtol=RTOL, slip=slip)
        (Xa, Qa), (Xb, Qb) = a.ensemble_get_config(), b.ensemble_get_config()
        print("reduction wall=%s, step %d: iterations %s" % (wall, n, ita))
        assert np.all(ita > 0) and np.all(ita < IT)
        assert np.array_equal(ita, itb) and resa.tobytes() == resb.tobytes() and Fa.tobytes() == Fb.tobytes()
        assert Xa.tobytes() == Xb.tobytes() and Qa.tobytes() == Qb.tobytes()
    assert np.abs(Xa - X0).max() > 1e-5
    a.close()
    b.close()


@pytest.mark.parametrize("model", [False, True])
def test_nobody_prescribed_is_bitwise_the_unmasked_step(model):
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 61)
    mdl = _model(c["a"]) if model else None
    rng = np.random.default_rng(62)
    F = rng.standard_normal((R, 6 * nb))
    slip = 0.1 * rng.standard_normal((R, 36 * nb))
    P = np.zeros((R, nb, 6), dtype=bool)
    a, b = _ensemble(c, X0, Q0, wall, dt=1e-3, model=mdl), _ensemble(c, X0, Q0, wall, dt=1e-3, model=mdl)
    for n in range(3):
        Fo, ita, resa = a.ensemble_step_mixed_dof(P, F, max_iter=80, rtol=1e-10, slip=slip)
        itb, resb = b.ensemble_step_deterministic(F, max_iter=80, rtol=1e-10, slip=slip)
        assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.all(ita > 0)
        (Xa, Qa), (Xb, Qb) = a.ensemble_get_config(), b.ensemble_get_config()
        assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)
    assert np.abs(Xa - X0).max() > 1e-5
    if not model:
        assert np.array_equal(Fo, F)                                                  # free loads echoed
    a.close()
    b.close()


# ---- 4. the steps ------------------------------------------------------------------------------------------------------------------
def test_three_steps_equal_three_single_context_steps():
    c = _shell12()
    R, nb, wall, dt = 7, 10, True, 0.01
    X0, Q0 = _configs(R, nb, wall)
    P = _masks6(R, nb, 51)
    # in every replica but the all-prescribed and the whole-rows one: body 0 has its three translations held and its rotation free
    # under its torque, body 1 is driven along x and free otherwise
    held_reps = [0, 3, 4, 5, 6]
    for r in held_reps:
        P[r, 0] = [True, True, True, False, False, False]
        P[r, 1] = [True, False, False, False, False, False]
    bi, slip = _inputs6(P, 52, speed=0.5)
    bi = bi.reshape(R, nb, 6)
    for r in held_reps:
        bi[r, 0, :3] = 0.0
        bi[r, 0, 3:] = [0.8, -0.5, 0.6]                     # a torque: it turns
        bi[r, 1, 0] = 0.25
    bi = bi.reshape(R, 6 * nb)
    ens = _ensemble(c, X0, Q0, wall)
    Xfirst = None
    for n in range(3):
        F, its, res = ens.ensemble_step_mixed_dof(P, bi, max_iter=IT, rtol=RTOL, slip=slip)
        assert np.all(its > 0) and np.all(its < IT) and np.all(res < RTOL)
        if n == 0:
            Xfirst = ens.ensemble_get_config()[0]
    Xe, Qe = ens.ensemble_get_config()
    ens.close()
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall)
        for _ in range(3):
            Fs, it, rs = _single_dof(s, "step", P[r], bi[r], slip[r], IT, RTOL, nb)
            assert 0 < it < IT and rs < RTOL
        Xs, Qs = s.get_config(nb)
        s.close()
        print("step_mixed_dof replica %d, %d of %d components prescribed: |X - single| %.2e |Q - single| %.2e, rel. diff F %.2e"
              % (r, int(P[r].sum()), P[r].size, np.abs(Xe[r] - Xs).max(), np.abs(Qe[r] - Qs).max(), _rel(F[r], Fs)))
        assert np.abs(Xe[r] - Xs).max() <= 1e-7 and np.abs(Qe[r] - Qs).max() <= 1e-7
        assert _rel(F[r], Fs) <= 1e-7
        # a driven translation component: X += dt U, one rounding of the sum (half an ulp of |X|), as test_ensemble_mixed_gpu.py
        pt = P[r][:, :3]
        Ut = bi[r].reshape(nb, 6)[:, :3]
        if pt.any():
            err = np.abs((Xfirst[r][pt] - X0[r][pt]) - dt * Ut[pt]).max()
            print("    driven translations: |dX - dt U| %.2e (bound %.2e)" % (err, 1e-15 * np.abs(Xfirst[r]).max()))
            assert err <= 1e-15 * np.abs(Xfirst[r]).max()
    for r in held_reps:
        print("    replica %d body 0 (translations held): |dX| %.1e, |dQ| %.2e" % (r, np.abs(Xe[r, 0] - X0[r, 0]).max(), np.abs(Qe[r, 0] - Q0[r, 0]).max()))
        assert np.array_equal(Xe[r, 0], X0[r, 0])                                      # held in place, bitwise ...
        assert np.abs(Qe[r, 0] - Q0[r, 0]).max() > 1e-6                                # ... while it turns
        assert abs(Xe[r, 1, 0] - X0[r, 1, 0]) > 1e-3                                   # the driven component moved


# ---- 5. a run ----------------------------------------------------------------------------------------------------------------------
def test_a_run_is_the_loop_bitwise_and_a_brownian_run_is_refused():
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, nb, steps = 5, 3, 6
    X0, Q0 = _configs(R, nb, True)
    rng = np.random.default_rng(11)
    P = rng.random((R, nb, 6)) < 0.4
    P[0] = False
    P[1, 0] = True
    P[2, :, 3:] = True
    body_in = np.where(P, 0.03 * rng.uniform(-1, 1, (R, nb, 6)), 0.5 * rng.standard_normal((R, nb, 6))).reshape(R, 6 * nb)
    slip = 0.01 * rng.standard_normal((R, 3 * nb * 12))
    kw = dict(max_iter=50, rtol=1e-8)

    def make():
        e = Ensemble(c["cfg"], X0, Q0, a=c["a"], eta=c["eta"], dt=c["dt"], kBT=1.0, wall=True)
        e.set_interactions(w=0.3, eps_wall=1.5, b_wall=0.1, eps_blob=2.0, b_blob=0.05, r_cut=2 * c["a"] + 20 * 0.05)
        return e
    ens = make()
    its, res, Fs, cfgs = [], [], [], []
    for n in range(steps):
        Fn, it, rs = ens.step_mixed_dof(P, body_in, slip=slip, **kw)
        Fs.append(Fn); its.append(it); res.append(rs); cfgs.append(ens.get_config())
    ens.close()
    ens = make()
    out = ens.run(n_steps=steps, prescribed_dof=P, body_in=body_in, brownian=False, stride=2, slip=slip, **kw)
    Xr, Qr = ens.get_config()
    print("run of %d steps with component masks: iterations per replica %s, |X - X0| %.2e" % (steps, out.iters_sum, np.abs(Xr - X0).max()))
    assert np.array_equal(Xr, cfgs[-1][0]) and np.array_equal(Qr, cfgs[-1][1])
    assert out.X.shape == (3, R, nb, 3) and out.Q.shape == (3, R, nb, 4)
    Fsum = np.zeros((R, 6 * nb))
    for Fn in Fs:
        Fsum += Fn                                          # in step order, as the device adds them
    for k in range(3):
        assert np.array_equal(out.X[k], cfgs[2 * k + 1][0]) and np.array_equal(out.Q[k], cfgs[2 * k + 1][1]), k
        assert np.array_equal(out.F[k], Fs[2 * k + 1]), k
        assert np.array_equal(out.accepted_at[k], np.full(R, 2 * k + 2))
    assert np.array_equal(out.F_sum, Fsum) and np.array_equal(out.F_mean, Fsum / steps)
    assert np.array_equal(out.iters_sum, np.sum(its, axis=0)) and np.array_equal(out.resid_max, np.max(res, axis=0))
    assert np.array_equal(out.accepted, np.full(R, steps)) and not out.rejected.any()
    assert (out.steps_done, out.stopped_at) == (steps, -1)
    assert np.abs(Xr - X0).max() > 1e-5
    # the same run with Brownian steps at kBT = 1: the argument error, nothing moves
    with pytest.raises(RblError) as e:
        ens.run(n_steps=steps, prescribed_dof=P, body_in=body_in, brownian=True, stride=2, slip=slip, **kw)
    print("Brownian run with component masks: %s" % e.value)
    assert "[rbl status 11]" in str(e.value) and "ensemble_run" in str(e.value) and "Brownian" in str(e.value)
    Xc, Qc = ens.get_config()
    assert np.array_equal(Xc, Xr) and np.array_equal(Qc, Qr)
    ens.close()


# ---- 6. the force model ------------------------------------------------------------------------------------------------------------
def test_force_model_enters_the_free_components_only():
    """model on: the step of a model-free ensemble that is handed interaction_forces() in the free slots and zeros in the
    prescribed ones -- the same system, the same bits, per replica (test_force_model_enters_the_free_components_only of
    test_prescribed_dof_gpu.py and test_force_model_enters_the_free_bodies_only of test_ensemble_mixed_gpu.py)"""
    R, nb, wall = 6, 5, True
    c, X0, Q0 = _packed(R, nb, 9)
    model = _model(c["a"])
    P = np.random.default_rng(12).random((R, nb, 6)) < 0.5
    P[:, 1] = True                                          # a fully prescribed body, an all-free one, a roller, in every replica
    P[:, 2] = False
    P[:, 3] = [False, False, False, True, True, True]
    on, off = _ensemble(c, X0, Q0, wall, dt=1e-3, model=model), _ensemble(c, X0, Q0, wall, dt=1e-3)
    share = on.ensemble_interaction_forces()[0].reshape(R, nb, 6)
    assert np.abs(share[P]).max() > 1e-3 and np.abs(share[~P]).max() > 1e-3          # the model loads prescribed components too
    handed = np.where(P, 0.0, share).reshape(R, 6 * nb)
    Fa, ita, resa = on.ensemble_step_mixed_dof(P, np.zeros(6 * nb), max_iter=IT, rtol=1e-10)
    Fb, itb, resb = off.ensemble_step_mixed_dof(P, handed, max_iter=IT, rtol=1e-10)
    print("model on, component masks: iterations %s; |F_on - F_handed| %.2e" % (ita, np.abs(Fa - Fb).max()))
    assert np.all(ita > 0) and np.all(ita < IT)
    assert np.array_equal(ita, itb) and np.array_equal(resa, resb) and np.array_equal(Fa, Fb)
    (Xa, Qa), (Xb, Qb) = on.ensemble_get_config(), off.ensemble_get_config()
    assert np.array_equal(Xa, Xb) and np.array_equal(Qa, Qb)
    assert np.array_equal(Xa[:, 1], X0[:, 1]) and np.abs(Xa[:, 2] - X0[:, 2]).max() > 1e-6
    assert np.array_equal(Fa.reshape(R, nb, 6)[~P], handed.reshape(R, nb, 6)[~P])      # free loads echoed WITH the model's share
    assert np.abs(Fa.reshape(R, nb, 6)[P]).max() > 1e-3                                # holding takes a load
    # with the model's loads handed to the prescribed slots too they would be read as velocities: far more than rounding
    off.ensemble_set_config(X0, Q0)
    Fbad = off.ensemble_step_mixed_dof(P, share.reshape(R, 6 * nb), max_iter=IT, rtol=1e-10)[0]
    assert _rel(Fbad, Fa) > 1e-4
    pairs = 0
    for r in range(R):
        s = _single(c, X0[r], Q0[r], wall, dt=1e-3, model=model)
        s.interaction_forces()
        pairs += s.interaction_stats()[1]
        s.close()
    assert pairs > 0                                                                   # the steric model was exercised
    on.close()
    off.close()


# ---- 7. reproducibility, poisoned workspaces --------------------------------------------------------------------------------------
def _run(poison):
    """test_ensemble_mixed_gpu.py's _run(poison), with the _dof calls"""
    from rigid_body_light_amd._lib import DeviceContext
    from test_poisoned_workspace_gpu import _poison_env
    import torch
    R, nb, wall = 7, 5, True
    c, X0, Q0 = _packed(R, nb, 81)
    P = _masks6(R, nb, 82)
    bi, slip = _inputs6(P, 83, speed=0.2)
    with _poison_env(poison):
        ens = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=1e-3, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    assert ens.get_option("poison_workspace") == int(poison)
    ens.ensemble_set_config(X0, Q0)
    ens.set_interactions(**_model(c["a"]))
    out = list(ens.ensemble_solve_mixed_dof(P, bi, max_iter=120, rtol=1e-10, slip=slip))
    out += list(ens.ensemble_solve_mixed_dof(P, bi, max_iter=40, rtol=1e-6))           # few iterations: the basis in LDS
    for n in range(2):
        out += list(ens.ensemble_step_mixed_dof(P, bi, max_iter=120, rtol=1e-10, slip=slip))
    res, rc = ens.ensemble_run(3, prescribed=P, body_in=bi, brownian=False, stride=1, slip=slip, max_iter=120, rtol=1e-10, per=6)
    assert rc == 0
    out += [res.F_sum, res.X, res.Q, res.F, res.iters_sum, res.resid_max]
    out += list(ens.ensemble_get_config())
    ens.close()
    return out


def test_same_call_same_bits_and_no_read_of_unwritten_memory():
    assert _basis_in_lds(5, 40) and not _basis_in_lds(5, 120)
    a, b, p = _run(False), _run(False), _run(True)
    assert all(np.all(np.isfinite(x)) for x in a)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                                                    # the same calls twice
    for x, y in zip(a, p):
        assert np.array_equal(x, y)                                                    # poisoned workspaces: the same bits


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_first_failing_replica_and_move_nobody():
    """configurations that are invalid from the start, in one replica only (test_ensemble_mixed_gpu.py's error test)"""
    from rigid_body_light_amd._lib import RblError
    c = _shell12()
    R, nb, wall = 4, 3, True
    X0, Q0 = _configs(R, nb, wall)
    ens = _ensemble(c, X0, Q0, wall)
    Xa, Qa = ens.ensemble_get_config()
    P = np.zeros((R, nb, 6), dtype=np.uint8)
    P[:, 2, 3:] = 1                                          # body 2: a roller
    P[:, 0, 2] = 1                                           # body 0: z held
    bi = np.tile([0.0, 0.0, -1.0, 0.1, 0.0, 0.0], nb)
    bi[12:] = [0.0, 0.0, 0.0, 0.0, 0.3, 0.0]
    bi[2] = 0.0
    for bad, code, rep in (("overlap", 1, 2), ("below", 2, 1)):
        Xb, Qb = Xa.copy(), Qa.copy()
        if bad == "overlap":
            Xb[2, 1], Qb[2, 1] = Xb[2, 0], Qb[2, 0]           # two bodies of replica 2 on top of each other
        else:
            Xb[1, 0, 2] = -0.5                               # a body of replica 1 below the wall
        ens.ensemble_set_config(Xb, Qb)
        for call in (lambda: ens.ensemble_step_mixed_dof(P, bi, max_iter=40, rtol=1e-8),
                     lambda: ens.ensemble_solve_mixed_dof(P, bi, max_iter=40, rtol=1e-8)):
            with pytest.raises(RblError) as e:
                call()
            print("%s in replica %d: %s" % (bad, rep, e.value))
            assert "[rbl status %d]" % code in str(e.value) and ("replica %d" % rep) in str(e.value)
            Xc, Qc = ens.ensemble_get_config()
            assert np.array_equal(Xc, Xb) and np.array_equal(Qc, Qb)
        res, rc = ens.ensemble_run(3, prescribed=P, body_in=bi, brownian=False, max_iter=40, rtol=1e-8, per=6)
        assert rc == code and res.stop_replica == rep and res.steps_done == 0
        Xc, Qc = ens.ensemble_get_config()
        assert np.array_equal(Xc, Xb) and np.array_equal(Qc, Qb)
    ens.ensemble_set_config(Xa, Qa)
    two = P.copy()
    two[3, 0, 5] = 2
    for call in (lambda: ens.ensemble_step_mixed_dof(two, bi), lambda: ens.ensemble_solve_mixed_dof(two, bi)):
        with pytest.raises(RblError) as e:
            call()
        assert "[rbl status 11]" in str(e.value) and "0 or 1" in str(e.value) and "replica 3" in str(e.value)
    with pytest.raises(RblError) as e:
        ens.ensemble_step_mixed_dof(P, bi, max_iter=256, rtol=1e-8)
    assert "[rbl status 4]" in str(e.value)
    Xc, Qc = ens.ensemble_get_config()
    assert np.array_equal(Xc, Xa) and np.array_equal(Qc, Qa)
    ens.ensemble_step_mixed_dof(P, bi, max_iter=40, rtol=1e-8)                         # and the ensemble still steps
    assert np.array_equal(ens.ensemble_get_config()[0][:, 0, 2], Xa[:, 0, 2])          # z of body 0 held
    ens.close()


def test_a_shape_that_fits_unmasked_but_not_with_the_mask_is_a_size_error_that_names_the_entry_point():
    """test_ensemble_mixed_gpu.py's shape: 58 bodies of 3 blobs with max_iter = 63 take 151 000 of the one-kernel solver's 153 600
    bytes of LDS, the mask's 6 N_bod flags (2 784 bytes) no longer fit beside them -- RBL_ERR_SIZE from the _dof calls and from a
    run with component masks, before anything is launched; with fewer iterations the same calls run"""
    from rigid_body_light_amd._lib import DeviceContext, RblError
    import torch
    nb, R = 58, 2
    cfg = np.array([[0.6, 0.0, 0.0], [-0.3, 0.52, 0.0], [-0.3, -0.52, 0.0]])
    ens = DeviceContext(0.5, 1.0, True, cfg=cfg, dt=0.01, kBT=1.0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    X = np.zeros((R, nb, 3))
    X[:, :, 0] = 4.0 * (np.arange(nb) % 8)
    X[:, :, 1] = 4.0 * (np.arange(nb) // 8)
    X[:, :, 2] = 3.0
    Q = np.zeros((R, nb, 4))
    Q[:, :, 0] = 1.0
    ens.ensemble_set_config(X, Q)
    F = np.zeros((R, 6 * nb))
    F[:, 2::6] = -1.0
    its, res = ens.ensemble_step_deterministic(F, max_iter=63, rtol=1e-6)             # the unmasked step fits and runs
    assert np.all(its > 0) and np.all(np.isfinite(res))
    X1, Q1 = ens.ensemble_get_config()
    P = np.zeros((R, nb, 6), dtype=bool)
    P[:, :, 2] = True                                                                  # z of every body
    F[:, 2::6] = 0.0                                                                   # ... held
    for name, call in (("ensemble_step_mixed_dof", lambda: ens.ensemble_step_mixed_dof(P, F, max_iter=63, rtol=1e-6)),
                       ("ensemble_solve_mixed_dof", lambda: ens.ensemble_solve_mixed_dof(P, F, max_iter=63, rtol=1e-6)),
                       ("ensemble_run", lambda: ens.ensemble_run(2, prescribed=P, body_in=F, brownian=False, max_iter=63, rtol=1e-6, per=6))):
        with pytest.raises(RblError) as e:
            call()
        print("%s: %s" % (name, e.value))
        assert "[rbl status 4]" in str(e.value) and "without prescribed bodies" in str(e.value) and name in str(e.value)
    Xc, Qc = ens.ensemble_get_config()
    assert np.array_equal(Xc, X1) and np.array_equal(Qc, Q1)
    ens.ensemble_step_mixed_dof(P, F, max_iter=40, rtol=1e-6)                          # fewer iterations: the mask fits again
    assert np.array_equal(ens.ensemble_get_config()[0][:, :, 2], X1[:, :, 2])          # z held
    ens.close()


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------
def test_example_ensemble_microrollers_roll_the_way_they_spin():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ensemble_microrollers.py"), "--replicas", "8", "--steps", "2", "--omega"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    procs = [subprocess.Popen(cmd + [om], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for om in ("10.0", "-10.0")]
    ux = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, out[-2000:] + err[-2000:]
        rows = [l.split() for l in out.splitlines() if l.startswith("roller ")]
        assert len(rows) == 8
        vals = np.array([[float(v) for v in r[1:]] for r in rows])
        assert np.all(np.isfinite(vals))
        print("ensemble_microrollers: height/radius %s\n    U_x %s\n    torque about y %s" % (vals[:, 1], vals[:, 2], vals[:, 4]))
        ux.append(vals[:, 2])
    # a shell spinning about +y above the wall rolls towards +x (test_microroller_example_rolls_the_way_it_spins), at every height
    assert np.all(ux[0] > 0.0) and np.all(ux[1] < 0.0)
    assert np.all(np.abs(ux[0][:-1]) > np.abs(ux[0][1:]))                              # and the slower the higher it is
