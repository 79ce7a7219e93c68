"""The inputs of tests/test_body_shapes_gpu.py are sound before any kernel sees them (tests/body_shapes.py): touching blobs, bodies
apart, everything above the wall, M positive definite, and cond(A) of the saddle matrix under 1e4 -- measured here for every
shape, wall and lattice seed the GPU tests use, printed, and held against the figures recorded in body_shapes.COND_A, on which
the GPU tests' solution bounds 10 cond(A) rtol rest.  The cap is a condition on the inputs, not a tolerance on the code.

Measured (a = 0.5, eta = 1; G8 at eta = 0.5, see body_shapes.ETA_OF), free space / wall:
    few-blob shapes (trimer, tetra, bipyramid, fib(7); G1-G4, G9, S1, S3-S5, E1, E3, E4)   cond(M) <= 2.2e2, cond(A) <= 2.7e2
    fib(238) x 1, fib(255) x 3, fib(256) x 1 and x 2, fib(257) x 2                          cond(M) <= 4.7e2, cond(A) 5.8e3 .. 6.4e3
    fib(513) x 1                                                                            cond(M) 3.4e2, cond(A) 1.27e4 at eta = 1
                                                                                            (over the cap), 6.4e3 at eta = 0.5

Also here: the one-kernel solver's size rule as body_shapes.small_fits restates it, held against the library's own host-side
check.  It is the finding of this sweep that needs no GPU: the documented limits (256 blobs, 64 bodies) are not the binding
ones -- 64 tetrahedra, one body of 256 blobs and 36 bodies of 7 blobs are all refused, for LDS."""
import numpy as np
import pytest

import body_shapes as bs

COND_CAP = 1.0e4
RBL_ERR_SIZE = 4


def _seeds(name):
    """lattice seeds in use for a case: 0 for the single configuration, and those of the replicas of its ensembles"""
    seeds = {0}
    for ens, (R, _) in bs.ENSEMBLES.items():
        if bs.ensemble_case(ens) == name:
            seeds |= {bs.replica_seed(r) for r in range(R)}
    return sorted(seeds)


def _check_geometry(c, r, wall):
    a, nblb = c["a"], c["nblb"]
    r = r.reshape(-1, 3)
    assert bs.min_distance(c["cfg"]) >= 2 * a * (1 - 1e-12) or nblb == 1
    assert bs.min_distance(r) >= 2 * a * (1 - 1e-12) or r.shape[0] == 1          # no two blobs closer than touching
    if wall:
        assert r[:, 2].min() > a                                                  # every blob above the wall, undamped
    # the bodies do not interpenetrate: blobs of different bodies are further apart than touching ones
    if c["nb"] > 1:
        body = np.repeat(np.arange(c["nb"]), nblb)
        d = np.linalg.norm(r[:, None, :] - r[None, :, :], axis=2) if r.shape[0] <= 600 else None
        if d is not None:
            other = body[:, None] != body[None, :]
            assert d[other].min() > 2 * a + 0.25
        else:                                                                     # 900 blobs: centres apart by more than two bounding spheres
            X = c["X"]
            dc = np.linalg.norm(X[:, None, :] - X[None, :, :], axis=2) + np.eye(c["nb"]) * 1e9
            assert dc.min() > 2 * (bs.radius(c["cfg"]) + a) + 0.25


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name", list(bs.CASES))
def test_inputs_are_sound_and_their_condition_numbers_are_the_recorded_ones(orc, name, wall):
    worst_M = worst_A = 0.0
    seeds = _seeds(name)
    for seed in seeds:
        c = bs.case(name, wall, seed)
        M, K, Am, r = bs.dense(orc, c["cfg"], c["X"], c["Q"], c["a"], c["eta"], wall)
        _check_geometry(c, r, wall)
        np.linalg.cholesky(M)                                                     # raises unless M is positive definite
        n3 = M.shape[0]
        if seed == 0:                                                             # cond(M): the first configuration is enough
            e = np.linalg.eigvalsh(M)
            worst_M = float(e[-1] / e[0])
        worst_A = max(worst_A, bs.cond2(Am, n3))
    print("%s %-4s %3d x %3d blobs, %3d seed(s): cond(M) %.3e  cond(A) %.3e  (recorded %.3e)"
          % (name, "wall" if wall else "free", c["nb"], c["nblb"], len(seeds), worst_M, worst_A, bs.COND_A[(name, wall)]))
    assert worst_A < COND_CAP
    rec = bs.COND_A[(name, wall)]
    assert 0.9 * rec <= worst_A <= rec < COND_CAP                                 # the record is an upper bound, and not a loose one


def test_fib513_at_unit_viscosity_is_over_the_cap(orc):
    """why G8 runs at eta = 0.5: at eta = 1 its saddle matrix has cond(A) = 1.27e4"""
    c = bs.case("G8", False)
    M, K, Am, r = bs.dense(orc, c["cfg"], c["X"], c["Q"], c["a"], 1.0, False)
    k = bs.cond2(Am, M.shape[0])
    print("fib(513) x 1 at eta = 1: cond(A) %.4e" % k)
    assert 1.2e4 < k < 1.35e4


def _probe(shape_name, nb):
    """the library's host-side answer to `does N_bod x shape fit the one-kernel solver at max_iter = 1`: rbl_ensemble_set_config
    checks it before it touches the device (without a GPU an accepted shape ends in another status, not RBL_ERR_SIZE)"""
    from rigid_body_light_amd._lib import lib
    L = lib()
    cfg = np.ascontiguousarray(bs.shape(shape_name))
    h = L.rbl_create()
    try:
        assert L.rbl_set_parameters(h, bs.A, 0.01, 1.0, bs.ETA, cfg.ctypes.data, cfg.shape[0]) == 0
        X, Q = bs.lattice(nb, cfg, True)
        rc = L.rbl_ensemble_set_config(h, 1, nb, X[None].copy().ctypes.data, Q[None].copy().ctypes.data)
        return rc != RBL_ERR_SIZE, L.rbl_last_error(h).decode()
    finally:
        L.rbl_destroy(h)


@pytest.mark.parametrize("shape_name,nbs", [("trimer", (1, 63, 64, 65)), ("tetra", (49, 51, 53, 54, 64, 65)), ("bipyramid", (42, 43, 51)),
                                            ("fib7", (30, 32, 33, 36)), ("fib238", (1,)), ("fib252", (1,)), ("fib253", (1,)),
                                            ("fib256", (1,)), ("fib257", (1,))])
def test_the_restated_size_rule_is_the_librarys(shape_name, nbs):
    nblb = bs.shape(shape_name).shape[0]
    for nb in nbs:
        ok, msg = _probe(shape_name, nb)
        assert ok == bs.small_fits(nblb, nb, 1), (shape_name, nb, msg)
        if not ok:
            assert "one-kernel solver" in msg and "LDS" in msg


def test_which_cases_the_one_kernel_solver_takes():
    """S1, S2 and S4 satisfy N <= 256 and N_bod <= 64 and are refused all the same, at every iteration limit; S3 fits at some
    limits and not at others (the triangular factor moves out of LDS beyond 64 iterations); E1-E4 fit where the GPU tests use them"""
    def fits(name, m, mixed=False):
        sh, nb = bs.CASES[name]
        return bs.small_fits(bs.shape(sh).shape[0], nb, m, mixed)
    for name in ("S1", "S2", "S4", "G9", "G7"):
        assert not any(fits(name, m) for m in range(1, 256)), name
    assert [m for m in range(1, 256) if fits("S3", m)] == list(range(1, 39)) + list(range(65, 190))
    assert [m for m in range(1, 256) if fits("S3", m, True)] == list(range(1, 29)) + list(range(65, 113))
    assert all(fits("S5", m, True) for m in range(1, 256)) and not fits("S5", 256)
    for name, (R, m) in bs.ENSEMBLES.items():
        assert fits(bs.ensemble_case(name), m) == (bs.ensemble_case(name) not in ("S1", "S2", "S4")), name
    # E1-E3: one more body (or blob) no longer fits at max_iter = 255; E4: the same at max_iter = 100, masked or not
    assert fits("E1", 255) and not bs.small_fits(4, 50, 255)
    assert fits("E2", 255) and not bs.small_fits(239, 1, 255)
    assert fits("E3", 255) and not bs.small_fits(7, 31, 255)
    assert fits("E4", 100) and fits("E4", 100, True) and not bs.small_fits(4, 52, 100)


def test_the_launchers_size_arithmetic_is_the_restated_one(tmp_path):
    """The one launcher of the one-kernel solver (small_launch, rbl_small_solve.hpp) takes its LDS bytes, its Krylov basis bytes and
    the workspace of a replica from constexpr functions of the same header.  Without joints they are body_shapes' restatement --
    what the launcher's three predecessors computed, each for itself -- and the placement that follows from them (basis in LDS
    under 64 KB, in LDS with the attribute, in global memory) is the one the GPU tests count on at 2 bodies of 12 blobs.  Checked
    by the compiler: one static_assert per shape, host side only, nothing is run.  The C ABI's own figure (rbl_ensemble_joints_fit
    with no joints) is the same number"""
    import ctypes
    import os
    import subprocess
    from rigid_body_light_amd import build as B
    shapes = [(12, 2, 40), (12, 2, 100), (12, 2, 255), (12, 10, 64), (12, 10, 65), (3, 63, 38), (3, 64, 189), (238, 1, 255), (4, 49, 255),
              (7, 30, 1), (1, 1, 1), (12, 3, 100)]
    lines = ['#include "rbl_small_solve.hpp"']
    for nblb, nb, m in shapes:
        args = "%d, %d, %d" % (nblb, nb, m)
        lines.append('static_assert(small_work_doubles(%s) == %dull && small_work_doubles(%s, 0) == %dull, "workspace %s");'
                     % (args, bs.small_work_doubles(nblb, nb, m), args, bs.small_work_doubles(nblb, nb, m), args))
        for mixed in (False, True):
            lines.append('static_assert(small_lds_base_bytes(%s, %s) == %dull && small_lds_base_bytes(%s, %s, 0) == %dull, "LDS %s");'
                         % (args, str(mixed).lower(), bs.small_lds_bytes(nblb, nb, m, mixed), args, str(mixed).lower(),
                            bs.small_lds_bytes(nblb, nb, m, mixed), args))
        lines.append('static_assert(small_basis_bytes(%s) == %dull && small_basis_bytes(%s, 0) == %dull, "basis %s");'
                     % (args, bs.small_basis_bytes(nblb, nb, m), args, bs.small_basis_bytes(nblb, nb, m), args))
    # the jointed variant's vectors are 3 n_joints longer: the workspace and the basis grow by exactly that
    lines.append('static_assert(small_work_doubles(12, 3, 100, 4) == %dull + 101 * 12 && small_basis_bytes(12, 3, 100, 4) == %dull + 8 * 101 * 12, "joints");'
                 % (bs.small_work_doubles(12, 3, 100), bs.small_basis_bytes(12, 3, 100)))
    src = tmp_path / "sizes.hip"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([B.HIPCC, "-std=c++17", "-x", "hip", "--offload-host-only", "-fsyntax-only", "-I" + B.CSRC, str(src)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    # the three placements of the 2-body, 12-blob shape: the basis beside the vectors under 64 KB, above it, and not at all
    total = {m: bs.small_lds_bytes(12, 2, m) + bs.small_basis_bytes(12, 2, m) for m in (40, 100, 255)}
    assert total[40] <= 64 * 1024 < total[100] <= bs.SMALL_LDS_MAX < total[255] and bs.small_fits(12, 2, 255, True)
    L = ctypes.CDLL(os.path.join(os.path.dirname(B.CSRC), "librbl.so"))
    for nblb, nb, m in shapes:
        lds = ctypes.c_int64(0)
        fit = L.rbl_ensemble_joints_fit(nblb, nb, m, 0, ctypes.byref(lds))
        assert lds.value == bs.small_lds_bytes(nblb, nb, m) and bool(fit) == bs.small_fits(nblb, nb, m), (nblb, nb, m)
