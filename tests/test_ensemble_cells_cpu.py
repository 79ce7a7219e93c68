"""A periodic cell per replica of an ensemble (include/rbl.h section 5: rbl_ensemble_set_cells, rbl_ensemble_get_cells) without a
GPU: the entry points are declared and exported, every argument refusal has its status, its message and its replica on a context
that has never seen a device -- they stand before the "no ensemble" refusal, where rbl_ensemble_set_periodic's stand --, the Python
wrappers check their arguments before the library is called, and the oracle's B M_per B is positive definite at every (shape, cell,
images) triple at which tests/test_ensemble_cells_gpu.py takes a Brownian step: the cases below are the ones that file imports.
No device is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402

vp, dbl, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
ERR_STATE, ERR_ARG = 7, 11
INF, NAN = float("inf"), float("nan")
ETA = 1.0


# ---- the cells of the GPU tests --------------------------------------------------------------------------------------------------
def scaled(L, s):
    """the cell L with its lengths scaled by s = (sx, sy); sy = 0 leaves y open"""
    return (L[0] * s[0], L[1] * s[1])


# shape A (pc.layers("tetra", 4, 2, 2, seed=r), replica r): four cells, the last with y open, and the images they are used with
A_SCALES = [(1.0, 1.0), (1.15, 1.15), (1.4, 1.25), (1.0, 0.0)]
A_IMAGES = [(1, 1), (2, 1), (1, 2), (3, 0)]
# shape D (pc.layer10() and two displaced copies): three cells
D_SCALES = [(1.0, 1.0), (1.2, 1.1), (1.5, 1.5)]
D_IMAGES = [(1, 1), (2, 1), (1, 2)]


def case_A(r):
    return pc.layers("tetra", 4, 2, 2, seed=r)


def D_replicas():
    """D itself and two copies with the bodies displaced by up to 0.05 (tests/test_ensemble_periodic_gpu.py's)"""
    c = pc.layer10()
    rng = np.random.default_rng(51)
    X = np.stack([c["X"], c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape), c["X"] + rng.uniform(-0.05, 0.05, c["X"].shape)])
    return c, X, np.stack([c["Q"]] * 3)


# the overlap test: A's replicas with body 1 one cell length of the SMALL cell (replica 1's) from body 0 and turned like it -- blob on
# blob through replica 1's boundary, 0.4 and 0.5 cell lengths of the small cell away in the two larger cells
OVERLAP_SCALES = [(1.4, 1.25), (1.0, 1.0), (1.5, 1.3)]


def overlap_case():
    cases = [case_A(s) for s in (0, 1, 2)]
    X, Q = np.stack([c["X"] for c in cases]), np.stack([c["Q"] for c in cases])
    Q = Q / np.linalg.norm(Q, axis=2, keepdims=True)
    for r in range(3):
        X[r, 1] = X[r, 0] + [cases[0]["L"][0], 0.0, 0.0]
        Q[r, 1] = Q[r, 0]
    return cases[0], X, Q


def brownian_triples():
    """(label, cfg, X, Q, a, L, images) of every replica that takes a Brownian step on the GPU: A with the shared (1, 1) images and
    with its own, D in its three cells, D's three replicas in the one cell of the equal-rows test, and the two replicas of the
    overlap test that have to step while replica 1 fails"""
    out = []
    for r in range(4):
        c = case_A(r)
        for n in sorted({(1, 1) if A_SCALES[r][1] else (1, 0), A_IMAGES[r]}):
            out.append(("A seed %d" % r, c["cfg"], c["X"], c["Q"], c["a"], scaled(c["L"], A_SCALES[r]), n))
    c, X, Q = D_replicas()
    for r in range(3):
        out.append(("D replica %d" % r, c["cfg"], X[r], Q[r], c["a"], scaled(c["L"], D_SCALES[r]), D_IMAGES[r]))
        if r:
            out.append(("D replica %d, shared cell" % r, c["cfg"], X[r], Q[r], c["a"], c["L"], (1, 1)))
    c, X, Q = overlap_case()
    for r in (0, 2):
        out.append(("A seed %d with body 1 moved" % r, c["cfg"], X[r], Q[r], c["a"], scaled(c["L"], OVERLAP_SCALES[r]), (1, 1)))
    return out


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    L.rbl_create.restype = vp
    L.rbl_destroy.argtypes = [vp]
    L.rbl_last_error.restype = ctypes.c_char_p
    L.rbl_last_error.argtypes = [vp]
    L.rbl_set_parameters.argtypes = [vp, dbl, dbl, dbl, dbl, vp, cint]
    L.rbl_set_comm_ops.argtypes = [vp, cint, cint, vp, vp, vp]
    L.rbl_ensemble_set_cells.argtypes = [vp, cint, vp, vp, vp, vp, cint]
    L.rbl_ensemble_get_cells.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.rbl_ensemble_get_periodic.argtypes = [vp, vp, vp, vp, vp, vp]
    return L


def _context(L, a):
    h = L.rbl_create()
    cfg = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5
    assert L.rbl_set_parameters(h, a, 0.01, 1.0, 1.0, cfg.ctypes.data, 4) == 0
    return h


def _set(L, h, Lx, Ly, nx, ny, on=1, R=None):
    Lx, Ly = np.array(Lx, dtype=np.float64), np.array(Ly, dtype=np.float64)
    nx, ny = np.array(nx, dtype=np.int32), np.array(ny, dtype=np.int32)
    return L.rbl_ensemble_set_cells(h, Lx.size if R is None else R, Lx.ctypes.data, Ly.ctypes.data, nx.ctypes.data, ny.ctypes.data, on)


def test_the_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for n in ("rbl_ensemble_set_cells", "rbl_ensemble_get_cells"):
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?rbl_ctx\s*\*\s*ctx" % n, code), n
        assert hasattr(L, n), n
    sec5 = text[text.index("5. Ensembles of independent replicas"):text.index("6. Fluid velocity")]
    assert "rbl_ensemble_set_cells" in sec5 and "rbl_ensemble_get_cells" in sec5


def test_every_argument_refusal_has_its_status_its_message_and_its_replica_and_stands_before_the_ensemble_check():
    """none of these contexts holds an ensemble, and none has a device: an argument refusal is what comes back, RBL_ERR_ARG naming
    the replica and the value; arguments that pass meet the "no ensemble" refusal, RBL_ERR_STATE"""
    L = _lib()
    h = _context(L, a=0.25)                                       # 4a = 1
    try:
        def bad(args, *words, code=ERR_ARG, **kw):
            assert _set(L, h, *args, **kw) == code, args
            msg = L.rbl_last_error(h).decode()
            for w in ("ensemble_set_cells",) + words:
                assert w in msg, (w, msg)
            # nothing is stored: the shared cell's query still answers (it refuses while cells per replica are stored), with zeros
            v = (dbl(-1.0), dbl(-1.0), cint(-1), cint(-1), cint(-1))
            assert L.rbl_ensemble_get_periodic(h, *[ctypes.byref(x) for x in v]) == 0
            assert [x.value for x in v] == [0.0, 0.0, 0, 0, 0]

        ok3 = ([7.0, 7.0, 7.0], [7.5, 7.5, 7.5], [1, 1, 1], [1, 1, 1])
        # a wrong R (without an ensemble: R < 1), a NULL array
        bad(ok3, "R = 0", R=0)
        bad(ok3, "R = -2", R=-2)
        arr = np.ones(3), np.ones(3, dtype=np.int32)
        for k in range(4):
            p = [arr[0].ctypes.data, arr[0].ctypes.data, arr[1].ctypes.data, arr[1].ctypes.data]
            p[k] = None
            assert L.rbl_ensemble_set_cells(h, 3, *p, 1) == ERR_ARG and b"NULL" in L.rbl_last_error(h)
        # replica k's values: the shared cell's checks in its order, the first offending replica named
        for k in range(3):
            for v in (NAN, INF, -INF, -1.0):
                Lx = [7.0] * 3
                Lx[k] = v
                bad((Lx, [7.5] * 3, [1] * 3, [1] * 3), "replica %d: Lx" % k, "finite")
                bad(([7.5] * 3, Lx, [1] * 3, [1] * 3), "replica %d: Ly" % k, "finite")
                bad((Lx, [7.5] * 3, [1] * 3, [1] * 3), "replica %d: Lx" % k, on=0)      # also while it would be stored switched off
            for n in (0, -1, 17):
                nn = [1] * 3
                nn[k] = n
                bad(([7.0] * 3, [7.5] * 3, nn, [1] * 3), "replica %d: nx = %d" % (k, n), "[1, 16]")
                bad(([7.0] * 3, [7.5] * 3, [1] * 3, nn), "replica %d: ny = %d" % (k, n), "[1, 16]")
            Lx, Ly = [7.0] * 3, [7.5] * 3
            Lx[k] = Ly[k] = 0.0
            bad((Lx, Ly, [1] * 3, [1] * 3), "replica %d: Lx = 0" % k, "Ly = 0")
            Lx = [7.0] * 3
            Lx[k] = 1.0                                               # L = 4a exactly is refused
            bad((Lx, [7.5] * 3, [1] * 3, [1] * 3), "replica %d: Lx" % k, "4a")
        bad(([7.0, NAN, -1.0], [7.5] * 3, [1, 1, 0], [1] * 3), "replica 1: Lx")          # the FIRST offending replica
        bad(([7.0, 7.0, 7.0], [7.5, 7.5, 0.5], [1, 0, 1], [1] * 3), "replica 1: nx = 0")  # replica by replica: 1's n before 2's length
        # arguments that pass, a replica with an open axis among them (its n is not looked at): the context holds no ensemble
        for args in (ok3, ([7.0, 0.0, 9.0], [7.5, 7.5, 0.0], [2, 17, 1], [3, 1, -4]), ([0.0] * 2, [0.0] * 2, [0] * 2, [0] * 2)):
            bad(args, "ensemble", "rbl_ensemble_set_config", code=ERR_STATE, on=0 if args[0][0] == 0.0 else 1)
        # a communicator is refused before the ensemble is looked for, after the arguments
        CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
        cb = CB(lambda user, buf, n: 0)
        assert L.rbl_set_comm_ops(h, 0, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
        bad(ok3, "communicator")
        bad(([7.0, 7.0, 7.0], [7.5] * 3, [1, 1, 0], [1] * 3), "replica 2: nx = 0")
        assert L.rbl_set_comm_ops(h, 0, 1, None, None, None) == 0
        # the query without an ensemble, and both calls without a context
        assert L.rbl_ensemble_get_cells(h, None, None, None, None, None, None) == ERR_STATE
        assert b"rbl_ensemble_set_config" in L.rbl_last_error(h)
        assert _set(L, None, *ok3) == ERR_ARG
        assert L.rbl_ensemble_get_cells(None, None, None, None, None, None, None) == ERR_ARG
    finally:
        L.rbl_destroy(h)
    # before rbl_set_parameters no radius is known: the 4a check waits, the "no ensemble" refusal does not
    h = L.rbl_create()
    try:
        assert _set(L, h, [1e-3, 2e-3], [0.0, 0.0], [1, 1], [0, 0]) == ERR_STATE and b"ensemble" in L.rbl_last_error(h)
        assert _set(L, h, [1e-3, -1.0], [0.0, 0.0], [1, 1], [0, 0]) == ERR_ARG and b"replica 1: Lx" in L.rbl_last_error(h)
    finally:
        L.rbl_destroy(h)


class _NoLibrary:
    """stands where the extension object would: any call into the library fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_python_wrappers_check_before_the_library():
    from rigid_body_light_amd import Ensemble
    from rigid_body_light_amd._lib import DeviceContext, cells_args
    ctx = DeviceContext.__new__(DeviceContext)
    ctx.L = ctx.h = _NoLibrary()
    ctx._borrowed = True
    ens = Ensemble.__new__(Ensemble)
    ens.ctx = _NoLibrary()
    ens.R, ens.N_bodies = 3, 4
    three = np.array([7.0, 8.0, 9.0])
    for Lx, Ly, images, exc, word in (("7", 7.0, (1, 1), TypeError, "Lx"), (7.0, None, (1, 1), TypeError, "Ly"),
                                      (7.0, True, (1, 1), TypeError, "Ly"), (three, np.array([True, False, True]), (1, 1), TypeError, "Ly"),
                                      (three, np.array(["a", "b", "c"]), (1, 1), TypeError, "Ly"),
                                      (three.reshape(3, 1), 7.0, (1, 1), ValueError, "Lx"), (np.zeros(0), 7.0, (1, 1), ValueError, "Lx"),
                                      (7.0, 7.0, 1, ValueError, "images"), (7.0, 7.0, (1, 1, 1), ValueError, "images"),
                                      (7.0, 7.0, (1.0, 1), TypeError, "images"), (7.0, 7.0, (1,), ValueError, "images"),
                                      (7.0, 7.0, np.ones((3, 3), dtype=int), ValueError, "images"),
                                      (7.0, 7.0, np.ones((3, 2)), TypeError, "images"), (7.0, 7.0, np.array([True, False]), TypeError, "images"),
                                      (three, np.array([7.0, 8.0]), (1, 1), ValueError, "Ly"),
                                      (three, 7.0, np.ones((2, 2), dtype=int), ValueError, "images")):
        with pytest.raises(exc, match=word):
            ctx.ensemble_set_cells(Lx, Ly, images=images)
        with pytest.raises(exc, match=word):
            ens.set_cells(Lx, Ly, images=images)
    # the ensemble knows its R: arrays of another length are refused there before the library is called
    with pytest.raises(ValueError, match="R = 3"):
        ens.set_cells(np.array([7.0, 8.0]), 7.0)
    with pytest.raises(ValueError, match="R = 3"):
        ens.set_cells(7.0, 7.0, images=np.ones((4, 2), dtype=int))
    # scalars broadcast, arrays pass through, images become (R, 2) of int32
    Lx, Ly, n = cells_args("t", 7.0, three, (2, 1), 3)
    assert Lx.tolist() == [7.0] * 3 and Ly.tolist() == three.tolist() and n.tolist() == [[2, 1]] * 3 and n.dtype == np.int32
    Lx, Ly, n = cells_args("t", [7, 8, 9], 0.0, [[1, 0], [2, 0], [3, 0]])
    assert Lx.tolist() == [7.0, 8.0, 9.0] and Ly.tolist() == [0.0] * 3 and n.tolist() == [[1, 0], [2, 0], [3, 0]]
    for name in ("ensemble_set_cells", "ensemble_cells"):
        assert callable(getattr(DeviceContext, name)), name
    for name in ("set_cells", "cells", "area_fraction"):
        assert callable(getattr(Ensemble, name)), name


def test_area_fraction_labels_the_replicas_that_are_periodic_in_both_axes():
    from rigid_body_light_amd import Ensemble

    class _Cells:
        def ensemble_cells(self):
            return dict(on=True, per_replica=True, Lx=np.array([10.0, 20.0, 10.0]), Ly=np.array([5.0, 5.0, 0.0]),
                        images=np.array([[1, 1], [1, 1], [1, 0]]))
    ens = Ensemble.__new__(Ensemble)
    ens.ctx, ens.R, ens.N_bodies = _Cells(), 3, 4
    phi = ens.area_fraction(2.5)
    assert phi[0] == 4 * 2.5 / 50.0 and phi[1] == 4 * 2.5 / 100.0 and np.isnan(phi[2])


# ---- positivity where the GPU tests take roots -------------------------------------------------------------------------------------
def test_M_per_is_positive_definite_at_every_cell_where_the_gpu_tests_take_a_brownian_step(orc):
    """the smallest eigenvalue of the oracle's B M_per B for every triple of brownian_triples(): recorded, only its sign asserted
    (positivity of the truncated sum is observed, not proven), with the symmetry that the Cholesky factor presumes"""
    for label, cfg, X, Q, a, L, n in brownian_triples():
        M, _, _ = po.dense_matrices(orc, cfg, X, Q, a, ETA, L, n)
        lam = np.linalg.eigvalsh(0.5 * (M + M.T)).min()
        print("%s, cell %.3f x %.3f, images %s: smallest eigenvalue %.5f" % (label, L[0], L[1], n, lam))
        assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
        assert lam > 0.0, (label, L, n, lam)
