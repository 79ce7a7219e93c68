"""The pair arithmetic of rigid_body_light_amd/csrc/rbl_pair.hpp in the shared length unit (coordinates divided by a / lambda,
lambda^2 = 3, every coefficient divided by lambda -- RBL_UNIT_SHARED, what the product kernels run), one pair at a time on the CPU:
the host build of tests/host_pair_units against the two reference fixtures tests/golden/pair_kernels.json and
pair_blocks_assembly.json (outputs of the reference's own compiled pair functions).

Figure: the worst error of the block the five scalars describe (nine entries, rbl_pair_block_fast; the ordered accumulation and the
symmetric form likewise), relative to the block's largest entry, over both fixtures -- and the same error on the suite's scale
max(|block|_F, free-space scale).  The form before the shared unit (radius units, the same harness built with -DPAIR_UNITS_RADIUS over
the previous header) gave PARENT_WORST = 4.31e-13 / 8.91e-15; the shared unit may exceed either by at most a factor 1.5 -- a changed
operation order moves last bits, a lost digit would show as 10 x.  Measured: 5.29e-13 / 1.14e-14 (x 1.23 / x 1.28); profiles/pair_units.md.
M_ji = M_ij^T must hold with the roles swapped: rbl_pair_symv evaluates one direction and applies the transpose."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O2", "-ffp-contract=fast", "-mfma", "-std=c++17", "-shared", "-fPIC"]
# the radius-unit form before the shared unit, measured with this harness over the previous header: (error / largest entry of the block,
# error / max(|block|_F, free-space scale)).  The second scale is the one the project's record of 9.5e-15 was taken with
PARENT_WORST = (4.3088e-13, 8.9139e-15)
FACTOR = 1.5


def build(outdir, extra=()):
    so = os.path.join(str(outdir), "libpair_units.so")
    subprocess.check_call(["g++"] + FLAGS + list(extra) + ["-I" + os.path.join(HERE, "host_pair"), "-o", so,
                                                            os.path.join(HERE, "host_pair_units", "pair_units_host.cpp")])
    return so


class Units:
    def __init__(self, so):
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        for fn in (L.units_block, L.units_accum):
            fn.argtypes = [dp, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp]
            fn.restype = C.c_uint
        L.units_sym.argtypes = [dp, dp, C.c_double, C.c_int, C.c_int, dp, dp]
        L.units_sym.restype = C.c_uint
        self.L, self.dp = L, dp

    def _p(self, x):
        return x.ctypes.data_as(self.dp)

    def _one(self, fn, ri, rj, i, j, a, wall):
        ri = np.ascontiguousarray(ri, dtype=np.float64); rj = np.ascontiguousarray(rj, dtype=np.float64)
        out = np.zeros(9)
        flags = fn(self._p(ri), self._p(rj), i, j, a, int(wall), self._p(out))
        return out.reshape(3, 3), flags

    def block(self, ri, rj, i, j, a, wall):
        return self._one(self.L.units_block, ri, rj, i, j, a, wall)

    def accum(self, ri, rj, i, j, a, wall):
        return self._one(self.L.units_accum, ri, rj, i, j, a, wall)

    def sym(self, ri, rj, a, wall, nearchk=1):
        ri = np.ascontiguousarray(ri, dtype=np.float64); rj = np.ascontiguousarray(rj, dtype=np.float64)
        mij, mji = np.zeros(9), np.zeros(9)
        flags = self.L.units_sym(self._p(ri), self._p(rj), a, int(wall), nearchk, self._p(mij), self._p(mji))
        return mij.reshape(3, 3), mji.reshape(3, 3), flags


def fixture_cases():
    """[(ri, rj, i, j, a, wall, reference block in units of 1 / (8 pi eta a))] of both fixtures, without the pairs the fast forms
    refuse (a blob below the wall)"""
    unhex = lambda v: np.array([float.fromhex(x) for x in v])
    cases = []
    with open(os.path.join(HERE, "golden", "pair_kernels.json")) as f:
        g = json.load(f)
    for c in g["rpy"]:                                    # free space: r = r_i - r_j
        o = unhex(c["out6"])
        cases.append((unhex(c["r"]), np.zeros(3), c["i"], c["j"], 1.0 / float.fromhex(c["inv_a"]), False,
                      o[[0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(3, 3)))
    for c in g["wall"]:                                   # args in radii: (dx, dy, z_i + z_j, z_j); M_out = free-space block + wall part
        dx, dy, Rz, hj = unhex(c["args"])
        cases.append((np.array([dx, dy, Rz - hj]), np.array([0.0, 0.0, hj]), c["i"], c["j"], 1.0, True, unhex(c["M_out"]).reshape(3, 3)))
    with open(os.path.join(HERE, "golden", "pair_blocks_assembly.json")) as f:
        g = json.load(f)
    for c in g["blocks"]:
        ri, rj = unhex(c["ri"]), unhex(c["rj"])
        if c["wall"] and (ri[2] < 0.0 or rj[2] < 0.0):
            continue
        cases.append((ri, rj, c["i"], c["j"], float.fromhex(c["a"]), bool(c["wall"]), unhex(c["out9"]).reshape(3, 3)))
    return cases


def worst_errors(u, cases):
    """{form: (worst max |got - ref| / max |ref|,  worst max |got - ref| / max(|ref|_F, free-space scale))} over the cases.  The first is
    the figure as stated (it is large where the wall part cancels the free-space part: two blobs near the wall, block << 1 / r^); the
    second is the suite's scale (tests/test_gpu_parity.py) and the one the project's record of 9.5e-15 was taken with"""
    w = {k: [0.0, 0.0] for k in ("block", "accum", "sym_ij", "sym_ji")}
    for ri, rj, i, j, a, wall, ref in cases:
        rhat = np.linalg.norm(ri - rj) / a
        scales = (np.abs(ref).max(), max(np.linalg.norm(ref), min(4.0 / 3.0, 1.0 / max(rhat, 1e-30))))
        got = {"block": u.block(ri, rj, i, j, a, wall)[0], "accum": u.accum(ri, rj, i, j, a, wall)[0]}
        if i != j:
            mij, mji, _ = u.sym(ri, rj, a, wall)
            got["sym_ij"], got["sym_ji"] = mij, mji.T
        for k, m in got.items():
            e = float(np.abs(m - ref).max())
            w[k] = [max(w[k][0], e / scales[0]), max(w[k][1], e / scales[1])]
    return w


def worst(w):
    return max(v[0] for v in w.values()), max(v[1] for v in w.values())


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    return Units(build(tmp_path_factory.mktemp("pair_units")))


@pytest.fixture(scope="module")
def cases():
    return fixture_cases()


def test_fixtures_hold_every_regime(cases):
    assert len(cases) > 1400
    rhat = np.array([np.linalg.norm(c[0] - c[1]) / c[4] for c in cases])
    same = np.array([c[2] == c[3] for c in cases])
    wall = np.array([c[5] for c in cases])
    assert (same & wall).sum() >= 5 and (~same & (rhat < 2.0)).sum() > 50 and (~same & wall & (rhat > 2.0)).sum() > 300
    assert (np.abs(rhat - 2.0) < 1e-8).sum() > 50                                  # the switch between the two formulas


def test_shared_unit_loses_no_digit(units, cases):
    w = worst_errors(units, cases)
    for k, v in sorted(w.items()):
        print("shared unit %-7s worst error / largest entry %.4e (before %.4e)   / suite scale %.4e (before %.4e)" % (
            k, v[0], PARENT_WORST[0], v[1], PARENT_WORST[1]))
    got = worst(w)
    assert got[0] <= FACTOR * PARENT_WORST[0] and got[1] <= FACTOR * PARENT_WORST[1], w


def test_radius_unit_form_still_gives_its_figure(tmp_path, cases):
    """the header's radius-unit form (what tests/host_pair runs) through the same harness: the figures the bound is made of"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    w = worst_errors(Units(build(tmp_path, ["-DPAIR_UNITS_RADIUS"])), cases)
    got = worst(w)
    print("radius units: %.4e %.4e" % got)
    assert got[0] <= PARENT_WORST[0] * 1.0001 and got[1] <= PARENT_WORST[1] * 1.0001, w


def test_transpose_with_the_roles_swapped(units, cases):
    """rbl_pair_symv evaluates the coefficients for one direction (h = z_j) and applies the transpose for the other: the block evaluated
    with the roles swapped must be that transpose -- cF, beta, mzz symmetric in the roles, gxz <-> -gzx with dl -> -dl.  In exact
    arithmetic an identity; in floating point the two evaluations round on their own (the form before the shared unit differs in 146 of
    these pairs too), and each lies within the fixture bound of the reference: their difference is held to twice that bound, on the
    suite's scale.  A coefficient that does not swap (a g where a k belongs) is an error of order one."""
    n, top = 0, 0.0
    for ri, rj, i, j, a, wall, ref in cases:
        if i == j:
            continue
        scale = max(np.linalg.norm(ref), min(4.0 / 3.0, a / np.linalg.norm(ri - rj)))
        bij, _ = units.block(ri, rj, 0, 1, a, wall)
        bji, _ = units.block(rj, ri, 0, 1, a, wall)
        mij, mji, _ = units.sym(ri, rj, a, wall)
        sij, sji, _ = units.sym(rj, ri, a, wall)
        top = max(top, np.abs(bij - bji.T).max() / scale, np.abs(mji - sij).max() / scale, np.abs(mij - sji).max() / scale)
        n += 1
    print("roles swapped: worst difference %.3e of the scale" % top)
    assert n > 1300 and top <= 2.0 * FACTOR * PARENT_WORST[1]


def test_overlap_verdict_at_the_same_separation(units):
    """the overlap flag at r < 1e-12 a and not above it, in every form, for three radii; across the 2a switch the block is continuous"""
    OVERLAP = 1
    for a in (1.0, 0.06752768, 2.5):
        rj = np.array([0.0, 0.0, 3.0 * a])
        for fac, want in ((0.5e-12, OVERLAP), (0.99e-12, OVERLAP), (1.01e-12, 0), (1e-6, 0)):
            ri = np.array([fac * a, 0.0, 3.0 * a])       # (a separation this small only exists next to a zero coordinate)
            for wall in (False, True):
                assert units.block(ri, rj, 0, 1, a, wall)[1] & OVERLAP == want, (a, fac, wall)
                assert units.sym(ri, rj, a, wall)[2] & OVERLAP == want, (a, fac, wall)
                assert units.accum(ri, rj, 0, 1, a, wall)[1] & OVERLAP == want, (a, fac, wall)
        for wall in (False, True):
            lo = units.block(np.array([2.0 * (1 - 1e-13) * a, 0, 2.5 * a]), np.array([0, 0, 2.5 * a]), 0, 1, a, wall)[0]
            hi = units.block(np.array([2.0 * (1 + 1e-13) * a, 0, 2.5 * a]), np.array([0, 0, 2.5 * a]), 0, 1, a, wall)[0]
            assert np.abs(lo - hi).max() < 1e-12
