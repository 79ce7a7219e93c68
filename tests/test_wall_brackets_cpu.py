"""The wall pair coefficients with the polynomial brackets kept un-multiplied (rbl_wall_coeffs of rigid_body_light_amd/csrc/rbl_pair.hpp,
shared length unit: cF = (A - w) + w^3 X, beta = Bw + w^5 Y, T1 / e_z = u (Y - 60 u), zz bracket w^3 [u (180v - 24) - v (Y + 12)]) against
the form they replace (b1 = -1 + u X, b2p = u Y and u^2 formed, multiplied by w and w^3), restated in
tests/host_wall_brackets/wall_brackets_host.cpp: the five scalars cF, beta, gxz, gzx, mzz of one pair, host build, pair by pair.

Inputs: the wall pairs of the two reference fixtures (tests/golden/pair_kernels.json, pair_blocks_assembly.json) and edge inputs --
one blob straight above the other (q = 0, v = 1), two blobs just above the wall far apart (Rz^2 << q, v -> 0), heights of 1.000001 a,
and R / r from 1 to 1e3 (a pair 2 a apart up to 1e3 a above the wall; a pair at 1.000001 a up to 2e3 a apart).

Bound: the two forms are the same polynomial in other groupings, so they may differ by roundings alone: 16 eps of max(|A|, a / r), the
free-space size of the block, for each scalar taken at the size of the block entries it makes (beta r^2, gxz r, gzx r: the lateral
scalars multiply dl, |dl| <= r) -- 16 roundings of that size; a constant off by one unit in the last place of a 1e-9 would show as 1e6 eps.
Measured: worst 1.60 eps (3.6e-16; beta r^2 and mzz) over the fixtures' 709 wall pairs, 1.32 eps (2.9e-16; mzz) over the 498 edge inputs;
cF 1.1 eps, gxz r and gzx r under 0.9 eps on both."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_pair_units_cpu import FLAGS, fixture_cases  # noqa: E402  (the same fixtures, the same compiler flags)

EPS = 2.0 ** -52
BOUND = 16.0 * EPS
NAMES = ("cF", "beta r^2", "gxz r", "gzx r", "mzz")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    so = os.path.join(str(tmp_path_factory.mktemp("wall_brackets")), "libwall_brackets.so")
    subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "host_pair"), "-o", so,
                                             os.path.join(HERE, "host_wall_brackets", "wall_brackets_host.cpp")])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.wall_brackets_pair.argtypes = [dp, dp, C.c_double, dp, dp, dp]
    L.wall_brackets_pair.restype = None

    def one(ri, rj, a):
        ri = np.ascontiguousarray(ri, dtype=np.float64); rj = np.ascontiguousarray(rj, dtype=np.float64)
        now, before, scale = np.zeros(5), np.zeros(5), np.zeros(2)
        L.wall_brackets_pair(ri.ctypes.data_as(dp), rj.ctypes.data_as(dp), a, now.ctypes.data_as(dp), before.ctypes.data_as(dp),
                             scale.ctypes.data_as(dp))
        return now, before, float(np.abs(scale).max())
    return one


def _worst(pair, pairs):
    """worst |now - before| / max(|A|, a / r) per scalar over (ri, rj, a) pairs, with the pair it came from"""
    worst, where = np.zeros(5), [None] * 5
    for ri, rj, a in pairs:
        now, before, scale = pair(ri, rj, a)
        assert np.isfinite(now).all() and np.isfinite(before).all() and scale > 0.0, (ri, rj, a)
        e = np.abs(now - before) / scale
        for k in range(5):
            if e[k] > worst[k]:
                worst[k], where[k] = e[k], (ri, rj, a)
    return worst, where


def edge_pairs():
    out = []
    for a in (1.0, 0.06752768, 2.5):
        near = 1.000001 * a
        for h in (1.000001, 1.5, 7.0, 333.0, 1e3):                       # one above the other: q = 0, v = 1
            for gap in (1.2, 2.0, 2.0000001, 3.7, 50.0):                 # (1.2: the near formula of the free-space part)
                out.append((np.array([0.3 * a, -0.2 * a, h * a + gap * a]), np.array([0.3 * a, -0.2 * a, h * a]), a))
                out.append((np.array([0.3 * a, -0.2 * a, h * a]), np.array([0.3 * a, -0.2 * a, h * a + gap * a]), a))
        for d in (2.0, 2.5, 10.0, 100.0, 1e3, 2e3):                      # both at 1.000001 a: Rz^2 << q, v -> 0, R / r -> 1
            for th in (0.0, 0.7, 2.9):
                out.append((np.array([d * a * np.cos(th), d * a * np.sin(th), near]), np.array([0.0, 0.0, near]), a))
                out.append((np.array([0.0, 0.0, near]), np.array([d * a * np.cos(th), d * a * np.sin(th), 1.3 * a]), a))
        for h in (1.000001, 2.0, 10.0, 100.0, 1e3):                      # a pair 2 a .. 2.5 a apart at height h: R / r = 1 .. 1e3
            for dirn in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8), (0.48, 0.64, 0.6)):
                for sep in (2.0, 2.5):
                    rj = np.array([0.0, 0.0, h * a])
                    out.append((rj + sep * a * np.array(dirn), rj, a))
                    out.append((rj, rj + sep * a * np.array(dirn), a))
    return out


def test_edge_inputs_cover_the_regimes():
    P = edge_pairs()
    q = np.array([((ri - rj)[:2] ** 2).sum() / a ** 2 for ri, rj, a in P])
    Rz = np.array([(ri[2] + rj[2]) / a for ri, rj, a in P])
    r = np.array([np.linalg.norm(ri - rj) / a for ri, rj, a in P])
    R = np.sqrt(q + Rz ** 2)
    zmin = np.array([min(ri[2], rj[2]) / a for ri, rj, a in P])
    assert (q == 0.0).sum() >= 50 and (Rz ** 2 < 2e-6 * q).sum() >= 6                   # v = 1 and v -> 0
    assert (np.abs(zmin - 1.000001) < 1e-12).sum() >= 50
    assert (R / r).min() < 1.000002 and (R / r).max() >= 1e3 - 1 and (r < 2.0).sum() >= 10


def test_fixture_pairs_agree_with_the_form_before(pair):
    P = [(ri, rj, a) for ri, rj, i, j, a, wall, _ in fixture_cases() if wall and i != j]
    assert len(P) >= 700
    worst, where = _worst(pair, P)
    for k in range(5):
        print("fixtures  %-9s worst difference %.3e = %.2f eps of max(|A|, a/r)" % (NAMES[k], worst[k], worst[k] / EPS))
    assert worst.max() <= BOUND, (worst / EPS, where[int(worst.argmax())])


def test_edge_inputs_agree_with_the_form_before(pair):
    worst, where = _worst(pair, edge_pairs())
    for k in range(5):
        print("edges     %-9s worst difference %.3e = %.2f eps of max(|A|, a/r)" % (NAMES[k], worst[k], worst[k] / EPS))
    assert worst.max() <= BOUND, (worst / EPS, where[int(worst.argmax())])


def test_a_wrong_constant_is_seen(pair, tmp_path):
    """the harness sees what it is for: the restated form with 12 replaced by 12 (1 + 1e-9) differs by far more than the bound"""
    src = open(os.path.join(HERE, "host_wall_brackets", "wall_brackets_host.cpp")).read()
    assert "__builtin_fma(12.0, u, b2p)" in src
    bad = tmp_path / "bad.cpp"
    bad.write_text(src.replace("__builtin_fma(12.0, u, b2p)", "__builtin_fma(12.000000012, u, b2p)")
                   .replace('"../../rigid_body_light_amd/csrc/rbl_pair.hpp"', '"%s"' % os.path.join(HERE, "..", "rigid_body_light_amd", "csrc", "rbl_pair.hpp")))
    so = str(tmp_path / "libbad.so")
    subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "host_pair"), "-o", so, str(bad)])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.wall_brackets_pair.argtypes = [dp, dp, C.c_double, dp, dp, dp]
    ri, rj = np.array([0.0, 0.0, 3.3]), np.array([2.1, 0.0, 1.1])
    now, before, scale = np.zeros(5), np.zeros(5), np.zeros(2)
    L.wall_brackets_pair(ri.ctypes.data_as(dp), rj.ctypes.data_as(dp), 1.0, now.ctypes.data_as(dp), before.ctypes.data_as(dp), scale.ctypes.data_as(dp))
    assert np.abs(now - before)[4] / np.abs(scale).max() > 100.0 * BOUND
