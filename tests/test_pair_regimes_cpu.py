"""The fast pair arithmetic of rigid_body_light_amd/csrc/rbl_pair.hpp, one pair at a time, on the CPU: the host build of
tests/host_pair (g++, a stand-in for the reciprocal-square-root seed instruction) against the oracle over the assembly
fixture and over the whole probe grid of tests/pair_probe.py, in every form a product kernel instantiates -- rbl_pair_accum
(plain and radius-scaled), rbl_pair_symv (both application directions, with and without the overlap test) and
rbl_pair_block_fast.  The GPU twin is tests/test_pair_regimes_gpu.py; tests/host_pair/check.py prints the same numbers.

Bound per pair (pair_probe.bound): max |got - ref| / max(|block|_F, free-space scale) <= 5e-13 + 6 eps (X / a) / r^.
Measured here: plain form <= 6e-15 everywhere; radius-scaled forms 3.2e-14 with the source at the origin, 2.7e-13 at 100 a,
2.0e-12 at 1000 a (at r^ = 0.1 above the wall, bounds 1.8e-12 / 1.4e-11 there) and <= 6e-15 with a = 1; the GPU gives 3.2e-14 /
4.3e-13 / 2.6e-12.  A coefficient of rbl_wall_coeffs off by 1e-9 or a swapped gxz / gzx in rbl_pair_symv fails the fixture and the
grid.  (The overlap switch moved by 1e-9 does not and cannot: the two formulas agree in value and slope at r^ = 2, the blocks move
by 1e-18.)"""
import numpy as np
import pytest

import pair_probe as pp


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = pp.build_host_pair(tmp_path_factory.mktemp("host_pair"))
    if so is None:
        pytest.skip("no g++ on this machine")
    return pp.HostPair(so)


def _fail_text(cases, errs, lims, form):
    e = errs[form]
    lines = []
    for k in np.argsort(-np.nan_to_num(e / lims))[:10]:
        ri, rj, i, j, a, wall, _ = cases[k]
        lines.append("a=%.8g wall=%d h_i/a=%.4g h_j/a=%.4g r^=%.17g |x|max/a=%.4g: err %.3e bound %.3e" % (
            a, wall, ri[2] / a, rj[2] / a, np.linalg.norm(ri - rj) / a, max(np.abs(ri).max(), np.abs(rj).max()) / a, e[k], lims[k]))
    return "%s\n%s" % (form, "\n".join(lines))


def test_layout_meets_every_sweep_of_the_symmetric_kernels():
    """The probe's tiles against k_tile_far's rule restated on the host (pair_probe.far_map): with two rows per lane -- the kernels
    that read the far map -- and the source first, in the middle and last, the r^ <= 2.5 targets meet the overlap-checked sweep, every
    target from r^ = 5 on the sweep without it, and the compact r^ = 30 tile passes the single-precision test; the last tile is ragged."""
    for a in pp.RADII:
        for h in pp.HEIGHTS:
            for off in pp.PLACEMENTS:
                for w, where in enumerate(pp.WHERE):
                    contact = (w + pp.HEIGHTS.index(h)) % 3 - 1
                    st = pp.star(a, h, off, where, contact)
                    N, TS = len(st["r"]), st["TS"]
                    assert 350 <= N <= 450 and N % TS != 0
                    ts, T = st["src"] // TS, (N + TS - 1) // TS
                    assert ts == {"first": 0, "middle": 2, "last": T - 1}[where]
                    assert (st["r"][:, 2] >= 0.0).all()
                    assert st["target"].sum() == 12 * len(pp.SEPARATIONS)
                    for s in pp.SEPARATIONS:
                        d = st["dirclass"][st["nominal"] == s]
                        axis = 0 if s in pp.CONTACT and s != pp.CONTACT[contact + 1] else 1
                        assert (d == "z").sum() == axis and (d == "x").sum() == axis and (d == "rand").sum() == 12 - 2 * axis
                    d = np.linalg.norm(st["r"][:, None] - st["r"][None], axis=2) + np.eye(N)
                    assert d.min() > 1e-6 * a                                  # no two blobs coincide (an error to kernels and oracle)
                    sw = pp.sweep_of(st, 2)
                    near = st["target"] & (st["nominal"] <= pp.NEAR_MAX)
                    assert (sw[near] == 0).all()
                    assert (sw[st["target"] & ~near] >= 1).all(), (a, h, off, where)
                    assert (sw[st["tile"] == "R"] == 3).all(), (a, h, off, where)
                    assert (sw[st["tile"] == "Z"] == 1).all()                  # ... and a far tile that stays fp64 under relaxation
                    rhat, _ = pp.pair_geometry(st)
                    assert rhat[st["target"] & ~near].min() > 4.5             # nearchk = 0 below is what the kernels would run


def test_assembly_fixture_through_every_form(host):
    cases = pp.assembly_fixture_cases()
    assert len(cases) > 100
    errs, lims = pp.host_errors(host, cases)
    for form, e in errs.items():
        ok = ~np.isnan(e)
        print("fixture %-10s worst %.2e over %d pairs" % (form, e[ok].max(), ok.sum()))
        assert (e[ok] <= lims[ok]).all(), _fail_text(cases, errs, lims, form)


@pytest.mark.parametrize("wall", [False, True])
def test_probe_grid_through_every_form(host, orc, wall):
    """every radius, height, separation, direction and placement of the probe; nothing skipped or masked"""
    worst = {}
    for a in pp.RADII:
        nf = 1.0 / (8.0 * np.pi * a)
        for off in pp.PLACEMENTS:
            cases, nearchk = [], []
            for h, contact in [(h, c) for h in pp.HEIGHTS for c in (-1, 0, 1)]:
                st = pp.star(a, h, off, "first", contact)
                r, s = st["r"], st["src"]
                for i in np.flatnonzero(st["target"] & (np.isin(st["nominal"], pp.CONTACT) | (contact == 0))):   # +-1: only what differs
                    cases.append((r[i], r[s], 0, 1, a, wall, orc.pair_block(r[i], r[s], 0, 1, a, 1.0, wall) / nf))
                    nearchk.append(0 if st["nominal"][i] >= 5.0 else 1)
                cases.append((r[s], r[s], 0, 0, a, wall, orc.pair_block(r[s], r[s], 0, 0, a, 1.0, wall) / nf))
                nearchk.append(1)
            errs, lims = pp.host_errors(host, cases, nearchk)
            for form, e in errs.items():
                ok = ~np.isnan(e)
                worst[(form, a, off)] = e[ok].max()
                assert (e[ok] <= lims[ok]).all(), _fail_text(cases, errs, lims, form)
    for (form, a, off), w in sorted(worst.items()):
        print("wall=%d %-10s a=%-10.8g offset %6ga  worst %.2e" % (wall, form, a, off, w))
