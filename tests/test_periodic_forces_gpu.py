"""The minimum-image force kernels away from 3 x 12 blobs: k_body_neighbours_per beyond one pass of its 64 lanes and with the cull
off, k_blob_interactions_per<0 ... 3> with 256-lane workgroups, two tiles and a second IA_CHUNK pass, k_body_dipoles_per<64> beyond
one pass and k_body_dipoles_per<256> -- against the vectorised oracles of tests/periodic_oracle.py (held against their defining
loops by tests/test_periodic_shapes_cpu.py, which also checks that every case here meets the uniqueness condition and has pairs
inside the cutoff both directly and through a boundary).  The cases are tests/periodic_cases.py: FORCE_CASES and DIPOLE_CASES.

Tolerance: that of tests/test_interactions_gpu.py, max |f - f_ref| <= 1e-12 max |f_ref|, for blob forces, body forces / torques and
the energy alike; the ordered pair count of rbl_interaction_stats equals the oracle's as an integer."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_cases as pc  # noqa: E402
import periodic_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ETA = 1.0


def _err(x, y):
    return np.abs(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)).max() / np.abs(np.asarray(y)).max()


def _body(c):
    from rigid_body_light_amd import RigidBody
    return RigidBody(c["cfg"], c["X"], c["Q"], c["a"], ETA, 0.01, wall_PC=True)


def _set_model(rb, c):
    if c["steric"]:
        rb.set_interactions(eps_blob=c["steric"][0], b_blob=c["steric"][1], r_cut=c["steric"][2], **c["builtin"])
    else:
        rb.set_interactions(on=False)
    if c["table"]:
        rb.set_pair_table(*c["table"])
    if c["height"]:
        rb.set_height_table(*c["height"])
    if c["traps"]:
        rb.set_traps(*c["traps"])


def _eval(rb):
    f, FT = rb.ctx.interaction_forces()
    return f, FT, rb.ctx.interaction_energy(), rb.ctx.interaction_stats()


@pytest.mark.parametrize("name", list(pc.FORCE_CASES))
def test_pair_forces_by_minimum_image_at_every_shape(name):
    c = pc.force_case(name)
    nb, L = c["X"].shape[0], c["L"]
    ref = po.force_model(c["r"], c["X"], c["nblb"], c["a"], L, builtin=c["builtin"], steric=c["steric"], table=c["table"],
                         height=c["height"], traps=c["traps"])
    rb = _body(c)
    assert np.abs(rb.get_blob_positions().reshape(-1) - c["r"].reshape(-1)).max() <= 1e-13
    _set_model(rb, c)
    f_open = rb.ctx.interaction_forces()[0]
    rb.set_periodic(L[0], L[1], images=(1, 1))
    f, FT, E, (bp, pairs) = _eval(rb)
    print("%s: blob forces %.2e, body forces / torques %.2e, energy %.2e; %d candidate body pairs, %d blob pairs (oracle %d + %d)"
          % (name, _err(f, ref["f"]), _err(FT, ref["FT"]), abs(E - ref["E"]) / abs(ref["E"]), bp, pairs, ref["direct"], ref["through"]))
    assert _err(f, ref["f"]) <= 1e-12 and _err(FT, ref["FT"]) <= 1e-12 and abs(E - ref["E"]) <= 1e-12 * abs(ref["E"])
    assert pairs == ref["direct"] + ref["through"]
    assert _err(f_open, ref["f"]) > 1e-6                              # the partners through the boundary do count
    f2, FT2, E2, st2 = _eval(rb)
    assert np.array_equal(f, f2) and np.array_equal(FT, FT2) and E == E2 and st2 == (bp, pairs)   # bitwise when repeated
    rb.ctx.set_option("interaction_cull", 0)                          # every body a candidate: each blob pair folds on its own
    f0, FT0, E0, (bp0, pairs0) = _eval(rb)
    rb.ctx.set_option("interaction_cull", 1)
    assert bp0 == nb * (nb - 1) and pairs0 == pairs and (bp < bp0 or nb <= 12)
    assert np.array_equal(f0, f) and np.array_equal(FT0, FT) and E0 == E


def test_a_cell_too_small_for_the_shape_is_refused_and_the_next_one_served():
    c = pc.force_case("3xfib130")
    L = c["L"]
    need = 2.0 * c["R"] + pc.pair_cutoff(c)
    rb = _body(c)
    _set_model(rb, c)
    rb.set_periodic(L[0], L[1], images=(1, 1))
    f, FT = rb.ctx.interaction_forces()
    for k, axis in enumerate("xy"):
        small = list(L)
        small[k] = np.floor(8.0 * need) / 4.0 - 0.25                  # a multiple of 1 / 4: L / 2 at least an eighth short of 2 R_body + r_cut
        rb.set_periodic(small[0], small[1], images=(1, 1))
        with pytest.raises(RuntimeError, match=r"periodic cell too small: L%s = %.2f0*,? .*needs 2 R_body \+ r_cut = %s.*<= L / 2 = %.3f"
                           % (axis, small[k], re.escape(("%.6f" % need)[:-1]), 0.5 * small[k])):
            rb.ctx.interaction_forces()
    rb.set_periodic(L[0], L[1], images=(1, 1))
    f2, FT2 = rb.ctx.interaction_forces()
    assert np.array_equal(f2, f) and np.array_equal(FT2, FT)


def _dipole_rule():
    """the launch condition of the four-wave dipole kernels from the source: (open system, periodic cell)"""
    src = open(os.path.join(ROOT, "rigid_body_light_amd", "csrc", "rbl_forces.hip")).read()
    m_open = re.search(r"if \(!per && win > (\d+)\)\s*\n\s*hipLaunchKernelGGL\(k_body_dipoles<256>", src)
    m_per = re.search(r"else if \(win > (\d+)\)\s*\n\s*hipLaunchKernelGGL\(k_body_dipoles_per<256>", src)
    assert m_open and m_per, "rbl_forces.hip no longer selects the four-wave dipole kernels by the window"
    return int(m_open.group(1)), int(m_per.group(1))


@pytest.mark.parametrize("nb", list(pc.DIPOLE_CASES))
def test_dipole_pairs_by_minimum_image_beyond_one_pass(nb):
    """65: a second pass of k_body_dipoles_per<64> with one partner; 130: a third; 515: k_body_dipoles_per<256>, three partners in
    its third pass -- selected by the open system's rule, win > 512, read from the source"""
    rule = _dipole_rule()
    assert rule == (512, 512) and (nb > rule[1]) == (nb == 515)
    c = pc.dipole_case(nb)
    L, D = c["L"], pc.DIPOLE
    rb = _body(c)
    rb.set_interactions(on=False)
    for core in c["cores"]:
        rb.set_periodic(L[0], L[1], images=(1, 1), on=False)
        rb.set_dipoles(c["m_body"], c_dd=D["c_dd"], r_core=core, r_cut=D["r_cut"])
        FT_open = rb.ctx.interaction_forces()[1]
        rb.set_periodic(L[0], L[1], images=(1, 1))
        f, FT = rb.ctx.interaction_forces()
        E = rb.ctx.interaction_energy()
        FT_ref, E_ref, nd, nt = po.dipole_pairs_v(c["X"], c["m_lab"], D["c_dd"], core, D["r_cut"], L)
        print("%d trimers, r_core %.3f: body forces / torques %.2e, energy %.2e (%d direct pairs, %d through a boundary)"
              % (nb, core, _err(FT, FT_ref), abs(E - E_ref) / abs(E_ref), nd, nt))
        assert not f.any() and np.abs(FT_ref).max() > 1e-3
        assert _err(FT, FT_ref) <= 1e-12 and abs(E - E_ref) <= 1e-12 * abs(E_ref)
        assert _err(FT_open, FT_ref) > 1e-3                           # the partners through the boundary do count
        f2, FT2 = rb.ctx.interaction_forces()
        assert np.array_equal(FT, FT2) and rb.ctx.interaction_energy() == E
    # a cell too small for the dipole cutoff: refused with its message, the next one served
    rb.set_periodic(2.0 * D["r_cut"] - 0.5, L[1], images=(1, 1))
    with pytest.raises(RuntimeError, match=r"periodic cell too small: Lx = 9\.5.*needs the dipole r_cut = 5\.0.*<= L / 2 = 4\.75"):
        rb.ctx.interaction_forces()
    rb.set_periodic(L[0], L[1], images=(1, 1))
    assert np.array_equal(rb.ctx.interaction_forces()[1], FT)
