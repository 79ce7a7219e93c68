#!/usr/bin/env python3
"""CPU check of the device pair arithmetic (host build of rbl_pair.hpp, see pair_host.cpp) against the reference fixture in
tests/golden/ and the oracle: prints the worst error of every form the product kernels run (the ordered accumulation plain and in
radius-scaled coordinates, the symmetric form M_ij and its transpose M_ji, the full block of the MFMA kernel) relative to
max(|block|, free-space scale), and the largest error / bound.  Development aid for algebra changes in rbl_pair.hpp; the numbers are
those tests/test_pair_regimes_cpu.py asserts (both go through tests/pair_probe.py).   python tests/host_pair/check.py"""
import os
import sys
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import pair_probe as pp
from oracle import Oracle

orc = Oracle()
with tempfile.TemporaryDirectory() as tmp:
    so = pp.build_host_pair(tmp)
    if so is None:
        sys.exit("no g++ on this machine")
    host = pp.HostPair(so)


def report(name, cases, nearchk=None):
    errs, lims = pp.host_errors(host, cases, nearchk)
    print(name, len(cases), "pairs; worst error (worst error / bound):",
          {k: "%.2e (%.2f)" % (np.nanmax(v), np.nanmax(v / lims)) for k, v in errs.items()})


report("assembly fixture:", pp.assembly_fixture_cases())
# random wall pairs at the BASELINE radii, checked against the C oracle (itself bit-exact vs the reference)
rng = np.random.default_rng(5)
cases = []
for a in (0.06752768, 0.13100878, 1.0):
    nf = 1.0 / (8 * np.pi * a)
    for _ in range(4000):
        ri = np.append(rng.uniform(-20, 20, 2), 10 ** rng.uniform(-3, 2)) * a
        rj = np.append(rng.uniform(-20, 20, 2), 10 ** rng.uniform(-3, 2)) * a
        if np.linalg.norm(ri - rj) < 2.0 * a and rng.uniform() < 0.7:
            continue
        cases.append((ri, rj, 0, 1, a, True, orc.pair_block(ri, rj, 0, 1, a, 1.0, True) / nf))
report("random wall pairs:", cases)
# the probe grid of the per-pair tests, by placement
for off in pp.PLACEMENTS:
    for wall in (False, True):
        cases, nearchk = [], []
        for a in pp.RADII:
            nf = 1.0 / (8 * np.pi * a)
            for h in pp.HEIGHTS:
                st = pp.star(a, h, off, "first")
                r, s = st["r"], st["src"]
                for i in np.flatnonzero(st["target"]):
                    cases.append((r[i], r[s], 0, 1, a, wall, orc.pair_block(r[i], r[s], 0, 1, a, 1.0, wall) / nf))
                    nearchk.append(0 if st["nominal"][i] >= 5.0 else 1)
        report("probe grid, source %ga from the origin, wall=%d:" % (off, wall), cases, nearchk)
