"""Probe configurations for per-pair checks of the mobility product kernels (a plain helper module, no test in here).

A STAR is one source blob and many target blobs.  A force on the source alone makes row i of a product exactly
B_i M_ij B_j F_j, so three unit-force products hand back every block M_ij of the star through whatever kernel ran; the
zero forces on all the other blobs contribute exact zeros, which is why targets may overlap each other freely.

star(a, h_s / a, offset / a, where) builds one star per (radius, source height, placement): ten separations x twelve
directions around the source, laid out in tiles of TS blobs (the column tile of the symmetric kernels, read from the
kernel source) so that those kernels meet every sweep they have:

  A   the source's own tile: the source and the targets with r^ <= 2.5 in eight directions (+z, +x, six random) --
      the diagonal sweep.  Ragged (57 blobs) when it is the last tile, padded to TS otherwise.
  B   the other four random directions of the same separations + pads inside the same cube: an off-diagonal tile
      within 2a of the source's -- the overlap-checked sweep.
  R   the ten random directions at r^ = 30, drawn in a cone of 1.9 degrees about +y, + pads: a compact cluster (box of
      ~2a) 27a from A and B.  Passes k_tile_far's single-precision test: the relaxed sweep when that is asked for,
      the sweep without the overlap test otherwise.
  P0  pads only, inside R's box (R's partner in a two-row super-tile, which has to be compact too).
  Z   +z at r^ = 5, 30, 1000 + pads along the axis: far (2.5a above A's box), far too long for single precision.
  X   +x at r^ = 5, 30, 1000 and the random directions at r^ = 5 and 1000, in a cone of 20 degrees about +x, + pads:
      far (2.2a beside A's box), not compact.
  P   a ragged tile of pads out of everyone's way, last when the source's tile is not.

The far random directions live in cones because "far" is decided per TILE from bounding boxes: a target at r^ = 5 in a
general direction lies within 2a of the cube around the r^ <= 2.5 targets whatever tile it is put in.  Targets that
would go below the wall are reflected upward (|z|), which shortens their separation: every check uses the separation
of the coordinates, not the nominal one.  Pads carry no force and are drawn at random inside the box of their tile.

The three separations around contact -- 2 (1 - eps), 2, 2 (1 + eps), neighbouring doubles -- cannot all sit on one axis: the targets
would lie 4e-16 a apart, and two blobs closer than 1e-12 a are an error to the kernels and to the oracle whatever their forces.  One
of the three (contact = -1, 0, +1) gets the two axis directions, the other two get two more random ones; the tests rotate contact
over the heights and the source's positions so that each meets every role.

where = "first" | "middle" | "last": the tile order, with the source's tile first, in the middle, or last and ragged --
the source is then a row blob, both, or a column blob of the symmetric sweeps (U_i += M F_j and U_j += M^T F_i).
"""
import ctypes as C
import functools
import json
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = float(np.finfo(np.float64).eps)

RADII = (0.06752768, 0.41642068, 1.0)                      # the project's two non-dyadic radii; 1: the scaling by 1/a is exact
HEIGHTS = (0.01, 0.05, 0.3, 1.0, 3.0, 100.0, 1000.0)       # h_s / a; below 1: the damping zone
# r^ = |r| / a: deep overlap .. contact to the ulp .. far.  (The overlap and the far formula agree in value AND slope at r^ = 2: which
# side of the switch a pair within a few ulp of contact takes is immaterial, and no pair can tell a switch misplaced by 1e-9.)
SEPARATIONS = (0.1, 0.5, 1.0, float(np.nextafter(2.0, 0.0)), 2.0, float(np.nextafter(2.0, 3.0)), 2.5, 5.0, 30.0, 1000.0)
CONTACT = SEPARATIONS[3:6]                                 # neighbouring doubles: on one axis they would coincide (see the module text)
PLACEMENTS = (0.0, 100.0, 1000.0)                          # offset of the source in x and in y, in radii
WHERE = ("first", "middle", "last")
NEAR_MAX = 2.5                                             # r^ <= this: tiles A and B
N_RANDOM = 10
N_IN_A = 8                                                 # directions per near separation in the source's own tile
SRC_LANE = 5                                               # the source's place inside its tile (not the tile's first blob)


@functools.lru_cache(maxsize=None)
def tile_size():
    """the column tile of the symmetric kernels, from their source"""
    with open(os.path.join(ROOT, "rigid_body_light_amd", "csrc", "rbl_kernels.hip")) as f:
        m = re.search(r"^constexpr int TS = (\d+);", f.read(), re.M)
    assert m, "rbl_kernels.hip no longer declares the symmetric kernels' tile TS"
    return int(m.group(1))


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _cone(rng, axis, half_angle_deg, n):
    """n seeded directions within half_angle of the coordinate axis `axis` (0: +x, 1: +y)"""
    c = np.cos(np.radians(half_angle_deg))
    mu = rng.uniform(c, 1.0, n); phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - mu * mu)
    d = np.zeros((n, 3))
    d[:, axis] = mu; d[:, (axis + 1) % 3] = s * np.cos(phi); d[:, (axis + 2) % 3] = s * np.sin(phi)
    return d


def star(a, h_over_a, offset_over_a, where, contact=0, seed=7):
    """contact = -1, 0, +1: which of r^ = 2 (1 - eps), 2, 2 (1 + eps) carries the two axis directions (see the module text)
    -> dict: r (N, 3) positions, src (index of the source), tile (N,) tile label per blob ("A", "B", ...), target (N,) bool
    (a probe target, not the source and not a pad), nominal (N,) the nominal r^ (nan: pads and the source), dirclass (N,) "z", "x",
    "rand", "pad" or "src", and TS"""
    TS = tile_size()
    assert where in WHERE
    rng = np.random.default_rng(seed)
    src = np.array([offset_over_a, offset_over_a, h_over_a]) * a
    axes = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    far_dirs = {5.0: _cone(rng, 0, 20.0, N_RANDOM), 30.0: _cone(rng, 1, 1.9, N_RANDOM), 1000.0: _cone(rng, 0, 20.0, N_RANDOM)}

    def put(direction, rhat):
        p = src + (rhat * a) * np.asarray(direction)
        p[2] = abs(p[2])                                                     # reflected upward
        return p

    def pads(n, centre, half):
        p = src + a * (np.asarray(centre) + rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half))
        p[:, 2] = np.abs(p[:, 2])
        return [(q, np.nan, "pad") for q in p]

    tiles = {k: [] for k in "ABRZX"}
    for s in SEPARATIONS:
        near_dirs = np.concatenate([axes, _unit(rng.standard_normal((N_RANDOM, 3)))])      # fresh random directions per separation
        spare = _unit(rng.standard_normal((2, 3)))
        dirclass12 = ["z", "x"] + ["rand"] * N_RANDOM
        if s in CONTACT and s != CONTACT[contact + 1]:
            near_dirs[:2] = spare; dirclass12[:2] = ["rand", "rand"]
        for k in range(12):
            if s <= NEAR_MAX:
                tiles["A" if k < N_IN_A else "B"].append((put(near_dirs[k], s), s, dirclass12[k]))
            elif k == 0:
                tiles["Z"].append((put(axes[0], s), s, "z"))
            elif k == 1:
                tiles["X"].append((put(axes[1], s), s, "x"))
            else:
                tiles["R" if s == 30.0 else "X"].append((put(far_dirs[s][k - 2], s), s, "rand"))
    tiles["A"].insert(SRC_LANE, (src.copy(), np.nan, "src"))
    assert len(tiles["A"]) <= TS and len(tiles["B"]) <= TS and len(tiles["X"]) <= TS, "the probe does not fit the kernels' tile any more"
    if where != "last":
        tiles["A"] += pads(TS - len(tiles["A"]), (0, 0, 0), (2.4, 2.4, 2.4))
    tiles["B"] += pads(TS - len(tiles["B"]), (0, 0, 0), (2.4, 2.4, 2.4))
    tiles["R"] += pads(TS - len(tiles["R"]), (0, 30, 0), (0.9, 0.0, 0.9))
    tiles["P0"] = pads(TS, (0, 30, 0), (0.9, 0.5, 0.9))
    tiles["Z"] += pads(TS - len(tiles["Z"]), (0, 0, 22.0), (0.5, 0.5, 17.0))
    tiles["X"] += pads(TS - len(tiles["X"]), (17.5, 0, 0), (12.5, 1.5, 1.5))
    tiles["P"] = pads(TS // 2 + 5, (-12.0, -12.0, 0.0), (1.0, 1.0, 1.0))
    order = {"first": ["A", "B", "R", "P0", "Z", "X", "P"], "middle": ["R", "P0", "A", "B", "Z", "X", "P"],
             "last": ["R", "P0", "Z", "X", "B", "A"]}[where]
    r, label, nominal, dirclass = [], [], [], []
    for t in order:
        for p, s, d in tiles[t]:
            r.append(p); label.append(t); nominal.append(s); dirclass.append(d)
    r = np.array(r); dirclass = np.array(dirclass)
    assert len(r) % TS != 0                                                  # a ragged last tile in every order
    return {"r": r, "src": int(np.flatnonzero(dirclass == "src")[0]), "tile": np.array(label), "nominal": np.array(nominal),
            "dirclass": dirclass, "target": ~np.isin(dirclass, ("pad", "src")), "TS": TS, "a": a, "where": where,
            "h_over_a": h_over_a, "offset_over_a": offset_over_a, "contact": contact}


def far_map(r, a, NI, TS):
    """k_tile_far restated: m[S, J] = 0 (overlap-checked sweep), 1 (no pair closer than 2a), 3 (... and single precision is safe)
    for row super-tile S (NI consecutive tiles) and column tile J, from the tile bounding boxes in radius-scaled coordinates"""
    x = np.asarray(r).reshape(-1, 3) / a
    T = (len(x) + TS - 1) // TS
    lo = np.array([x[t * TS:(t + 1) * TS].min(axis=0) for t in range(T)]); hi = np.array([x[t * TS:(t + 1) * TS].max(axis=0) for t in range(T)])
    nsup = (T + NI - 1) // NI
    m = np.zeros((nsup, T), dtype=int)
    for S in range(nsup):
        rows = range(NI * S, min(NI * S + NI, T))
        slo = lo[list(rows)].min(axis=0); shi = hi[list(rows)].max(axis=0)
        for J in range(T):
            gap2 = min(float(np.sum(np.maximum(np.maximum(lo[J] - hi[I], lo[I] - hi[J]), 0.0) ** 2)) for I in rows)
            far = gap2 > 4.0001
            ok32 = far and np.linalg.norm(shi - slo) + 2.0 * np.linalg.norm(hi[J] - lo[J]) <= 15.0 * np.sqrt(gap2)
            m[S, J] = 3 if ok32 else (1 if far else 0)
    return m


def sweep_of(st, NI):
    """per blob: the far-map class of the tile pair (its tile, the source's tile) in a kernel with NI rows per lane (the row
    super-tile is the one of the lower tile index: the symmetric kernels sweep the upper triangle)"""
    TS = st["TS"]
    m = far_map(st["r"], st["a"], NI, TS)
    ts = st["src"] // TS
    out = np.zeros(len(st["r"]), dtype=int)
    for i in range(len(out)):
        t = i // TS
        lo_t, hi_t = min(t, ts), max(t, ts)
        out[i] = 0 if lo_t // NI == hi_t // NI else m[lo_t // NI, hi_t]      # inside one super-tile: its diagonal sweep
    return out


# ---- the per-pair measure and its bound ------------------------------------------------------------------------------------------
def pair_geometry(st):
    """(r^ of the coordinates, X / a) per blob against the source; X the largest absolute coordinate of the two blobs, z included"""
    r, a, s = st["r"], st["a"], st["src"]
    rhat = np.linalg.norm(r - r[s], axis=1) / a
    X = np.maximum(np.abs(r).max(axis=1), np.abs(r[s]).max()) / a
    return rhat, X


def bound(rhat, X_over_a):
    """5e-13: the project's bound for the fast wall arithmetic (test_assembly_blocks_vs_reference_golden).  6 eps (X / a) / r^: the
    kernels subtract coordinates AFTER scaling them by 1 / a, which leaves every coordinate a rounding of eps / 2 |x| / a: the
    separation is off by at most eps X / a, i.e. by eps (X / a) / r^ of itself, the 1/r and 1/r^3 terms amplify that about 3 x,
    and a margin of 2.  The self block (r^ = 0) subtracts equal numbers: the first term alone."""
    rhat = np.asarray(rhat, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(rhat > 0.0, 5e-13 + 6.0 * EPS * np.asarray(X_over_a) / rhat, 5e-13)


def block_scale(ref_blocks, rhat, unit):
    """max(|block|_F, unit min(4/3, 1 / r^)): the block, or the free-space block the wall term was added to (unit = B_i B_j nf)"""
    with np.errstate(divide="ignore"):
        free = np.minimum(4.0 / 3.0, 1.0 / np.asarray(rhat)) * unit
    return np.maximum(np.linalg.norm(ref_blocks, axis=(1, 2)), free)


def pair_errors(got, ref, rhat, unit):
    """max |got - ref| / scale per block; got, ref (n, 3, 3)"""
    return np.abs(got - ref).max(axis=(1, 2)) / block_scale(ref, rhat, unit)


def worst_report(st, err, lim, wall, n=10):
    """the n worst pairs of a star as text: (a, h_i/a, h_j/a, r^, direction class, tile, source role)"""
    rhat, _ = pair_geometry(st)
    a, s = st["a"], st["src"]
    lines = []
    for i in np.argsort(-(err / lim))[:n]:
        lines.append("a=%.8g wall=%d h_i/a=%.4g h_j/a=%.4g r^=%.17g dir=%s tile=%s source=%s(%s) offset=%g: err %.3e bound %.3e" % (
            a, wall, st["r"][i, 2] / a, st["r"][s, 2] / a, rhat[i], st["dirclass"][i], st["tile"][i],
            "row" if s < i else "column", st["where"], st["offset_over_a"], err[i], lim[i]))
    return "\n".join(lines)


# ---- host build of the device pair arithmetic (tests/host_pair) --------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-ffp-contract=fast", "-mfma", "-std=c++17", "-shared", "-fPIC"]


def build_host_pair(outdir):
    """g++ build of tests/host_pair/pair_host.cpp into outdir -> path of the library, or None without g++"""
    if shutil.which("g++") is None:
        return None
    so = os.path.join(str(outdir), "libpair_host.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ["-I" + os.path.join(HERE, "host_pair"), "-o", so, os.path.join(HERE, "host_pair", "pair_host.cpp")])
    return so


class HostPair:
    """the forms of rbl_pair.hpp the product kernels run, one pair at a time, blocks in units of 1 / (8 pi eta a) (P.nf = 1):
    accum: rbl_pair_accum<WALL, true, UNIT = false> (the debug kernel's form);  accum_unit: ... UNIT = true on coordinates times
    1 / a (the ordered-rows kernel);  sym: rbl_pair_symv<WALL, true, NEARCHK> -> (M_ij, M_ji) (the symmetric kernels, both
    application directions);  block: rbl_pair_block_fast<WALL, true, true> (the MFMA kernel)"""

    def __init__(self, so):
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        L.fast_block.argtypes = [dp, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp]
        L.fast_block_unit.argtypes = [dp, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp]
        L.block_fast_unit.argtypes = [dp, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp]
        L.sym_blocks.argtypes = [dp, dp, C.c_double, C.c_int, C.c_int, dp, dp]
        self.L, self._dp = L, dp

    def _p(self, x):
        return x.ctypes.data_as(self._dp)

    def _one(self, fn, ri, rj, i, j, a, wall):
        ri = np.ascontiguousarray(ri, dtype=np.float64); rj = np.ascontiguousarray(rj, dtype=np.float64)
        out = np.zeros(9)
        fn(self._p(ri), self._p(rj), i, j, a, int(wall), self._p(out))
        return out.reshape(3, 3)

    def accum(self, ri, rj, i, j, a, wall):
        return self._one(self.L.fast_block, ri, rj, i, j, a, wall)

    def accum_unit(self, ri, rj, i, j, a, wall):
        return self._one(self.L.fast_block_unit, ri, rj, i, j, a, wall)

    def block(self, ri, rj, i, j, a, wall):
        return self._one(self.L.block_fast_unit, ri, rj, i, j, a, wall)

    def sym(self, ri, rj, a, wall, nearchk):
        ri = np.ascontiguousarray(ri, dtype=np.float64); rj = np.ascontiguousarray(rj, dtype=np.float64)
        mij, mji = np.zeros(9), np.zeros(9)
        self.L.sym_blocks(self._p(ri), self._p(rj), a, int(wall), int(nearchk), self._p(mij), self._p(mji))
        return mij.reshape(3, 3), mji.reshape(3, 3)

    def all_forms(self, ri, rj, i, j, a, wall, nearchk=1):
        """{form: block to compare with M_ij}; the symmetric form's M_ji comes back transposed (M_ji = M_ij^T)"""
        out = {"accum": self.accum(ri, rj, i, j, a, wall), "accum_unit": self.accum_unit(ri, rj, i, j, a, wall),
               "block": self.block(ri, rj, i, j, a, wall)}
        if i != j:
            mij, mji = self.sym(ri, rj, a, wall, nearchk)
            out["sym_ij"] = mij; out["sym_ji"] = mji.T
        return out


def assembly_fixture_cases():
    """tests/golden/pair_blocks_assembly.json -> [(ri, rj, i, j, a, wall, block in units of 1 / (8 pi eta a))], without the pairs
    the fast forms refuse (a blob below the wall: the reference only tests z_j)"""
    unhex = lambda v: np.array([float.fromhex(x) for x in v])
    with open(os.path.join(HERE, "golden", "pair_blocks_assembly.json")) as f:
        g = json.load(f)
    cases = []
    for c in g["blocks"]:
        ri, rj = unhex(c["ri"]), unhex(c["rj"])
        if c["wall"] and (ri[2] < 0.0 or rj[2] < 0.0):
            continue
        cases.append((ri, rj, c["i"], c["j"], float.fromhex(c["a"]), bool(c["wall"]), unhex(c["out9"]).reshape(3, 3)))
    return cases


def host_errors(host, cases, nearchk=None):
    """{form: (n,) errors} of the host forms over cases [(ri, rj, i, j, a, wall, ref)], and the (n,) bounds.  nearchk: per case, 1 when
    None (the symmetric form with the overlap test)"""
    errs, lims = {}, []
    for k, (ri, rj, i, j, a, wall, ref) in enumerate(cases):
        rhat = np.linalg.norm(ri - rj) / a
        X = max(np.abs(ri).max(), np.abs(rj).max()) / a
        lims.append(float(bound(rhat if i != j else 0.0, X)))
        for form, blk in host.all_forms(ri, rj, i, j, a, wall, 1 if nearchk is None else nearchk[k]).items():
            errs.setdefault(form, np.full(len(cases), np.nan))[k] = pair_errors(blk[None], ref[None], np.array([rhat]), 1.0)[0]
    return errs, np.array(lims)
