"""The configurations that tests/test_periodic_cpu.py and tests/test_periodic_gpu.py share, so that the CPU test checks the
positivity of M_per exactly where the GPU tests take roots and Brownian steps.  Plain numpy."""
import numpy as np


def blob_positions(cfg, X, Q):
    """r_k = X_b + R(Q_b) c_k, body-major (N_bod N_blb, 3); cfg with its mean removed, Q normalised"""
    from oracle import oracle as O
    cfg = O.remove_mean(cfg)
    Qn = O.normalize_quats(Q)
    return np.concatenate([cfg @ O.rot_matrix(Qn[b]).T + np.asarray(X, dtype=np.float64).reshape(-1, 3)[b] for b in range(Qn.shape[0])])


def spacing(a):
    return 2.0 * (1.0 + a) + 0.5                              # make_config's lattice


def layer10():
    """10 x shell_N_12 of make_config(10, 12, wall): a 3 x 3 x 2 lattice (one body in the upper layer), in a cell of three
    lattice spacings by three plus 0.7: the bodies of the first and the last column / row are neighbours across both boundaries"""
    from rigid_body_light_amd.synth import make_config
    c = make_config(10, 12, True)
    s = spacing(c["a"])
    c["L"] = (3.0 * s, 3.0 * s + 0.7)
    c["r"] = blob_positions(c["cfg"], c["X"], c["Q"])
    return c


# ---- bodies of tests/body_shapes.py (a = 0.5, eta = 1) in a cell: the cases tests/test_periodic_shapes_cpu.py checks for
# soundness and tests/test_periodic_shapes_gpu.py, tests/test_periodic_forces_gpu.py run on the device -------------------------
def layers(shape, nb, nx, ny, spots=None, seed=0, extra=(0, 0)):
    """nb bodies `shape` on make_config's lattice (x fastest, jitter +-0.1 per coordinate, random unit quaternions) with nx x ny
    spots per layer and the spacing of body_shapes.lattice, 2 (R_body + a) + 0.5, the lowest layer R_body + a + 0.3 +- 0.1 above
    the wall; spots: the (ix, iy, iz) to fill instead of the first nb.  The cell is nx + extra[0] spacings in x and ny + extra[1]
    spacings plus 0.7 in y, as layer10()'s.  -> dict(cfg, X, Q, a, L, r, nblb, R, s)"""
    import body_shapes as bs
    cfg = bs.shape(shape)
    R, a = bs.radius(cfg), bs.A
    s = 2.0 * (R + a) + 0.5
    if spots is None:
        idx = np.arange(nb)
        spots = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1)
    spots = np.asarray(spots, dtype=np.float64).reshape(nb, 3)
    assert spots[:, 0].max() < nx and spots[:, 1].max() < ny
    X = spots * s + np.random.default_rng(seed).uniform(-0.1, 0.1, (nb, 3))
    X[:, 2] += R + a + 0.3
    Q = np.random.default_rng(seed + 1).standard_normal((nb, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    c = dict(cfg=cfg, X=X, Q=Q, a=a, L=((nx + extra[0]) * s, (ny + extra[1]) * s + 0.7), nblb=cfg.shape[0], R=R, s=s)
    c["r"] = blob_positions(cfg, X, Q)
    return c


# -- the product at the tile edges (k_apply_M_per: column and row tiles of 256 blobs).  name: (builder, images, sampled rows)
def _row3():
    return layers("fib255", 3, 3, 1)


# rows: the first and the last of every tile, and the first and the last of a body on either side of a tile boundary
ROWS_765 = [0, 100, 254, 255, 256, 400, 509, 510, 511, 512, 700, 764]            # tiles 0, 256, 512; bodies 0, 255, 510
ROWS_765_AXIS = [0, 254, 255, 256, 509, 510, 511, 512, 764]
PRODUCT_CASES = {
    # no ragged tile at all
    "64xtetra": (lambda: layers("tetra", 64, 8, 8), (1, 1), [0, 3, 4, 127, 128, 131, 132, 251, 252, 255]),
    # a column tile of one blob, a row tile with one valid row; one body alone in a cell of two spacings (its diameter + 2a + 1 < L)
    "1xfib257": (lambda: layers("fib257", 1, 1, 1, extra=(1, 1)), (1, 1), [0, 1, 100, 254, 255, 256]),
    # three tiles, the last of 253; j-split 2 gives chunks of two tiles and of one
    "3xfib255": (_row3, (1, 1), ROWS_765),
    "3xfib255_x": (_row3, (2, 0), ROWS_765_AXIS),            # k_apply_M_per<true, false> beyond one tile (y open)
    "3xfib255_y": (_row3, (0, 2), ROWS_765_AXIS),            # k_apply_M_per<false, true>
}
RANGES_765 = ((100, 700), (255, 257), (764, 765))            # (100, 700): row tiles at 100, 356, 612, the last of 88 rows
ROWS_765_RANGE = [355, 356, 611, 612, 699]                   # their first and last rows, beside those of ROWS_765 (100 among them)


def product_case(name):
    build, images, which = PRODUCT_CASES[name]
    c = build()
    c["L"] = tuple(l if n else 0.0 for l, n in zip(c["L"], images))
    c["images"], c["rows"] = images, list(which)
    return c


# -- the minimum-image force model.  The tables are those of tests/test_periodic_gpu.py: test_pair_forces_by_minimum_image
GRID = np.linspace(0.5, 2.5, 41)
PAIR_TABLE = (0.4 * np.exp(-GRID) * np.cos(3.0 * GRID), 0.4 * np.exp(-GRID) * (-np.cos(3.0 * GRID) - 3.0 * np.sin(3.0 * GRID)), 0.5, 2.5)
HGRID = np.linspace(0.3, 4.0, 38)
HEIGHT_TABLE = (0.3 * np.exp(-0.5 * HGRID) * np.sin(2.0 * HGRID),
                0.3 * np.exp(-0.5 * HGRID) * (2.0 * np.cos(2.0 * HGRID) - 0.5 * np.sin(2.0 * HGRID)), 0.3, 4.0)
BUILTIN = dict(w=0.3, eps_wall=0.5, b_wall=0.2)


def _steric(a):
    return (1.5, 0.1, 2.0 * a + 2.0)                          # (eps, b, r_cut) of the same test


def _shells12():
    """12 x shell_N_12 of make_config: a 3 x 3 x 2 lattice (three bodies in the upper layer) in layer10()'s cell"""
    from rigid_body_light_amd.synth import make_config
    c = make_config(12, 12, True)
    s = spacing(c["a"])
    c.update(L=(3.0 * s, 3.0 * s + 0.7), nblb=12, s=s, r=blob_positions(c["cfg"], c["X"], c["Q"]))
    c["R"] = float(np.linalg.norm(c["cfg"] - c["cfg"].mean(axis=0), axis=1).max())
    return c


def _model(c, steric=True, table=False, height=False, traps=False):
    c["builtin"] = dict(BUILTIN) if steric else None
    c["steric"] = _steric(c["a"]) if steric else None
    c["table"] = PAIR_TABLE if table else None
    c["height"] = HEIGHT_TABLE if height else None
    nb = c["X"].shape[0]
    rng = np.random.default_rng(31)
    c["traps"] = (rng.uniform(0.0, 2.0, (nb, 3)), c["X"] + rng.uniform(-0.3, 0.3, (nb, 3))) if traps else None
    return c


# spots of three bodies: 0 - 1 direct and 1 - 2 direct, 0 - 2 through the boundary -- every list mixes both kinds or holds both
# partners; along x and along y.  Two bodies: one pair, through the x boundary (see test_periodic_shapes_cpu.py: with two bodies the
# uniqueness condition leaves no room for pairs of both kinds)
FORCE_CASES = {
    # second and third pass of k_body_neighbours_per's 64 lanes
    "65xtetra": lambda: _model(layers("tetra", 65, 9, 8)),
    "130xtetra": lambda: _model(layers("tetra", 130, 12, 11)),
    # the height table together with the cell: k_blob_interactions_per<2>, <3>, <1>, and <3> with the built-in terms off
    "12xshell_height": lambda: _model(_shells12(), height=True, traps=True),
    "12xshell_height_pair": lambda: _model(_shells12(), table=True, height=True),
    "12xshell_pair": lambda: _model(_shells12(), table=True),
    "12xshell_height_pair_only": lambda: _model(_shells12(), steric=False, table=True, height=True),
    # bt = 256; two tiles, one live lane in the second; the second IA_CHUNK pass of one blob
    "3xfib130": lambda: _model(layers("fib130", 3, 3, 3, spots=[(0, 0, 0), (1, 0, 0), (2, 0, 0)])),
    "3xfib257": lambda: _model(layers("fib257", 3, 3, 3, spots=[(0, 0, 0), (0, 1, 0), (0, 2, 0)]), table=True),
    "2xfib513": lambda: _model(layers("fib513", 2, 3, 3, spots=[(0, 0, 0), (2, 0, 0)])),
}
TWO_BODIES = ("2xfib513",)


def force_case(name):
    return FORCE_CASES[name]()


def pair_cutoff(c):
    """the larger cutoff of the pair terms that are on"""
    return max(c["steric"][2] if c["steric"] else 0.0, c["table"][3] if c["table"] else 0.0)


# -- dipoles on trimers: c_dd, r_core, r_cut of the same test (r_cut = 5 <= L / 2 in every cell below), and a second core radius of
# one lattice spacing, which the nearest neighbours straddle (r_core = 1 is below every centre distance: no pair in the core)
DIPOLE = dict(c_dd=0.8, r_core=1.0, r_cut=5.0)
DIPOLE_CASES = {65: (9, 8), 130: (12, 11), 515: (17, 16)}     # nb: (nx, ny); 515 fills two layers


def dipole_case(nb):
    from oracle import oracle as O
    c = layers("trimer", nb, *DIPOLE_CASES[nb])
    c["m_body"] = np.random.default_rng(41).standard_normal((nb, 3))
    c["m_lab"] = np.array([O.rot_matrix(q) @ m for q, m in zip(O.normalize_quats(c["Q"]), c["m_body"])])
    c["cores"] = (DIPOLE["r_core"], c["s"])
    return c
