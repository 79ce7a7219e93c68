"""numpy restatement of the periodic cell of include/rbl.h section 10 on the CPU oracle's pair block: the image-summed mobility
M_per (dense, or single rows for sampled blobs) and the minimum-image force model as a plain double loop.  It calls no library
code.  TEST INFRASTRUCTURE: a pair costs about 40 microseconds per image, so the dense form is for <= 120 blobs and the rows for
<= 16 sampled blobs of anything larger.

    d0         = (dx - Lx rint(dx / Lx), dy - Ly rint(dy / Ly), dz)        np.rint rounds half to even, an odd function
    M_per[i,j] = sum_{|p| <= nx} sum_{|q| <= ny} B(d0 + (p Lx, q Ly, 0); z_i, z_j)

with the reference's roles: the block of (lower index, higher index) is evaluated, h = z of the higher index, and the mirror block is
its transpose.  The (p, q) != 0 terms of i = j are a blob's own images: ordinary pairs of two DIFFERENT blobs at equal height.

The force model's double loops (pair_forces, dipole_pairs) are the definition; pair_forces_v and dipole_pairs_v at the end of the
module are the same terms broadcast over rows of blobs, for systems the loops are too slow for, and count the pairs inside the
cutoff by whether their minimum image is the direct displacement or one through a boundary."""
import numpy as np


def nearest(d, L):
    """d - L rint(d / L) on the periodic axes (L[k] > 0), d otherwise; d (..., 3) or (3,)"""
    d = np.array(d, dtype=np.float64)
    for k in (0, 1):
        if L[k] > 0.0:
            d[..., k] -= L[k] * np.rint(d[..., k] / L[k])
    return d


def _images(L, n):
    px = range(-n[0], n[0] + 1) if L[0] > 0.0 else (0,)
    py = range(-n[1], n[1] + 1) if L[1] > 0.0 else (0,)
    return [(p, q) for p in px for q in py]


def block_terms(orc, ri, rj, i, j, a, eta, L, n):
    """the 3 x 3 blocks of row blob i and column blob j, i <= j (h = z_j), one per image: [((p, q), block), ...] in the order of
    the sum (p outer, q inner); unscaled by the damping"""
    assert i <= j
    d0 = nearest(np.asarray(ri, dtype=np.float64) - np.asarray(rj, dtype=np.float64), L)
    out = []
    rj0 = np.array([0.0, 0.0, rj[2]])
    for p, q in _images(L, n):
        ri0 = np.array([d0[0] + p * L[0], d0[1] + q * L[1], ri[2]])
        if i == j and p == 0 and q == 0:
            b = orc.pair_block(ri0, rj0, i, i, a, eta, True)               # the self block
        elif i == j:
            b = orc.pair_block(ri0, rj0, i, i + 1, a, eta, True)           # its own image: two different blobs
        else:
            b = orc.pair_block(ri0, rj0, i, j, a, eta, True)
        out.append(((p, q), b))
    return out


def block(orc, ri, rj, i, j, a, eta, L, n):
    """their sum: the block of M_per"""
    out = np.zeros((3, 3))
    for _, b in block_terms(orc, ri, rj, i, j, a, eta, L, n):
        out += b
    return out


def image_terms(orc, r, a, eta, L, nmax):
    """M_per split by image, undamped: {(p, q): (3 N, 3 N)} for |p| <= nmax[0], |q| <= nmax[1]; the matrix of n <= nmax images is
    the sum of the entries with |p| <= n[0] and |q| <= n[1] (truncated()), so a convergence study evaluates every pair once"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    N = r.shape[0]
    assert N <= 120, "the dense form is for <= 120 blobs"
    T = {pq: np.zeros((3 * N, 3 * N)) for pq in _images(L, nmax)}
    for i in range(N):
        for j in range(i, N):
            for pq, b in block_terms(orc, r[i], r[j], i, j, a, eta, L, nmax):
                T[pq][3 * i:3 * i + 3, 3 * j:3 * j + 3] = b
                if j != i:
                    T[pq][3 * j:3 * j + 3, 3 * i:3 * i + 3] = b.T
    return T


def truncated(T, n, B=None):
    """sum of the image terms T with |p| <= n[0], |q| <= n[1] (p outer, q inner), damped by B (3 N,) when given"""
    M = None
    for (p, q) in sorted(T):
        if abs(p) <= n[0] and abs(q) <= n[1]:
            M = T[(p, q)].copy() if M is None else M + T[(p, q)]
    return M if B is None else B[:, None] * M * B[None, :]


def dense_M(orc, r, a, eta, L, n, damped=True):
    """B M_per B (damped, as apply_M applies it) or M_per of the blob positions r (N, 3) with the wall"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    return truncated(image_terms(orc, r, a, eta, L, n), n, orc.damp(r.reshape(-1), a) if damped else None)


def rows(orc, r, which, a, eta, L, n, damped=True):
    """the rows of the blobs `which` of the same matrix: (3 len(which), 3 N)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    N = r.shape[0]
    assert len(which) <= 16, "at most 16 sampled rows"
    out = np.zeros((3 * len(which), 3 * N))
    for k, i in enumerate(which):
        for j in range(N):
            b = block(orc, r[i], r[j], i, j, a, eta, L, n) if i <= j else block(orc, r[j], r[i], j, i, a, eta, L, n).T
            out[3 * k:3 * k + 3, 3 * j:3 * j + 3] = b
    if damped:
        B = orc.damp(r.reshape(-1), a)
        idx = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in which])
        out = B[idx][:, None] * out * B[None, :]
    return out


def dense_matrices(orc, cfg, X, Q, a, eta, L, n):
    """(B M_per B, K, blob positions) of a configuration: what tests/joint_oracle.py: dense_matrices is to the open system"""
    from oracle import oracle as O
    cfg = np.asarray(cfg) - np.asarray(cfg).mean(axis=0)
    Qn = O.normalize_quats(np.asarray(Q, dtype=np.float64).reshape(-1, 4))
    r = orc.multi_body_pos(X, Qn, cfg)
    return dense_M(orc, r, a, eta, L, n), O.K_matrix(X, Qn, cfg), r


# ---- the force model with the minimum-image convention ----------------------------------------------------------------------
def hermite(U, dU, lo, hi, x):
    """(T, dT/dx) of the cubic Hermite table on the uniform grid lo .. hi at lo <= x <= hi (include/rbl.h section 4)"""
    n = len(U)
    h = (hi - lo) / (n - 1)
    s = (x - lo) / h
    k = min(int(s), n - 2)
    t = s - k
    D0, D1 = h * dU[k], h * dU[k + 1]
    c0, c1 = U[k], D0
    c2 = 3.0 * (U[k + 1] - U[k]) - 2.0 * D0 - D1
    c3 = 2.0 * (U[k] - U[k + 1]) + D0 + D1
    return c0 + t * (c1 + t * (c2 + t * c3)), (c1 + t * (2.0 * c2 + 3.0 * c3 * t)) / h


def pair_forces(r, n_blb, a, L, steric=None, table=None):
    """physical forces on the blobs r (N, 3) from the pair terms between blobs of DIFFERENT bodies, displacement by minimum image.
    steric = (eps, b, r_cut): U = eps (2a / r) exp(-(r - 2a) / b) for 2a <= r <= r_cut, the tangent at 2a continued inwards;
    table = (U, dU, r_min, r_cut): the tabulated potential, its tangent at r_min continued inwards.  -> (f (N, 3), energy)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    N = r.shape[0]
    f = np.zeros((N, 3))
    E = 0.0
    for i in range(N):
        for j in range(N):
            if i // n_blb == j // n_blb:
                continue
            d = nearest(r[i] - r[j], L)
            x = np.linalg.norm(d)
            g = 0.0                                                    # -U'(x) / x
            if steric is not None and x <= steric[2]:
                eps, b, _ = steric
                if x >= 2.0 * a:
                    U = eps * (2.0 * a / x) * np.exp(-(x - 2.0 * a) / b)
                    g += U * (1.0 / x + 1.0 / b) / x
                else:
                    slope = eps * (1.0 / (2.0 * a) + 1.0 / b)
                    U = eps + slope * (2.0 * a - x)
                    g += slope / x
                E += 0.5 * U
            if table is not None and x <= table[3]:
                Ut, dUt, lo, hi = table
                if x >= lo:
                    T, dT = hermite(Ut, dUt, lo, hi, x)
                else:
                    T, dT = Ut[0] + dUt[0] * (x - lo), dUt[0]
                E += 0.5 * T
                g -= dT / x
            f[i] += g * d
    return f, E


def KT(f, lever):
    """body force / torque about the centres of blob forces f (N_bod, N_blb, 3) with lever arms of the same shape: (6 N_bod,)"""
    return np.concatenate([f.sum(axis=1), np.cross(lever, f).sum(axis=1)], axis=1).reshape(-1)


def dipole_pairs(X, m_lab, c_dd, r_core, r_cut, L):
    """force and torque on every body from the dipole pairs between the body centres X (N_bod, 3), lab-frame moments m_lab,
    U = c_dd [m_i.m_j / s^3 - 3 (m_i.r)(m_j.r) / s^5], s = max(|r|, r_core), r by minimum image, skipped beyond r_cut
    -> (FT (6 N_bod,), energy)"""
    nb = X.shape[0]
    FT = np.zeros((nb, 6))
    E = 0.0
    for i in range(nb):
        for j in range(nb):
            if i == j:
                continue
            r = nearest(X[i] - X[j], L)
            d = np.linalg.norm(r)
            if d > r_cut:
                continue
            mi, mj = m_lab[i], m_lab[j]
            core = d < r_core
            s = r_core if core else d
            a_, b_, mm = mi @ r, mj @ r, mi @ mj
            k5 = 3.0 * c_dd / s ** 5
            kr = 0.0 if core else mm - 5.0 * a_ * b_ / s ** 2
            FT[i, :3] += k5 * (a_ * mj + b_ * mi + kr * r)
            h = k5 * b_ * r - c_dd / s ** 3 * mj                           # the partner's field at i
            FT[i, 3:] += np.cross(mi, h)
            E += 0.5 * c_dd * (mm / s ** 3 - 3.0 * a_ * b_ / s ** 5)
    return FT.reshape(-1), E


# ---- the same pair terms broadcast over rows of blobs: what the GPU tests beyond a few dozen blobs compare with.  The double loops
# above stay the definition; tests/test_periodic_shapes_cpu.py holds each form below against its loop -----------------------------
def _folds(d, L):
    """True where the minimum image of the displacements d (..., 3) is NOT the direct displacement (a fold on either axis)"""
    out = np.zeros(d.shape[:-1], dtype=bool)
    for k in (0, 1):
        if L[k] > 0.0:
            out |= np.rint(d[..., k] / L[k]) != 0.0
    return out


def hermite_v(U, dU, lo, hi, x):
    """hermite() on an array of lo <= x <= hi"""
    U, dU = np.asarray(U, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    n = len(U)
    h = (hi - lo) / (n - 1)
    s = (x - lo) / h
    k = np.minimum(s.astype(np.int64), n - 2)
    t = s - k
    D0, D1 = h * dU[k], h * dU[k + 1]
    c0, c1 = U[k], D0
    c2 = 3.0 * (U[k + 1] - U[k]) - 2.0 * D0 - D1
    c3 = 2.0 * (U[k] - U[k + 1]) + D0 + D1
    return c0 + t * (c1 + t * (c2 + t * c3)), (c1 + t * (2.0 * c2 + 3.0 * c3 * t)) / h


def pair_forces_v(r, n_blb, a, L, steric=None, table=None, rows=128):
    """pair_forces() in blocks of `rows` row blobs against all column blobs -> (f (N, 3), energy, n_direct, n_through): the ordered
    pairs of blobs of different bodies inside the cutoff of a term that is on, by whether their minimum image is the direct
    displacement or one through a boundary (n_direct + n_through is what rbl_interaction_stats counts)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    N = r.shape[0]
    body = np.arange(N) // n_blb
    f = np.zeros((N, 3))
    E = 0.0
    count = [0, 0]
    for i0 in range(0, N, rows):
        raw = r[i0:i0 + rows, None, :] - r[None, :, :]
        d = nearest(raw, L)
        x = np.sqrt((d * d).sum(axis=2))
        other = body[i0:i0 + rows, None] != body[None, :]
        g = np.zeros_like(x)                                           # -U'(x) / x
        inside = np.zeros_like(other)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if steric is not None:
                eps, b, rc = steric
                m = other & (x <= rc)
                far = x >= 2.0 * a
                Uf = eps * (2.0 * a / x) * np.exp(-(x - 2.0 * a) / b)
                slope = eps * (1.0 / (2.0 * a) + 1.0 / b)
                U = np.where(far, Uf, eps + slope * (2.0 * a - x))
                g += np.where(m, np.where(far, Uf * (1.0 / x + 1.0 / b) / x, slope / x), 0.0)
                E += 0.5 * U[m].sum()
                inside |= m
            if table is not None:
                Ut, dUt, lo, hi = table
                m = other & (x <= hi)
                T, dT = hermite_v(Ut, dUt, lo, hi, np.clip(x, lo, hi))
                below = x < lo
                T = np.where(below, Ut[0] + dUt[0] * (x - lo), T)
                dT = np.where(below, dUt[0], dT)
                g -= np.where(m, dT / x, 0.0)
                E += 0.5 * T[m].sum()
                inside |= m
        f[i0:i0 + rows] = (g[:, :, None] * d).sum(axis=1)
        through = _folds(raw, L)
        count[0] += int((inside & ~through).sum())
        count[1] += int((inside & through).sum())
    return f, E, count[0], count[1]


def dipole_pairs_v(X, m_lab, c_dd, r_core, r_cut, L):
    """dipole_pairs() with every partner of a body at once -> (FT (6 N_bod,), energy, n_direct, n_through), the counts as in
    pair_forces_v over the ordered pairs of bodies inside r_cut"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    m_lab = np.asarray(m_lab, dtype=np.float64).reshape(-1, 3)
    nb = X.shape[0]
    FT = np.zeros((nb, 6))
    E = 0.0
    count = [0, 0]
    for i in range(nb):
        raw = X[i] - X
        r = nearest(raw, L)
        d = np.sqrt((r * r).sum(axis=1))
        m = d <= r_cut
        m[i] = False
        r, d, mj, raw = r[m], d[m], m_lab[m], raw[m]
        mi = m_lab[i]
        core = d < r_core
        s = np.where(core, r_core, d)
        a_, b_, mm = r @ mi, (mj * r).sum(axis=1), mj @ mi
        k5 = 3.0 * c_dd / s ** 5
        kr = np.where(core, 0.0, mm - 5.0 * a_ * b_ / s ** 2)
        FT[i, :3] = (k5[:, None] * (a_[:, None] * mj + b_[:, None] * mi + kr[:, None] * r)).sum(axis=0)
        h = (k5 * b_)[:, None] * r - (c_dd / s ** 3)[:, None] * mj     # the partners' fields at i
        FT[i, 3:] = np.cross(mi, h).sum(axis=0)
        E += 0.5 * c_dd * (mm / s ** 3 - 3.0 * a_ * b_ / s ** 5).sum()
        through = _folds(raw, L)
        count[0] += int((~through).sum())
        count[1] += int(through.sum())
    return FT.reshape(-1), E, count[0], count[1]


def one_body_terms(r, X, n_blb, a, wall, builtin=None, height=None, traps=None):
    """weight, wall repulsion, height table and traps: they do not see the cell, so they are the open-system oracle's
    (tests/table_oracle.py) with every pair term off.  builtin: dict(w, eps_wall, b_wall) -> (f (N, 3), FT (6 N_bod,), energy)"""
    import table_oracle as to
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    bi = None if builtin is None else dict(w=builtin["w"], eps_wall=builtin["eps_wall"], b_wall=builtin["b_wall"], eps_blob=0.0,
                                           b_blob=1.0, r_cut=-1.0)      # no pair lies inside a negative cutoff
    # the blob terms as ONE body of all the blobs (no pair loop at all), K^T f about the real centres by KT(); the traps act on
    # the centres alone: the bodies as single blobs, no other term on
    f, _, E, npairs = to.interactions(r, np.zeros((1, 3)), r.shape[0], a, wall, builtin=bi, height=height)
    assert npairs == 0
    nb = X.shape[0]
    FT = KT(f.reshape(nb, n_blb, 3), r.reshape(nb, n_blb, 3) - X[:, None, :])
    if traps is not None:
        _, FTt, Et, npairs = to.interactions(X, X, 1, a, False, builtin=dict(w=0.0, eps_wall=0.0, b_wall=1.0, eps_blob=0.0, b_blob=1.0, r_cut=-1.0),
                                             traps=traps)
        assert npairs == 0
        FT = FT + FTt
        E += Et
    return f, FT, E


def force_model(r, X, n_blb, a, L, wall=True, builtin=None, steric=None, table=None, height=None, traps=None):
    """the whole blob force model in the cell: the minimum-image pair terms and the one-body terms added
    -> dict(f (N, 3), FT (6 N_bod,), E, direct, through)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    nb = X.shape[0]
    fp, Ep, nd, nt = pair_forces_v(r, n_blb, a, L, steric=steric, table=table)
    f1, FT1, E1 = one_body_terms(r, X, n_blb, a, wall, builtin=builtin, height=height, traps=traps)
    FT = KT(fp.reshape(nb, n_blb, 3), r.reshape(nb, n_blb, 3) - X[:, None, :]) + FT1
    return dict(f=fp + f1, FT=FT, E=Ep + E1, direct=nd, through=nt)
