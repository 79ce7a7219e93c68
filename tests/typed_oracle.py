"""Pure-numpy all-pairs restatement of the force model of include/rbl.h section 4 WITH blob types (test infrastructure, no build
step, no library code): tests/table_oracle.py's loop -- its statements in its order, so that one type with T_00 = X gives the very
numbers of table_oracle.interactions(pair=X) -- with the table of the two blobs' types added to every pair, and the same loop with
the pair displacement by minimum image (tests/periodic_oracle.py: nearest)."""
import numpy as np

import periodic_oracle
import table_oracle


def type_table(tables, s, t):
    """the table of the unordered type pair (s, t) from {(s, t): (U, dU, lo, hi)}, None: the pair has none"""
    return tables.get((s, t), tables.get((t, s)))


def cutoffs(builtin=None, pair=None, tables=None):
    """every pair cutoff that is on"""
    out = [] if builtin is None else [builtin["r_cut"]]
    if pair is not None:
        out.append(pair[3])
    return out + [tab[3] for tab in (tables or {}).values()]


def interactions(r, X, N_blb, a, wall, types=None, tables=None, builtin=None, pair=None, height=None, traps=None, L=None):
    """table_oracle.interactions' arguments and: types (N,) integers, one per blob of the system; tables {(s, t): (U, dU, lo, hi)},
    one per unordered type pair (both orders name the same table; giving both is an error); L = (Lx, Ly) the periodic cell (0: that
    axis is open), None: the open system.
    -> f_blob (N, 3) (without the traps), FT_body (6 N_bod) about X (with them), total energy, ordered blob pairs inside the
    cutoff of a pair term that is on, ordered blob pairs inside the cutoff of THEIR type table"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    nb = X.shape[0]
    assert r.shape[0] == nb * N_blb
    tables = dict(tables or {})
    assert not any((t, s) in tables for (s, t) in tables if s != t), "one table per unordered type pair"
    if tables:
        types = np.asarray(types).reshape(-1)
        assert types.shape[0] == r.shape[0]
    f = np.zeros_like(r)
    E = 0.0
    npairs = 0
    ntyped = 0
    for i in range(nb):
        si = slice(i * N_blb, (i + 1) * N_blb)
        for j in range(nb):
            if j == i:
                continue
            sj = slice(j * N_blb, (j + 1) * N_blb)
            d = r[si, None, :] - r[None, sj, :]
            if L is not None:
                d = periodic_oracle.nearest(d, L)
            dist = np.sqrt((d * d).sum(axis=2))
            U = np.zeros_like(dist)
            dU = np.zeros_like(dist)
            counted = np.zeros(dist.shape, dtype=bool)
            if builtin is not None:
                m = dist <= builtin["r_cut"]
                Ub, dUb = table_oracle.steric(dist, a, builtin["eps_blob"], builtin["b_blob"])
                U += np.where(m, Ub, 0.0)
                dU += np.where(m, dUb, 0.0)
                counted |= m
            if pair is not None:
                m = dist <= pair[3]
                Ut, dUt = table_oracle.table_eval(pair, dist)
                U += np.where(m, Ut, 0.0)
                dU += np.where(m, dUt, 0.0)
                counted |= m
            for (s, t), tab in tables.items():
                ti, tj = types[si, None], types[None, sj]
                m = (((ti == s) & (tj == t)) | ((ti == t) & (tj == s))) & (dist <= tab[3])
                if not m.any():
                    continue
                Ut, dUt = table_oracle.table_eval(tab, dist[m])      # the pairs of these types inside the cutoff only: the same numbers
                U[m] += Ut
                dU[m] += dUt
                counted |= m
                ntyped += int(m.sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(dist > 0.0, -dU / dist, 0.0)
            f[si] += (g[:, :, None] * d).sum(axis=1)
            E += 0.5 * U.sum()
            npairs += int(counted.sum())
    z = r[:, 2]
    if builtin is not None:
        f[:, 2] -= builtin["w"]
        E += builtin["w"] * z.sum()
        if wall:
            ew, bw = builtin["eps_wall"], builtin["b_wall"]
            zs = np.where(z >= a, z, a)
            Uw = ew * np.exp(-(zs - a) / bw)
            f[:, 2] += np.where(z >= a, Uw / bw, ew / bw)
            E += np.where(z >= a, Uw, ew + ew / bw * (a - z)).sum()
    if height is not None:
        Uh, dUh = table_oracle.table_eval(height, z)
        f[:, 2] -= dUh
        E += Uh.sum()
    FT = np.zeros(6 * nb)
    for b in range(nb):
        sl = slice(b * N_blb, (b + 1) * N_blb)
        FT[6 * b:6 * b + 3] = f[sl].sum(axis=0)
        FT[6 * b + 3:6 * b + 6] = np.cross(r[sl] - X[b], f[sl]).sum(axis=0)
    if traps is not None:
        k, X0 = np.asarray(traps[0], dtype=np.float64).reshape(nb, 3), np.asarray(traps[1], dtype=np.float64).reshape(nb, 3)
        FT.reshape(nb, 6)[:, :3] -= k * (X - X0)
        E += 0.5 * (k * (X - X0) ** 2).sum()
    return f, FT, E, npairs, ntyped


def pair_distances(r, N_blb, L=None):
    """distances between blobs of different bodies (unordered pairs), by minimum image in the cell L"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    nb = r.shape[0] // N_blb
    out = []
    for i in range(nb):
        for j in range(i + 1, nb):
            d = r[i * N_blb:(i + 1) * N_blb, None, :] - r[None, j * N_blb:(j + 1) * N_blb, :]
            if L is not None:
                d = periodic_oracle.nearest(d, L)
            out.append(np.sqrt((d * d).sum(axis=2)).ravel())
    return np.concatenate(out)


def clear_of_cutoffs(r, N_blb, cuts, L=None, margin=1e-9):
    """no pair distance lies within `margin` of any cutoff: the pair counts of two implementations can then be compared exactly"""
    d = pair_distances(r, N_blb, L)
    return all(np.abs(d - c).min() > margin for c in cuts)
