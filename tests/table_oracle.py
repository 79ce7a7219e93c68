"""Pure-numpy all-pairs restatement of the whole force model of include/rbl.h section 4 (test infrastructure, no build step):
the built-in weight / wall / steric terms, the tabulated pair and height potentials (cubic Hermite in (U, dU/dr) on a uniform
grid, tangent continuation below the grid, nothing beyond it) and the harmonic traps on the body centres."""
import numpy as np


def hermite_coef(U, dU, lo, hi):
    """the four coefficients per interval, (n - 1, 4): with D = h dU and t = (x - x_k) / h,
    U = c0 + t (c1 + t (c2 + t c3)) and dU/dx = (c1 + t (2 c2 + 3 c3 t)) / h"""
    U, dU = np.asarray(U, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    n = U.size
    h = (hi - lo) / (n - 1)
    D = h * dU
    c = np.empty((n - 1, 4))
    c[:, 0] = U[:-1]
    c[:, 1] = D[:-1]
    c[:, 2] = 3.0 * (U[1:] - U[:-1]) - 2.0 * D[:-1] - D[1:]
    c[:, 3] = 2.0 * (U[:-1] - U[1:]) + D[:-1] + D[1:]
    return c


def table_eval(tab, x):
    """tab = (U, dU, lo, hi); -> (U(x), dU/dx(x)); zero above hi, the tangent at lo below it"""
    U, dU, lo, hi = tab
    U, dU = np.asarray(U, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    n = U.size
    c = hermite_coef(U, dU, lo, hi)
    x = np.asarray(x, dtype=np.float64)
    inv_h = (n - 1) / (hi - lo)
    s = (x - lo) * inv_h
    k = np.clip(np.floor(np.where(s > 0, s, 0.0)).astype(np.int64), 0, n - 2)
    t = s - k
    ck = c[k]
    Ui = ck[..., 0] + t * (ck[..., 1] + t * (ck[..., 2] + t * ck[..., 3]))
    dUi = (ck[..., 1] + t * (2.0 * ck[..., 2] + 3.0 * ck[..., 3] * t)) * inv_h
    below = x < lo
    Ui = np.where(below, U[0] + dU[0] * (x - lo), Ui)
    dUi = np.where(below, dU[0], dUi)
    out = x > hi
    return np.where(out, 0.0, Ui), np.where(out, 0.0, dUi)


def steric(r, a, eps, b):
    """the built-in pair term -> (U, dU/dr), tangent continued below 2a"""
    two_a = 2.0 * a
    rs = np.where(r >= two_a, r, two_a)
    Uo = eps * (two_a / rs) * np.exp(-(rs - two_a) / b)
    dUo = -Uo * (1.0 / rs + 1.0 / b)
    slope = eps * (1.0 / two_a + 1.0 / b)
    inside = r < two_a
    return np.where(inside, eps + slope * (two_a - r), Uo), np.where(inside, -slope, dUo)


def interactions(r, X, N_blb, a, wall, builtin=None, pair=None, height=None, traps=None):
    """r (N, 3) blob positions, X (N_bod, 3) body centres.  builtin: dict(w, eps_wall, b_wall, eps_blob, b_blob, r_cut) or None;
    pair, height: (U, dU, lo, hi) or None; traps: (k (N_bod, 3), X0 (N_bod, 3)) or None.
    -> f_blob (N, 3) (without the traps), FT_body (6 N_bod) physical force / torque about X (with them), total energy,
    ordered blob pairs inside the cutoff of a pair term that is on"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    nb = X.shape[0]
    assert r.shape[0] == nb * N_blb
    f = np.zeros_like(r)
    E = 0.0
    npairs = 0
    for i in range(nb):
        si = slice(i * N_blb, (i + 1) * N_blb)
        for j in range(nb):
            if j == i:
                continue
            d = r[si, None, :] - r[None, j * N_blb:(j + 1) * N_blb, :]
            dist = np.sqrt((d * d).sum(axis=2))
            U = np.zeros_like(dist)
            dU = np.zeros_like(dist)
            counted = np.zeros(dist.shape, dtype=bool)
            if builtin is not None:
                m = dist <= builtin["r_cut"]
                Ub, dUb = steric(dist, a, builtin["eps_blob"], builtin["b_blob"])
                U += np.where(m, Ub, 0.0)
                dU += np.where(m, dUb, 0.0)
                counted |= m
            if pair is not None:
                m = dist <= pair[3]
                Ut, dUt = table_eval(pair, dist)
                U += np.where(m, Ut, 0.0)
                dU += np.where(m, dUt, 0.0)
                counted |= m
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
        Uh, dUh = table_eval(height, z)
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
    return f, FT, E, npairs
