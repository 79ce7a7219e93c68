"""numpy restatement of what rbl_ensemble_mc samples (include/rbl.h sections 4 and 5), written from the header: the energies of one
replica term by term, the part of them a body takes part in (what a trial of that body changes), the body update of a proposal,
and the replay of a trace.  One replica at a time; a helper -- no test in it.

A model is a dict: a, wall, and optionally builtin = dict(w, eps_wall, b_wall, eps_blob, b_blob, r_cut), pair / height =
(U, dU, lo, hi), traps = (k (N_bod, 3), X0 (N_bod, 3)), types (N_bod N_blb,) with tables {(s, t): (U, dU, lo, hi)},
bonds = dict(body (n, 2), anchor (n, 6), k (n,), l0 (n,), kind (n,), table), L = (Lx, Ly) the periodic cell (0: open axis)."""
import numpy as np


def rot(q):
    """rotation matrix of the unit quaternion (w, x, y, z): lab = R body"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def positions(cfg, X, Q):
    """blob positions (N_bod, N_blb, 3) of the structure cfg (its mean removed, as the library does) at centres X, orientations Q"""
    c = np.asarray(cfg, dtype=np.float64).reshape(-1, 3)
    c = c - c.mean(axis=0)
    return np.stack([X[b] + c @ rot(Q[b]).T for b in range(len(X))])


def update_X_Q(X, Q, d):
    """the body update of a proposal: X + dX, and the quaternion of the rotation vector phi multiplied from the left, normalised"""
    phi = np.asarray(d[3:], dtype=np.float64)
    n = np.sqrt(phi @ phi)
    qr = np.array([np.cos(n / 2.0), 0.0, 0.0, 0.0])
    if n > 1e-10:
        qr[1:] = np.sin(n / 2.0) / n * phi
    qr /= np.sqrt(qr @ qr)
    w, x, y, z = qr
    p = Q
    out = np.array([w * p[0] - x * p[1] - y * p[2] - z * p[3], w * p[1] + x * p[0] + y * p[3] - z * p[2],
                    w * p[2] + y * p[0] + z * p[1] - x * p[3], w * p[3] + z * p[0] + x * p[2] - y * p[1]])
    return X + np.asarray(d[:3]), out / np.sqrt(out @ out)


def hermite(tab, x, beyond="zero"):
    """U of a tabulated potential (U, dU, lo, hi) at x: cubic Hermite inside the grid, the tangent at lo below it; above hi
    nothing ("zero": pair, type and height tables) or the tangent at hi ("tangent": the bond table)"""
    U, dU, lo, hi = tab
    U, dU = np.asarray(U, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n = U.size
    h = (hi - lo) / (n - 1)
    s = (x - lo) / h
    k = np.clip(np.floor(np.maximum(s, 0.0)).astype(int), 0, n - 2)
    t = s - k
    D0, D1 = h * dU[k], h * dU[k + 1]
    c2 = 3.0 * (U[k + 1] - U[k]) - 2.0 * D0 - D1
    c3 = 2.0 * (U[k] - U[k + 1]) + D0 + D1
    val = U[k] + t * (D0 + t * (c2 + t * c3))
    val = np.where(x < lo, U[0] + dU[0] * (x - lo), val)
    above = U[-1] + dU[-1] * (x - hi) if beyond == "tangent" else 0.0
    return np.where(x > hi, above, val)


def steric(r, a, eps, b):
    two_a = 2.0 * a
    rs = np.maximum(r, two_a)
    return np.where(r >= two_a, eps * (two_a / rs) * np.exp(-(rs - two_a) / b), eps + eps * (1.0 / two_a + 1.0 / b) * (two_a - r))


def blob_terms(m, z):
    """single-blob energies at the heights z -> list of arrays, one per term that is on"""
    out = []
    bi = m.get("builtin")
    if bi is not None:
        out.append(bi["w"] * z)
        if m["wall"]:
            a, ew, bw = m["a"], bi["eps_wall"], bi["b_wall"]
            out.append(np.where(z >= a, ew * np.exp(-(np.maximum(z, a) - a) / bw), ew + ew / bw * (a - z)))
    if m.get("height") is not None:
        out.append(hermite(m["height"], z))
    return out


def pair_terms(m, ri, rj, ti=None, tj=None):
    """energies of the blob pairs (ri (n, 3)) x (rj (n', 3)) of two different bodies -> list of (n, n') arrays, one per term"""
    d = ri[:, None, :] - rj[None, :, :]
    L = m.get("L")
    if L is not None:
        for ax in range(2):
            if L[ax] > 0.0:
                d[..., ax] -= L[ax] * np.rint(d[..., ax] / L[ax])
    r = np.sqrt((d * d).sum(axis=2))
    out = []
    bi = m.get("builtin")
    if bi is not None:
        out.append(np.where(r <= bi["r_cut"], steric(r, m["a"], bi["eps_blob"], bi["b_blob"]), 0.0))
    if m.get("pair") is not None:
        out.append(np.where(r <= m["pair"][3], hermite(m["pair"], r), 0.0))
    for (s, t), tab in (m.get("tables") or {}).items():
        sel = ((ti[:, None] == s) & (tj[None, :] == t)) | ((ti[:, None] == t) & (tj[None, :] == s))
        out.append(np.where(sel & (r <= tab[3]), hermite(tab, r), 0.0))
    return out


def bond_energy(m, X, Q, b):
    B = m["bonds"]
    i, j = int(B["body"][b][0]), int(B["body"][b][1])
    an = np.asarray(B["anchor"][b], dtype=np.float64)
    pA = X[i] + rot(Q[i]) @ an[:3]
    pB = X[j] + rot(Q[j]) @ an[3:] if j >= 0 else an[3:]
    d = np.sqrt((pA - pB) @ (pA - pB))
    if int(B["kind"][b]) == 0:
        return 0.5 * B["k"][b] * (d - B["l0"][b]) ** 2
    return B["k"][b] * float(hermite(B["table"], d, beyond="tangent"))


def trap_energy(m, X, b):
    k, X0 = m["traps"]
    return 0.5 * float((np.asarray(k)[b] * (X[b] - np.asarray(X0)[b]) ** 2).sum())


def body_energy(m, cfg, X, Q, b, r=None):
    """everything of the total energy that body b takes part in -- its blobs' single-blob terms, the FULL energy of every pair with a
    blob of another body, its trap, the bonds that end on it -- and the sum of the magnitudes of those contributions"""
    r = positions(cfg, X, Q) if r is None else r
    nb, nbl = r.shape[0], r.shape[1]
    ty = None if m.get("types") is None else np.asarray(m["types"]).reshape(nb, nbl)
    E = S = 0.0
    for term in blob_terms(m, r[b, :, 2]):
        E += term.sum()
        S += np.abs(term).sum()
    for j in range(nb):
        if j == b:
            continue
        for term in pair_terms(m, r[b], r[j], None if ty is None else ty[b], None if ty is None else ty[j]):
            E += term.sum()
            S += np.abs(term).sum()
    if m.get("traps") is not None:
        e = trap_energy(m, X, b)
        E += e
        S += abs(e)
    if m.get("bonds") is not None:
        for k in range(len(m["bonds"]["body"])):
            if b in (int(m["bonds"]["body"][k][0]), int(m["bonds"]["body"][k][1])):
                e = bond_energy(m, X, Q, k)
                E += e
                S += abs(e)
    return float(E), float(S)


def energy_terms(m, cfg, X, Q):
    """the total energy of one replica, term by term -> dict(blob, pairs, traps, bonds, total)"""
    r = positions(cfg, X, Q)
    nb, nbl = r.shape[0], r.shape[1]
    ty = None if m.get("types") is None else np.asarray(m["types"]).reshape(nb, nbl)
    out = dict(blob=0.0, pairs=0.0, traps=0.0, bonds=0.0)
    out["blob"] = float(sum(t.sum() for t in blob_terms(m, r[:, :, 2].ravel())))
    for i in range(nb):
        for j in range(i + 1, nb):
            out["pairs"] += float(sum(t.sum() for t in pair_terms(m, r[i], r[j], None if ty is None else ty[i], None if ty is None else ty[j])))
    if m.get("traps") is not None:
        out["traps"] = sum(trap_energy(m, X, b) for b in range(nb))
    if m.get("bonds") is not None:
        out["bonds"] = sum(bond_energy(m, X, Q, k) for k in range(len(m["bonds"]["body"])))
    out["total"] = out["blob"] + out["pairs"] + out["traps"] + out["bonds"]
    return out


def replay(m, cfg, X0, Q0, trace):
    """apply a replica's trace (rows: body, dX (3), phi (3), dE, u_6, verdict) to (X0, Q0): every trial's oracle dE and the scale
    of its bound (the magnitudes of the moved body's contributions, old plus new; nan for a trial rejected at the wall, whose
    energy is not evaluated), whether the proposal puts a blob below z = 0, and the configuration after the accepted trials"""
    X, Q = np.array(X0, dtype=np.float64), np.array(Q0, dtype=np.float64)
    dE, scale, below = [], [], []
    for row in trace:
        b = int(row[0])
        if b < 0:
            break
        Xn, Qn = X.copy(), Q.copy()
        Xn[b], Qn[b] = update_X_Q(X[b], Q[b], row[1:7])
        rn = positions(cfg, Xn, Qn)
        below.append(bool((rn[b, :, 2] < 0.0).any()))
        if int(row[9]) == 2:
            dE.append(np.nan)
            scale.append(np.nan)
        else:
            Eo, So = body_energy(m, cfg, X, Q, b)
            En, Sn = body_energy(m, cfg, Xn, Qn, b, rn)
            dE.append(En - Eo)
            scale.append(So + Sn)
        if int(row[9]) == 1:
            X, Q = Xn, Qn
    return np.array(dE), np.array(scale), np.array(below), X, Q
