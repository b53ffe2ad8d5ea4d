"""Numpy model of the particle heat transfer (host/heat.c, csrc/k_heat.hip), written from the rules in include/dedflow.h
"particle heat transfer": Batchelor-O'Brien contact conduction over all pairs or over a cell list, Ranz-Marshall
convection, the implicit temperature update and the node scatter of the heat source.  float64, with np.longdouble sums
where a bound needs them.  Shared by test_heat_cpu.py and test_gpu_heat.py."""
import numpy as np

K_F, CP_F = 0.66, 1.0          # the reference's kKAPPA and kCP: the defaults of DflParticleHeat
EPS = np.finfo(np.float64).eps


def conductance(ri, rj, dist, k_p):
    """H = 2 k_p sqrt(r* delta), r* = r_i r_j / (r_i + r_j), delta = (r_i + r_j) - dist (commutative in i, j)"""
    rs = ri + rj
    return (2.0 * k_p) * np.sqrt((ri * rj) / rs * (rs - dist))


def contacts_all_pairs(x, r):
    """(i, j, dist) of every ordered pair in contact: 0 < dist^2 < (r_i + r_j)^2, the force kernel's test"""
    x = np.asarray(x, float).reshape(-1, 3)
    r = np.broadcast_to(np.asarray(r, float), (len(x),))
    d = x[:, None, :] - x[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    rs = r[:, None] + r[None, :]
    i, j = np.nonzero((d2 < rs * rs) & (d2 > 0.0))
    return i, j, np.sqrt(d2[i, j])


def contacts_cell_list(x, r, cell):
    """the same contacts found through a uniform cell list of edge `cell` >= 2 max(r) (27-cell search)"""
    x = np.asarray(x, float).reshape(-1, 3)
    r = np.broadcast_to(np.asarray(r, float), (len(x),))
    c = np.floor(x / cell).astype(np.int64)
    bins = {}
    for p, key in enumerate(map(tuple, c)):
        bins.setdefault(key, []).append(p)
    I, J, D = [], [], []
    for p in range(len(x)):
        cx, cy, cz = c[p]
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    for q in bins.get((cx + dx, cy + dy, cz + dz), ()):
                        if q == p:
                            continue
                        e = x[p] - x[q]
                        d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
                        rs = r[p] + r[q]
                        if 0.0 < d2 < rs * rs:
                            I.append(p); J.append(q); D.append(np.sqrt(d2))
    o = np.lexsort((J, I))
    return np.array(I, np.int64)[o], np.array(J, np.int64)[o], np.array(D)[o]


def conduction(x, r, T, k_p, pairs=None):
    """q_i = sum_j H_ij (T_j - T_i) summed in np.longdouble; also sum_j |H_ij (T_j - T_i)|, the contact count per
    particle, sum_j H_ij and sum_j |term| (r_i + r_j + dist) / delta: delta = (r_i + r_j) - dist cancels, so one rounding of
    its operands moves H = O(sqrt(delta)) by eps (r_i + r_j + dist) / (2 delta) relative"""
    x = np.asarray(x, float).reshape(-1, 3)
    P = len(x)
    r = np.broadcast_to(np.asarray(r, float), (P,))
    T = np.asarray(T, float)
    i, j, dist = contacts_all_pairs(x, r) if pairs is None else pairs
    H = conductance(r[i], r[j], dist, k_p)
    term = (H * (T[j] - T[i])).astype(np.longdouble)
    q = np.zeros(P, np.longdouble)
    qa = np.zeros(P, np.longdouble)
    hs = np.zeros(P)
    qc = np.zeros(P)
    np.add.at(q, i, term)
    np.add.at(qa, i, np.abs(term))
    np.add.at(hs, i, H)
    rs = r[i] + r[j]
    np.add.at(qc, i, np.abs(term).astype(float) * (rs + dist) / (rs - dist))
    return q, qa, np.bincount(i, minlength=P), hs, qc


def nusselt(re, pr):
    """Ranz-Marshall"""
    return 2.0 + 0.6 * np.sqrt(np.asarray(re, np.longdouble)) * np.cbrt(np.longdouble(pr))


def tau_T(C, nu, k_f, d):
    return C / (nu * k_f * np.pi * d)


def update(T, q, C, dt, Tf=None, tau=None, located=None):
    """the temperature update: returns (T', heat_rate, e).  Convection (implicit) where `located`, else explicit conduction"""
    T = np.asarray(T, np.longdouble)
    q = np.zeros_like(T) if q is None else np.asarray(q, np.longdouble)
    C = np.asarray(C, np.longdouble)
    Tn = T + dt * q / C
    e = np.zeros_like(T)
    if Tf is not None:
        located = np.ones(T.shape, bool) if located is None else np.asarray(located, bool)
        tau = np.where(located, tau, 1.0)
        Tc = (T + dt * (q / C + np.asarray(Tf, np.longdouble) / tau)) / (1.0 + dt / tau)
        Tn = np.where(located, Tc, Tn)
        e = np.where(located, dt * C * (Tf - Tn) / tau, 0.0)
    return Tn, C * (Tn - T) / dt, e


def convection(w, N, ien, tet, lam, vel, mass, radius, cp_p, dt, rho_f, mu_f, k_f=K_F, cp_f=CP_F):
    """(T_f, Re, Nu, tau_T, located) of every particle in the fluid state w [6N] at its tet / lambda"""
    ien4 = np.asarray(ien).reshape(-1, 4)
    tet = np.asarray(tet)
    located = tet >= 0
    nodes = ien4[np.where(located, tet, 0)]
    lam = np.asarray(lam, np.longdouble)
    Tn = np.asarray(w)[5 * N:6 * N]
    u = np.asarray(w)[:3 * N].reshape(-1, 3)
    Tf = np.einsum("na,na->n", lam, Tn[nodes].astype(np.longdouble))
    uf = np.einsum("na,nad->nd", lam, u[nodes].astype(np.longdouble))
    d = 2.0 * np.asarray(radius, np.longdouble)
    s = uf - np.asarray(vel, np.longdouble).reshape(-1, 3)
    re = rho_f * np.sqrt((s * s).sum(axis=1)) * d / mu_f
    nu = nusselt(re, cp_f * mu_f / k_f)
    tau = tau_T(np.asarray(mass, np.longdouble) * cp_p, nu, k_f, d)
    return Tf, re, nu, tau, located


def node_scatter(num_node, ien, tets, lam, e, elapsed):
    """q[a] = -sum_p lambda_{a,p} e_p / elapsed over the located particles, and sum |terms| per node, term counts"""
    ien4 = np.asarray(ien).reshape(-1, 4)
    tets = np.asarray(tets)
    ok = tets >= 0
    nodes = ien4[tets[ok]].reshape(-1)
    terms = (np.asarray(lam, np.longdouble)[ok] * np.asarray(e, np.longdouble)[ok][:, None]).reshape(-1)
    q = np.zeros(num_node, np.longdouble)
    qa = np.zeros(num_node, np.longdouble)
    np.add.at(q, nodes, terms)
    np.add.at(qa, nodes, np.abs(terms))
    return -q / elapsed, qa / elapsed, np.bincount(nodes, minlength=num_node)
