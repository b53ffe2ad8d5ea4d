"""numpy model of the DEM walls from a mesh's boundary faces (include/dedflow.h, "particle walls"): a brute-force loop over
all wall triangles per particle with the library's contact law and de-duplication rule, plus the particle pairs and the
"outside the padded box" rule.  The unit-box law is here too, for comparison."""
import numpy as np

MAX_CONTACTS = 8


class Walls:
    """wall triangles of the groups in `groups`: vertices (nf, 3, 3) in ascending local index of the parent tet, inward unit
    normals, plane offsets, node ids; the mesh's bounding box and tolerance"""

    def __init__(self, m, groups=range(6)):
        xg, ien = m.xg.reshape(-1, 3), m.ien.reshape(-1, 4)
        sel = []
        for g in groups:
            sel.extend(range(m.bound_elem_offset[g], m.bound_elem_offset[g + 1]))
        sel = np.asarray(sel, dtype=np.int64)
        tet, opp = m.bound_f2e[sel].astype(np.int64), m.bound_forn[sel].astype(np.int64)
        keep = np.ones((sel.size, 4), dtype=bool)
        keep[np.arange(sel.size), opp] = False
        self.node = ien[tet][keep].reshape(-1, 3).astype(np.int64)
        self.v = xg[self.node]
        n = np.cross(self.v[:, 1] - self.v[:, 0], self.v[:, 2] - self.v[:, 0])
        n /= np.linalg.norm(n, axis=1)[:, None]
        inward = np.einsum("ij,ij->i", n, xg[ien[tet, opp]] - self.v[:, 0])
        n[inward < 0] *= -1.0
        self.n = n
        self.off = np.einsum("ij,ij->i", n, self.v[:, 0])
        self.lo, self.hi = xg.min(axis=0), xg.max(axis=0)
        self.tol = 1e-12 * np.linalg.norm(self.hi - self.lo)


def closest_features(v, p):
    """closest point of every triangle v (n, 3, 3) to the point p, by Voronoi region (Ericson 5.1.5).
    Returns kind (0 face, 1 edge, 2 vertex), local vertices e0, e1 (-1 unused), q (n, 3)"""
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    dot = lambda x, y: np.einsum("ij,ij->i", x, y)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    n = len(v)
    kind, e0, e1, q = np.zeros(n, np.int64), np.full(n, -1), np.full(n, -1), np.zeros((n, 3))
    done = np.zeros(n, bool)

    def take(m, k, i0, i1, qq):
        m = m & ~done
        kind[m], e0[m], e1[m] = k, i0, i1
        q[m] = qq[m]
        done[m] = True

    with np.errstate(divide="ignore", invalid="ignore"):
        take((d1 <= 0) & (d2 <= 0), 2, 0, -1, a)
        take((d3 >= 0) & (d4 <= d3), 2, 1, -1, b)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1, 0, 1, a + (d1 / (d1 - d3))[:, None] * ab)
        take((d6 >= 0) & (d5 <= d6), 2, 2, -1, c)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), 1, 0, 2, a + (d2 / (d2 - d6))[:, None] * ac)
        take((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1, 1, 2, b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        take(np.ones(n, bool), 0, -1, -1, a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None])
    return kind, e0, e1, q


def wall_contacts(W, p, v, R, kn, gn):
    """wall force on one particle and the number of contacts dropped by the cap; also the contact list
    [(kind, key, delta, normal)]"""
    # only triangles whose bounding box comes within R can matter (a superset of those within R)
    near = np.nonzero(np.all((W.v.min(axis=1) - R <= p) & (p <= W.v.max(axis=1) + R), axis=1))[0]
    f = np.zeros(3)
    contacts, dropped = [], 0
    if near.size == 0:
        return f, dropped, contacts
    kind, e0, e1, q = closest_features(W.v[near], p)
    node = W.node[near]
    s = np.einsum("ij,ij->i", p - W.v[near, 0], W.n[near])
    dist = np.linalg.norm(p - q, axis=1)
    key = []
    for r in range(near.size):
        if kind[r] == 1:
            a, b = node[r, e0[r]], node[r, e1[r]]
            key.append((min(a, b), max(a, b)))
        elif kind[r] == 2:
            key.append((node[r, e0[r]], -1))
        else:
            key.append(None)
    planes, keys = [], []
    for r in range(near.size):  # ascending triangle id
        t = near[r]
        if kind[r] != 0 or not (-R < s[r] < R):
            continue
        if any(np.all(np.abs(pn - W.n[t]) <= 1e-12) and abs(po - W.off[t]) <= W.tol for pn, po in planes):
            continue
        if len(planes) + len(keys) >= MAX_CONTACTS:
            dropped += 1
            continue
        planes.append((W.n[t], W.off[t]))
        fm = kn * (R - s[r]) - gn * (v @ W.n[t])
        f += fm * W.n[t]
        contacts.append((0, None, R - s[r], W.n[t]))
    for r in range(near.size):
        if kind[r] == 0 or not (s[r] > 0) or not (dist[r] < R):
            continue
        if any(abs(q[r] @ pn - po) <= W.tol for pn, po in planes):
            continue
        if key[r] in keys:
            continue
        k0, k1 = key[r]
        inc = [u for u in range(near.size) if u != r and k0 in node[u] and (k1 < 0 or k1 in node[u])]
        if any(dist[u] < dist[r] - W.tol for u in inc):
            continue
        if len(planes) + len(keys) >= MAX_CONTACTS:
            dropped += 1
            continue
        keys.append(key[r])
        nrm = (p - q[r]) / dist[r]
        fm = kn * (R - dist[r]) - gn * (v @ nrm)
        f += fm * nrm
        contacts.append((int(kind[r]), key[r], R - dist[r], nrm))
    return f, dropped, contacts


def padded_inside(W, x, R):
    """centres inside the mesh's bounding box padded by R (up to the cell rounding of the grid: points within 1e-9 of its
    faces should be avoided by tests)"""
    return np.all((x >= W.lo - R) & (x <= W.hi + R), axis=1)


def pair_forces(x, v, R, kn, gn, active, idx=None):
    """particle-pair forces on the particles idx (default all) from every other active particle"""
    from scipy.spatial import cKDTree
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    act = np.nonzero(active)[0]
    tree = cKDTree(x[act])
    F = np.zeros((len(idx), 3))
    for r, i in enumerate(idx):
        if not active[i]:
            continue
        for j in act[tree.query_ball_point(x[i], 2 * R)]:
            if j == i:
                continue
            rv = x[i] - x[j]
            d = np.linalg.norm(rv)
            if d >= 2 * R or d == 0.0:
                continue
            nrm = rv / d
            F[r] += (kn * (2 * R - d) - gn * ((v[i] - v[j]) @ nrm)) * nrm
    return F


def forces(W, x, v, R, mass=1.0, kn=1.0e4, gn=1.0, idx=None):
    """acc of the particles idx (default all) with walls W; also the total of dropped contacts"""
    x, v = x.reshape(-1, 3), v.reshape(-1, 3)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    active = padded_inside(W, x, R)
    F = pair_forces(x, v, R, kn, gn, active, idx)
    dropped = 0
    for r, i in enumerate(idx):
        if not active[i]:
            continue
        fw, nd, _ = wall_contacts(W, x[i], v[i], R, kn, gn)
        F[r] += fw
        dropped += nd
    return F / mass, dropped


def unit_box_wall_forces(x, v, R, kn, gn):
    """the six walls of the unit box (csrc/k_dem.hip)"""
    x, v = x.reshape(-1, 3), v.reshape(-1, 3)
    f = np.zeros_like(x)
    lo, hi = R - x, x + R - 1.0
    f += np.where(lo > 0, kn * lo - gn * v, 0.0)
    f -= np.where(hi > 0, kn * hi + gn * v, 0.0)
    return f
