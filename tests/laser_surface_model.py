"""numpy model of the laser on the level-set surface (include/dedflow.h, "laser on the level-set surface"), written from the
header.  It imports laser_model and redistance_model and changes neither.  Everything that DECIDES something -- which facets
are candidates, (i, j, t) of their vertices, which facet a column's centre ray hits first -- is float64 with the header's
association, so the library takes the same decisions; every compared value (lambda, nodal power, tally) is np.longdouble,
summed sequentially in the defined order.  Shared by test_laser_surface_cpu.py and test_gpu_laser_surface.py."""
import numpy as np

import laser_model as lm
import redistance_model as rm

EPS = lm.EPS
LD = np.longdouble


def refusal(laser_on, coupled, level, side):
    """why ParticleContextSetLaserSurface refuses, or None"""
    if not laser_on:
        return "laser"
    if not coupled:
        return "coupling"
    if side not in (1, -1):
        return "side"
    if not np.isfinite(level):
        return "level"
    return None


class Candidates:
    """the candidate facets of phi = level for a beam: F [nf, 9], tet [nf], and per vertex the edge (i, j) [nf, 3] and t
    [nf, 3].  As a candidate list of laser_model.hits: id = -2 - tet, v = F"""

    def __init__(self, xg, ien, phi, level, side, direction):
        xg = np.asarray(xg, np.float64).reshape(-1, 3)
        ien = np.asarray(ien).reshape(-1, 4)
        phi = np.asarray(phi, np.float64)
        F, tet = rm.facets(xg, ien, phi, level)                     # ascending tet, a quad's first triangle first
        _, x, ph, f, pos = rm._tets(xg, ien, phi, level, np.float64)
        npos, order = rm._cases(pos)
        # the edge of every facet vertex, in the header's order
        I, J = np.zeros((len(ien), 2, 3), np.int64), np.zeros((len(ien), 2, 3), np.int64)
        k = npos == 1
        I[k, 0], J[k, 0] = order[k, 0][:, None], order[k, 1:4]
        k = npos == 3
        I[k, 0], J[k, 0] = order[k, 0:3], order[k, 3][:, None]
        k = npos == 2
        a, b, c, d = (order[k, q] for q in range(4))
        I[k, 0], J[k, 0] = np.stack([a, a, b], 1), np.stack([c, d, d], 1)      # P_ac, P_ad, P_bd
        I[k, 1], J[k, 1] = np.stack([a, b, b], 1), np.stack([c, d, c], 1)      # P_ac, P_bd, P_bc
        which = np.concatenate([np.arange(n) for n in np.bincount(tet, minlength=len(ien))]).astype(np.int64) if len(tet) \
            else np.zeros(0, np.int64)
        i, j = I[tet, which], J[tet, which]
        r = tet[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = f[r, i] / (f[r, i] - f[r, j])
            P = x[r, i] + t[..., None] * (x[r, j] - x[r, i])
        same = (P.reshape(-1, 9) == F) | (np.isnan(P.reshape(-1, 9)) & np.isnan(F))
        assert same.all()                                           # the same crossing points, bit for bit
        # the tet gradient: g = ((phi1 - phi0) c23 + (phi2 - phi0) c31 + (phi3 - phi0) c12) / det
        e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
        c23, c31, c12 = rm.cross(e2, e3), rm.cross(e3, e1), rm.cross(e1, e2)
        det = rm.dot(e1, c23)
        dvec = np.asarray(direction, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = (((ph[:, 1] - ph[:, 0])[:, None] * c23 + (ph[:, 2] - ph[:, 0])[:, None] * c31) + (ph[:, 3] - ph[:, 0])[:, None] * c12) \
                / det[:, None]
            gn = np.sqrt(rm.dot(g, g))
            gd = (g[:, 0] * dvec[0] + g[:, 1] * dvec[1]) + g[:, 2] * dvec[2]
            enters = (float(side) * gd > 0.0) & (gn > 0.0)          # a NaN is not greater
        keep = enters[tet] & np.isfinite(F).all(axis=1)
        self.F, self.tet, self.i, self.j, self.t = F[keep], tet[keep], i[keep], j[keep], t[keep]
        self.nodes = ien[self.tet].astype(np.int64)                 # [nf, 4]
        self.id, self.v = -2 - self.tet, self.F
        self.node = np.full((len(self.tet), 3), -1, np.int64)       # (a facet has no boundary nodes)

    def vertex_weights(self):
        """c[f, k, a] in longdouble: 1 - t at local node i, t at j"""
        nf = len(self.tet)
        c = np.zeros((nf, 3, 4), LD)
        r, k = np.arange(nf)[:, None], np.arange(3)[None, :]
        c[r, k, self.i] = LD(1) - self.t.astype(LD)
        c[r, k, self.j] = self.t.astype(LD)
        return c


class Merged:
    """boundary candidates (laser_model.Substrate or None) followed by the facets: one list, as the library's"""

    def __init__(self, sub, cand):
        self.nb = 0 if sub is None else len(sub.id)
        parts = [p for p in (sub, cand) if p is not None and len(p.id)]
        self.id = np.concatenate([np.asarray(p.id, np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
        self.v = np.concatenate([np.asarray(p.v, np.float64).reshape(-1, 3, 3) for p in parts]) if parts else np.zeros((0, 3, 3))
        self.node = np.concatenate([np.asarray(p.node, np.int64) for p in parts]) if parts else np.zeros((0, 3), np.int64)


def first_hit(sub, cand, beam, o):
    """laser_model.hits on the boundary candidates and on the facets, the smaller depth wins, a tie goes to the boundary
    face.  Returns per column: face (index in the merged list, -1), wts, depth, kappa, edge_dist"""
    fb, wb, db, kb, eb = lm.hits(sub, beam, o)
    fs, ws, ds, ks, es = lm.hits(cand if cand is not None and len(cand.id) else None, beam, o)
    nb = 0 if sub is None else len(sub.id)
    surf = (fs >= 0) & ((fb < 0) | (ds < db))
    face = np.where(surf, fs + nb, fb)
    return (face, np.where(surf[:, None], ws, wb), np.where(surf, ds, db), np.where(surf, ks, kb), np.minimum(eb, es))


def step(beam, x, r, t=0.0, sub=None, cand=None):
    """one laser step with boundary candidates `sub` and surface candidates `cand`.  laser_model.step on the merged list
    gives rate, T, face (record id: -2 - tet for a surface hit) and the tally; added here: surf (columns that hit a facet),
    facet (its index in cand), lam [ncol, 4], power {node: W} and power_bound {node: W} of the surface, q / q_bound of the
    boundary faces alone"""
    mg = Merged(sub, cand)
    out = lm.step(beam, x, r, t=t, sub=mg if len(mg.id) else None)
    face, wts, depth, kappa, edge_dist = out["hit"]
    sep = first_hit(sub, cand, beam, beam.at(t))                    # the two lists hit separately, depths compared
    assert np.array_equal(sep[0], face) and np.array_equal(sep[2], depth)
    has = face >= 0
    surf = has & (face >= mg.nb)
    T, T_rel = out["T"], out["T_rel"]
    sub_c = np.where(has, LD(beam.eta_s) * T, LD(0))
    q, qb, qn = {}, {}, {}
    for c in np.nonzero(has & ~surf)[0]:                            # the boundary deposit, as laser_model.step
        for k in range(3):
            nd = int(mg.node[face[c], k])
            q[nd] = q.get(nd, LD(0)) + sub_c[c] * wts[c, k]
            qn[nd] = qn.get(nd, 0) + 1
            qb[nd] = qb.get(nd, 0.0) + float(sub_c[c]) * (8 * EPS * kappa[c] + abs(float(wts[c, k])) * (T_rel[c] + 4 * EPS))
    for nd in q:
        qb[nd] += (qn[nd] + 4) * EPS * float(abs(q[nd]))
    lam = np.zeros((beam.ncol, 4), LD)
    facet = np.where(surf, face - mg.nb, -1)
    power, pb, pn = {}, {}, {}
    if surf.any():
        cw = cand.vertex_weights()
        for c in np.nonzero(surf)[0]:                               # ascending column id
            f = facet[c]
            for a in range(4):
                terms = [wts[c, k] * cw[f, k, a] for k in range(3)]
                lam[c, a] = (terms[0] + terms[1]) + terms[2]
                nd = int(cand.nodes[f, a])
                power[nd] = power.get(nd, LD(0)) + sub_c[c] * lam[c, a]
                pn[nd] = pn.get(nd, 0) + 1
                # the bound of laser_model.step's q_bound, term by term: 8 eps kappa on every barycentric weight w_k, here
                # weighted by c_ka <= 1; T_rel on T_c and 4 eps for eta_s T_c and the product with lambda; and 6 roundings
                # of lambda itself on sum_k |w_k| c_ka -- 1 - t (1), the three products (3), the two-level sum (2); t is the
                # model's own float64 t, bit for bit, and carries none
                csum = float(sum(cw[f, k, a] for k in range(3)))
                mag = float(sum(abs(wts[c, k]) * cw[f, k, a] for k in range(3)))
                pb[nd] = pb.get(nd, 0.0) + float(sub_c[c]) * (8 * EPS * kappa[c] * csum + abs(float(lam[c, a])) * (T_rel[c] + 4 * EPS)
                                                             + 6 * EPS * mag)
        for nd in power:
            pb[nd] += (pn[nd] + 4) * EPS * float(abs(power[nd]))   # the sequential sum, every term >= 0
    out.update(q=q, q_bound=qb, surf=surf, facet=facet, lam=lam, power=power, power_bound=pb, merged=mg)
    return out


def entering_under(cand, sub, beam, o):
    """per column: how many candidates (both lists) hold the centre ray in their projection (edges included)"""
    cu, cv = beam.centres()
    n = np.zeros(beam.ncol, np.int64)
    for p in (sub, cand):
        if p is None or len(p.id) == 0:
            continue
        u, v, _ = (a.reshape(-1, 3) for a in beam.project(np.asarray(p.v, np.float64).reshape(-1, 3), o))
        a, b = u[:, None, :] - cu[None, :, None], v[:, None, :] - cv[None, :, None]
        w0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        w1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        w2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        tot = (w0 + w1) + w2
        inside = (tot != 0) & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
        n += inside.sum(axis=0)
    return n


# ---- the inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------
DIRECTIONS = {"vertical": (0.0, 0.0, -1.0), "oblique": (0.15, -0.1, -1.0)}
PLANE_N, PLANE_LEVEL = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13), 0.03
SIDE = -1                                                           # metal where phi < level: below the plane


def mesh():
    from dedflow_amd.meshgen import kuhn_cube
    return kuhn_cube(4, jitter=0.2)


def beam_args(direction="vertical", **kw):
    a = dict(origin=(0.5137, 0.4929, 1.3), direction=DIRECTIONS[direction], power=400.0, w=0.2, h=0.05, r_cut=0.4, eta_p=0.35,
             eta_s=0.7)
    a.update(kw)
    return a


def plane_phi(xg):
    return (np.asarray(xg, np.float64).reshape(-1, 3) - 0.5) @ PLANE_N


def two_layer_phi(xg):
    z = np.asarray(xg, np.float64).reshape(-1, 3)[:, 2]
    return np.minimum(z - 0.3, np.maximum(0.55 - z, z - 0.8))
