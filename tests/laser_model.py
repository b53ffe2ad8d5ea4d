"""Model of the laser energy deposition (host/laser.c, csrc/k_laser.hip), written from the rules in include/dedflow.h
"laser energy deposition".  Geometry that DECIDES something (the column of a particle, the depth order, the frame) is
float64 with the operation order the header fixes, so that model and library bin alike; every sum and product that feeds
a compared value is np.longdouble, sequential in the defined order; the column weights use math.erf.
Shared by test_laser_cpu.py and test_gpu_laser.py."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble
ULP_EXP = 3.0     # allowance for the device exp and expm1 in ulp: see test_gpu_laser.py


def dot3(a, d):
    """(d0 a0 + d1 a1) + d2 a2 in float64, no fused multiply-add; d (..., 3)"""
    d = np.asarray(d, np.float64)
    return (d[..., 0] * a[0] + d[..., 1] * a[1]) + d[..., 2] * a[2]


class Beam:
    def __init__(self, origin, direction, power, w, h, r_cut, eta_p=1.0, eta_s=1.0, scan_vel=(0.0, 0.0, 0.0)):
        d = np.asarray(direction, np.float64)
        self.dir = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        k = int(np.argmin(np.abs(self.dir)))            # the first smallest
        t = np.where(np.arange(3) == k, 1.0, 0.0) - self.dir[k] * self.dir
        self.e1 = t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        dd, e = self.dir, self.e1
        self.e2 = np.array([dd[1] * e[2] - dd[2] * e[1], dd[2] * e[0] - dd[0] * e[2], dd[0] * e[1] - dd[1] * e[0]])
        self.origin, self.scan_vel = np.asarray(origin, np.float64), np.asarray(scan_vel, np.float64)
        self.power, self.w, self.h, self.r_cut, self.eta_p, self.eta_s = map(float, (power, w, h, r_cut, eta_p, eta_s))
        self.n = 2 * int(math.ceil(self.r_cut / self.h))
        self.ncol = self.n * self.n
        x = [float(i - self.n // 2) * self.h for i in range(self.n + 1)]
        E = [math.erf((math.sqrt(2.0) * xi) / self.w) for xi in x]
        self.g = np.array([E[i + 1] - E[i] for i in range(self.n)], np.float64)
        self.r_edge = self.n * self.h / 2.0

    def at(self, t):
        return self.origin + self.scan_vel * float(t)

    def column_power(self):
        """P_c [ncol] in float64, the library's expression ((P / 4) gx[i]) gy[j], column id i + n j"""
        return (((self.power / 4.0) * self.g)[None, :] * self.g[:, None]).reshape(-1)

    def project(self, x, o):
        d = np.asarray(x, np.float64).reshape(-1, 3) - o
        return dot3(self.e1, d), dot3(self.e2, d), dot3(self.dir, d)

    def columns(self, x, o):
        """column id of every particle (ncol: outside the grid) and its depth"""
        u, v, s = self.project(x, o)
        qu, qv, half = np.floor(u / self.h), np.floor(v / self.h), self.n // 2
        inside = (qu >= -half) & (qu < half) & (qv >= -half) & (qv < half)
        col = np.where(inside, (qu + half) + self.n * (qv + half), self.ncol).astype(np.int64)
        return col, s

    def centres(self):
        c = (np.arange(self.n) - self.n // 2 + 0.5) * self.h
        return np.tile(c, self.n), np.repeat(c, self.n)           # cu, cv by column id


class Substrate:
    """candidate faces: the wall records (tests/walls_model.Walls) of `groups` with n . dir < 0, ascending record id"""

    def __init__(self, m, groups, beam):
        import walls_model as wm
        W = wm.Walls(m, groups)
        sel = np.nonzero(dot3(beam.dir, W.n) < 0.0)[0]
        self.id, self.v, self.node = sel, W.v[sel], W.node[sel]


def hits(sub, beam, o):
    """per column: local candidate face (-1: none), barycentric weights, depth, and kappa = the conditioning of the
    weights, sum(|a_i b_j| + |a_j b_i|) / |sum of the edge functions|; also the distance (in the beam's plane) of every
    column centre to the nearest projected candidate edge"""
    cu, cv = beam.centres()
    nc = beam.ncol
    face, wts = np.full(nc, -1, np.int64), np.zeros((nc, 3), LD)
    depth, kappa, edge_dist = np.full(nc, np.inf, LD), np.zeros(nc), np.full(nc, np.inf)
    if sub is None or len(sub.id) == 0:
        return face, wts, depth, kappa, edge_dist
    u, v, s = (a.reshape(-1, 3) for a in beam.project(sub.v.reshape(-1, 3), o))
    for f in range(len(sub.id)):                                  # ascending id: a tie keeps the earlier face
        lo_u, hi_u, lo_v, hi_v = u[f].min(), u[f].max(), v[f].min(), v[f].max()
        pad = beam.h
        near = np.nonzero((cu >= lo_u - pad) & (cu <= hi_u + pad) & (cv >= lo_v - pad) & (cv <= hi_v + pad))[0]
        if near.size == 0:
            continue
        a = u[f].astype(LD)[None, :] - cu[near].astype(LD)[:, None]
        b = v[f].astype(LD)[None, :] - cv[near].astype(LD)[:, None]
        w0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        w1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        w2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        tot = (w0 + w1) + w2
        for k in range(3):                                        # distance to the three edge lines (segments: clamp)
            p0 = np.array([u[f][k], v[f][k]])
            p1 = np.array([u[f][(k + 1) % 3], v[f][(k + 1) % 3]])
            e = p1 - p0
            q = np.stack([cu[near], cv[near]], axis=1) - p0
            t = np.clip((q @ e) / (e @ e), 0.0, 1.0)
            dist = np.linalg.norm(q - t[:, None] * e[None, :], axis=1)
            edge_dist[near] = np.minimum(edge_dist[near], dist)
        inside = (tot != 0) & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
        for r in np.nonzero(inside)[0]:
            c = near[r]
            ww = np.array([w0[r], w1[r], w2[r]], LD) / tot[r]
            d = (ww[0] * LD(s[f][0]) + ww[1] * LD(s[f][1])) + ww[2] * LD(s[f][2])
            if d < depth[c]:
                face[c], wts[c], depth[c] = f, ww, d
                mag = (abs(a[r, 1] * b[r, 2]) + abs(a[r, 2] * b[r, 1]) + abs(a[r, 2] * b[r, 0]) + abs(a[r, 0] * b[r, 2]) +
                       abs(a[r, 0] * b[r, 1]) + abs(a[r, 1] * b[r, 0]))
                kappa[c] = float(mag / abs(tot[r]))
    return face, wts, depth, kappa, edge_dist


def step(beam, x, r, t=0.0, sub=None):
    """one laser step with the axis at origin + scan_vel t.  Returns a dict: rate [P] (longdouble), rate_bound [P] (the
    a-priori bound of test_gpu_laser.py), col (column of every particle), T [ncol], face (record id, -1), tally (six
    longdoubles), q {node: W}, q_bound {node: W}, hit (the tuple of hits())"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    P = len(x)
    r = np.broadcast_to(np.asarray(r, np.float64), (P,))
    o = beam.at(t)
    col, s = beam.columns(x, o)
    hit = hits(sub, beam, o)
    face, wts, depth, kappa, _ = hit
    pc = beam.column_power()
    a = beam.h * beam.h
    rate, bound, bound1 = np.zeros(P, LD), np.zeros(P), np.zeros(P)
    T, T_rel = pc.astype(LD).copy(), np.full(beam.ncol, 4 * EPS)
    absorbed, scattered = LD(0), LD(0)
    order = np.lexsort((np.arange(P), s, col))
    starts = np.searchsorted(col[order], np.arange(beam.ncol + 1))
    for c in range(beam.ncol):
        run = order[starts[c]:starts[c + 1]]
        if run.size == 0:
            continue
        S = LD(0)
        for k, i in enumerate(run):                               # ascending (s, id)
            tau = LD(0) if (face[c] >= 0 and LD(s[i]) > depth[c]) else (LD(np.pi) * (LD(r[i]) * LD(r[i]))) / LD(a)
            p_in = LD(pc[c]) * np.exp(-S)
            got = p_in * (-np.expm1(-tau))
            rate[i] = LD(beam.eta_p) * got
            # (n_before + c) eps S on the optical depth, times the conditioning of exp (1: absolute error of the argument).
            # c = 12: every term pi r^2 / a carries 4 roundings, the scan's tree adds at most 6 levels per 64 entries and one
            # carry per chunk (n_before / 64 <= n_before), against the model's exact sequential sum.  Plus the ulp allowance
            # of exp and expm1, the 4 roundings of the particle's own A / a through expm1 (condition <= 1) and 8 products
            bound[i] = float(rate[i]) * ((k + 12) * EPS * float(S) + (2 * ULP_EXP + 12) * EPS)
            bound1[i] = float(rate[i]) * ((k + 12) * EPS * float(S) + (2 * 1.0 + 12) * EPS)   # the same at 1 ulp (logged only)
            absorbed += rate[i]
            scattered += got - rate[i]
            S += tau
        T[c] = LD(pc[c]) * np.exp(-S)
        T_rel[c] = (run.size + 12) * EPS * float(S) + (ULP_EXP + 4) * EPS
    has = face >= 0
    sub_c = np.where(has, LD(beam.eta_s) * T, LD(0))
    tally = dict(outside=LD(beam.power) - pc.astype(LD).sum(), absorbed_particles=absorbed, scattered=scattered,
                 substrate=sub_c.sum(), reflected=np.where(has, (LD(1) - LD(beam.eta_s)) * T, LD(0)).sum(),
                 missed=np.where(has, LD(0), T).sum())
    q, qb, qn = {}, {}, {}
    for c in np.nonzero(has)[0]:                                  # ascending column; a node's faces interleave, the bound covers it
        for k in range(3):
            nd = int(sub.node[face[c], k])
            term = sub_c[c] * wts[c, k]
            q[nd] = q.get(nd, LD(0)) + term
            qn[nd] = qn.get(nd, 0) + 1
            qb[nd] = qb.get(nd, 0.0) + float(sub_c[c]) * (8 * EPS * kappa[c] + abs(float(wts[c, k])) * (T_rel[c] + 4 * EPS))
    for nd in q:
        qb[nd] += (qn[nd] + 4) * EPS * float(abs(q[nd]))   # the sum itself, every term positive
    fid = np.where(has, sub.id[np.maximum(face, 0)] if sub is not None and len(sub.id) else -1, -1)
    return dict(rate=rate, rate_bound=bound, rate_bound_1ulp=bound1, col=col, s=s, T=T, T_rel=T_rel, face=fid, tally=tally, q=q, q_bound=qb, hit=hit)


def tally_sum(t):
    return sum(LD(t[k]) for k in ("outside", "absorbed_particles", "scattered", "substrate", "reflected", "missed"))
