"""numpy model of polydisperse DEM particles (include/dedflow.h, "polydisperse particles"): per-particle radius r_i and mass
m_i in the pair, unit-box and mesh-wall laws, with and without the tangential law, by brute force over the pairs.  Mesh-wall
contacts come from tests/walls_model.py and the tangential law of equal-radius pairs and walls from tests/friction_model.py;
a pair of unequal radii uses the levers of the overlap's middle.  Like friction_model, the history has no
DFL_DEM_MAX_HISTORY cap: compare states without overflow.  The inflow part (slot radii, blocking) follows the operation
order of the header exactly, so the device must match it bit for bit."""
import math

import numpy as np

import flow_model as flm
import friction_model as fm
import walls_model as wm


def default_mass(radius, R, M):
    """m_i = M ((q q) q), q = r_i / R: the reference particle's density (q = 1 gives M exactly)"""
    q = np.asarray(radius, dtype=np.float64) / R
    return M * ((q * q) * q)


def inertia(mass, radius):
    return 0.4 * mass * radius * radius


def tangential_lever(xi, n, fn, ell_i, lw, v, mu, kt, gt, dt):
    """friction_model.tangential with the contact-point velocity v - lw (lw = ell_i w_i x n + ell_j w_j x n) and the
    torque lever ell_i"""
    vrel = v - lw
    vt = vrel - (vrel @ n) * n
    if xi is None:
        xi = np.zeros(3)
    else:
        p = xi - (xi @ n) * n
        pp = p @ p
        xi = p * (np.sqrt(xi @ xi) / np.sqrt(pp)) if pp > 0.0 else np.zeros(3)
    xi = xi + vt * dt
    F = -kt * xi - gt * vt
    cap = mu * max(fn, 0.0)
    Fm = np.sqrt(F @ F)
    if Fm > cap:
        F = F * (cap / Fm)
        xi = -(F + gt * vt) / kt
    return F, np.cross(-ell_i * n, F), xi


class Model:
    """x, v, w: (P, 3); r, m: (P,); W: walls_model.Walls (None: the unit box); mu None: no friction.  rmax: the context's
    Rmax (the mesh walls' padded box)"""

    def __init__(self, x, v, r, m, kn=1.0e4, gn=1.0, mu=None, kt=None, gamma_t=None, dt=1.0e-4, gravity=(0, 0, 0), W=None,
                 w=None, rmax=None):
        self.x = np.array(x, float).reshape(-1, 3)
        self.v = np.array(v, float).reshape(-1, 3)
        self.w = np.zeros_like(self.x) if w is None else np.array(w, float).reshape(-1, 3)
        self.r = np.array(r, float).reshape(-1)
        self.m = np.array(m, float).reshape(-1)
        self.I = inertia(self.m, self.r)
        self.rmax = float(self.r.max()) if rmax is None else float(rmax)
        self.kn, self.gn, self.mu, self.dt = kn, gn, mu, dt
        self.kt = 2.0 / 7.0 * kn if kt is None else kt
        self.gt = gn if gamma_t is None else gamma_t
        self.g = np.asarray(gravity, float)
        self.W = W
        self.hist = [dict() for _ in range(len(self.x))]

    def _contact(self, h_old, h_new, key, n, fn, ell, v, w, f, tau):
        if self.mu is None:
            f += fn * n
            return
        F, t, xi = fm.tangential(h_old.get(key), n, fn, ell, v, w, self.mu, self.kt, self.gt, self.dt)
        h_new[key] = xi
        f += fn * n + F
        tau += t

    def _walls(self, i, h_old, h_new, f, tau):
        p, v, w, R = self.x[i], self.v[i], self.w[i], self.r[i]
        if self.W is None:
            for d in range(3):
                for side in range(2):
                    delta = R - p[d] if side == 0 else p[d] + R - 1.0
                    if not delta > 0.0:
                        continue
                    n = np.zeros(3)
                    n[d] = 1.0 if side == 0 else -1.0
                    fn = self.kn * delta - self.gn * (v @ n)
                    self._contact(h_old, h_new, fm.KEY_WALL | (2 * d + side), n, fn, max(R - delta, 0.0), v, w, f, tau)
            return
        _, _, contacts = wm.wall_contacts(self.W, p, v, R, self.kn, self.gn)
        for kind, k, delta, n in contacts:
            if kind == 0:
                key = fm.KEY_WALL | fm.plane_id(self.W, n, p @ n - (R - delta))
            elif kind == 1:
                key = fm.KEY_EDGE | (int(k[0]) << 31) | int(k[1])
            else:
                key = fm.KEY_VERTEX | int(k[0])
            fn = self.kn * delta - self.gn * (v @ n)
            self._contact(h_old, h_new, key, n, fn, max(R - delta, 0.0), v, w, f, tau)

    def forces(self, idx=None):
        """one contact sweep: (acc, alpha) of the particles idx (default all; the history advances only for a full sweep)"""
        from scipy.spatial import cKDTree
        x, v, w, r = self.x, self.v, self.w, self.r
        P = len(x)
        full = idx is None
        idx = np.arange(P) if full else np.asarray(idx)
        active = np.ones(P, bool) if self.W is None else wm.padded_inside(self.W, x, self.rmax)
        act = np.nonzero(active)[0]
        tree = cKDTree(x[act]) if act.size else None
        acc, alpha = np.zeros((len(idx), 3)), np.zeros((len(idx), 3))
        hist = [dict() for _ in range(P)]
        for row, i in enumerate(idx):
            if not active[i]:
                continue
            f, tau = np.zeros(3), np.zeros(3)
            for j in sorted(act[tree.query_ball_point(x[i], r[i] + self.rmax)]):
                if j == i:
                    continue
                d = x[i] - x[j]
                d2 = d @ d
                rs = r[i] + r[j]
                if d2 >= rs * rs or d2 == 0.0:
                    continue
                dist = np.sqrt(d2)
                n = d / dist
                dv = v[i] - v[j]
                fn = self.kn * (rs - dist) - self.gn * (dv @ n)
                key = fm.KEY_PARTNER | int(j)
                if r[i] == r[j] or self.mu is None:
                    self._contact(self.hist[i], hist[i], key, n, fn, 0.5 * dist, dv, w[i] + w[j], f, tau)
                    continue
                ell_i, ell_j = 0.5 * (dist + (r[i] - r[j])), 0.5 * (dist + (r[j] - r[i]))
                lw = ell_i * np.cross(w[i], n) + ell_j * np.cross(w[j], n)
                F, t, xi = tangential_lever(self.hist[i].get(key), n, fn, ell_i, lw, dv, self.mu, self.kt, self.gt, self.dt)
                hist[i][key] = xi
                f += fn * n + F
                tau += t
            self._walls(i, self.hist[i], hist[i], f, tau)
            acc[row] = f * (1.0 / self.m[i])
            alpha[row] = tau / self.I[i]
        if full:
            self.hist = hist
        return acc, alpha

    def step(self):
        """ParticleContextUpdate: sweep, then v += dt (a + g), x += dt v, w += dt alpha"""
        acc, alpha = self.forces()
        self.v = self.v + self.dt * (acc + self.g)
        self.x = self.x + self.dt * self.v
        self.w = self.w + self.dt * alpha
        return acc, alpha

    def momentum(self):
        return (self.m[:, None] * self.v).sum(axis=0)

    def angular_momentum(self):
        return (self.m[:, None] * np.cross(self.x, self.v)).sum(axis=0) + (self.I[:, None] * self.w).sum(axis=0)


# ---- inflow ---------------------------------------------------------------------------------------------------------
def slot_radius(seed, call, k, r_lo, r_hi):
    """r = r_lo + (r_hi - r_lo) u, u = (H(c, k, 3) >> 11) 2^-53"""
    u = float(flm.slot_hash(seed, call, k, 3) >> 11) * 2.0 ** -53
    return r_lo + (r_hi - r_lo) * u


def slot_radii(inlet, call, r_lo, r_hi):
    return np.array([slot_radius(inlet.seed, call, k, r_lo, r_hi) for k in range(inlet.nslot)])


def blocked(inlet, call, coord, radius, r_lo, r_hi):
    """slot flags: an existing centre y with dist^2 < (r_y + r_k)^2 (inlet built for r_hi)"""
    c = inlet.centres(call)
    y = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    if len(y) == 0 or inlet.nslot == 0:
        return np.zeros(inlet.nslot, bool)
    rk = slot_radii(inlet, call, r_lo, r_hi)
    dd = y[:, None, :] - c[None, :, :]
    d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
    rr = np.asarray(radius, dtype=np.float64)[:, None] + rk[None, :]
    return (d2 < rr * rr).any(axis=0)


class InflowModel(flm.InflowModel):
    """ParticleContextAdd of a polydisperse context: flow_model.InflowModel with slot radii, the (r_y + r_k) blocking test
    and the default masses of the reference particle (R, M)"""

    def __init__(self, inlet, per_call, max_particles, r_lo, r_hi, R, M, vel=(0.0, 0.0, 0.0)):
        super().__init__(inlet, per_call, max_particles, vel)
        self.r_lo, self.r_hi, self.R, self.M = float(r_lo), float(r_hi), float(R), float(M)

    def add_sized(self, coord, vel, tags, next_tag, radius, mass):
        call = self.call
        self.call += 1
        self.credit += self.per_call
        want = math.floor(self.credit)
        self.credit -= want
        P = len(coord)
        want = int(min(want, max(self.max_particles - P, 0)))
        if want <= 0:
            return coord, vel, tags, radius, mass, 0
        bl = blocked(self.inlet, call, coord, radius, self.r_lo, self.r_hi)
        free = self.inlet.ranked_free(call, bl) if self.inlet.nslot else []
        take = free[:want]
        n = len(take)
        self.blocked_total += want - n
        c = self.inlet.centres(call)[take] if n else np.empty((0, 3))
        rk = np.array([slot_radius(self.inlet.seed, call, k, self.r_lo, self.r_hi) for k in take])
        coord = np.concatenate([coord, c])
        vel = np.concatenate([vel, np.tile(self.vel, (n, 1))])
        tags = np.concatenate([tags, next_tag + np.arange(n, dtype=np.int64)])
        radius = np.concatenate([radius, rk])
        mass = np.concatenate([mass, default_mass(rk, self.R, self.M)])
        return coord, vel, tags, radius, mass, n


# ---- closed forms ---------------------------------------------------------------------------------------------------
def head_on(m1, m2, v1, v2, kn):
    """elastic head-on collision (gamma_n = 0): contact time pi sqrt(m_eff / kn) and the exit velocities"""
    meff = m1 * m2 / (m1 + m2)
    u1 = ((m1 - m2) * v1 + 2.0 * m2 * v2) / (m1 + m2)
    u2 = ((m2 - m1) * v2 + 2.0 * m1 * v1) / (m1 + m2)
    return math.pi * math.sqrt(meff / kn), u1, u2


def stack_overlaps(m1, m2, g, kn):
    """a small sphere (m2) resting on a big one (m1) on the floor: floor overlap (m1 + m2) g / kn, pair overlap m2 g / kn"""
    return (m1 + m2) * g / kn, m2 * g / kn
