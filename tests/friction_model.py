"""numpy model of the DEM contact friction and rotation (include/dedflow.h, "contact friction and particle rotation"): a
brute-force loop over the contacts of every particle with the Cundall-Strack tangential law, the contact history held in a
dict per particle keyed like the library's 64-bit keys, and the semi-implicit Euler step with rotation.  Mesh-wall contacts
come from tests/walls_model.py.  The model keeps every contact's history: it has no DFL_DEM_MAX_HISTORY cap (the device
fills the entries in its cell-sorted visit order, which the model does not reproduce), so compare states without overflow."""
import numpy as np

import walls_model as wm

KEY_PARTNER, KEY_WALL, KEY_EDGE, KEY_VERTEX = 0, 1 << 62, 2 << 62, 3 << 62


def tangential(xi, n, fn, ell, v, w, mu, kt, gt, dt):
    """one contact: xi = the spring of the previous sweep (None: new contact); v, w = the velocity and angular velocity
    relative to the partner (pair: v_i - v_j, w_i + w_j).  Returns (F_t, torque, new xi)"""
    vrel = v - ell * np.cross(w, n)
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
    return F, np.cross(-ell * n, F), xi


def plane_id(W, n, off):
    """the smallest triangle id whose plane equals (n, off) under de-duplication rule 1"""
    m = np.all(np.abs(W.n - n) <= 1e-12, axis=1) & (np.abs(W.off - off) <= W.tol)
    return int(np.nonzero(m)[0].min())


class Model:
    """x, v, w: (P, 3); W: walls_model.Walls (None: the unit box); kt None = 2/7 kn, gamma_t None = gamma_n"""

    def __init__(self, x, v, R, mass=1.0, kn=1.0e4, gn=1.0, mu=0.5, kt=None, gamma_t=None, dt=1.0e-4, gravity=(0, 0, 0),
                 W=None, w=None):
        self.x = np.array(x, float).reshape(-1, 3)
        self.v = np.array(v, float).reshape(-1, 3)
        self.w = np.zeros_like(self.x) if w is None else np.array(w, float).reshape(-1, 3)
        self.R, self.mass, self.kn, self.gn, self.mu, self.dt = R, mass, kn, gn, mu, dt
        self.kt = 2.0 / 7.0 * kn if kt is None else kt
        self.gt = gn if gamma_t is None else gamma_t
        self.I = 0.4 * mass * R * R
        self.g = np.asarray(gravity, float)
        self.W = W
        self.hist = [dict() for _ in range(len(self.x))]
        self._planes = {}

    def _contact(self, h_old, h_new, key, n, fn, ell, v, w, f, tau):
        F, t, xi = tangential(h_old.get(key), n, fn, ell, v, w, self.mu, self.kt, self.gt, self.dt)
        h_new[key] = xi
        f += fn * n + F
        tau += t

    def _walls(self, i, h_old, h_new, f, tau):
        p, v, w, R = self.x[i], self.v[i], self.w[i], self.R
        if self.W is None:
            for d in range(3):
                for side in range(2):
                    delta = R - p[d] if side == 0 else p[d] + R - 1.0
                    if not delta > 0.0:
                        continue
                    n = np.zeros(3)
                    n[d] = 1.0 if side == 0 else -1.0
                    fn = self.kn * delta - self.gn * (v @ n)
                    self._contact(h_old, h_new, KEY_WALL | (2 * d + side), n, fn, max(R - delta, 0.0), v, w, f, tau)
            return 0
        _, dropped, contacts = wm.wall_contacts(self.W, p, v, R, self.kn, self.gn)
        for kind, k, delta, n in contacts:
            if kind == 0:
                off = p @ n - (R - delta)
                key = KEY_WALL | plane_id(self.W, n, off)
            elif kind == 1:
                key = KEY_EDGE | (int(k[0]) << 31) | int(k[1])
            else:
                key = KEY_VERTEX | int(k[0])
            fn = self.kn * delta - self.gn * (v @ n)
            self._contact(h_old, h_new, key, n, fn, max(R - delta, 0.0), v, w, f, tau)
        return dropped

    def forces(self):
        """one contact sweep: (acc, alpha); advances the history"""
        from scipy.spatial import cKDTree
        x, v, w, R = self.x, self.v, self.w, self.R
        P = len(x)
        active = np.ones(P, bool) if self.W is None else wm.padded_inside(self.W, x, R)
        act = np.nonzero(active)[0]
        tree = cKDTree(x[act]) if act.size else None
        acc, alpha = np.zeros((P, 3)), np.zeros((P, 3))
        hist = [dict() for _ in range(P)]
        for i in act:
            f, tau = np.zeros(3), np.zeros(3)
            for j in sorted(act[tree.query_ball_point(x[i], 2 * R)]):
                if j == i:
                    continue
                r = x[i] - x[j]
                d2 = r @ r
                if d2 >= 4 * R * R or d2 == 0.0:
                    continue
                dist = np.sqrt(d2)
                n = r / dist
                dv = v[i] - v[j]
                fn = self.kn * (2 * R - dist) - self.gn * (dv @ n)
                self._contact(self.hist[i], hist[i], KEY_PARTNER | int(j), n, fn, 0.5 * dist, dv, w[i] + w[j], f, tau)
            self._walls(i, self.hist[i], hist[i], f, tau)
            acc[i] = f / self.mass
            alpha[i] = tau / self.I
        self.hist = hist
        return acc, alpha

    def step(self):
        """ParticleContextUpdate: sweep, then v += dt (a + g), x += dt v, w += dt alpha"""
        acc, alpha = self.forces()
        self.v = self.v + self.dt * (acc + self.g)
        self.x = self.x + self.dt * self.v
        self.w = self.w + self.dt * alpha
        return acc, alpha

    def angular_momentum(self):
        return (self.mass * np.cross(self.x, self.v)).sum(axis=0) + self.I * self.w.sum(axis=0)
