"""Numpy model of the particle-fluid coupling (host/couple.c, csrc/k_couple.hip), written from the rules in
include/dedflow.h "particle-fluid coupling": brute-force point location, barycentric coordinates, the implicit
Schiller-Naumann drag update and the node scatter of the reaction load.  Shared by test_coupling_cpu.py and
test_gpu_coupling.py."""
import numpy as np

LAMBDA_EPS = 1e-12
RHO_F, MU_F = 1.0e3, 10.0 / 3.0


def barycentric(xg, ien, tets, pts):
    """lambda[n][4] of the points pts[n] in the tets tets[n] (the kernel's formula: scaled triple products)"""
    x = np.asarray(xg).reshape(-1, 3)[np.asarray(ien).reshape(-1, 4)[tets]]   # [n][4][3]
    p = np.asarray(pts).reshape(-1, 3)
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    r = p - x[:, 0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    inv = 1.0 / np.einsum("ij,ij->i", e1, c23)
    lam = np.empty((len(p), 4))
    lam[:, 1] = np.einsum("ij,ij->i", r, c23) * inv
    lam[:, 2] = np.einsum("ij,ij->i", r, c31) * inv
    lam[:, 3] = np.einsum("ij,ij->i", r, c12) * inv
    lam[:, 0] = 1.0 - lam[:, 1] - lam[:, 2] - lam[:, 3]
    return lam


def contains(xg, ien, tets, pts):
    """the model's containment test: min lambda >= -1e-12 (False for tet < 0)"""
    tets = np.asarray(tets)
    ok = tets >= 0
    out = np.zeros(len(tets), bool)
    if ok.any():
        out[ok] = barycentric(xg, ien, tets[ok], np.asarray(pts).reshape(-1, 3)[ok]).min(axis=1) >= -LAMBDA_EPS
    return out


def locate_brute(xg, ien, pts, chunk=256):
    """lowest-id tet containing each point (every tet tested), -1 when none does"""
    p = np.asarray(pts).reshape(-1, 3)
    T = np.asarray(ien).size // 4
    out = np.full(len(p), -1, np.int64)
    all_t = np.arange(T)
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk]
        tt = np.repeat(all_t[None, :], len(q), axis=0).reshape(-1)
        pp = np.repeat(q, T, axis=0)
        inside = (barycentric(xg, ien, tt, pp).min(axis=1) >= -LAMBDA_EPS).reshape(len(q), T)
        has = inside.any(axis=1)
        out[s:s + chunk] = np.where(has, inside.argmax(axis=1), -1)
    return out


def interpolate(w, ien, tets, lam):
    """u_f[n] = sum_a lambda_a u(node_a); u = the first 3N entries of the state"""
    N3 = np.asarray(ien).reshape(-1, 4)[tets]
    u = np.asarray(w)[: 3 * (np.asarray(w).size // 6)].reshape(-1, 3)
    return np.einsum("na,nad->nd", lam, u[N3])


def schiller_naumann(re):
    re = np.asarray(re, dtype=float)
    return np.where(re <= 1000.0, 1.0 + 0.15 * re ** 0.687, 0.44 * re / 24.0)


def particle_density(mass, radius):
    return mass / (4.0 / 3.0 * np.pi * radius ** 3)


def response_time(mass, radius, mu_f=MU_F):
    return particle_density(mass, radius) * (2.0 * radius) ** 2 / (18.0 * mu_f)


def drag_step(x, v, a_contact, uf, inside, mass, radius, dt, rho_f=RHO_F, mu_f=MU_F, gravity=(0.0, 0.0, 0.0)):
    """one fluid sub-step of every particle: returns (x', v', acc, impulse) with acc = (v' - v)/dt and impulse the drag
    impulse m f (u_f - v') / tau dt (zero outside); outside the fluid (inside False) gravity only"""
    x, v, a, uf = (np.asarray(q, float).reshape(-1, 3) for q in (x, v, a_contact, uf))
    g = np.asarray(gravity, float)[None, :]
    inside = np.asarray(inside, bool)
    rho_p = particle_density(mass, radius)
    d = 2.0 * radius
    re = rho_f * np.linalg.norm(uf - v, axis=1) * d / mu_f
    k = (schiller_naumann(re) / response_time(mass, radius, mu_f))[:, None]
    vin = (v + dt * (a + (1.0 - rho_f / rho_p) * g + k * uf)) / (1.0 + dt * k)
    vout = v + dt * (a + g)
    vn = np.where(inside[:, None], vin, vout)
    imp = np.where(inside[:, None], mass * k * (uf - vn) * dt, 0.0)
    return x + dt * vn, vn, (vn - v) / dt, imp


def node_scatter(num_node, ien, tets, lam, imp, elapsed):
    """load[a] = -sum_p lambda_{a,p} imp_p / elapsed over the located particles (tet >= 0)"""
    ien4 = np.asarray(ien).reshape(-1, 4)
    tets = np.asarray(tets)
    ok = tets >= 0
    load = np.zeros((num_node, 3))
    nodes = ien4[tets[ok]]                               # [n][4]
    contrib = lam[ok][:, :, None] * np.asarray(imp).reshape(-1, 3)[ok][:, None, :]
    np.add.at(load, nodes.reshape(-1), contrib.reshape(-1, 3))
    return (-load / elapsed).reshape(-1)


def terminal_velocity(mass, radius, gravity, rho_f=RHO_F, mu_f=MU_F, iters=200):
    """settling fixed point v_t = (1 - rho_f/rho_p) g tau / f(Re_t), Re_t = rho_f |v_t| d / mu_f (fixed-point iteration)"""
    g = np.asarray(gravity, float)
    rho_p = particle_density(mass, radius)
    tau = response_time(mass, radius, mu_f)
    v0 = (1.0 - rho_f / rho_p) * g * tau
    vt = v0.copy()
    for _ in range(iters):
        re = rho_f * np.linalg.norm(vt) * 2.0 * radius / mu_f
        vt = v0 / schiller_naumann(re)
    return vt
