"""Numpy model of the solid-surface contact (host/surface_contact.c, csrc/k_surface_contact.hip), written from the rules in
include/dedflow.h "solid-surface contact", in np.longdouble.  The interpolation and the tet gradient are capture_model's, the
tangential law is friction_model's.  Tet and lambda come from the library (location is tested elsewhere) or, in the CPU
checks, from capture_model.brute_locate.  Shared by test_surface_contact_cpu.py and test_gpu_surface_contact.py."""
import numpy as np

import capture_model as cm
import friction_model as fm

EPS, LD = cm.EPS, cm.LD
KEY_SURFACE = (1 << 62) | (1 << 61)
LEVEL, T_SOLID = cm.LEVEL, cm.T_MELT
CLASSES = ("gas", "inside", "buried", "clear", "hot", "outside")


def gradient_condition(x4, f4):
    """per tet and component: the sum of the absolute terms of the closed form of g over |det|,
    sum_k |f_k - f_0| |c_k|_abs / |det| with |c_k|_abs the two products of every component of c_k at their absolute values"""
    x4, f4 = np.asarray(x4, LD), np.asarray(f4, LD)
    e = [np.abs(x4[:, k] - x4[:, 0]) for k in (1, 2, 3)]

    def cross_abs(a, b):
        return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)
    c_abs = [cross_abs(e[1], e[2]), cross_abs(e[2], e[0]), cross_abs(e[0], e[1])]
    x = [x4[:, k] - x4[:, 0] for k in (1, 2, 3)]
    det = (x[0] * cm._cross(x[1], x[2])).sum(axis=1)
    d = np.abs(f4[:, 1:] - f4[:, :1])
    return (d[:, 0:1] * c_abs[0] + d[:, 1:2] * c_abs[1] + d[:, 2:3] * c_abs[2]) / np.abs(det)[:, None]


def decide(xg, ien, w, tet, lam, radius, level, side, T_solid):
    """per particle: f, s, n, delta, |g|, T_f, the contact and buried masks and the condition term of g"""
    xg = np.asarray(xg, float).reshape(-1, 3)
    N = len(xg)
    ien4 = np.asarray(ien).reshape(-1, 4)
    tet = np.asarray(tet)
    dec = cm.decide(xg, ien, w, tet, lam, radius, level, side, 0.0, -np.inf)
    located = dec["located"]
    nodes = ien4[np.where(located, tet, 0)]
    phi = np.asarray(w, float)[4 * N:5 * N]
    g = cm.tet_gradient(xg[nodes], phi[nodes])
    gn = dec["gn"]
    r = np.broadcast_to(np.asarray(radius, LD), tet.shape)
    f = dec["phi_p"] - LD(level)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = -(LD(side) * f) / gn
        n = -(LD(side) * g) / gn[:, None]
        ok = located & (gn > 0) & (dec["T_f"] < T_solid)
        contact = ok & (s > -r) & (s < r)
        buried = ok & (s <= -r)
    return dict(f=f, s=s, n=n, delta=r - s, gn=gn, g=g, T_f=dec["T_f"], located=located, contact=contact, buried=buried, r=r,
                g_cond=gradient_condition(xg[nodes], phi[nodes]))


def forces(dec, vel, mass, kn, gamma_n, friction=None, omega=None, xi_old=None):
    """force [P][3], torque [P][3], the new springs (None without contact or friction) and f_n of every particle; friction =
    dict(mu, kt, gamma_t, dt); xi_old[i] = the surface spring of the previous sub-step or None"""
    P = len(dec["s"])
    vel = np.asarray(vel, LD).reshape(-1, 3)
    F, tau, xi, fn_all = np.zeros((P, 3), LD), np.zeros((P, 3), LD), [None] * P, np.zeros(P, LD)
    for i in np.nonzero(dec["contact"])[0]:
        n = dec["n"][i]
        vn = (vel[i, 0] * n[0] + vel[i, 1] * n[1]) + vel[i, 2] * n[2]
        fn = LD(kn) * dec["delta"][i] - LD(gamma_n) * vn
        fn_all[i] = fn
        F[i] = fn * n
        if friction is not None:
            ell = max(dec["r"][i] - dec["delta"][i], LD(0))
            Ft, t, x = fm.tangential(None if xi_old is None else xi_old[i], n, fn, ell, vel[i], np.asarray(omega, LD).reshape(-1, 3)[i],
                                     LD(friction["mu"]), LD(friction["kt"]), LD(friction["gamma_t"]), LD(friction["dt"]))
            F[i] = F[i] + Ft
            tau[i], xi[i] = t, x
    return F, tau, xi, fn_all


def accelerations(F, tau, mass, radius):
    """(F / m, tau / I) with I = 2/5 m r^2"""
    P = len(F)
    m = np.broadcast_to(np.asarray(mass, LD), (P,))
    r = np.broadcast_to(np.asarray(radius, LD), (P,))
    return F / m[:, None], tau / (LD(0.4) * m * r * r)[:, None]


def margins_ok(dec, T_solid):
    """no located particle has |s -+ r| < 1e-9, |s| < 1e-9 or |T_f - T_solid| < 1e-6: no rounding can flip a decision"""
    loc = dec["located"] & (dec["gn"] > 0)
    s, r = dec["s"][loc], dec["r"][loc]
    ok = bool(np.all(np.abs(s - r) >= 1e-9) and np.all(np.abs(s + r) >= 1e-9) and np.all(np.abs(s) >= 1e-9))
    if np.isfinite(T_solid):
        ok = ok and bool(np.all(np.abs(dec["T_f"][dec["located"]] - T_solid) >= 1e-6))
    return ok


def classify(dec, T_solid):
    """the class of every particle, an index into CLASSES"""
    c = np.full(len(dec["s"]), 3)
    with np.errstate(invalid="ignore"):
        c[dec["contact"] & (dec["s"] > 0)] = 0
        c[dec["contact"] & (dec["s"] < 0)] = 1
        c[dec["buried"]] = 2
        c[dec["located"] & ~(dec["T_f"] < T_solid)] = 4
    c[~dec["located"]] = 5
    return c


# ---- fields and cases ------------------------------------------------------------------------------------------------

PLANE_DIR = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
PLANE_G = 1.7                       # |grad phi| of the plane field: arbitrary, not 1
SPHERE_C, SPHERE_R = np.array([0.5, 0.5, 0.15]), 0.4


def plane_fields(xg, side):
    """w [6N] with phi = level + side G a . (x - 1/2) (the metal lies below the plane a . x = a . 1/2 for either side),
    T = 1000 + 1000 x and capture_model's velocity"""
    x = np.asarray(xg, float).reshape(-1, 3)
    N = len(x)
    w = cm.linear_fields(xg)
    w[4 * N:5 * N] = LEVEL - side * PLANE_G * ((x - 0.5) @ PLANE_DIR)
    return w


def sphere_fields(xg, side):
    """phi = the distance to a sphere sampled at the nodes (not linear in a tet): metal inside the sphere"""
    x = np.asarray(xg, float).reshape(-1, 3)
    N = len(x)
    w = cm.linear_fields(xg)
    w[4 * N:5 * N] = LEVEL - side * (np.linalg.norm(x - SPHERE_C, axis=1) - SPHERE_R)
    return w


def _particles(pts, rng, R):
    P = len(pts)
    r = rng.uniform(0.5 * R, R, P)
    rho_p = 7800.0
    vel = np.array([0.0, 0.0, -1.0]) + rng.uniform(-0.3, 0.3, (P, 3))
    return dict(pts=pts, vel=vel, omega=rng.normal(scale=20.0, size=(P, 3)), R=R, mass=rho_p * 4.0 / 3.0 * np.pi * R ** 3, r=r,
                m=rho_p * 4.0 / 3.0 * np.pi * r ** 3)


# signed gas-side distance of every class in particle radii (the three contact-like ranges are reused by the hot class)
_S_RANGE = {0: (0.1, 0.9), 1: (-0.9, -0.1), 2: (-3.0, -1.2), 3: (1.2, 6.0)}


def _targets(P, rng, poly_r):
    """class and target distance of every particle: the classes cycle; particle 5 (when there is one) lies outside the
    mesh, the other particles of that residue are gas-side contacts"""
    cls = np.arange(P) % 6
    geo = np.where(cls == 4, rng.integers(0, 3, P), np.where(cls == 5, 0, cls))
    lo = np.array([_S_RANGE[k][0] for k in geo])
    hi = np.array([_S_RANGE[k][1] for k in geo])
    return cls, rng.uniform(lo, hi) * poly_r


def plane_case(P, poly, R=0.02, seed=11):
    """P particles around the plane of plane_fields: a point of the plane inside the cube, moved by the class's distance
    along the gas normal; the hot class over x > 0.55 (T_f > T_SOLID), every other one over x < 0.42"""
    rng = np.random.default_rng(seed + P)
    case = _particles(np.zeros((P, 3)), rng, R)
    cls, s = _targets(P, rng, case["r"] if poly else np.full(P, R))
    x = np.where(cls == 4, rng.uniform(0.58, 0.85, P), rng.uniform(0.15, 0.42, P))
    y = rng.uniform(0.15, 0.85, P)
    z = 0.5 - (PLANE_DIR[0] * (x - 0.5) + PLANE_DIR[1] * (y - 0.5)) / PLANE_DIR[2]
    case["pts"] = np.stack([x, y, z], axis=1) + s[:, None] * PLANE_DIR
    if P > 5:
        case["pts"][5] = (1.2, 0.5, 0.3)
    return case


def sphere_case(P, poly, R=0.02, seed=23):
    """the same classes around the sphere of sphere_fields, placed by the true distance; the interpolated phi of a coarse
    mesh moves a particle by less than the gaps between the classes' ranges only roughly, so the tests classify with the
    model and assert that every class is present"""
    rng = np.random.default_rng(seed + P)
    case = _particles(np.zeros((P, 3)), rng, R)
    cls, s = _targets(P, rng, case["r"] if poly else np.full(P, R))
    th = rng.uniform(0.15, 0.55, P)                                    # polar angle from the sphere's top
    ph = np.where(cls == 4, rng.uniform(-0.5, 0.5, P), rng.uniform(np.pi - 0.6, np.pi + 0.6, P))   # hot: towards x > 1/2
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    case["pts"] = SPHERE_C + (SPHERE_R + s)[:, None] * d
    if P > 5:
        case["pts"][5] = (1.2, 0.5, 0.3)
    return case


def plane_wall_force(p, v, r, kn, gamma_n):
    """the closed-form plane-wall law through walls_model's face contact: one large triangle in the plane of plane_fields
    with the gas normal; returns the wall force on the particle"""
    import walls_model as wm
    a = np.array([0.5, 0.5, 0.5])
    e1 = np.cross(PLANE_DIR, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_DIR, e1)
    W = object.__new__(wm.Walls)
    W.v = np.array([[a - 50.0 * e1 - 50.0 * e2, a + 100.0 * e1, a + 100.0 * e2]])
    W.node = np.array([[0, 1, 2]])
    W.n = PLANE_DIR[None, :].copy()
    W.off = np.array([PLANE_DIR @ a])
    W.lo, W.hi = np.zeros(3), np.ones(3)
    W.tol = 1e-12 * np.sqrt(3.0)
    f, dropped, contacts = wm.wall_contacts(W, np.asarray(p, float), np.asarray(v, float), float(r), kn, gamma_n)
    assert dropped == 0
    return f, contacts
