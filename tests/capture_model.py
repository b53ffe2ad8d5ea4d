"""Numpy model of the melt-pool capture (host/capture.c, csrc/k_capture.hip), written from the rules in include/dedflow.h
"melt-pool capture": the decision, the deposits of a captured particle and the node accumulator, all in np.longdouble.
Tet and lambda come from the library (location is tested elsewhere), as heat_model.py takes them for convection.  Shared by
test_capture_cpu.py and test_gpu_capture.py."""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def tet_gradient(x4, f4):
    """g = sum_a f_a grad N_a of the tets with vertices x4 [n][4][3] and nodal values f4 [n][4], in closed form"""
    x4, f4 = np.asarray(x4, LD), np.asarray(f4, LD)
    e1, e2, e3 = x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0], x4[:, 3] - x4[:, 0]
    c23, c31, c12 = _cross(e2, e3), _cross(e3, e1), _cross(e1, e2)
    det = (e1 * c23).sum(axis=1)
    d = f4[:, 1:] - f4[:, :1]
    return (d[:, 0:1] * c23 + d[:, 1:2] * c31 + d[:, 2:3] * c12) / det[:, None]


def decide(xg, ien, w, tet, lam, radius, level, side, reach, T_melt):
    """per particle: c_i, T_f, phi_p, u_f, |g| and the captured mask (tet >= 0, c_i >= 0, T_f >= T_melt; NaN: not captured)"""
    xg = np.asarray(xg, float).reshape(-1, 3)
    N = len(xg)
    ien4 = np.asarray(ien).reshape(-1, 4)
    tet = np.asarray(tet)
    located = tet >= 0
    nodes = ien4[np.where(located, tet, 0)]
    lam = np.asarray(lam, LD)
    w = np.asarray(w, float)
    phi, T, u = w[4 * N:5 * N], w[5 * N:6 * N], w[:3 * N].reshape(-1, 3)
    phi_p = (lam * phi[nodes].astype(LD)).sum(axis=1)
    T_f = (lam * T[nodes].astype(LD)).sum(axis=1)
    u_f = np.einsum("na,nad->nd", lam, u[nodes].astype(LD))
    g = tet_gradient(xg[nodes], phi[nodes])
    gn = np.sqrt((g * g).sum(axis=1))
    r = np.broadcast_to(np.asarray(radius, LD), tet.shape)
    c = LD(side) * (phi_p - LD(level)) + (LD(reach) * r) * gn
    with np.errstate(invalid="ignore"):
        captured = located & (c >= 0) & (T_f >= T_melt)
    return dict(c=c, T_f=T_f, phi_p=phi_p, u_f=u_f, gn=gn, located=located, captured=captured)


def deposits(dec, mass, vel, rho_f, cp_p=None, temp=None):
    """[P][5] = (V, dP, E) of every particle (zero rows for the ones not captured); E = 0 with heat off (cp_p None)"""
    P = len(dec["c"])
    m = np.broadcast_to(np.asarray(mass, LD), (P,))
    out = np.zeros((P, 5), LD)
    out[:, 0] = m / LD(rho_f)
    out[:, 1:4] = m[:, None] * (np.asarray(vel, LD).reshape(-1, 3) - dec["u_f"])
    if cp_p is not None:
        out[:, 4] = (m * LD(cp_p)) * (np.asarray(temp, LD) - dec["T_f"])
    out[~dec["captured"]] = 0
    return out


def node_accumulate(num_node, ien, tet, lam, dep, captured):
    """A[N][5] = sum over the captured particles of lambda_a dep, with per node and component sum |terms|, and the number of
    terms per node"""
    ien4 = np.asarray(ien).reshape(-1, 4)
    k = np.nonzero(captured)[0]
    nodes = ien4[np.asarray(tet)[k]].reshape(-1)
    terms = (np.asarray(lam, LD)[k][:, :, None] * np.asarray(dep, LD)[k][:, None, :]).reshape(-1, 5)
    A = np.zeros((num_node, 5), LD)
    Aa = np.zeros((num_node, 5), LD)
    np.add.at(A, nodes, terms)
    np.add.at(Aa, nodes, np.abs(terms))
    return A, Aa, np.bincount(nodes, minlength=num_node)


def brute_locate(xg, ien, pts, eps=1e-12):
    """(tet, lambda) of every point by testing every tet, the lowest id winning; tet -1 and lambda 0 outside the mesh.  For
    the CPU checks, where no library locates: the margins asserted there are far above the difference in lambda"""
    xg = np.asarray(xg, float).reshape(-1, 3)
    x4 = xg[np.asarray(ien).reshape(-1, 4)]
    inv = np.linalg.inv(np.stack([x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0], x4[:, 3] - x4[:, 0]], axis=2))
    pts = np.asarray(pts, float).reshape(-1, 3)
    tet = np.full(len(pts), -1, np.int32)
    lam = np.zeros((len(pts), 4))
    for i, p in enumerate(pts):
        l123 = np.einsum("tij,tj->ti", inv, p[None, :] - x4[:, 0])
        l = np.concatenate([1.0 - l123.sum(axis=1, keepdims=True), l123], axis=1)
        ok = np.nonzero(l.min(axis=1) >= -eps)[0]
        if len(ok):
            tet[i], lam[i] = ok[0], l[ok[0]]
    return tet, lam


U_GRAD = np.array([[0.05, -0.02, 0.03], [0.01, 0.04, -0.05], [-0.03, 0.02, 0.06]])
U_0 = np.array([0.02, -0.01, 0.03])
LEVEL, T_MELT = 0.05, 1500.0


def linear_fields(xg):
    """w [6N] with phi = z - 0.5, T = 1000 + 1000 x and u = U_0 + U_GRAD x: P1 tets interpolate them exactly and |grad phi| = 1"""
    x = np.asarray(xg, float).reshape(-1, 3)
    N = len(x)
    w = np.zeros(6 * N)
    w[:3 * N] = (U_0 + x @ U_GRAD.T).reshape(-1)
    w[4 * N:5 * N] = x[:, 2] - 0.5
    w[5 * N:] = 1000.0 + 1000.0 * x[:, 0]
    return w


def decision_case(mesh, P=300, R=0.02, seed=5):
    """P particles for the decision tests on `mesh` (a kuhn_cube): particle 0 outside the mesh, particle 1 on a mesh node,
    particles 2-4 in one tet, the rest uniform in the cube; falling velocities well away from u_f, temperatures well above
    every T_f (the deposits then do not cancel), radii in [R/2, R] and their masses for the polydisperse runs"""
    rng = np.random.default_rng(seed)
    xg = mesh.xg.reshape(-1, 3)
    ien4 = mesh.ien.reshape(-1, 4)
    pts = rng.uniform(0.02, 0.98, (P, 3))
    if P > 5:
        M = mesh.M
        pts[0] = (1.2, 0.5, 0.3)
        pts[1] = xg[(M - 1) + (M + 1) * (1 + (M + 1) * 1)]          # node (M-1, 1, 1): hot, below the surface
        t = int(np.argmin(np.abs(xg[ien4].mean(axis=1) - np.array([0.8, 0.4, 0.3])).sum(axis=1)))
        for k, l in enumerate(([0.4, 0.3, 0.2, 0.1], [0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.3, 0.2])):
            pts[2 + k] = np.asarray(l) @ xg[ien4[t]]
    vel = np.array([0.0, 0.0, -1.0]) + rng.uniform(-0.1, 0.1, (P, 3))
    r = rng.uniform(0.5 * R, R, P)
    rho_p = 7800.0
    return dict(pts=pts, vel=vel, R=R, mass=rho_p * 4.0 / 3.0 * np.pi * R ** 3, r=r, m=rho_p * 4.0 / 3.0 * np.pi * r ** 3,
                temp=rng.uniform(4000.0, 5000.0, P), cp_p=500.0, rho_f=1.0e3)


def margins_ok(dec, T_melt):
    """the margins every decision test asserts in the model first: no |c_i| < 1e-9, no |T_f - T_melt| < 1e-6 among the located"""
    loc = dec["located"]
    ok = bool(np.all(np.abs(dec["c"][loc]) >= 1e-9))
    if np.isfinite(T_melt):
        ok = ok and bool(np.all(np.abs(dec["T_f"][loc] - T_melt) >= 1e-6))
    return ok
