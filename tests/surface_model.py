"""numpy model of the free-surface forces (include/dedflow.h, "free-surface forces"): the text of that section, tet by tet in
np.longdouble, node sums in ascending tet order.  Test infrastructure only; shared by test_surface_cpu.py (which checks the
model against closed forms) and test_gpu_surface.py (which checks the kernel against the model)."""
import numpy as np

LD = np.longdouble
SHA, SHB, GW = LD("0.5854101966249685"), LD("0.1381966011250105"), LD("0.0416666666666667")
KSB = LD("5.670374419e-8")
SHL = np.where(np.eye(4, dtype=bool), SHA, SHB)          # SHL[a, q]

DEFAULTS = dict(level=0.0, side=1, eps=None, sigma0=0.0, dsigma_dT=0.0, T_ref=0.0, recoil_p0=0.0, recoil_a=0.0, T_boil=0.0,
                h_conv=0.0, emissivity=0.0, T_amb=0.0, evap_q0=0.0, in_time_step=False)
REAL = [k for k in DEFAULTS if k not in ("side", "in_time_step")]


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def refusal(cfg):
    """why DflMeshSetSurfaceForces refuses the configuration, or None"""
    if cfg["side"] not in (1, -1):
        return "side"
    for k in REAL:
        if not np.isfinite(cfg[k]):
            return k
    if not cfg["eps"] > 0.0:
        return "eps"
    if (cfg["recoil_p0"] > 0.0 or cfg["evap_q0"] > 0.0) and not cfg["T_boil"] > 0.0:
        return "T_boil"
    return None


def loss(cfg, T):
    """loss_q of the header at temperature T (W / m^2)"""
    T = np.asarray(T, LD)
    c = {k: LD(cfg[k]) for k in REAL}
    out = np.zeros_like(T)
    if cfg["h_conv"] > 0.0:
        out = out + c["h_conv"] * (T - c["T_amb"])
    if cfg["emissivity"] > 0.0:
        out = out + c["emissivity"] * KSB * (T ** 4 - c["T_amb"] ** 4)
    if cfg["evap_q0"] > 0.0:
        out = out + c["evap_q0"] * np.exp(c["recoil_a"] * (1 - c["T_boil"] / T)) * np.sqrt(c["T_boil"] / T)
    return out


def recoil(cfg, T):
    T = np.asarray(T, LD)
    if not cfg["recoil_p0"] > 0.0:
        return np.zeros_like(T)
    return LD(cfg["recoil_p0"]) * np.exp(LD(cfg["recoil_a"]) * (1 - LD(cfg["T_boil"]) / T))


def tet_terms(xg, ien, w, cfg):
    """per tet inside the band: ids e [K] (ascending) and f [K, 4, 3], heat [K, 4], area [K, 4], S [K] in longdouble"""
    assert refusal(cfg) is None
    N = xg.size // 3
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, LD).reshape(-1, 3)[ien]                      # [T, 4, 3]
    w = np.asarray(w, np.float64)
    phi = w[4 * N:5 * N].astype(LD)[ien]
    Tn = w[5 * N:6 * N].astype(LD)[ien]
    c = {k: LD(cfg[k]) for k in REAL}
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = (e1 * c23).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gN = np.stack([-((c23 + c31) + c12), c23, c31, c12], axis=1) / det[:, None, None]   # [T, 4, 3]
        g = ((phi[:, 1] - phi[:, 0])[:, None] * c23 + (phi[:, 2] - phi[:, 0])[:, None] * c31
             + (phi[:, 3] - phi[:, 0])[:, None] * c12) / det[:, None]
        gn = np.sqrt((g * g).sum(axis=1))
        ok = gn > 0
        d = (phi - c["level"]) / gn[:, None]
    eps = c["eps"]
    ok &= ~((d >= eps).all(axis=1) | (d <= -eps).all(axis=1))
    e = np.flatnonzero(ok)
    gN, g, gn, d, det, Tn = gN[e], g[e], gn[e], d[e], det[e], Tn[e]
    n = g / gn[:, None]
    dq, Tq = d @ SHL, Tn @ SHL                                        # [K, 4 (q)]
    t = dq / eps
    delta = np.where(np.abs(t) < 1, LD(15) / (16 * eps) * (1 - t * t) ** 2, LD(0))
    W = GW * np.abs(det)[:, None] * delta
    sigma = np.maximum(LD(0), c["sigma0"] + c["dsigma_dT"] * (Tq - c["T_ref"]))
    hot = Tq > 0
    Tsafe = np.where(hot, Tq, LD(1))
    E = np.where(hot, np.exp(c["recoil_a"] * (1 - c["T_boil"] / Tsafe)), LD(0))
    pq = c["recoil_p0"] * E if cfg["recoil_p0"] > 0.0 else np.zeros_like(E)
    lq = np.zeros_like(E)
    if cfg["h_conv"] > 0.0:
        lq = lq + c["h_conv"] * (Tq - c["T_amb"])
    if cfg["emissivity"] > 0.0:
        lq = lq + c["emissivity"] * KSB * (Tq ** 4 - c["T_amb"] ** 4)
    if cfg["evap_q0"] > 0.0:
        lq = lq + np.where(hot, c["evap_q0"] * E * np.sqrt(c["T_boil"] / Tsafe), LD(0))
    S = (W * sigma).sum(axis=1)
    ndg = (gN * n[:, None, :]).sum(axis=2)                            # [K, 4]
    P = (W * pq) @ SHL.T                                              # [K, 4 (a)]: sum_q W p shl(a, q)
    f = -S[:, None, None] * (gN - n[:, None, :] * ndg[:, :, None]) + LD(cfg["side"]) * n[:, None, :] * P[:, :, None]
    heat = -((W * lq) @ SHL.T)
    area = W @ SHL.T
    return dict(e=e, f=f, heat=heat, area=area, S=S)


def node_sums(N, ien, terms):
    """(load [N, 3], q_heat [N], area [N], active [N] = the node has a tet inside the band): every node adds its tets in
    ascending tet id (np.add.at adds in index order, and the tets come ascending)"""
    nodes = np.asarray(ien).reshape(-1, 4)[terms["e"]].reshape(-1)
    load, heat, area = np.zeros((N, 3), LD), np.zeros(N, LD), np.zeros(N, LD)
    np.add.at(load, nodes, terms["f"].reshape(-1, 3))
    np.add.at(heat, nodes, terms["heat"].reshape(-1))
    np.add.at(area, nodes, terms["area"].reshape(-1))
    active = np.zeros(N, bool)
    active[nodes] = True
    return load, heat, area, active


def surface_load(xg, ien, w, cfg):
    N = xg.size // 3
    t = tet_terms(xg, ien, w, cfg)
    return node_sums(N, ien, t) + (t,)


def state(N, phi, T):
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = phi
    w[5 * N:] = T
    return w
