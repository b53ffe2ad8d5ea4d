"""numpy model of the phase change (include/dedflow.h, "phase change"): the text of that section, tet by tet in
np.longdouble, node sums in ascending tet order, the two row updates and the statistics.  Written from the header, not from
the kernel.  Test infrastructure only; shared by test_phase_cpu.py (which checks the model against closed forms) and
test_gpu_phase.py (which checks the kernels against the model)."""
import numpy as np

LD = np.longdouble
SHA, SHB, GW = LD("0.5854101966249685"), LD("0.1381966011250105"), LD("0.0416666666666667")
SHL = np.where(np.eye(4, dtype=bool), SHA, SHB)          # SHL[a, q]
kRHOC, kDT = 0.5, 5e-2
kALPHAM = (3.0 - kRHOC) / (1.0 + kRHOC)
kALPHAF = 1.0 / (1.0 + kRHOC)
kGAMMA = 0.5 + kALPHAM - kALPHAF
FACT2 = kDT * kALPHAF * kGAMMA

DEFAULTS = dict(T_solidus=None, T_liquidus=None, latent=0.0, darcy_c=0.0, darcy_b=1e-3, use_phi=False, level=0.0, side=1,
                eps=1.0)
REAL = ["T_solidus", "T_liquidus", "latent", "darcy_c", "darcy_b", "level", "eps"]


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def refusal(cfg):
    """why DflMeshSetPhaseChange refuses the configuration, or None"""
    for k in REAL:
        if not np.isfinite(cfg[k]):
            return k
    if not cfg["T_liquidus"] > cfg["T_solidus"]:
        return "T_liquidus"
    if cfg["darcy_c"] > 0.0 and not cfg["darcy_b"] > 0.0:
        return "darcy_b"
    if cfg["use_phi"] and cfg["side"] not in (1, -1):
        return "side"
    if cfg["use_phi"] and not cfg["eps"] > 0.0:
        return "eps"
    return None


def liquid_fraction(cfg, T):
    """(fl, fl', C) at the temperatures T; a NaN gives 0, 0, 0"""
    T = np.asarray(T, LD)
    Ts, Tl = LD(cfg["T_solidus"]), LD(cfg["T_liquidus"])
    nan = np.isnan(T)
    with np.errstate(invalid="ignore"):
        s = np.where(nan, LD(0), np.minimum(LD(1), np.maximum(LD(0), (np.where(nan, Ts, T) - Ts) / (Tl - Ts))))
    fl = s * s * (3 - 2 * s)
    dfl = 6 * s * (1 - s) / (Tl - Ts)
    C = np.zeros_like(fl)
    if cfg["darcy_c"] > 0.0:
        C = np.where(nan, LD(0), LD(cfg["darcy_c"]) * (1 - fl) ** 2 / (fl ** 3 + LD(cfg["darcy_b"])))
    return fl, dfl, C


def smooth_step(t):
    """Hs: 0 for t <= -1, 1 for t >= 1, the integral of the biweight kernel between; a NaN gives 0"""
    t = np.asarray(t, LD)
    with np.errstate(invalid="ignore"):
        tc = np.where(np.isnan(t), LD(-1), np.clip(t, -1, 1))
    inner = LD("0.5") + LD(15) / 16 * (tc - LD(2) / 3 * tc ** 3 + LD(1) / 5 * tc ** 5)
    return np.where(tc <= -1, LD(0), np.where(tc >= 1, LD(1), inner))


def tet_terms(xg, ien, w, cfg):
    """per tet D, H, G [T, 4] in longdouble and the two skip decisions coeff [T] (adds to D / H), vol [T] (adds to G)"""
    assert refusal(cfg) is None
    N = xg.size // 3
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, LD).reshape(-1, 3)[ien]                      # [T, 4, 3]
    w = np.asarray(w, np.float64)
    phi = w[4 * N:5 * N].astype(LD)[ien]
    Tn64 = w[5 * N:6 * N][ien]
    Tn = Tn64.astype(LD)
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = (e1 * c23).sum(axis=1)
    nt = len(ien)
    m = np.ones((nt, 4), LD)                                          # m[t, q]
    gas = np.zeros(nt, bool)
    if cfg["use_phi"]:
        side, eps, level = LD(cfg["side"]), LD(cfg["eps"]), LD(cfg["level"])
        with np.errstate(divide="ignore", invalid="ignore"):
            g = ((phi[:, 1] - phi[:, 0])[:, None] * c23 + (phi[:, 2] - phi[:, 0])[:, None] * c31
                 + (phi[:, 3] - phi[:, 0])[:, None] * c12) / det[:, None]
            gn = np.sqrt((g * g).sum(axis=1))
            sloped = gn > 0
            d = (phi - level) / np.where(sloped, gn, LD(1))[:, None]
            m = smooth_step(side * (d @ SHL) / eps)
            mean = ((phi[:, 0] + phi[:, 1]) + (phi[:, 2] + phi[:, 3])) / 4
            mflat = np.where(side * (mean - level) > 0, LD(1), LD(0))
            m = np.where(sloped[:, None], m, mflat[:, None])
            gas = np.where(sloped, (side * d <= -eps).all(axis=1), mflat == 0)
    with np.errstate(invalid="ignore"):
        liquid = (Tn64 >= cfg["T_liquidus"]).all(axis=1)
        solid = (Tn64 <= cfg["T_solidus"]).all(axis=1)
    coeff = ~gas & ~liquid & (cfg["darcy_c"] > 0.0 or cfg["latent"] > 0.0)
    vol = ~gas & ~solid
    Tq = Tn @ SHL
    fl, dfl, C = liquid_fraction(cfg, Tq)
    W = GW * np.abs(det)[:, None] * m                                 # [T, q]
    D = np.where(coeff[:, None], (W * C) @ SHL.T, LD(0))
    lat = LD(cfg["latent"]) if cfg["latent"] > 0.0 else LD(0)
    H = np.where(coeff[:, None], (W * lat * dfl) @ SHL.T, LD(0))
    G = np.where(vol[:, None], (W * fl) @ SHL.T, LD(0))
    return dict(D=D, H=H, G=G, coeff=coeff, vol=vol, det=det)


def coefficients(xg, ien, w, cfg):
    """D, H, G [N] (every node adds its tets in ascending tet id: np.add.at adds in index order), touched_c / touched_v [N]
    = the node has a tet that adds to D / H, to G; and the tet terms"""
    N = xg.size // 3
    t = tet_terms(xg, ien, w, cfg)
    nodes = np.asarray(ien).reshape(-1)
    out = {}
    for k in ("D", "H", "G"):
        out[k] = np.zeros(N, LD)
        np.add.at(out[k], nodes, t[k].reshape(-1))
    for k, flag in (("touched_c", t["coeff"]), ("touched_v", t["vol"])):
        out[k] = np.zeros(N, bool)
        out[k][np.asarray(ien).reshape(-1, 4)[flag].reshape(-1)] = True
    out["tets"] = t
    return out


def nodal_volume(xg, ien):
    """lumped nodal volume V_a = sum over a's tets of |det| / 24 (the four N_a(q) of a node sum to 1 to rounding)"""
    N = xg.size // 3
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, LD).reshape(-1, 3)[ien]
    det = np.abs((np.cross(x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]) * (x[:, 1] - x[:, 0])).sum(axis=1))
    V = np.zeros(N, LD)
    np.add.at(V, ien.reshape(-1), np.repeat(GW * det * (SHA + 3 * SHB), 4))
    return V


# ---- the row updates, in the fp64 arithmetic of the header: products rounded before the add ----------------------------------
def update_F(F, D, H, wgalpha, dwgalpha):
    """F with R[3a + d] += D_a u_a[d] and R[5N + a] += H_a dT_a (D or H None: that part is off)"""
    F = np.array(F, np.float64)
    N = F.size // 6
    if D is not None:
        F[:3 * N] = F[:3 * N] + np.repeat(np.asarray(D, np.float64), 3) * wgalpha[:3 * N]
    if H is not None:
        F[5 * N:] = F[5 * N:] + np.asarray(H, np.float64) * dwgalpha[5 * N:]
    return F


def diagonal_positions(row_ptr, col_ind):
    rows = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    k = np.flatnonzero(rows == col_ind)
    assert k.size == row_ptr.size - 1
    return k


def update_J(val, D, row_ptr, col_ind):
    """block values [nnz, 16] with fact2 D_a on the entries (d, d), d < 3, of node a's diagonal block"""
    val = np.array(val, np.float64).reshape(-1, 16)
    k = diagonal_positions(row_ptr, col_ind)
    add = FACT2 * np.asarray(D, np.float64)
    for d in range(3):
        val[k, 5 * d] = val[k, 5 * d] + add
    return val.reshape(-1)


def update_JT(val, H, row_ptr, col_ind):
    val = np.array(val, np.float64)
    k = diagonal_positions(row_ptr, col_ind)
    val[k] = val[k] + kALPHAM * np.asarray(H, np.float64)
    return val


def stats(xg, w, cfg, G):
    """liquid volume (longdouble sum of the G given), T_max over the metal nodes, count and bounding box of the molten nodes"""
    N = xg.size // 3
    x = np.asarray(xg, np.float64).reshape(-1, 3)
    w = np.asarray(w, np.float64)
    phi, T = w[4 * N:5 * N], w[5 * N:6 * N]
    metal = np.ones(N, bool)
    if cfg["use_phi"]:
        with np.errstate(invalid="ignore"):
            metal = cfg["side"] * (phi - cfg["level"]) > 0
    fl, _, _ = liquid_fraction(cfg, T)
    molten = metal & (fl >= LD("0.5"))
    Tm = T[metal & ~np.isnan(T)]
    return dict(liquid_volume=np.asarray(G, LD).sum(), T_max=float(Tm.max()) if Tm.size else -np.inf, molten=int(molten.sum()),
                lo=x[molten].min(axis=0) if molten.any() else np.full(3, np.inf),
                hi=x[molten].max(axis=0) if molten.any() else np.full(3, -np.inf))


def state(N, phi, T, u=None):
    w = np.zeros(6 * N)
    if u is not None:
        w[:3 * N] = np.asarray(u).reshape(-1)
    w[4 * N:5 * N] = phi
    w[5 * N:] = T
    return w
