"""numpy model of the fluid material (include/dedflow.h, "fluid material"): the text of that section, tet by tet in
np.longdouble, node sums in ascending tet order.  Written from the header, not from the kernels.  Test infrastructure only;
shared by test_fluid_cpu.py (which checks the model against the oracle's element tensors and against closed forms) and
test_gpu_fluid.py (which checks the kernels against the model).  The smoothstep Hs is phase_model's, the metal fraction
thermal_model's.

Every output comes with the sum of the absolute values of its terms ("abs"), the scale a rounding bound has to use where the
output itself cancels: the same expressions evaluated with |factor| for every factor and + for every -, down to the nodal
values and the shape gradients (element_E / element_B with absolute=True); a difference E(rho, mu, f) - E(kRHO, kMU, 0) has
the sum of the abs-sums of both sides."""
import numpy as np

import phase_model as pm
import scalar_model as sm
import thermal_model as tm

LD = np.longdouble
SHL, GW = pm.SHL, pm.GW                                                  # SHL[a, q]
kRHO, kMU = sm.kRHO, 10.0 / 3.0
F1, F2 = LD(sm.F1), LD(sm.F2)
T0 = LD(4.0) / (LD(sm.kDT) * LD(sm.kDT))

DEFAULTS = dict(rho_gas=None, rho_metal=None, mu_gas=None, mu_metal=None, gravity=(0.0, 0.0, 0.0), beta=0.0, T_ref=0.0,
                use_phi=False, level=0.0, side=1, eps=1.0)
REAL = ["rho_gas", "rho_metal", "mu_gas", "mu_metal", "beta", "T_ref", "level", "eps"]
NEUTRAL = dict(rho_gas=kRHO, rho_metal=kRHO, mu_gas=kMU, mu_metal=kMU)


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, **kw)
    if c["rho_gas"] is None:
        c["rho_gas"] = c["rho_metal"]
    if c["mu_gas"] is None:
        c["mu_gas"] = c["mu_metal"]
    c["gravity"] = tuple(float(v) for v in c["gravity"])
    return c


def refusal(cfg):
    """why DflMeshSetFluidMaterial refuses the configuration, or None"""
    for k in REAL[:4]:
        if not np.isfinite(cfg[k]):
            return k
    for d in range(3):
        if not np.isfinite(cfg["gravity"][d]):
            return "gravity"
    for k in REAL[4:]:
        if not np.isfinite(cfg[k]):
            return k
    for k in REAL[:4]:
        if not cfg[k] > 0.0:
            return k
    if cfg["use_phi"] and cfg["side"] not in (1, -1):
        return "side"
    if cfg["use_phi"] and not cfg["eps"] > 0.0:
        return "eps"
    return None


def tet_coefficients(xg, ien, w, cfg):
    """per tet: gN [T, 4, 3], W [T], gg, tr [T], m, rho, mu [T, q], f [T, q, 3] in longdouble"""
    assert refusal(cfg) is None
    N = xg.size // 3
    t = tm.tet_coefficients(xg, ien, w, dict(tm.config(k_solid=1.0, c_metal=1.0), use_phi=cfg["use_phi"], level=cfg["level"],
                                             side=cfg["side"], eps=cfg["eps"]))
    m, ien4 = t["m"], t["ien"]
    gN = t["cr"] / t["det"][:, None, None]
    G = np.einsum("tir,tjr->tij", gN[:, 1:], gN[:, 1:])                 # G(i,j) = sum_r dxi_i/dx_r dxi_j/dx_r
    rho = LD(cfg["rho_gas"]) + m * (LD(cfg["rho_metal"]) - LD(cfg["rho_gas"]))
    mu = LD(cfg["mu_gas"]) + m * (LD(cfg["mu_metal"]) - LD(cfg["mu_gas"]))
    fac = np.ones_like(m)
    if cfg["beta"] != 0.0:
        Tq = t["Tn"] @ SHL
        with np.errstate(invalid="ignore"):
            fac = np.where(np.isnan(Tq), LD(1), LD(1) - m * LD(cfg["beta"]) * (Tq - LD(cfg["T_ref"])))
    f = fac[:, :, None] * np.asarray(cfg["gravity"], LD)[None, None, :]
    return dict(ien=ien4, gN=gN, W=t["W"], gg=np.einsum("tij,tij->t", G, G), tr=np.einsum("tii->t", G), m=m, rho=rho, mu=mu, f=f)


def base_coefficients(nt):
    return np.full((nt, 4), LD(kRHO)), np.full((nt, 4), LD(kMU)), np.zeros((nt, 4, 3), LD)


def fields(N, ien4, w, dw):
    """u, du [T, 4, 3] and the pressure p [T, 4] (from the rate vector, as the assembly takes it)"""
    w, dw = np.asarray(w, np.float64), np.asarray(dw, np.float64)
    return (w[:3 * N].astype(LD).reshape(-1, 3)[ien4], dw[:3 * N].astype(LD).reshape(-1, 3)[ien4],
            dw[3 * N:4 * N].astype(LD)[ien4])


def element_E(g, u, du, p, rho, mu, f, absolute=False):
    """E [T, a, 4]: the three momentum rows and the continuity row of every node of every tet (the element residual of the
    assembly with rho_q, mu_q, f_q).  absolute: every factor by its absolute value and every difference as a sum"""
    gN, W = g["gN"], g["W"]
    s = LD(1) if absolute else LD(-1)
    u_signed = u
    if absolute:
        gN, u, du, p, f = np.abs(gN), np.abs(u), np.abs(du), np.abs(p), np.abs(f)
    grad = np.einsum("tbd,tbi->tid", gN, u)                             # grad[i, d] = d u_i / d x_d
    gp = np.einsum("tbd,tb->td", gN, p)
    divu = np.einsum("tii->t", grad)
    uq = np.einsum("bq,tbi->tqi", SHL, u)
    acc = np.einsum("bq,tbi->tqi", SHL, du) + s * f
    pq = np.einsum("bq,tb->tq", SHL, p)
    r = rho[:, :, None]
    rLi = r * acc + r * np.einsum("tqd,tid->tqi", uq, grad) + gp[:, None, :]
    # u.G.u as the residual forms it: sum_r (sum_i dxi_i/dx_r u_i)^2 (always from the signed values: tau is a coefficient)
    v = np.einsum("tkr,tqk->tqr", g["gN"][:, 1:], np.einsum("bq,tbi->tqi", SHL, u_signed))
    y = (v * v).sum(axis=2) + 3 * (mu / rho) ** 2 * g["gg"][:, None]
    tau0 = 1 / np.sqrt(T0 + y) / rho
    tau1 = np.sqrt(y) / g["tr"][:, None]
    tmp0 = r * acc + np.einsum("tqd,tid->tqi", r * (uq + s * tau0[:, :, None] * rLi), grad)
    sym = grad + np.swapaxes(grad, 1, 2)
    tmp1 = (mu[:, :, None, None] * sym[:, None] + (rho * tau0)[:, :, None, None] * rLi[:, :, :, None] * uq[:, :, None, :]
            + s * (rho * tau0 * tau0)[:, :, None, None] * rLi[:, :, :, None] * rLi[:, :, None, :])
    diag = rho * tau1 * divu[:, None] + s * pq
    tmp1 = tmp1 + diag[:, :, None, None] * np.eye(3, dtype=LD)[None, None]
    E = np.empty(gN.shape[:1] + (4, 4), LD)
    E[:, :, :3] = (np.einsum("aq,tqi->tai", SHL, tmp0) + np.einsum("tad,tqid->tai", gN, tmp1)) * W[:, None, None]
    E[:, :, 3] = (np.einsum("aq,t->ta", SHL, divu) + np.einsum("tq,tqd,tad->ta", tau0, rLi, gN)) * W[:, None]
    return E


def element_B(g, u, rho, mu, absolute=False):
    """B [T, a, b, 4, 4]: the (u,p) blocks of the element Jacobian with rho_q, mu_q inside the quadrature sums"""
    gN, W = g["gN"], g["W"]
    s = LD(1) if absolute else LD(-1)
    uq = np.einsum("bq,tbi->tqi", SHL, u)
    c = np.einsum("tqd,tbd->tqb", uq, gN)                               # c_b(q) = u_q . grad N_b
    y = (c[:, :, 1:] ** 2).sum(axis=2) + 3 * (mu / rho) ** 2 * g["gg"][:, None]     # |J^-1 u_q|^2 + ...
    tau0 = 1 / np.sqrt(T0 + y) / rho
    tau1 = np.sqrt(y) / g["tr"][:, None]
    if absolute:
        gN = np.abs(gN)
        c = np.einsum("tqd,tbd->tqb", np.einsum("bq,tbi->tqi", SHL, np.abs(u)), gN)
    eK = np.einsum("tad,tbd->tab", gN, gN)
    sa = SHL.T                                                          # [q, a]
    rt0 = rho * tau0
    diag = (F1 * np.einsum("tq,qa,qb->tab", rho, sa, sa) + F1 * np.einsum("tq,tqa,qb->tab", rho * rt0, c, sa)
            + F2 * np.einsum("tq,qa,tqb->tab", rho, sa, c) + F2 * np.einsum("tq,tqa,tqb->tab", rho * rt0, c, c)
            + F2 * mu.sum(axis=1)[:, None, None] * eK) * W[:, None, None]
    cK = F2 * W * mu.sum(axis=1)
    cT = F2 * W * (rho * tau1).sum(axis=1)
    B = np.zeros(gN.shape[:1] + (4, 4, 4, 4), LD)
    B[:, :, :, :3, :3] = (cK[:, None, None, None, None] * np.einsum("taj,tbi->tabij", gN, gN)
                          + cT[:, None, None, None, None] * np.einsum("tai,tbj->tabij", gN, gN))
    for i in range(3):
        B[:, :, :, i, i] += diag
    cP0 = W[:, None] * sa.sum(axis=0)[None, :]                          # [T, b]
    cP1 = W[:, None] * np.einsum("tq,tqa->ta", rt0, c)                  # [T, a]
    B[:, :, :, :3, 3] = cP1[:, :, None, None] * gN[:, None, :, :] + s * cP0[:, None, :, None] * gN[:, :, None, :]
    cU0 = W[:, None] * (F1 * np.einsum("tq,qb->tb", rt0, sa) + F2 * np.einsum("tq,tqb->tb", rt0, c))   # [T, b]
    cU1 = W[:, None] * F2 * sa.sum(axis=0)[None, :]                     # [T, a]
    B[:, :, :, 3, :3] = cU0[:, None, :, None] * gN[:, :, None, :] + cU1[:, :, None, None] * gN[:, None, :, :]
    B[:, :, :, 3, 3] = (W * tau0.sum(axis=1))[:, None, None] * eK
    return B


def _node_sum(N, ien4, v):
    out = np.zeros((N,) + v.shape[2:], LD)
    np.add.at(out, ien4.reshape(-1), v.reshape((-1,) + v.shape[2:]))    # in index order: ascending tet id per node
    return out


def _pack(rn):
    """[N, 4] -> the layout of r: r[3a + d], r[3N + a]"""
    return np.concatenate([rn[:, :3].reshape(-1), rn[:, 3]])


def rows(xg, ien, w, dw, cfg):
    """r [4N], Rn, Mn [N] in longdouble at (w, dw) taken as the alpha states, their abs-sums r_abs, Rn_abs, Mn_abs, and the
    tet terms"""
    N = xg.size // 3
    g = tet_coefficients(xg, ien, w, cfg)
    ien4 = g["ien"]
    u, du, p = fields(N, ien4, w, dw)
    rho0, mu0, f0 = base_coefficients(len(ien4))
    with np.errstate(invalid="ignore"):
        live = ~((g["rho"] == rho0) & (g["mu"] == mu0) & (g["f"] == 0).all(axis=2)).all(axis=1)
        E = element_E(g, u, du, p, g["rho"], g["mu"], g["f"]) - element_E(g, u, du, p, rho0, mu0, f0)
        E_abs = element_E(g, u, du, p, g["rho"], g["mu"], g["f"], True) + element_E(g, u, du, p, rho0, mu0, f0, True)
    zero = ~live[:, None, None]                                         # such a tet adds +0.0 whatever its fields hold
    out = dict(tets=g, live=live)
    out["r"] = _pack(_node_sum(N, ien4, np.where(zero, LD(0), E)))
    out["r_abs"] = _pack(_node_sum(N, ien4, np.where(zero, LD(0), E_abs)))
    for name, c in (("Rn", g["rho"]), ("Mn", g["mu"])):
        v = np.einsum("t,tq,aq->ta", g["W"], c, SHL)
        out[name] = _node_sum(N, ien4, v)
        out[name + "_abs"] = _node_sum(N, ien4, np.abs(v))
    return out


def element_jm(xg, ien, w, cfg):
    """jm [T, a, b, 4, 4] in longdouble and its abs-sum: the difference blocks, coefficients frozen at the state w"""
    N = xg.size // 3
    g = tet_coefficients(xg, ien, w, cfg)
    u = np.asarray(w, np.float64)[:3 * N].astype(LD).reshape(-1, 3)[g["ien"]]
    rho0, mu0, _ = base_coefficients(len(g["ien"]))
    jm = element_B(g, u, g["rho"], g["mu"]) - element_B(g, u, rho0, mu0)
    jm_abs = element_B(g, u, g["rho"], g["mu"], True) + element_B(g, u, rho0, mu0, True)
    same = ((g["rho"] == rho0) & (g["mu"] == mu0)).all(axis=1)
    jm[same] = 0
    return jm, jm_abs


def on_pattern(ien, N, rp, ci, Be):
    """S [nnz, 16]: for every nonzero (a, b) of the nodal pattern the sum of Be[t, la, lb] over a's tets that hold b, in
    ascending tet id"""
    ien4 = np.asarray(ien).reshape(-1, 4).astype(np.int64)
    rows_of = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
    key = rows_of * N + np.asarray(ci, np.int64)
    order = np.argsort(key, kind="stable")
    want = (np.repeat(ien4, 4, axis=1) * N + np.tile(ien4, (1, 4))).reshape(-1)    # (t, a, b) in index order
    at = order[np.searchsorted(key[order], want)]
    assert np.array_equal(key[at], want)
    S = np.zeros((len(ci), 16), LD)
    np.add.at(S, at, Be.reshape(-1, 16))
    return S


def state(N, phi, T, u=None):
    return pm.state(N, phi, T, u)


def rates(N, du=None, p=None):
    """dw [6N] with the rates of u and the pressure slot"""
    dw = np.zeros(6 * N)
    if du is not None:
        dw[:3 * N] = np.asarray(du).reshape(-1)
    if p is not None:
        dw[3 * N:4 * N] = p
    return dw
