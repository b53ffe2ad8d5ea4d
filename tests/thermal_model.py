"""numpy model of the thermal material (include/dedflow.h, "thermal material"): the text of that section, tet by tet in
np.longdouble, node sums in ascending tet order.  Written from the header, not from the kernels.  Test infrastructure only;
shared by test_thermal_cpu.py (which checks the model against closed forms) and test_gpu_thermal.py (which checks the kernels
against the model).  The smoothstep Hs and the liquid fraction are phase_model's, the base element matrices and the pattern
helpers scalar_model's.

Every output comes with the sum of the absolute values of its terms ("abs"), the scale a rounding bound has to use where the
output itself cancels: products are taken with |factor| down to the nodal differences T_b - T_0 (which the closed form of
grad T forms first) and to k_q and the built-in constant of dk_q = k_q - kKAPPA, likewise dc_q."""
import numpy as np

import phase_model as pm
import scalar_model as sm

LD = np.longdouble
SHL, GW = pm.SHL, pm.GW
K0, C0 = LD(sm.kKAPPA), LD(sm.kRHO) * LD(sm.kCP)
F1, F2 = LD(sm.F1), LD(sm.F2)

DEFAULTS = dict(k_gas=None, k_solid=None, k_liquid=None, c_gas=None, c_metal=None, T_solidus=0.0, T_liquidus=0.0,
                use_phi=False, level=0.0, side=1, eps=1.0)
REAL = ["k_gas", "k_solid", "k_liquid", "c_gas", "c_metal", "T_solidus", "T_liquidus", "level", "eps"]
NEUTRAL = dict(k_gas=sm.kKAPPA, k_solid=sm.kKAPPA, k_liquid=sm.kKAPPA, c_gas=sm.kRHO * sm.kCP, c_metal=sm.kRHO * sm.kCP)


def config(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, **kw)
    if c["k_liquid"] is None:
        c["k_liquid"] = c["k_solid"]
    if c["k_gas"] is None:
        c["k_gas"] = c["k_solid"]
    if c["c_gas"] is None:
        c["c_gas"] = c["c_metal"]
    return c


def refusal(cfg):
    """why DflMeshSetThermalMaterial refuses the configuration, or None"""
    for k in REAL:
        if not np.isfinite(cfg[k]):
            return k
    for k in REAL[:5]:
        if not cfg[k] > 0.0:
            return k
    if cfg["k_liquid"] != cfg["k_solid"] and not cfg["T_liquidus"] > cfg["T_solidus"]:
        return "T_liquidus"
    if cfg["use_phi"] and cfg["side"] not in (1, -1):
        return "side"
    if cfg["use_phi"] and not cfg["eps"] > 0.0:
        return "eps"
    return None


def tet_coefficients(xg, ien, w, cfg):
    """per tet: gradN [T, 4, 3], det [T], W [T], m, fl, k, c [T, q] in longdouble"""
    assert refusal(cfg) is None
    N = xg.size // 3
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, LD).reshape(-1, 3)[ien]
    w = np.asarray(w, np.float64)
    phi = w[4 * N:5 * N].astype(LD)[ien]
    Tn = w[5 * N:6 * N].astype(LD)[ien]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = (e1 * c23).sum(axis=1)
    cr = np.stack([-(c23 + c31 + c12), c23, c31, c12], axis=1)          # grad N_a = cr[a] / det
    nt = len(ien)
    m = np.ones((nt, 4), LD)
    if cfg["use_phi"]:                                                  # (phase_model.tet_terms, the same rules)
        side, eps, level = LD(cfg["side"]), LD(cfg["eps"]), LD(cfg["level"])
        with np.errstate(divide="ignore", invalid="ignore"):
            g = ((phi[:, 1] - phi[:, 0])[:, None] * c23 + (phi[:, 2] - phi[:, 0])[:, None] * c31
                 + (phi[:, 3] - phi[:, 0])[:, None] * c12) / det[:, None]
            gn = np.sqrt((g * g).sum(axis=1))
            sloped = gn > 0
            d = (phi - level) / np.where(sloped, gn, LD(1))[:, None]
            m = pm.smooth_step(side * (d @ SHL) / eps)
            mean = ((phi[:, 0] + phi[:, 1]) + (phi[:, 2] + phi[:, 3])) / 4
            mflat = np.where(side * (mean - level) > 0, LD(1), LD(0))
            m = np.where(sloped[:, None], m, mflat[:, None])
    fl = np.zeros((nt, 4), LD)
    if cfg["k_liquid"] != cfg["k_solid"]:
        fl = pm.liquid_fraction(dict(T_solidus=cfg["T_solidus"], T_liquidus=cfg["T_liquidus"], darcy_c=0.0), Tn @ SHL)[0]
    kg, ks, kl = LD(cfg["k_gas"]), LD(cfg["k_solid"]), LD(cfg["k_liquid"])
    cg, cm = LD(cfg["c_gas"]), LD(cfg["c_metal"])
    k = kg + m * ((ks + fl * (kl - ks)) - kg)
    c = cg + m * (cm - cg)
    return dict(ien=ien, cr=cr, det=det, W=GW * np.abs(det), m=m, fl=fl, k=k, c=c, Tn=Tn)


def _node_sum(N, ien, v):
    out = np.zeros(N, LD)
    np.add.at(out, ien.reshape(-1), v.reshape(-1))                      # in index order: ascending tet id per node
    return out


def rows(xg, ien, w, dw, cfg):
    """r, Kn, Cn [N] in longdouble at (w, dw) taken as the alpha states, their abs-sums r_abs, Kn_abs, Cn_abs, the conduction
    part r_cond alone, and the tet terms"""
    N = xg.size // 3
    t = tet_coefficients(xg, ien, w, cfg)
    ien4, cr, det, W = t["ien"], t["cr"], t["det"], t["W"]
    w = np.asarray(w, np.float64)
    u = w[:3 * N].astype(LD).reshape(-1, 3)[ien4]                       # [T, 4, 3]
    dT = np.asarray(dw, np.float64)[5 * N:6 * N].astype(LD)[ien4]
    Tn = t["Tn"]
    dk, dc = t["k"] - K0, t["c"] - C0                                   # [T, q]
    dk_abs, dc_abs = np.abs(t["k"]) + K0, np.abs(t["c"]) + C0
    with np.errstate(invalid="ignore"):
        live = ((dk != 0) | (dc != 0)).any(axis=1)                      # a tet whose eight differences are all 0 adds +0.0
    tk = (Tn[:, 1:] - Tn[:, :1])[:, :, None] * cr[:, 1:] / det[:, None, None]      # [T, 3, d]: the terms of gT
    gT, gT_abs = tk.sum(axis=1), np.abs(tk).sum(axis=1)
    gN = cr / det[:, None, None]
    cond = np.einsum("tad,td->ta", gN, gT)                              # grad N_a . gT
    cond_abs = np.einsum("tad,td->ta", np.abs(gN), gT_abs)
    uq = np.einsum("bq,tbd->tqd", SHL, u)
    adv = np.einsum("tqd,td->tq", uq, gT)
    adv_abs = np.einsum("tqd,td->tq", np.einsum("bq,tbd->tqd", SHL, np.abs(u)), gT_abs)
    dTq, dTq_abs = dT @ SHL, np.abs(dT) @ SHL
    # r_a = sum_q W [ dc_q N_a(q) (dT_q + u_q . gT) + dk_q cond_a ]
    cap = np.einsum("t,tq,aq->ta", W, dc * (dTq + adv), SHL)
    con = np.einsum("t,tq,ta->ta", W, dk, cond)
    r_abs = np.einsum("t,tq,aq->ta", W, dc_abs * (dTq_abs + adv_abs), SHL) + np.einsum("t,tq,ta->ta", W, dk_abs, cond_abs)
    zero = ~live[:, None]
    out = dict(tets=t, live=live)
    out["r"] = _node_sum(N, ien4, np.where(zero, LD(0), cap + con))
    out["r_cond"] = _node_sum(N, ien4, np.where(zero, LD(0), con))
    out["r_abs"] = _node_sum(N, ien4, np.where(zero, LD(0), r_abs))
    for name, f in (("Kn", t["k"]), ("Cn", t["c"])):
        v = np.einsum("t,tq,aq->ta", W, f, SHL)
        out[name] = _node_sum(N, ien4, v)
        out[name + "_abs"] = _node_sum(N, ien4, np.abs(v))
    return out


def element_jm(xg, ien, w, cfg, lumped=False):
    """jm [T, 4, 4] in longdouble and its abs-sum: the entries the section adds to the T Jacobian's element matrices,
    coefficients frozen at the state w.  lumped: the capacity correction's N_a N_b replaced by its row sum on the diagonal (what
    the section deliberately does not do)"""
    N = xg.size // 3
    t = tet_coefficients(xg, ien, w, cfg)
    ien4, cr, det, W = t["ien"], t["cr"], t["det"], t["W"]
    u = np.asarray(w, np.float64)[:3 * N].astype(LD).reshape(-1, 3)[ien4]
    dk, dc = t["k"] - K0, t["c"] - C0
    dk_abs, dc_abs = np.abs(t["k"]) + K0, np.abs(t["c"]) + C0
    gN = cr / det[:, None, None]
    gab = np.einsum("tad,tbd->tab", gN, gN)
    gab_abs = np.einsum("tad,tbd->tab", np.abs(gN), np.abs(gN))
    uq = np.einsum("bq,tbd->tqd", SHL, u)
    cb = np.einsum("tqd,tbd->tqb", uq, gN)                              # u_q . grad N_b
    cb_abs = np.einsum("tqd,tbd->tqb", np.einsum("bq,tbd->tqd", SHL, np.abs(u)), np.abs(gN))
    col = F1 * SHL.T[None] + F2 * cb                                    # [T, q, b]
    col_abs = F1 * SHL.T[None] + F2 * cb_abs
    if lumped:
        mass = np.einsum("t,tq,aq,ab->tab", W, dc, SHL, np.eye(4, dtype=LD)) * F1
        jm = mass + np.einsum("t,tq,aq,tqb->tab", W, dc, SHL, F2 * cb)
    else:
        jm = np.einsum("t,tq,aq,tqb->tab", W, dc, SHL, col)
    jm = jm + F2 * np.einsum("t,tq,tab->tab", W, dk, gab)
    jm_abs = np.einsum("t,tq,aq,tqb->tab", W, dc_abs, SHL, col_abs) + F2 * np.einsum("t,tq,tab->tab", W, dk_abs, gab_abs)
    return jm, jm_abs


def jacobian_T(xg, ien, w, cfg, lumped=False):
    """(JT = scalar_model's base + jm, its abs-sum) as N x N scipy CSR in float64 (the base model's precision)"""
    N = xg.size // 3
    w = np.asarray(w, np.float64)
    _, Jt = sm.element_matrices(xg, ien, w)
    jm, jm_abs = element_jm(xg, ien, w, cfg, lumped)
    A = sm.scatter(ien, N, Jt + jm.astype(np.float64))
    A_abs = sm.scatter(ien, N, np.abs(Jt) + jm_abs.astype(np.float64))
    return A, A_abs


def total_matrices(xg, ien, w, cfg):
    """(K, C) as N x N scipy CSR: the conduction matrix sum_q W k_q grad N_a . grad N_b and the consistent capacity matrix
    sum_q W c_q N_a N_b that base + correction amount to at u = 0 (without the f1, f2 factors)"""
    N = xg.size // 3
    t = tet_coefficients(xg, ien, w, cfg)
    gN = t["cr"] / t["det"][:, None, None]
    Ke = np.einsum("t,tq,tad,tbd->tab", t["W"], t["k"], gN, gN)
    Ce = np.einsum("t,tq,aq,bq->tab", t["W"], t["c"], SHL, SHL)
    return sm.scatter(ien, N, Ke.astype(np.float64)), sm.scatter(ien, N, Ce.astype(np.float64))


def matvec_jm(ien, N, jm, v):
    """(sum over the tets of jm_e) v in longdouble, and the abs-sum of the same products"""
    ien4 = np.asarray(ien).reshape(-1, 4)
    ve = np.asarray(v, LD)[ien4]                                        # [T, b]
    p = jm * ve[:, None, :]
    return _node_sum(N, ien4, p.sum(axis=2)), _node_sum(N, ien4, np.abs(p).sum(axis=2))


def state(N, phi, T, u=None):
    return pm.state(N, phi, T, u)


def rate(N, dT):
    dw = np.zeros(6 * N)
    dw[5 * N:] = dT
    return dw


# ---- the two-layer slab shared by test_thermal_cpu.py and test_gpu_thermal.py -------------------------------------------------
SLAB = dict(cells=(2, 2, 16), size=(0.25, 0.25, 1.0), z_i=0.5 + 0.25 / 16, eps=1.0 / 16, k_solid=0.66, k_gas=0.66e-3,
            c=1.0e-6, T_bottom=1.0, T_top=0.0, groups=(4, 5), rtol=1e-10,
            cond=1.5e6, steps=16)       # (the last two: checked by test_thermal_cpu.py, used by test_gpu_thermal.py)


def slab(cells=None, eps=None):
    """the slab: metal (k_solid) below z_i, gas (k_gas) above, T held at bottom and top (kuhn_box groups z-, z+); returns
    (mesh, configuration, w0 with phi = z - z_i and the straight line between the held values as T, held [N])"""
    from dedflow_amd.meshgen import kuhn_box
    m = kuhn_box(cells or SLAB["cells"], (0.0, 0.0, 0.0), SLAB["size"])
    z = m.xg.reshape(-1, 3)[:, 2]
    cfg = config(k_gas=SLAB["k_gas"], k_solid=SLAB["k_solid"], c_metal=SLAB["c"], use_phi=True, level=0.0, side=-1,
                 eps=SLAB["eps"] if eps is None else eps)
    held = np.zeros(m.num_node, bool)
    for g in SLAB["groups"]:
        held[m.bound_node[m.bound_node_offset[g]:m.bound_node_offset[g + 1]]] = True
    line = SLAB["T_bottom"] + (SLAB["T_top"] - SLAB["T_bottom"]) * z / SLAB["size"][2]
    return m, cfg, state(m.num_node, z - SLAB["z_i"], line), held


def slab_analytic(z):
    """the two-layer profile: the interface temperature by series resistances"""
    zi, H, Tb, Tt = SLAB["z_i"], SLAB["size"][2], SLAB["T_bottom"], SLAB["T_top"]
    Rs, Rg = zi / SLAB["k_solid"], (H - zi) / SLAB["k_gas"]
    Ti = Tb - (Tb - Tt) * Rs / (Rs + Rg)
    return np.where(z <= zi, Tb + (Ti - Tb) * z / zi, Ti + (Tt - Ti) * (z - zi) / (H - zi)), Ti


def slab_steady(m, cfg, w0, held):
    """the discrete steady solution K T = 0 with the held values of w0 (scipy), and the system matrix A = f1 C + f2 K of one
    solve with unit rows on the held nodes (dense)"""
    import scipy.sparse.linalg as spl
    N = m.num_node
    K, C = total_matrices(m.xg, m.ien, w0, cfg)
    T = np.array(w0[5 * N:])
    free = ~held
    T[free] = spl.spsolve(K[free][:, free].tocsc(), -(K[free][:, held] @ T[held]))
    A = (sm.F1 * C + sm.F2 * K).toarray()
    A[held] = 0.0
    A[held, held] = 1.0
    return T, A


def slab_march_step(T, dT, solve):
    """one generalized-alpha step of the T equation at u = 0: the predictor, solve(T_alpha, dT_alpha) -> the increment dx of
    the new rate (one Newton update: the problem is linear), the corrector.  Returns the new (T, dT)"""
    dT_new = (sm.kGAMMA - 1.0) / sm.kGAMMA * dT
    dT_new = dT_new - solve(T, dT, dT_new)
    return T + sm.kDT * ((1.0 - sm.kGAMMA) * dT + sm.kGAMMA * dT_new), dT_new
