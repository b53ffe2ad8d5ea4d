"""numpy model of the phi / T transport Jacobians (include/dedflow.h "scalar transport", csrc/k_scalar.hip): per-tet
element matrices of the exact derivatives of the residual's level-set and temperature rows with respect to the rates
dphi / dT, scattered with scipy.sparse.  Test infrastructure only."""
import numpy as np
import scipy.sparse as sp

kRHOC, kDT = 0.5, 5e-2
kALPHAM = (3.0 - kRHOC) / (1.0 + kRHOC)
kALPHAF = 1.0 / (1.0 + kRHOC)
kGAMMA = 0.5 + kALPHAM - kALPHAF
kRHO, kCP, kKAPPA = 1.0e3, 1.0, 0.66
GW = 0.0416666666666667
SHA, SHB = 0.5854101966249685, 0.1381966011250105
F1 = kALPHAM                    # d(dphi_alpha) / d(dphi)
F2 = kDT * kALPHAF * kGAMMA     # d(phi_alpha) / d(dphi)


def shl(q):
    """N_b at quadrature point q, b = 0..3"""
    n = np.full(4, SHB)
    n[q] = SHA
    return n


def geometry(xg, ien):
    """shape gradients [T,4,3], |det J| [T], metric G [T,3,3] (G_ij = sum_r dxi_i/dx_r dxi_j/dx_r)"""
    x = xg.reshape(-1, 3)[ien.reshape(-1, 4)]
    J = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]], axis=2)  # J[:, d, k] = dx_d / dxi_k
    invJ = np.linalg.inv(J)                                                         # invJ[:, k, d] = dxi_k / dx_d
    shg = np.empty((len(x), 4, 3))
    shg[:, 1:] = invJ
    shg[:, 0] = -invJ.sum(axis=1)
    G = np.einsum("tir,tjr->tij", invJ, invJ)
    return shg, np.abs(np.linalg.det(J)), G, invJ


def element_matrices(xg, ien, wga):
    """Jphi_e, JT_e [T,4,4] at the alpha-level state wga (u = wga[:3N])"""
    ien4 = ien.reshape(-1, 4)
    shg, detJ, G, invJ = geometry(xg, ien)
    u = wga[:3 * (xg.size // 3)].reshape(-1, 3)[ien4]     # [T,4,3]
    gg = np.einsum("tij,tij->t", G, G)
    w = GW * detJ
    rc = kRHO * kCP
    kap = kKAPPA / rc
    t0 = 4.0 / (kDT * kDT)
    kg = F2 * kKAPPA * np.einsum("tad,tbd->tab", shg, shg)
    Jp = np.zeros((len(ien4), 4, 4))
    Jt = np.zeros((len(ien4), 4, 4))
    for q in range(4):
        n = shl(q)
        uq = np.einsum("b,tbd->td", n, u)
        v = np.einsum("tkr,tk->tr", invJ, uq)              # u.G.u = |v|^2 as GetStabTau forms it
        t1 = (v * v).sum(axis=1)
        tau2 = 1.0 / np.sqrt(t0 + t1)
        tau3 = 1.0 / np.sqrt(t0 + t1 + 3.0 * kap * kap * gg) / rc
        c = np.einsum("tad,td->ta", shg, uq)
        col = F1 * n[None, :] + F2 * c
        rp = n[None, :] + tau2[:, None] * c
        rt = rc * (n[None, :] + rc * tau3[:, None] * c)
        Jp += w[:, None, None] * rp[:, :, None] * col[:, None, :]
        Jt += w[:, None, None] * (rt[:, :, None] * col[:, None, :] + kg)
    return Jp, Jt


def scatter(ien, N, Ae):
    ien4 = ien.reshape(-1, 4)
    rows = np.repeat(ien4, 4, axis=1).reshape(-1)
    cols = np.tile(ien4, (1, 4)).reshape(-1)
    A = sp.coo_matrix((Ae.reshape(-1), (rows, cols)), shape=(N, N)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def jacobians(xg, ien, wga):
    """(Jphi, JT) as N x N scipy CSR"""
    N = xg.size // 3
    Jp, Jt = element_matrices(xg, ien, wga)
    return scatter(ien, N, Jp), scatter(ien, N, Jt)


def on_pattern(A, rp, ci):
    """values of A in the nonzero order of the nodal pattern (rp, ci)"""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    return np.asarray(A[rows, ci]).reshape(-1)


def mass_matrix(xg, ien):
    """consistent mass matrix of linear tets"""
    _, detJ, _, _ = geometry(xg, ien)
    Me = (detJ / 120.0)[:, None, None] * (np.ones((4, 4)) + np.eye(4))[None]
    return scatter(ien, xg.size // 3, Me)


def alpha_states(N, wgold, dwgold, dwg):
    dwga = (1.0 - kALPHAM) * dwgold + kALPHAM * dwg
    dwga[3 * N:4 * N] = dwg[3 * N:4 * N]
    wga = wgold + kDT * kALPHAF * (1.0 - kGAMMA) * dwgold + kDT * kALPHAF * kGAMMA * dwg
    wga[3 * N:4 * N] = 0.0
    return wga, dwga
