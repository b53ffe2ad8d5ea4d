"""numpy model of the scalar recurrences of the paired raw-basis Arnoldi step (csrc/cgs_device.hpp:
givens_step_block; csrc/k_cgs_block.hip: pair_first_kernel, pair_second_kernel) and of a whole paired GMRES on a dense operator.
Test infrastructure only.

A pair advances iterations k and k+1 with one pass over the basis: p1 = B v_k, p2 = B p1; the raw dots of both against
r_0..r_k, the two-vector update, the one-column fix-up q = p2' - c p1'.  H is column-major with leading dimension ldh;
Hraw is its copy before the Givens rotations.
"""
import numpy as np


def drotg(a, b):
    """BLAS drotg as drotg_dev: returns r, z, c, s"""
    roe = a if abs(a) > abs(b) else b
    scale = abs(a) + abs(b)
    if scale == 0.0:
        return 0.0, 0.0, 1.0, 0.0
    r = scale * np.sqrt((a / scale) ** 2 + (b / scale) ** 2)
    r = -r if roe < 0.0 else r
    c, s = a / r, b / r
    z = 1.0
    if abs(a) > abs(b):
        z = s
    if abs(b) >= abs(a) and c != 0.0:
        z = 1.0 / c
    return r, z, c, s


def givens_step(it, nrm, H, ldh, gv, beta, hist):
    """column `it` of H holds h[0..it]; nrm goes below, the earlier rotations are applied, a new one is formed"""
    col = H[it * ldh: it * ldh + it + 2]
    col[it + 1] = nrm
    for i in range(it):
        c, s = gv[2 * i], gv[2 * i + 1]
        x, y = col[i], col[i + 1]
        col[i], col[i + 1] = c * x + s * y, c * y - s * x
    r, _, c, s = drotg(col[it], col[it + 1])
    col[it], col[it + 1] = r, 0.0
    gv[2 * it], gv[2 * it + 1] = c, s
    b0 = beta[it]
    beta[it + 1], beta[it] = -s * b0, b0 * c
    hist[it] = abs(beta[it + 1])


def pair_first(s11, s12, s22, k, nu, H, Hraw, ldh, gv, beta, hist):
    """after the two-vector update: returns sc = [c, d, s22, nu1]; column k of H (rows 0..k = h1 already there)"""
    nu1 = np.sqrt(s11)
    nu[k + 1] = nu1
    Hraw[k * ldh + k + 1] = nu1
    givens_step(k, nu1, H, ldh, gv, beta, hist)
    return np.array([s12 / s11, s12 / nu1, s22, nu1])


def pair_second(qq, k, nu, H, Hraw, ldh, e, sc, gv, beta, hist):
    """after the fix-up: nu[k+2], column k+1 of H and Hraw, its Givens step; returns the cancellation flag"""
    nu1, d = sc[3], sc[1]
    nuq = np.sqrt(qq)
    nu[k + 2] = nuq
    flag = int(nuq < 1e-4 * np.sqrt(sc[2]))
    h1 = Hraw[k * ldh: k * ldh + k + 1].copy()
    col = np.zeros(k + 3)
    for i in range(k + 1):
        t = e[i]
        for j in range(max(i - 1, 0), k):
            t -= h1[j] * Hraw[j * ldh + i]
        t -= h1[k] * h1[i]
        col[i] = t / nu1
    col[k + 1] = (d - h1[k] * nu1) / nu1
    col[k + 2] = nuq / nu1
    Hraw[(k + 1) * ldh: (k + 1) * ldh + k + 3] = col
    H[(k + 1) * ldh: (k + 1) * ldh + k + 2] = col[:k + 2]
    givens_step(k + 1, col[k + 2], H, ldh, gv, beta, hist)
    return flag


def gmres_reference(B, r0, m):
    """classical Gram-Schmidt Arnoldi with a normalised basis: (H un-rotated (m+1, m), residual history)"""
    n = r0.size
    V = np.zeros((m + 1, n))
    ldh = m + 2
    H, gv, beta, hist = np.zeros(ldh * m), np.zeros(2 * m), np.zeros(m + 1), np.zeros(m)
    Hraw = np.zeros((m + 1, m))
    beta[0] = np.linalg.norm(r0)
    V[0] = r0 / beta[0]
    for k in range(m):
        w = B @ V[k]
        h = V[:k + 1] @ w
        w = w - h @ V[:k + 1]
        nrm = np.linalg.norm(w)
        V[k + 1] = w / nrm
        H[k * ldh: k * ldh + k + 1] = h
        Hraw[:k + 1, k], Hraw[k + 1, k] = h, nrm
        givens_step(k, nrm, H, ldh, gv, beta, hist)
    return Hraw, hist


def gmres_paired(B, r0, m):
    """the paired scheme on raw columns r_j = nu_j v_j, pairs while two iterations fit, one single step for an odd tail"""
    n = r0.size
    R = np.zeros((m + 1, n))
    ldh = m + 2
    H, Hraw, gv, beta, hist = np.zeros(ldh * m), np.zeros(ldh * m), np.zeros(2 * m), np.zeros(m + 1), np.zeros(m)
    nu = np.zeros(m + 2)
    nu[0] = beta[0] = np.linalg.norm(r0)
    R[0] = r0
    k, flags = 0, 0
    while k < m:
        p1 = (B @ R[k]) / nu[k]
        g1 = R[:k + 1] @ p1
        h1 = g1 / nu[:k + 1]
        H[k * ldh: k * ldh + k + 1] = h1
        Hraw[k * ldh: k * ldh + k + 1] = h1
        if k + 2 > m:  # the single raw-basis step
            p1 = p1 - (h1 / nu[:k + 1]) @ R[:k + 1]
            nu[k + 1] = np.linalg.norm(p1)
            Hraw[k * ldh + k + 1] = nu[k + 1]
            R[k + 1] = p1
            givens_step(k, nu[k + 1], H, ldh, gv, beta, hist)
            k += 1
            continue
        p2 = B @ p1
        e = (R[:k + 1] @ p2) / nu[:k + 1]
        p1 = p1 - (h1 / nu[:k + 1]) @ R[:k + 1]
        p2 = p2 - (e / nu[:k + 1]) @ R[:k + 1]
        sc = pair_first(p1 @ p1, p1 @ p2, p2 @ p2, k, nu, H, Hraw, ldh, gv, beta, hist)
        q = p2 - sc[0] * p1
        R[k + 1], R[k + 2] = p1, q
        flags |= pair_second(q @ q, k, nu, H, Hraw, ldh, e, sc, gv, beta, hist)
        k += 2
    return Hraw.reshape(m, ldh).T[:m + 1], hist, flags
