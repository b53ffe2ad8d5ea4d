"""numpy model of the raw-basis Arnoldi step that takes s = 1..4 iterations per pass over the basis (csrc/k_cgs_block.hip:
block_first_kernel, cgs_fixup_block_kernel, block_second_kernel; host/gmres.c: gmres_block) and of a whole blocked GMRES on a
dense operator.  Test infrastructure only; two_step_model.py is the s = 2 case written out.

A block at k takes p_0 = B v_k, p_i = B p_{i-1} (i < s), the raw dots e_i[j] = <r_j, p_i> / nu_j of all of them against
r_0..r_k, the update p_i' = p_i - sum_j (e_i[j] / nu_j) r_j, the Gram matrix G = [<p_a', p_b'>], the unit lower triangular C
with q_i = sum_{l<=i} C[i,l] p_l' orthogonal, U[l,i] = C[l].G[:,i] = <q_l, p_i'>, the measured norms nu_{k+1+i} = ||q_i||.
The scalars travel as sc = [G | C | U], three 4 x 4 row-major tables.  H is column-major with leading dimension ldh; Hraw
is its copy before the Givens rotations.
"""
import numpy as np

from two_step_model import givens_step

SC_G, SC_C, SC_U = 0, 16, 32


def gram_coefficients(G):
    """C and U of an s x s Gram matrix, in the order block_first_kernel takes them"""
    s = G.shape[0]
    Cm, Um, d = np.eye(4), np.zeros((4, 4)), np.zeros(4)
    for i in range(s):
        for l in range(i):
            u = 0.0
            for m in range(l + 1):
                u += Cm[l, m] * G[m, i]
            Um[l, i] = u
            f = u / d[l]
            for m in range(l + 1):
                Cm[i, m] -= f * Cm[l, m]
        dd = 0.0
        for a in range(i + 1):
            r = 0.0
            for b in range(i + 1):
                r += G[a, b] * Cm[i, b]
            dd += Cm[i, a] * r
        d[i] = dd
    return Cm, Um


def block_first(G, k, nu, H, Hraw, ldh, gv, beta, hist):
    """after the s-vector update: nu[k+1], column k of H (rows 0..k = e_0 already there) with its Givens step; returns sc"""
    s = G.shape[0]
    Cm, Um = gram_coefficients(G)
    G4 = np.zeros((4, 4))
    G4[:s, :s] = G
    nu1 = np.sqrt(G[0, 0])
    nu[k + 1] = nu1
    Hraw[k * ldh + k + 1] = nu1
    givens_step(k, nu1, H, ldh, gv, beta, hist)
    return np.concatenate([G4.reshape(-1), Cm.reshape(-1), Um.reshape(-1)])


def fixup(P, sc):
    """rows of P: p_0'..p_{s-1}'; returns q_0..q_{s-1} (q_i = p_i' + sum_{l<i} C[i,l] p_l', l ascending)"""
    s = P.shape[0]
    Cm = sc[SC_C:SC_C + 16].reshape(4, 4)
    Qn = P.copy()
    for a in range(1, s):
        for l in range(a):
            Qn[a] = Qn[a] + Cm[a, l] * P[l]
    return Qn


def block_second(qq, k, nu, H, Hraw, ldh, e, lde, sc, gv, beta, hist):
    """after the fix-up (qq[i-1] = ||q_i||^2, i = 1..s-1): nu[k+1+i], columns k+i of H and Hraw, their Givens steps; returns the flag"""
    s = len(qq) + 1
    G, Um = sc[SC_G:SC_G + 16].reshape(4, 4), sc[SC_U:SC_U + 16].reshape(4, 4)
    flag = 0
    for i in range(1, s):
        nu[k + 1 + i] = np.sqrt(qq[i - 1])
        flag |= int(nu[k + 1 + i] < 1e-4 * np.sqrt(G[i, i]))
    t = np.zeros((s, s))
    for l in range(s):
        for i in range(l + 1, s):
            t[l, i] = Um[l, i] / nu[k + 1 + l]

    def rho(i, r):  # coordinate r of p_i in v_0..v_{k+1+i}
        if r <= k:
            return e[i * lde + r]
        return t[r - k - 1, i] if r - k - 1 < i else nu[k + 1 + i]

    for i in range(1, s):
        c = k + i
        col = np.zeros(c + 2)
        for r in range(c + 2):
            v = rho(i, r)
            for j in range(max(r - 1, 0), c):
                v -= rho(i - 1, j) * Hraw[j * ldh + r]
            col[r] = v / nu[k + i]
        Hraw[c * ldh: c * ldh + c + 2] = col
        H[c * ldh: c * ldh + c + 1] = col[:c + 1]
        givens_step(c, col[c + 1], H, ldh, gv, beta, hist)
    return flag


def block_sizes(m, block):
    """the driver's rule inside one cycle of m columns without checks: as many iterations per trip as fit"""
    k, out = 0, []
    while k < m:
        out.append(min(block, m - k))
        k += out[-1]
    return out


def gmres_blocked(B, r0, m, block):
    """the blocked scheme on raw columns r_j = nu_j v_j: (H un-rotated (m+1, m), residual history, flags, smallest ||q_i|| / ||p_i'||)"""
    n = r0.size
    R = np.zeros((m + 1, n))
    ldh = m + 2
    H, Hraw, gv, beta, hist = np.zeros(ldh * m), np.zeros(ldh * m), np.zeros(2 * m), np.zeros(m + 1), np.zeros(m)
    nu = np.zeros(m + 2)
    nu[0] = beta[0] = np.linalg.norm(r0)
    R[0] = r0
    k, flags, ratio = 0, 0, 1.0
    for s in block_sizes(m, block):
        P = np.zeros((s, n))
        P[0] = (B @ R[k]) / nu[k]
        for i in range(1, s):
            P[i] = B @ P[i - 1]
        e = np.zeros(s * ldh)
        for i in range(s):
            e[i * ldh: i * ldh + k + 1] = (R[:k + 1] @ P[i]) / nu[:k + 1]
        H[k * ldh: k * ldh + k + 1] = e[:k + 1]
        Hraw[k * ldh: k * ldh + k + 1] = e[:k + 1]
        for i in range(s):
            P[i] = P[i] - (e[i * ldh: i * ldh + k + 1] / nu[:k + 1]) @ R[:k + 1]
        if s == 1:  # the single raw-basis step
            nu[k + 1] = np.linalg.norm(P[0])
            Hraw[k * ldh + k + 1] = nu[k + 1]
            R[k + 1] = P[0]
            givens_step(k, nu[k + 1], H, ldh, gv, beta, hist)
            k += 1
            continue
        G = P @ P.T
        sc = block_first(G, k, nu, H, Hraw, ldh, gv, beta, hist)
        Qn = fixup(P, sc)
        R[k + 1: k + 1 + s] = Qn
        qq = [Qn[i] @ Qn[i] for i in range(1, s)]
        flags |= block_second(qq, k, nu, H, Hraw, ldh, e, ldh, sc, gv, beta, hist)
        ratio = min([ratio] + [np.sqrt(qq[i - 1] / G[i, i]) for i in range(1, s)])
        k += s
    return Hraw.reshape(m, ldh).T[:m + 1], hist, flags, ratio
