"""Numpy model of PC_AMGX (host/pc_amgx.c, csrc/k_amgx.hip), written from the rules in DESIGN.md "PC_AMGX": pairwise
aggregation, Galerkin coarse matrices, greedy colouring, multicolour-DILU / Jacobi smoothing, the truncated dense LU of the
coarsest level and the V-cycle.  Shared by test_amgx_cpu.py and test_gpu_amgx.py."""
import numpy as np
import scipy.sparse as sp

REFERENCE_INLINE = (
    "config_version=2,"
    "solver:preconditioner:error_scaling=0,"
    "solver:preconditioner:print_grid_stats=1,"
    "solver:preconditioner:max_uncolored_percentage=0.05,"
    "solver:preconditioner:algorithm=AGGREGATION,"
    "solver:preconditioner:solver=AMG,"
    "solver:preconditioner:smoother=MULTICOLOR_DILU,"
    "solver:preconditioner:presweeps=0,"
    "solver:preconditioner:selector=SIZE_2,"
    "solver:preconditioner:coarse_solver=DENSE_LU_SOLVER,"
    "solver:preconditioner:max_iters=1,"
    "solver:preconditioner:postsweeps=3,"
    "solver:preconditioner:min_coarse_rows=32,"
    "solver:preconditioner:relaxation_factor=0.75,"
    "solver:preconditioner:scope=amg,"
    "solver:preconditioner:max_levels=100,"
    "solver:preconditioner:matrix_coloring_scheme=PARALLEL_GREEDY,"
    "solver:preconditioner:cycle=V,"
    "solver:use_scalar_norm=1,"
    "solver:solver=FGMRES,"
    "solver:print_solve_stats=1,"
    "solver:obtain_timings=1,"
    "solver:max_iters=100,"
    "solver:monitor_residual=1,"
    "solver:gmres_n_restart=10,"
    "solver:convergence=RELATIVE_INI_CORE,"
    "solver:scope=main,"
    "solver:tolerance=1e-10,"
    "solver:norm=L2")

REFERENCE_JSON = """{
  "config_version": 2,
  "solver": {
    "preconditioner": {
      "error_scaling": 0, "print_grid_stats": 1, "max_uncolored_percentage": 0.05,
      "algorithm": "AGGREGATION", "solver": "AMG", "smoother": "MULTICOLOR_DILU", "presweeps": 0,
      "selector": "SIZE_2", "coarse_solver": "DENSE_LU_SOLVER", "max_iters": 1, "postsweeps": 3,
      "min_coarse_rows": 32, "relaxation_factor": 0.75, "scope": "amg", "max_levels": 100,
      "matrix_coloring_scheme": "PARALLEL_GREEDY", "cycle": "V"
    },
    "use_scalar_norm": 1, "solver": "FGMRES", "print_solve_stats": 1, "obtain_timings": 1, "max_iters": 100,
    "monitor_residual": 1, "gmres_n_restart": 10, "convergence": "RELATIVE_INI_CORE", "scope": "main",
    "tolerance": 1e-10, "norm": "L2"
  }
}
"""


def p1_stiffness(mesh):
    """P1 Laplacian stiffness matrix of a tet mesh (CSR, columns ascending, explicit zeros kept)."""
    x = mesh.xg.reshape(-1, 3)
    ien = mesh.ien.reshape(-1, 4).astype(np.int64)
    N = x.shape[0]
    D = np.concatenate([np.ones((ien.shape[0], 4, 1)), x[ien]], axis=2)
    G = np.linalg.inv(D)[:, 1:, :]                       # gradients of the barycentric functions (T x 3 x 4)
    vol = np.abs(np.linalg.det(D)) / 6.0
    K = vol[:, None, None] * np.einsum("tdi,tdj->tij", G, G)
    rows = np.repeat(ien, 4, axis=1).reshape(-1)
    cols = np.tile(ien, (1, 4)).reshape(-1)
    A = sp.coo_matrix((K.reshape(-1), (rows, cols)), shape=(N, N)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def dirichlet_identity(A, nodes):
    """Rows and columns of `nodes` replaced by the identity, pattern kept."""
    A = A.tocsr(copy=True)
    mask = np.zeros(A.shape[0], bool)
    mask[nodes] = True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    hit = mask[rows] | mask[A.indices]
    A.data[hit] = 0.0
    A.data[hit & (rows == A.indices)] = 1.0
    return A


def _find(rp, ci, i, j):
    lo, hi = rp[i], rp[i + 1]
    k = lo + np.searchsorted(ci[lo:hi], j)
    return k if k < hi and ci[k] == j else -1


def pairwise(rp, ci, val):
    n = len(rp) - 1
    dg = np.zeros(n)
    for i in range(n):
        d = _find(rp, ci, i, i)
        dg[i] = abs(val[d]) if d >= 0 else 0.0
    w = np.zeros(len(ci))
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            j = ci[k]
            if j == i:
                continue
            t = _find(rp, ci, j, i)
            aij = abs(val[k]) / dg[i] if dg[i] > 0 else 0.0
            aji = abs(val[t]) / dg[j] if (t >= 0 and dg[j] > 0) else 0.0
            w[k] = 0.5 * (aij + aji)
    label = -np.ones(n, np.int64)
    for _ in range(4):
        pick = -np.ones(n, np.int64)
        for i in range(n):
            if label[i] >= 0:
                continue
            best = 0.0
            for k in range(rp[i], rp[i + 1]):
                j = ci[k]
                if j != i and label[j] < 0 and w[k] > best:
                    best, pick[i] = w[k], j
        for i in range(n):
            j = pick[i]
            if j > i and pick[j] == i:
                label[i] = label[j] = i
    strongest = -np.ones(n, np.int64)
    for i in range(n):
        if label[i] >= 0:
            continue
        best = 0.0
        for k in range(rp[i], rp[i + 1]):
            if ci[k] != i and w[k] > best:
                best, strongest[i] = w[k], ci[k]
    new = label.copy()
    for i in range(n):
        if label[i] < 0:
            s = strongest[i]
            new[i] = label[s] if (s >= 0 and label[s] >= 0) else i
    minm = {}
    for i in range(n):
        minm[new[i]] = min(minm.get(new[i], n), i)
    order = sorted(minm, key=lambda l: minm[l])
    ids = {l: c for c, l in enumerate(order)}
    return np.array([ids[l] for l in new], np.int64), len(order)


def galerkin(A, agg, nc):
    n = A.shape[0]
    P = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
    Ac = (P.T @ A @ P).tocsr()
    Ac.sort_indices()
    return Ac


def galerkin_pattern(A, agg, nc):
    """P^T A P with every structurally reachable entry kept (explicit zeros too), as the library stores it."""
    B = A.tocsr(copy=True)
    B.data = np.ones_like(B.data)
    S = galerkin(B, agg, nc)
    return S


def aggregate(A, passes=1):
    A = A.tocsr()
    agg, nc = pairwise(A.indptr, A.indices, A.data)
    cur = A
    step_agg = agg
    for _ in range(1, passes):
        if nc <= 1:
            break
        C = galerkin_with_zeros(cur, step_agg, nc)
        step_agg, nc2 = pairwise(C.indptr, C.indices, C.data)
        agg = step_agg[agg]
        cur, nc = C, nc2
    return agg, nc


def galerkin_with_zeros(A, agg, nc):
    """P^T A P on the library's structural pattern (explicit zeros stay stored), every coarse entry summed over its fine
    nonzeros in ascending order -- the library's order, so the values are bitwise the library's."""
    A = A.tocsr()
    out = galerkin_pattern(A, agg, nc).astype(np.float64)
    out.data[:] = 0.0
    rp, ci = out.indptr, out.indices
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    for k in range(A.nnz):
        out.data[_find(rp, ci, agg[rows[k]], agg[A.indices[k]])] += A.data[k]
    return out


def greedy_colors(rp, ci):
    n = len(rp) - 1
    col = -np.ones(n, np.int64)
    for i in range(n):
        used = {col[j] for j in ci[rp[i]:rp[i + 1]] if j != i and col[j] >= 0}
        c = 0
        while c in used:
            c += 1
        col[i] = c
    return col


# ---- smoother, coarse solve, cycle ---------------------------------------------------------------------------------------
def dilu_einv(A, color):
    A = A.tocsr()
    rp, ci, v = A.indptr, A.indices, A.data
    n = A.shape[0]
    einv = np.zeros(n)
    for c in range(color.max() + 1 if n else 0):
        for i in np.nonzero(color == c)[0]:
            s = 0.0
            for k in range(rp[i], rp[i + 1]):
                j = ci[k]
                if color[j] < c:
                    t = _find(rp, ci, j, i)
                    if t >= 0:
                        s += v[k] * v[t] * einv[j]
            aii = v[_find(rp, ci, i, i)]
            e = aii - s
            if abs(e) < 1e-12 * abs(aii):
                e = aii
            einv[i] = 1.0 / e
    return einv


def lu_factor(Ad):
    """Partial pivoting (largest |value|, lowest row on ties); pivots <= 1e-12 * running max count as zero."""
    a = np.array(Ad, dtype=np.float64)
    n = a.shape[0]
    piv = np.zeros(n, np.int64)
    zero = np.zeros(n, bool)
    runmax = 0.0
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        pv = abs(a[p, k])
        runmax = max(runmax, pv)
        piv[k] = p
        zero[k] = pv <= 1e-12 * runmax
        if p != k:
            a[[k, p], :] = a[[p, k], :]
        if zero[k]:
            a[k + 1:, k] = 0.0
        else:
            a[k + 1:, k] /= a[k, k]
            a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    return a, piv, zero


def lu_solve(fac, b):
    a, piv, zero = fac
    x = np.array(b, dtype=np.float64)
    n = len(x)
    for k in range(n):
        p = piv[k]
        if p != k:
            x[k], x[p] = x[p], x[k]
    for k in range(n):
        x[k + 1:] -= a[k + 1:, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = 0.0 if zero[k] else x[k] / a[k, k]
        x[:k] -= a[:k, k] * x[k]
    return x


class Model:
    """V-cycle model over a given hierarchy: mats[l] (scipy CSR), aggs[l] (l < L-1), colors[l]."""

    def __init__(self, mats, aggs, colors, smoother="DILU", pre=0, post=3, omega=0.75, max_iters=1, fac=None):
        self.A = [m.tocsr() for m in mats]
        self.agg, self.col = aggs, colors
        self.jacobi = smoother == "JACOBI"
        self.pre, self.post, self.omega, self.max_iters = pre, post, omega, max_iters
        L = len(self.A)
        self.einv = []
        for l in range(L - 1):
            if self.jacobi:
                self.einv.append(1.0 / self.A[l].diagonal())
            else:
                self.einv.append(dilu_einv(self.A[l], self.col[l]))
        self.fac = fac if fac is not None else lu_factor(self.A[-1].toarray())

    def smooth(self, l, b, x):
        A, einv, om = self.A[l], self.einv[l], self.omega
        r = b - A @ x
        if self.jacobi:
            return x + om * einv * r
        col = self.col[l]
        rp, ci, v = A.indptr, A.indices, A.data
        w = np.zeros_like(x)
        nc = col.max() + 1
        for c in range(nc):                      # (E + L) y = r
            for i in np.nonzero(col == c)[0]:
                s = 0.0
                for k in range(rp[i], rp[i + 1]):
                    if col[ci[k]] < c:
                        s += v[k] * w[ci[k]]
                w[i] = (r[i] - s) * einv[i]
        for c in range(nc - 1, -1, -1):          # (E + U) z = E y
            for i in np.nonzero(col == c)[0]:
                s = 0.0
                for k in range(rp[i], rp[i + 1]):
                    if col[ci[k]] > c:
                        s += v[k] * w[ci[k]]
                w[i] = w[i] - einv[i] * s
        return x + om * w

    def vcycle(self, l, b):
        if l == len(self.A) - 1:
            return lu_solve(self.fac, b)
        x = np.zeros_like(b)
        for _ in range(self.pre):
            x = self.smooth(l, b, x)
        nc = self.A[l + 1].shape[0]
        rc = np.bincount(self.agg[l], weights=b - self.A[l] @ x, minlength=nc)
        x = x + self.vcycle(l + 1, rc)[self.agg[l]]
        for _ in range(self.post):
            x = self.smooth(l, b, x)
        return x

    def apply(self, r):
        z = self.vcycle(0, r)
        for _ in range(1, self.max_iters):
            z = z + self.vcycle(0, r - self.A[0] @ z)
        return z
