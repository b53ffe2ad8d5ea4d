"""numpy model of the matrix and preconditioner kernels of dedflow_amd/csrc/k_matrix.hip, k_dilu.hip and k_amg.hip: one
function per operation, with the launcher's argument meaning (include/dedflow_kernels.h), on host arrays, plus the
synthetic pattern and value generators of tests/test_gpu_matrix_kernels.py.  Test infrastructure only: no GPU, no import
of the library.

Layouts.  Block CSR over a nodal pattern (rp, ci): val[k*16 + r*4 + c], rows / columns 0..2 velocity, 3 pressure.
Vectors: [u: N x 3 AoS | p: N | tail].  Row-expanded scalar layout of a br x bc sub-matrix over the same nodal pattern
(csr_impl.cu:24-59): node row i (start s, length L) owns the L*br*bc values from s*br*bc on; scalar row ii of it holds
L*bc entries, entry kk*bc + jj for the kk-th nonzero.

Every operation takes a `dtype`: np.int64 (exact tier: inputs are small integers, the result is an integer below 2**53
in any order; exact power-of-two scalings are applied in float64 afterwards), np.longdouble (reference of the rounded
tier) or np.float64.  Operations return the values of the entries they own, as (index array, values) where the set is
not the whole array, so a test can tell "written" from "must stay".  The sums are numpy reductions over gathered
arrays: no lane mapping, no unrolling.
"""
import numpy as np

from krylov_model import EXTENDED_REASON, HAVE_EXTENDED, U  # noqa: F401  (re-exported)

F64, F32, LD, I64, I32 = np.float64, np.float32, np.longdouble, np.int64, np.int32

SPMV_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 100)
DIAG_LENS = tuple(L for L in SPMV_LENS if L >= 1)
ROW_COUNTS = (1, 7, 31, 32, 33, 255, 256, 257, 513)
CSR_LENS = (0, 1, 7, 8, 9, 17, 100)
AGG_SIZES = (1, 2, 3, 15, 16, 17, 33, 70)
COARSE_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 40)
DILU_LIST_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 13)
DILU_COLOR_SIZES = (1, 31, 32, 33)
VMAX = 2 ** 10  # |a|, |x| of the exact tier


def gamma(k):
    k = np.asarray(k, F64)
    return k * U / (1.0 - k * U)


def _conv(a, dtype):
    a = np.asarray(a)
    if dtype == I64:
        r = a.astype(I64)
        assert np.array_equal(r, a), "exact tier needs integer input"
        return r
    return a.astype(dtype)


# ======================================================================================================================
# patterns
# ======================================================================================================================
def cycle_lens(lens, nrows, seed, cap=None):
    """`lens`, rotated by the seed, cycled to nrows entries and shuffled; capped at `cap` (the column count)"""
    out = np.resize(np.roll(np.asarray(lens, I64), -(seed % len(lens))), nrows)
    np.random.default_rng(seed).shuffle(out)
    return np.minimum(out, cap) if cap is not None else out


def pattern(row_lens, ncols, seed, with_diag=False, ghost_from=None):
    """(rp, ci) with the given row lengths, sorted unique columns in [0, ncols); columns 0 and ncols-1 both occur when
    any row has two entries (or two rows have one).  with_diag: row i stores column i, as its first, its last or a middle
    entry in turn (i % 3) where the row allows it.  ghost_from = nrows < ncols: the shortest non-empty row that fits
    references only columns >= ghost_from."""
    rng = np.random.default_rng(seed)
    row_lens = np.asarray(row_lens, I64)
    nrows = row_lens.size
    assert row_lens.max(initial=0) <= ncols and (not with_diag or (row_lens.min() >= 1 and nrows <= ncols))
    ghost_row = -1
    if ghost_from is not None:
        fit = np.flatnonzero((row_lens >= 1) & (row_lens <= ncols - ghost_from))
        assert fit.size and not with_diag
        ghost_row = int(fit[np.argmin(row_lens[fit])])
    need0, need1 = True, True
    cols = []
    for i, L in enumerate(row_lens):
        L = int(L)
        if i == ghost_row:
            c = ghost_from + rng.choice(ncols - ghost_from, L, replace=False)
        elif with_diag:
            below, above, want = i, ncols - 1 - i, i % 3
            lo, hi = max(0, L - 1 - above), min(below, L - 1)
            if want == 0 and lo == 0:
                nb = 0
            elif want == 1 and hi == L - 1:
                nb = L - 1
            elif max(lo, 1) <= min(hi, L - 2):
                nb = int(rng.integers(max(lo, 1), min(hi, L - 2) + 1))
            else:
                nb = lo
            c = np.concatenate([rng.choice(below, nb, replace=False) if nb else np.zeros(0, I64), [i],
                                i + 1 + rng.choice(above, L - 1 - nb, replace=False) if L - 1 - nb else np.zeros(0, I64)])
        else:
            c = rng.choice(ncols, L, replace=False)
            forced = []
            if need0 and L >= 1:
                forced.append(0)
                need0 = False
            if need1 and L > len(forced) and ncols > 1:
                forced.append(ncols - 1)
                need1 = False
            if forced:
                rest = np.setdiff1d(c, forced)[: L - len(forced)]
                c = np.concatenate([forced, rest])
                if c.size < L:  # the draw already held a forced column
                    extra = np.setdiff1d(np.arange(ncols), c)
                    c = np.concatenate([c, rng.choice(extra, L - c.size, replace=False)])
        c = np.sort(np.asarray(c, I64))
        assert c.size == L and np.unique(c).size == L
        cols.append(c)
    rp = np.concatenate([[0], np.cumsum(row_lens)]).astype(I32)
    ci = (np.concatenate(cols) if cols else np.zeros(0)).astype(I32)
    return rp, ci


def row_of_nnz(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def diag_pos(rp, ci):
    """index of the stored diagonal of every row"""
    k = np.flatnonzero(ci == row_of_nnz(rp))
    assert k.size == rp.size - 1
    return k


def expand_pattern(rp, ci, bs):
    """scalar CSR whose rows / columns are node*bs + component (MatrixCSRAddElementLHSGPU)"""
    n = rp.size - 1
    rows = []
    for i in range(n):
        c = ci[rp[i]: rp[i + 1]].astype(I64)
        rows += [(c[:, None] * bs + np.arange(bs)).ravel()] * bs
    lens = np.array([r.size for r in rows], I64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(I32), np.concatenate(rows).astype(I32)


def elements_pattern(nel, nshl, N, seed, extra=3):
    """`nel` elements on disjoint node sets (conflict-free), a nodal pattern that holds every (row, col) pair of every
    element and `extra` more columns per row -- except ONE off-diagonal pair of element 0, which is absent.  Returns
    ien [nel*nshl], rp, ci, the absent (row, col)."""
    rng = np.random.default_rng(seed)
    assert nel * nshl <= N
    ien = rng.permutation(N)[: nel * nshl].astype(I32)
    adj = [set() for _ in range(N)]
    for e in range(nel):
        nodes = ien[e * nshl: (e + 1) * nshl]
        for a in nodes:
            adj[a].update(int(b) for b in nodes)
    absent = (int(ien[1]), int(ien[2]))
    for i in range(N):
        adj[i].update(int(c) for c in rng.choice(N, extra, replace=False))
    adj[absent[0]].discard(absent[1])
    lens = np.array([len(a) for a in adj], I64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(I32)
    ci = np.concatenate([np.sort(np.fromiter(a, I64, len(a))) for a in adj]).astype(I32)
    return ien, rp, ci, absent


# ---- symmetric pattern + greedy colouring + triangle lists (DILU) ----------------------------------------------------
def greedy_colors(nown, N, rp, ci):
    """first-fit in node order over the owned nodes; 255 = ghost (host/pc_dilu.c, header comment)"""
    color = np.full(N, 255, np.uint8)
    for i in range(nown):
        nb = ci[rp[i]: rp[i + 1]]
        nb = nb[(nb != i) & (nb < nown)]
        used = set(int(c) for c in color[nb] if c != 255)
        c = 0
        while c in used:
            c += 1
        color[i] = c
    return color


def dilu_lists(nown, rp, ci, color):
    """rows grouped by colour (ascending node index inside a colour), colour offsets, and per row slot the lists of the
    lower- and the higher-coloured owned neighbours as (ptr, nodal nonzero, column node), in row order"""
    ncol = int(color[:nown].max()) + 1 if nown else 0
    rows = np.argsort(color[:nown], kind="stable").astype(I32)
    coff = np.concatenate([[0], np.cumsum(np.bincount(color[:nown], minlength=ncol))]).astype(I32)
    out = []
    for lower in (True, False):
        ptr, nz, col = [0], [], []
        for i in rows:
            k = np.arange(rp[i], rp[i + 1])
            j = ci[k]
            ok = (j < nown) & (j != i)
            ok &= (color[j] < color[i]) if lower else (color[j] > color[i])
            nz.append(k[ok])
            col.append(j[ok])
            ptr.append(ptr[-1] + int(ok.sum()))
        out.append((np.array(ptr, I32), np.concatenate(nz).astype(I32) if nz else np.zeros(0, I32),
                    np.concatenate(col).astype(I32) if col else np.zeros(0, I32)))
    return rows, coff, out[0], out[1]


def dilu_pattern(seed, ncolors=20, sizes=None, nghost=0, nextra=400, nisolated=3):
    """A symmetric nodal pattern (diagonal stored) built around a target colouring that the greedy colouring reproduces:
    node i of target colour c is joined to one earlier node of every colour < c and to no node of colour c.  The first
    `ncolors` nodes form a clique (node k: colour k, exactly k lower neighbours), `nisolated` nodes have no neighbour at
    all, `nextra` random edges join nodes of different colours, `nghost` trailing nodes (not preconditioned, nown < N)
    are joined symmetrically to owned nodes.  Returns N, nown, rp, ci, target colours."""
    rng = np.random.default_rng(seed)
    if sizes is None:  # rows per colour: 33, 32, 31 and 257 (two blocks of the one-thread-per-row setup), 1 for the last
        sizes = [33, 32, 31, 257] + [int(s) for s in rng.integers(4, 9, ncolors - 5)] + [1]
    assert len(sizes) == ncolors
    assert sizes[0] > nisolated
    rest = np.concatenate([np.full(s - 1 - (nisolated if c == 0 else 0), c) for c, s in enumerate(sizes)])
    rng.shuffle(rest)
    target = np.concatenate([np.arange(ncolors), np.zeros(nisolated, I64), rest]).astype(I64)
    nown = target.size
    N = nown + nghost
    adj = [set([i]) for i in range(N)]
    by_color = [[] for _ in range(ncolors)]
    frozen = set(range(ncolors)) | set(range(ncolors, ncolors + nisolated))

    def join(a, b):
        adj[a].add(b)
        adj[b].add(a)

    for i in range(nown):
        c = int(target[i])
        if i < ncolors:
            for j in range(i):
                join(i, j)
        elif i >= ncolors + nisolated:
            for cc in range(c):
                cand = [j for j in by_color[cc] if j not in frozen]
                join(i, int(rng.choice(cand)) if cand else cc)
            by_color[c].append(i)
    free = np.array([i for i in range(nown) if i not in frozen])
    for _ in range(nextra):
        a, b = (int(v) for v in rng.choice(free, 2, replace=False))
        if target[a] != target[b]:
            join(a, b)
    # two rows with at least 9 neighbours on either side
    side = min(9, (ncolors - 1) // 2)
    mid = [i for i in free if side <= target[i] <= ncolors - 1 - side][:2]
    assert len(mid) == 2
    for i in mid:
        for cc in range(int(target[i]) + 1, ncolors):
            cand = [j for j in free if target[j] == cc]
            join(int(i), int(rng.choice(cand)) if cand else cc)
    for g in range(nown, N):
        for j in rng.choice(free, 3, replace=False):
            join(g, int(j))
    lens = np.array([len(a) for a in adj], I64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(I32)
    ci = np.concatenate([np.sort(np.fromiter(a, I64, len(a))) for a in adj]).astype(I32)
    full = np.full(N, 255, np.uint8)
    full[:nown] = target
    return N, nown, rp, ci, full


def aggregates(sizes, seed):
    """node lists of aggregates of the given sizes over a shuffled node set: aoff, anode, agg (node -> aggregate)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, I64)
    N = int(sizes.sum())
    anode = rng.permutation(N).astype(I32)
    aoff = np.concatenate([[0], np.cumsum(sizes)]).astype(I32)
    agg = np.empty(N, I32)
    agg[anode] = np.repeat(np.arange(sizes.size), sizes)
    return aoff, anode, agg


def coarse_lists(lens, nnz_fine, seed):
    """off / idx of dfl_amg_galerkin: list cz holds lens[cz] fine nonzeros (each fine nonzero in at most one list)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, I64)
    assert lens.sum() <= nnz_fine
    idx = rng.permutation(nnz_fine)[: lens.sum()].astype(I32)
    return np.concatenate([[0], np.cumsum(lens)]).astype(I32), idx


# ======================================================================================================================
# values
# ======================================================================================================================
def ints(rng, n, vmax=VMAX):
    """integers of [-vmax, vmax] as float64; both extremes occur when n >= 2"""
    v = rng.integers(-vmax, vmax + 1, n).astype(F64)
    if n >= 2:
        v[rng.choice(n, 2, replace=False)] = (vmax, -vmax)
    return v


def unimodular3(rng, n, steps=6):
    """n integer 3x3 matrices of determinant +-1: products of elementary integer matrices (shears by -2..2, a row swap,
    a sign flip), entries kept below 2**10"""
    out = np.empty((n, 3, 3), I64)
    for b in range(n):
        while True:
            m = np.eye(3, dtype=I64)
            for _ in range(steps):
                e = np.eye(3, dtype=I64)
                kind = rng.integers(0, 4)
                i, j = rng.choice(3, 2, replace=False)
                if kind <= 1:
                    e[i, j] = rng.integers(-2, 3)
                elif kind == 2:
                    e[[i, j]] = e[[j, i]]
                else:
                    e[i, i] = -1
                m = e @ m
            if np.abs(m).max() <= VMAX and np.abs(adjugate3(m[None])[0]).max() <= VMAX:
                break
        out[b] = m
    return out


def signed_perm_pow2_4(rng, n):
    """n 4x4 matrices P * D: a signed permutation times powers of two 2**-2 .. 2**3 -- the exact inverse is D^-1 P^T"""
    out = np.zeros((n, 4, 4), F64)
    for b in range(n):
        p = rng.permutation(4)
        out[b, np.arange(4), p] = rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.integers(-2, 4, 4)
    return out


def dominant_blocks(rng, n, m):
    """n diagonally dominant m x m blocks of normal data: |a_ii| = 2 * sum_{j != i} |a_ij| + 0.5 and every row scaled
    to the same absolute sum, so ||A|| ||A^-1|| <= (|a_ii| + off) / (|a_ii| - off) <= 3 in the infinity norm (the CPU test
    computes it: <= 10); a random scale per block on top"""
    a = rng.normal(size=(n, m, m))
    d = np.arange(m)
    off = np.abs(a).sum(axis=2) - np.abs(a[:, d, d])
    a[:, d, d] = np.where(rng.random((n, m)) < 0.5, -1.0, 1.0) * (2.0 * off + 0.5)
    a /= np.abs(a).sum(axis=2, keepdims=True)
    return a * (0.5 + 1.5 * rng.random((n, 1, 1)))


def dyadic(rng, n, k=2, vmax=8):
    """integers of [-vmax, vmax] over 2**k"""
    return rng.integers(-vmax, vmax + 1, n).astype(F64) / 2.0 ** k


def tier_a_blocks(rng, rp, ci, with_diag):
    """integer block values; with_diag: unimodular velocity diagonal blocks and a power-of-two A_pp on the diagonal"""
    nnz = ci.size
    val = ints(rng, 16 * nnz).reshape(nnz, 4, 4)
    if with_diag:
        kd = diag_pos(rp, ci)
        val[kd, :3, :3] = unimodular3(rng, kd.size)
        val[kd, 3, 3] = rng.choice([-1.0, 1.0], kd.size) * 2.0 ** rng.integers(-3, 6, kd.size)
    return val.reshape(-1)


def tier_b_blocks(rng, rp, ci, with_diag):
    nnz = ci.size
    val = rng.normal(size=(nnz, 4, 4))
    if with_diag:
        kd = diag_pos(rp, ci)
        val[kd, :3, :3] = dominant_blocks(rng, kd.size, 3)
        val[kd, 3, 3] = np.where(rng.random(kd.size) < 0.5, -1.0, 1.0) * (0.5 + rng.random(kd.size))
    return val.reshape(-1)


def dilu_values(rng, N, rp, ci, exact):
    """block values of a DILU case.  exact: integers off the diagonal, signed-permutation-times-power-of-two diagonal
    blocks (their inverse is exact).  Otherwise normal data scaled so that every 4x4 block row is dominated by its
    diagonal block, itself diagonally dominant: E stays well conditioned through the colours."""
    nnz = ci.size
    kd = diag_pos(rp, ci)
    if exact:
        val = ints(rng, 16 * nnz).reshape(nnz, 4, 4)
        val[kd] = signed_perm_pow2_4(rng, N)
        return val.reshape(-1)
    val = rng.normal(size=(nnz, 4, 4)) * (0.25 / np.maximum(np.diff(rp), 1))[row_of_nnz(rp), None, None]
    val[kd] = dominant_blocks(rng, N, 4)
    return val.reshape(-1)


# ======================================================================================================================
# small dense helpers
# ======================================================================================================================
def adjugate3(m):
    """adjugate of [n,3,3] by cross products of the rows: column j of adj(m) = row_{j+1} x row_{j+2}"""
    r0, r1, r2 = m[:, 0], m[:, 1], m[:, 2]
    return np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], axis=2)


def inv3(m, dtype):
    """inverse of [n,3,3].  int64: the blocks are unimodular, adj / det is an integer matrix"""
    m = _conv(m, dtype)
    adj = adjugate3(m)
    det = (m[:, 0] * adj[:, :, 0]).sum(axis=1)
    if dtype == I64:
        assert np.all(np.abs(det) == 1)
        return adj * det[:, None, None]
    return adj / det[:, None, None]


def inv_gj(a, dtype):
    """inverse of [n,m,m] by Gauss-Jordan elimination with partial pivoting in `dtype` (float64: the restatement the
    constant c of the inverse budgets is measured on; longdouble: the reference inverse)"""
    a = np.array(a, dtype)
    n, m = a.shape[0], a.shape[1]
    b = np.broadcast_to(np.eye(m, dtype=dtype), a.shape).copy()
    ar = np.arange(n)
    for c in range(m):
        p = c + np.argmax(np.abs(a[:, c:, c]), axis=1)
        for x in (a, b):
            t = x[ar, p].copy()
            x[ar, p] = x[ar, c]
            x[ar, c] = t
        ip = dtype(1) / a[:, c, c]
        a[:, c] *= ip[:, None]
        b[:, c] *= ip[:, None]
        for r in range(m):
            if r != c:
                f = a[:, r, c].copy()
                a[:, r] -= f[:, None] * a[:, c]
                b[:, r] -= f[:, None] * b[:, c]
    return b


def inv3_closed_f64(m):
    """the closed form (cofactors over the determinant, one reciprocal) in float64 numpy"""
    m = np.asarray(m, F64)
    adj = adjugate3(m)
    det = (m[:, 0] * adj[:, :, 0]).sum(axis=1)
    return adj * (1.0 / det)[:, None, None]


def kappa_inf(a, ainv):
    n = lambda x: np.abs(x).sum(axis=-1).max(axis=-1)
    return n(np.asarray(a, LD)) * n(np.asarray(ainv, LD))


def inverse_budget(c, a, ainv):
    """c * u * kappa_inf(block) * max|inverse| per block"""
    return c * U * np.asarray(kappa_inf(a, ainv), F64) * np.abs(np.asarray(ainv, F64)).max(axis=(-1, -2))


# ======================================================================================================================
# vectors
# ======================================================================================================================
def vec_idx(nodes, N):
    """[len(nodes), 4] positions of (u0, u1, u2, p) of the nodes in the [u AoS | p] layout"""
    nodes = np.asarray(nodes, I64)
    return np.stack([3 * nodes, 3 * nodes + 1, 3 * nodes + 2, 3 * N + nodes], axis=1)


def node4(x, N, dtype, nodes=None):
    """x as [N, 4] node values (only `nodes` are converted; the others are zero: they may hold anything)"""
    nodes = np.arange(N) if nodes is None else np.unique(nodes)
    out = np.zeros((N, 4), dtype)
    out[nodes] = _conv(np.asarray(x)[vec_idx(nodes, N)], dtype)
    return out


def interleave4(node0, node1, N, x):
    """rows [node0, node1) of x4[node][4] = (u0, u1, u2, p): pure copy"""
    nodes = np.arange(node0, max(node0, node1))
    return (4 * nodes[:, None] + np.arange(4)).ravel(), np.asarray(x)[vec_idx(nodes, N)].ravel()


# ======================================================================================================================
# SpMV family
# ======================================================================================================================
def _row_sums(terms, rp, rows):
    """sum of terms[rp[i]:rp[i+1]] for i in rows (terms: [nnz, ...]); an empty row gives zero"""
    full = np.zeros((rp.size - 1,) + terms.shape[1:], terms.dtype)
    np.add.at(full, row_of_nnz(rp), terms)
    return full[rows]


def bcsr_spmv(rows, N, rp, ci, val, alpha, x, beta, y, dtype, absolute=False):
    """(idx [nr,4], values [nr,4]) of y = alpha A x + beta y on the node rows `rows` (dfl_bcsr_spmv / _rows / _range,
    _x4 and _f32 with alpha = 1, beta = 0).  beta == 0: y is not read.  absolute: |alpha| |A| |x| + |beta| |y| instead
    (the scale of the a-priori bound)."""
    rows = np.asarray(rows, I64)
    rp = np.asarray(rp, I64)
    keep = np.zeros(rp.size - 1, bool)
    keep[rows] = True
    knz = keep[row_of_nnz(rp)]
    v = np.zeros((ci.size, 4, 4), dtype)
    v[knz] = _conv(np.asarray(val).reshape(-1, 4, 4)[knz], dtype)
    X = node4(x, N, dtype, ci[knz])
    if absolute:
        v, X = np.abs(v), np.abs(X)
    sums = _row_sums((v * X[ci][:, None, :]).sum(axis=2), rp, rows)
    idx = vec_idx(rows, N)
    return idx, _axpby(alpha, sums, beta, None if beta == 0 else np.asarray(y)[idx], dtype, absolute)


def _axpby(alpha, s, beta, y, dtype, absolute):
    """alpha s + beta y (y None: alpha s).  int64: the integer sums are combined in float64, where every operand and
    result is exact, so that the sign of a zero is the device's: alpha * (+0) keeps the sign of alpha"""
    ft = F64 if dtype == I64 else dtype
    if absolute:
        alpha, beta = abs(alpha), abs(beta)
    out = ft(alpha) * s.astype(ft)
    if y is not None:
        yv = _conv(y, dtype).astype(ft)
        out = out + ft(beta) * (np.abs(yv) if absolute else yv)
    return out


def spmv_bound(rows, N, rp, ci, val, alpha, x, beta, y):
    """gamma_k (|alpha| sum |a||x| + |beta||y_i|), k = 4 len + 3: holds for every summation order (Higham 3.1)"""
    _, s = bcsr_spmv(rows, N, rp, ci, val, alpha, x, beta, y, LD if HAVE_EXTENDED else F64, absolute=True)
    k = 4 * np.diff(rp)[np.asarray(rows, I64)] + 3
    return gamma(k)[:, None] * s.astype(F64)


def csr_spmv(nrow, rp, ci, val, alpha, x, beta, y, dtype, absolute=False):
    v, xv = _conv(val, dtype), _conv(np.asarray(x)[ci], dtype) if ci.size else np.zeros(0, dtype)
    if absolute:
        v, xv = np.abs(v), np.abs(xv)
    sums = _row_sums(v * xv, np.asarray(rp, I64), np.arange(nrow))
    return _axpby(alpha, sums, beta, None if beta == 0 else np.asarray(y)[:nrow], dtype, absolute)


def csr_jacobi(n, data, rp, ci, x, dtype):
    """(rows with a stored diagonal, x_i / a_ii); the other rows are left untouched.  int64: a_ii is a power of two"""
    rows = row_of_nnz(rp)
    k = np.flatnonzero((ci == rows) & (rows < n))
    i = rows[k]
    if dtype == I64:
        assert np.all(np.frexp(np.abs(np.asarray(data)[k]))[0] == 0.5)
        return i, _conv(np.asarray(x)[i], I64).astype(F64) / np.asarray(data, F64)[k]
    return i, _conv(np.asarray(x)[i], dtype) / _conv(np.asarray(data)[k], dtype)


def values_to_f32(n, val):
    return np.asarray(val[:n], F64).astype(F32)


# ======================================================================================================================
# Jacobi tree
# ======================================================================================================================
def pc_setup(nrows, rp, ci, val, dtype):
    """(dinv33 [nrows*9]: inv(D) row-major per node, dinv1 [nrows]: 1 / A_pp)"""
    b = np.asarray(val).reshape(-1, 4, 4)[diag_pos(rp, ci)[:nrows]]
    app = b[:, 3, 3]
    if dtype == I64:
        assert np.all(np.frexp(np.abs(app))[0] == 0.5)
        d1 = 1.0 / app
    else:
        d1 = dtype(1) / _conv(app, dtype)
    return inv3(b[:, :3, :3], dtype).reshape(-1), d1


def block3_apply(N, dinv33, x, dtype):
    """y_node = A x_node with A the COLUMN-major reading of the 9 stored numbers: A(r, c) = image[r + 3c]"""
    A = _conv(np.asarray(dinv33)[: 9 * N], dtype).reshape(N, 3, 3).transpose(0, 2, 1)
    return (A * _conv(np.asarray(x)[: 3 * N], dtype).reshape(N, 1, 3)).sum(axis=2).reshape(-1)


def pc_apply(nrows, N, n, dinv33, dinv1, x, nrm, dtype, absolute=False):
    """dfl_pc_jacobi_apply[_scaled][_rows][_x4].  nrm None: unscaled.  Returns dict of (idx, values): 'q' (the scaled
    input, scaled form only), 'y', 'y4' (rows [0, nrows) interleaved), each over the owned rows and the tail [4N, n).
    int64: dinv1 and nrm are powers of two and applied in float64."""
    x = np.asarray(x)
    rows = np.arange(nrows)
    idx = vec_idx(rows, N)
    tail = np.arange(4 * N, max(n, 4 * N))
    exact = dtype == I64
    xs = _conv(x[idx], dtype)
    xt = _conv(x[tail], dtype)
    A = _conv(np.asarray(dinv33)[: 9 * nrows], dtype).reshape(nrows, 3, 3).transpose(0, 2, 1)
    if absolute:
        xs, A = np.abs(xs), np.abs(A)
    if exact:
        s = 1.0 if nrm is None else 1.0 / float(nrm)
        assert np.frexp(s)[0] == 0.5 and np.all(np.frexp(np.abs(np.asarray(dinv1)[:nrows]))[0] == 0.5)
        yu = (A * xs[:, None, :3]).sum(axis=2).astype(F64) * s
        yp = xs[:, 3].astype(F64) * s * np.asarray(dinv1, F64)[:nrows]
        q, qt = xs.astype(F64) * s, xt.astype(F64) * s
    else:
        s = dtype(1) if nrm is None else dtype(1) / dtype(nrm)
        q, qt = xs * s, xt * s
        yu = (A * q[:, None, :3]).sum(axis=2)
        d1 = _conv(np.asarray(dinv1)[:nrows], dtype)
        yp = q[:, 3] * (np.abs(d1) if absolute else d1)
    y = np.concatenate([yu, yp[:, None]], axis=1)
    out = {"y": (np.concatenate([idx.ravel(), tail]), np.concatenate([y.ravel(), qt])),
           "y4": (np.arange(4 * nrows), y.ravel())}
    if nrm is not None:
        out["q"] = (np.concatenate([idx.ravel(), tail]), np.concatenate([q.ravel(), qt]))
    return out


def get_diag(N, rp, ci, val):
    """(d33 [N*9] row-major velocity diagonal block, dp [N] = A_pp, du [N*3] its velocity diagonal): pure copies"""
    b = np.asarray(val).reshape(-1, 4, 4)[diag_pos(rp, ci)[:N]]
    return b[:, :3, :3].reshape(-1), b[:, 3, 3].copy(), b[:, [0, 1, 2], [0, 1, 2]].reshape(-1)


def csr_get_diag(val, rp, ci, nrow):
    return np.asarray(val)[diag_pos(rp, ci)[:nrow]]


def expanded_index(rp, br, bc):
    """index [nnz, br, bc] of block entry (ii, jj) of nodal nonzero k in the row-expanded layout"""
    rp = np.asarray(rp, I64)
    rows = row_of_nnz(rp)
    start, L = rp[:-1][rows], np.diff(rp)[rows]
    kk = np.arange(rows.size) - start
    return (start * br * bc)[:, None, None] + np.arange(br)[None, :, None] * (L * bc)[:, None, None] \
        + (kk * bc)[:, None, None] + np.arange(bc)[None, None, :]


def get_diag_block(matval, bs, nrow, rp, ci, lda, stride):
    """(idx, values) of out[i*stride + ii*lda + jj] = diagonal block (ii, jj) of node row i"""
    src = expanded_index(rp, bs, bs)[diag_pos(rp, ci)[:nrow]]
    dst = np.arange(nrow)[:, None, None] * stride + np.arange(bs)[None, :, None] * lda + np.arange(bs)[None, None, :]
    return dst.ravel(), np.asarray(matval)[src].ravel()


# ======================================================================================================================
# Dirichlet
# ======================================================================================================================
def zero_rows(N, rp, ci, val, bnode, comp, diag):
    """row `comp` of every block of the node rows bnode (entries outside [0, N) skipped) <- 0, diag on the diagonal"""
    out = np.array(val, F64).reshape(-1, 4, 4)
    for node in bnode:
        if 0 <= node < N:
            k = np.arange(rp[node], rp[node + 1])
            out[k, comp, :] = 0.0
            out[k[ci[k] == node], comp, comp] = diag
    return out.reshape(-1)


def zero_scalar_rows(N, rp, ci, val, row, shift, diag):
    """the same for scalar rows node*3 + comp = row[i] + shift; rows outside [0, 3N) skipped"""
    out = np.asarray(val, F64)
    for r in np.asarray(row, I64) + shift:
        if 0 <= r < 3 * N:
            out = zero_rows(N, rp, ci, out, [r // 3], int(r % 3), diag)
    return out


def csr_zero_row(matval, num_row, rp, ci, row, shift, diag):
    out = np.array(matval, F64)
    for r in np.asarray(row, I64) + shift:
        if 0 <= r < num_row:
            k = np.arange(rp[r], rp[r + 1])
            out[k] = diag * (ci[k] == r).astype(F64)  # (a negative diag leaves -0.0 off the diagonal, as in the reference)
    return out


def dirichlet_vec(b, bnode, shape, comp):
    out = np.array(b, F64)
    out[np.asarray(bnode, I64) * shape + comp] = 0.0
    return out


# ======================================================================================================================
# layout
# ======================================================================================================================
def export_fs(N, rp, val):
    """the four row-expanded sub-matrix arrays (A00 3x3, A01 3x1, A10 1x3, A11 1x1) of the block values"""
    v = np.asarray(val).reshape(-1, 4, 4)
    out = []
    for r0, br, c0, bc in ((0, 3, 0, 3), (0, 3, 3, 1), (3, 1, 0, 3), (3, 1, 3, 1)):
        a = np.empty(v.shape[0] * br * bc, v.dtype)
        a[expanded_index(rp, br, bc)] = v[:, r0: r0 + br, c0: c0 + bc]
        out.append(a)
    return out


# ======================================================================================================================
# scatter launchers (exact tier only)
# ======================================================================================================================
def _find(rp, ci, row, col):
    k = rp[row] + np.flatnonzero(ci[rp[row]: rp[row + 1]] == col)
    return int(k[0]) if k.size else -1


def elem_scatter(target, index, alpha, nshl, batch_size, batch_index, ien, rp, ci, br, bc, val, lda, stride, beta, mask):
    """m = alpha m + beta b for the br x bc block of every (batch slot, a, b) whose (row, col) is in the pattern and
    whose slot is not masked out; b starts at val[(slot*nshl*nshl + a*nshl + b) * stride], row stride lda.
    `index` [nnz, br, bc]: where block entry (ii, jj) of nonzero k lives in `target`."""
    out = _conv(target, I64).copy()
    val = np.asarray(val)
    for slot in range(batch_size):
        if mask is not None and mask[slot] == 0:
            continue
        iel = slot if batch_index is None else int(batch_index[slot])
        for a in range(nshl):
            for b in range(nshl):
                k = _find(rp, ci, int(ien[iel * nshl + a]), int(ien[iel * nshl + b]))
                if k < 0:
                    continue
                base = (slot * nshl * nshl + a * nshl + b) * stride
                src = base + np.arange(br)[:, None] * lda + np.arange(bc)[None, :]
                out[index[k]] = int(alpha) * out[index[k]] + int(beta) * _conv(val[src], I64)
    return out


def csr_set_blocked(matval, alpha, rp, ci, brow, bcol, br, bc, A, beta, lda, stride):
    out = _conv(matval, I64).copy()
    index = expanded_index(rp, br, bc)
    for t in range(len(brow)):
        k = _find(rp, ci, int(brow[t]), int(bcol[t]))
        if k >= 0:
            src = t * stride + np.arange(br)[:, None] * lda + np.arange(bc)[None, :]
            out[index[k]] = int(beta) * _conv(np.asarray(A)[src], I64) + int(alpha) * out[index[k]]
    return out


def csr_add_element_lhs(matval, nshl, bs, rp, ci, batch_size, batch_ptr, ien, val):
    """scalar CSR over node*bs + component; element `slot` adds its dense (nshl*bs)^2 block, row-major, stored at
    val[slot * (nshl*bs)^2]; pairs absent from the pattern are dropped"""
    out = _conv(matval, I64).copy()
    m = nshl * bs
    for slot in range(batch_size):
        iel = slot if batch_ptr is None else int(batch_ptr[slot])
        dof = (np.asarray(ien[iel * nshl: (iel + 1) * nshl], I64)[:, None] * bs + np.arange(bs)).ravel()
        blk = _conv(np.asarray(val)[slot * m * m: (slot + 1) * m * m], I64).reshape(m, m)
        for a in range(m):
            for b in range(m):
                k = _find(rp, ci, int(dof[a]), int(dof[b]))
                if k >= 0:
                    out[k] += blk[a, b]
    return out


# ======================================================================================================================
# DILU
# ======================================================================================================================
def dilu_setup(N, nown, rp, ci, val, color, rows, coff, dtype):
    """E_i^-1 of every owned row, colour by colour: E_i = A_ii - sum_{j ~ i owned, colour(j) < colour(i)} A_ij E_j^-1 A_ji.
    Returns Einv [N,4,4] (ghost rows zero).  longdouble / float64 only."""
    v = np.asarray(val).reshape(-1, 4, 4).astype(dtype)
    kd = diag_pos(rp, ci)
    Einv = np.zeros((N, 4, 4), dtype)
    for c in range(coff.size - 1):
        rc = rows[coff[c]: coff[c + 1]]
        E = v[kd[rc]].copy()
        for t, i in enumerate(rc):
            for k in range(rp[i], rp[i + 1]):
                j = ci[k]
                if j < nown and color[j] < color[i]:
                    E[t] -= v[k] @ Einv[j] @ v[_find(rp, ci, j, i)]
        Einv[rc] = inv_gj(E, dtype)
    return Einv


def exact_inverse_perm4(blocks):
    """inverse of signed-permutation-times-power-of-two blocks: transpose with every nonzero replaced by its reciprocal"""
    b = np.asarray(blocks, F64)
    assert np.all((b != 0).sum(axis=2) == 1) and np.all((b != 0).sum(axis=1) == 1)
    with np.errstate(divide="ignore"):
        return np.where(b != 0, 1.0 / b, 0.0).transpose(0, 2, 1)


def dilu_sweep(forward, slot0, nrows_c, rows, N, eptr, enz, ecol, val, Einv, r, z, dtype, einv_shift=0, zerr=None):
    """one colour of a triangular sweep on the row slots [slot0, slot0 + nrows_c):
         forward:  z_i = E_i^-1 (r_i - sum_list A_ij z_j)        backward: z_i -= E_i^-1 sum_list A_ij z_j
    Returns (idx [nr,4], values [nr,4], bound [nr,4]).  int64: Einv = integers / 2**einv_shift, applied exactly.
    bound (rounded tier) = gamma_k (|E^-1| (S + sum |a| e_j) + [backward] (|z_i| + e_i)) + |E^-1| sum |a| e_j
    + [backward] e_i with S = [forward] |r_i| + sum |a||z_j|, k = 4 len + 7 and e = zerr the bound on the error the
    input z already carries (None: zero): 4 len + 1 operations for t = r - sum, 4 + 1 for the E^-1 product, one for the
    subtraction from z, and gamma_j + gamma_k + gamma_j gamma_k <= gamma_{j+k}."""
    sl = np.arange(slot0, slot0 + nrows_c)
    rw = np.asarray(rows, I64)[sl]
    idx = vec_idx(rw, N)
    lens = np.diff(np.asarray(eptr, I64))[sl]
    q = np.concatenate([np.arange(eptr[s], eptr[s + 1]) for s in sl]) if sl.size else np.zeros(0, I64)
    q = q.astype(I64)
    owner = np.repeat(np.arange(sl.size), lens)
    a = _conv(np.asarray(val).reshape(-1, 4, 4)[enz[q]], dtype)
    Z = node4(z, N, dtype, ecol[q] if forward else np.concatenate([ecol[q], rw]))  # forward: z_i itself is not read
    zj = Z[ecol[q]]
    acc = np.zeros((sl.size, 4), dtype)
    np.add.at(acc, owner, (a * zj[:, None, :]).sum(axis=2))
    exact = dtype == I64
    if exact:
        Ei = _conv(np.asarray(Einv).reshape(-1, 4, 4)[rw] * 2.0 ** einv_shift, I64)
    else:
        Ei = _conv(np.asarray(Einv).reshape(-1, 4, 4)[rw], dtype)
    t = (_conv(np.asarray(r)[idx], dtype) - acc) if forward else acc
    part = (Ei * t[:, None, :]).sum(axis=2)
    if exact:
        part = part.astype(F64) / 2.0 ** einv_shift
        return idx, (part if forward else Z[rw].astype(F64) - part), None
    out = part if forward else Z[rw] - part
    # the bound
    S = np.zeros((sl.size, 4), dtype)
    np.add.at(S, owner, (np.abs(a) * np.abs(zj)[:, None, :]).sum(axis=2))
    prop = np.zeros((sl.size, 4), dtype)
    ei = np.zeros((sl.size, 4), dtype)
    if zerr is not None:
        np.add.at(prop, owner, (np.abs(a) * np.asarray(zerr, dtype)[ecol[q]][:, None, :]).sum(axis=2))
        ei = np.asarray(zerr, dtype)[rw]
    if forward:
        S = S + np.abs(_conv(np.asarray(r)[idx], dtype))
    aE = np.abs(Ei)
    g = gamma(4 * lens + 7)[:, None]
    mul = lambda w: (aE * w[:, None, :]).sum(axis=2)
    bound = g * mul(S + prop) + mul(prop)
    if not forward:
        bound = bound + g * (np.abs(Z[rw]) + ei) + ei
    return idx, out, bound.astype(F64)


def dilu_apply(N, nown, rows, coff, low, up, val, Einv, r, dtype, valf=None):
    """z = M^-1 r: forward sweep over the colours ascending, backward descending.  Returns z [N,4] (owned rows) and the
    propagated a-priori bound on the error of a float64 run of the same sweeps."""
    z = np.zeros(4 * N, dtype)
    zerr = np.zeros((N, 4), F64)
    v = val if valf is None else np.asarray(valf, F64)
    nc = coff.size - 1
    for fwd, lists, order in ((1, low, range(nc)), (0, up, range(nc - 1, -1, -1))):
        for c in order:
            idx, out, b = dilu_sweep(fwd, coff[c], coff[c + 1] - coff[c], rows, N, lists[0], lists[1], lists[2], v, Einv,
                                     r, z, dtype, zerr=zerr)
            z[idx] = out
            zerr[rows[coff[c]: coff[c + 1]]] = b
    return z, zerr


def dilu_dense_apply(N, nown, rp, ci, val, color, r4):
    """independent restatement for the CPU test: M = (E + L) E^-1 (E + U) as a dense 4 nown x 4 nown matrix in node order
    (E by the recurrence on dense blocks), z = solve(M, r); float64"""
    A = np.zeros((nown, nown, 4, 4))
    v = np.asarray(val, F64).reshape(-1, 4, 4)
    for i in range(nown):
        for k in range(rp[i], rp[i + 1]):
            if ci[k] < nown:
                A[i, ci[k]] = v[k]
    E = np.zeros((nown, 4, 4))
    for i in np.argsort(color[:nown], kind="stable"):
        E[i] = A[i, i]
        for j in range(nown):
            if j != i and color[j] < color[i] and np.any(A[i, j]):
                E[i] -= A[i, j] @ np.linalg.inv(E[j]) @ A[j, i]
    lower = (color[:nown, None] > color[None, :nown])
    upper = (color[:nown, None] < color[None, :nown])
    big = lambda blocks: blocks.transpose(0, 2, 1, 3).reshape(4 * nown, 4 * nown)
    Ed = np.zeros_like(A)
    Ed[np.arange(nown), np.arange(nown)] = E
    EL, EU = big(Ed + A * lower[:, :, None, None]), big(Ed + A * upper[:, :, None, None])
    M = EL @ np.linalg.inv(big(Ed)) @ EU
    return np.linalg.solve(M, np.asarray(r4, F64)[:nown].reshape(-1)).reshape(nown, 4), E


# ======================================================================================================================
# two-level transfer
# ======================================================================================================================
def _list_sums(off, terms):
    out = np.zeros((off.size - 1,) + terms.shape[1:], terms.dtype)
    np.add.at(out, np.repeat(np.arange(off.size - 1), np.diff(off)), terms)
    return out


def galerkin(nnzc, off, idx, vf, dtype, absolute=False):
    """vc[cz] = sum of the fine blocks of list cz, [nnzc, 16]; an empty list gives +0"""
    t = _conv(np.asarray(vf).reshape(-1, 16)[idx[: off[nnzc]]], dtype)
    return _list_sums(np.asarray(off[: nnzc + 1], I64), np.abs(t) if absolute else t)


def restrict_diff(Nc, aoff, anode, N, r, sub, dtype, absolute=False):
    """rc (coarse layout [u: Nc x 3 | p: Nc]) = sum over the nodes of every aggregate of r - sub"""
    nodes = anode[: aoff[Nc]]
    d = node4(r, N, dtype, nodes)[nodes] - node4(sub, N, dtype, nodes)[nodes]
    s = _list_sums(np.asarray(aoff[: Nc + 1], I64), np.abs(d) if absolute else d)
    return vec_idx(np.arange(Nc), Nc), s


def prolong_add(nrows, N, agg, Nc, xc, z, dtype):
    """z_i += xc[agg[i]] on the rows [0, nrows)"""
    rows = np.arange(nrows)
    idx = vec_idx(rows, N)
    return idx, _conv(np.asarray(z)[idx], dtype) + _conv(np.asarray(xc)[vec_idx(agg[:nrows], Nc)], dtype)


# ======================================================================================================================
# inputs of the device tests (shared with the CPU test, which proves the integer range on exactly these)
# ======================================================================================================================
def values(rng, n, exact):
    return ints(rng, n) if exact else rng.normal(size=n)


SPMV_CASES = [(nr, nr) for nr in ROW_COUNTS] + [(nr, (max(nr, 100) + 38) | 1) for nr in ROW_COUNTS]  # (nrows, N)


def spmv_inputs(nrows, N, seed, exact, lens=SPMV_LENS):
    """rp, ci, val [16 nnz], x [4N], y [4N] of an SpMV case; N > nrows: ghost columns, one row references only ghosts"""
    rp, ci = pattern(cycle_lens(lens, nrows, seed, cap=N), N, seed + 1, ghost_from=nrows if N > nrows else None)
    rng = np.random.default_rng(seed + 2)
    return rp, ci, values(rng, 16 * ci.size, exact), values(rng, 4 * N, exact), values(rng, 4 * N, exact)


def diag_inputs(N, seed, exact, lens=DIAG_LENS):
    """square pattern with a stored diagonal (first / last / middle entry) and block values with invertible diagonals"""
    rp, ci = pattern(cycle_lens(lens, N, seed, cap=N), N, seed + 1, with_diag=True)
    rng = np.random.default_rng(seed + 2)
    return rp, ci, (tier_a_blocks if exact else tier_b_blocks)(rng, rp, ci, True)
