"""CPU checks of tests/matrix_model.py, the numpy model and the input generators the matrix-kernel tests
(tests/test_gpu_matrix_kernels.py) compare the device with:

  (1) the integer range of the exact tier, from the longest row and the largest magnitudes the generators actually
      give: every product and partial sum of every exact case stays an integer (or a dyadic rational with an integer
      numerator) below 2**53, the condition under which the device tests may demand bitwise equality whatever the
      kernel's order of summation or FMA contraction;
  (2) every model against an independent dense or scipy.sparse computation;
  (3) the promises of the generators: the row lengths hit, first / last / middle diagonals within one case, the
      ghost-only row, symmetry and validity of the DILU colouring, the residues of the list lengths;
  (4) the int64 and the longdouble model agree exactly on exact-tier inputs;
  (5) the condition numbers of the rounded-tier blocks, computed in longdouble: <= 10;
  (6) mutations on the model side: the inputs can tell a dropped last entry of a length-17 row, or a swapped (u2, p)
      pair, from the right answer.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import matrix_model as M

F64, LD, I64 = np.float64, np.longdouble, np.int64
LIMIT = 2.0 ** 53
needs_extended = pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON)


def dense_block_matrix(nrows, N, rp, ci, val):
    """the (u,p) operator as a dense [4 nrows, 4 N] matrix in the vector layout [u AoS | p]"""
    A = np.zeros((4 * nrows, 4 * N))
    v = np.asarray(val, F64).reshape(-1, 4, 4)
    for i in range(nrows):
        for k in range(rp[i], rp[i + 1]):
            A[np.ix_(M.vec_idx([i], nrows)[0], M.vec_idx([ci[k]], N)[0])] = v[k]
    return A


# ---- (1) the integer range ---------------------------------------------------------------------------------------------
def test_exact_tier_stays_below_2_to_53():
    worst = 0.0
    for nrows, N in M.SPMV_CASES:
        for seed in (1000, 2000, 3000):
            rp, ci, val, x, y = M.spmv_inputs(nrows, N, seed + nrows, True)
            for a in (val, x, y):
                assert np.array_equal(a, np.round(a)) and np.abs(a).max(initial=0) <= M.VMAX
                assert np.array_equal(a.astype(np.float32).astype(F64), a)  # the same integers are exact in float32
            longest = int(np.diff(rp).max())
            # |alpha| <= 3, |beta| <= 3: every partial sum of a row is below this, in any order
            worst = max(worst, 3.0 * 4 * longest * np.abs(val).max(initial=0) * np.abs(x).max() + 3.0 * np.abs(y).max())
    assert longest <= 100 and worst < LIMIT
    # scalar CSR (|alpha| <= 3), Jacobi apply (integer images, nrm = 8, dinv1 = +-2**k: a dyadic result with an integer
    # numerator 3 * VMAX * VMAX), galerkin (40 terms), restriction (70 terms of a difference)
    assert 3.0 * 100 * M.VMAX ** 2 + 3.0 * M.VMAX < LIMIT
    assert 3.0 * M.VMAX ** 2 * 2 ** 3 < LIMIT and 40.0 * M.VMAX < LIMIT and 70.0 * 2 * M.VMAX < LIMIT
    # the DILU sweep: t = r - sum over the longest list, then E^-1 = integers <= 8 over 4
    for seed, nghost in ((3, 0), (4, 7)):
        N, nown, rp, ci, target = M.dilu_pattern(seed, nghost=nghost)
        t = M.VMAX + 4.0 * int(np.diff(rp).max()) * M.VMAX ** 2
        assert 4.0 * 8 * t + M.VMAX * 4 < LIMIT
    # unimodular blocks: entries and inverse entries <= VMAX, so every cofactor and the determinant are far below
    b = M.unimodular3(np.random.default_rng(0), 200)
    assert np.abs(b).max() <= M.VMAX and np.abs(M.inv3(b, I64)).max() <= M.VMAX and 6.0 * M.VMAX ** 3 < LIMIT


# ---- (2) models against independent computations, (4) int64 == longdouble ------------------------------------------------
@pytest.mark.parametrize("nrows,N", [(33, 33), (31, 139), (257, 295)])
def test_bcsr_spmv_model(nrows, N):
    rp, ci, val, x, y = M.spmv_inputs(nrows, N, 7 + nrows, True)
    A = dense_block_matrix(nrows, N, rp, ci, val)
    rows = np.arange(nrows)
    for alpha, beta in ((1.0, 0.0), (-2.0, -3.0)):
        idx, got = M.bcsr_spmv(rows, N, rp, ci, val, alpha, x, beta, y, I64)
        yv = y[M.vec_idx(rows, N)]
        want = alpha * (A @ x[:4 * N])[M.vec_idx(rows, nrows)] + beta * yv
        assert np.array_equal(got, want)
        if M.HAVE_EXTENDED:
            assert np.array_equal(M.bcsr_spmv(rows, N, rp, ci, val, alpha, x, beta, y, LD)[1], got)
    # a range writes (and reads) only its rows
    idx, got = M.bcsr_spmv(np.arange(5, 9), N, rp, ci, val, 1.0, x, 0.0, None, I64)
    assert np.array_equal(idx, M.vec_idx(np.arange(5, 9), N)) and np.array_equal(got, (A @ x)[M.vec_idx(np.arange(5, 9), nrows)])
    # the bound's scale is |A||x|
    s = M.bcsr_spmv(rows, N, rp, ci, val, -2.0, x, 0.0, None, F64, absolute=True)[1]
    assert np.array_equal(s, 2.0 * (np.abs(A) @ np.abs(x))[M.vec_idx(rows, nrows)])
    # interleave4 is the gather of (u0, u1, u2, p)
    i4, v4 = M.interleave4(2, 6, N, x)
    assert np.array_equal(i4, np.arange(8, 24)) and np.array_equal(v4.reshape(4, 4)[:, 3], x[3 * N + 2: 3 * N + 6])


def test_csr_models():
    rp, ci = M.pattern(M.cycle_lens(M.CSR_LENS, 33, 1, cap=150), 150, 2)
    rng = np.random.default_rng(3)
    val, x, y = M.ints(rng, ci.size), M.ints(rng, 150), M.ints(rng, 33)
    A = sp.csr_matrix((val, ci, rp), shape=(33, 150))
    assert np.array_equal(M.csr_spmv(33, rp, ci, val, -2.0, x, 3.0, y, I64), -2.0 * (A @ x) + 3.0 * y)
    if M.HAVE_EXTENDED:
        assert np.array_equal(M.csr_spmv(33, rp, ci, val, -2.0, x, 3.0, y, LD), -2.0 * (A @ x) + 3.0 * y)
    rp, ci = M.pattern(M.cycle_lens(M.CSR_LENS, 33, 4, cap=101), 101, 5)
    data = np.random.default_rng(6).normal(size=ci.size)
    A = sp.csr_matrix((data, ci, rp), shape=(33, 101)).toarray()
    rows, got = M.csr_jacobi(33, data, rp, ci, x, F64)
    has = np.array([i in ci[rp[i]: rp[i + 1]] for i in range(33)])
    assert np.array_equal(rows, np.flatnonzero(has)) and 0 < rows.size < 33
    assert np.array_equal(got, x[rows] / A[rows, rows])


def test_jacobi_tree_models():
    N = 40
    rp, ci, val = M.diag_inputs(N, 11, True)
    A = dense_block_matrix(N, N, rp, ci, val)
    d33, d1 = M.pc_setup(N, rp, ci, val, I64)
    for i in (0, 17, 39):
        D = A[3 * i: 3 * i + 3, 3 * i: 3 * i + 3]
        assert np.array_equal(d33[9 * i: 9 * i + 9].reshape(3, 3) @ D, np.eye(3))  # inv(D), row-major
        assert d1[i] * A[3 * N + i, 3 * N + i] == 1.0
    if M.HAVE_EXTENDED:
        l33, l1 = M.pc_setup(N, rp, ci, val, LD)
        assert np.array_equal(l33, d33) and np.array_equal(l1, d1)
    g33, gp, gu = M.get_diag(N, rp, ci, val)
    assert np.array_equal(g33.reshape(N, 3, 3)[5], A[15:18, 15:18]) and gp[5] == A[3 * N + 5, 3 * N + 5]
    assert np.array_equal(gu.reshape(N, 3)[5], np.diag(A)[15:18])
    # the apply reads the image column-major: z_u = image^T r_u
    rng = np.random.default_rng(12)
    img, x = M.ints(rng, 9 * N), M.ints(rng, 6 * N)
    y = M.block3_apply(N, img, x, I64)
    assert np.array_equal(y[:3], img[:9].reshape(3, 3).T @ x[:3])
    d1 = 2.0 ** rng.integers(-3, 4, N)
    for nrows, n, nrm in ((N, 4 * N, None), (31, 4 * N + 1, 8.0), (N, 6 * N, 8.0)):
        out = M.pc_apply(nrows, N, n, img, d1, x, nrm, I64)
        s = 1.0 if nrm is None else 1.0 / nrm
        idx, yv = out["y"]
        want = np.full(6 * N, np.nan)
        want[: 3 * nrows] = (M.block3_apply(nrows, img, x, I64) * s)
        want[3 * N: 3 * N + nrows] = x[3 * N: 3 * N + nrows] * s * d1[:nrows]
        want[4 * N: n] = x[4 * N: n] * s
        assert np.array_equal(np.sort(idx), np.flatnonzero(~np.isnan(want))) and np.array_equal(yv, want[idx])
        assert np.array_equal(out["y4"][1].reshape(nrows, 4), want[M.vec_idx(np.arange(nrows), N)])
        assert ("q" in out) == (nrm is not None)
        if nrm is not None:
            assert np.array_equal(out["q"][1], x[out["q"][0]] * s)
        if M.HAVE_EXTENDED:
            assert np.array_equal(M.pc_apply(nrows, N, n, img, d1, x, nrm, LD)["y"][1], yv)
    # scalar diagonal getters
    sval = rng.normal(size=ci.size)
    S = sp.csr_matrix((sval, ci, rp), shape=(N, N))
    assert np.array_equal(M.csr_get_diag(sval, rp, ci, N), S.diagonal())
    mv = rng.normal(size=9 * ci.size)
    idx, w = M.get_diag_block(mv, 3, N, rp, ci, 5, 18)
    full = np.zeros((3 * N, 3 * N))
    ei = M.expanded_index(rp, 3, 3)
    for k in range(ci.size):
        i = M.row_of_nnz(rp)[k]
        full[3 * i: 3 * i + 3, 3 * ci[k]: 3 * ci[k] + 3] = mv[ei[k]]
    out = np.zeros(N * 18)
    out[idx] = w
    assert np.array_equal(out.reshape(N, 18)[7, :15].reshape(3, 5)[:, :3], full[21:24, 21:24])


def test_inverse_helpers_and_condition_numbers():
    rng = np.random.default_rng(20)
    for m in (3, 4):
        b = M.dominant_blocks(rng, 300, m)
        ref = M.inv_gj(b, LD)
        assert np.abs(ref.astype(F64) - np.linalg.inv(b)).max() < 1e-13
        assert float(M.kappa_inf(b, ref).max()) <= 10.0
    b3 = M.dominant_blocks(rng, 300, 3)
    assert np.abs(M.inv3(b3, LD).astype(F64) - np.linalg.inv(b3)).max() < 1e-13
    assert np.abs(M.inv3_closed_f64(b3) - np.linalg.inv(b3)).max() < 1e-13
    p4 = M.signed_perm_pow2_4(rng, 50)
    assert np.array_equal(M.exact_inverse_perm4(p4) @ p4, np.broadcast_to(np.eye(4), p4.shape))
    assert np.array_equal(M.inv_gj(p4, F64), M.exact_inverse_perm4(p4))  # Gauss-Jordan is exact on these
    u3 = M.unimodular3(rng, 50)
    assert np.array_equal(M.inv3(u3, I64) @ u3, np.broadcast_to(np.eye(3, dtype=I64), u3.shape))


@needs_extended
def test_rounded_tier_blocks_are_well_conditioned():
    for N in (1, 33, 257, 513):
        rp, ci, val = M.diag_inputs(N, 60 + N, False)
        D = val.reshape(-1, 4, 4)[M.diag_pos(rp, ci)][:, :3, :3]
        assert float(M.kappa_inf(D, M.inv_gj(D, LD)).max()) <= 10.0
    for seed, nghost in ((3, 0), (4, 7)):
        N, nown, rp, ci, color = M.dilu_pattern(seed, nghost=nghost)
        rows, coff, low, up = M.dilu_lists(nown, rp, ci, color)
        for s in (160, 180):
            val = M.dilu_values(np.random.default_rng(s + seed), N, rp, ci, False)
            Einv = M.dilu_setup(N, nown, rp, ci, val, color, rows, coff, LD)[:nown]
            assert float(M.kappa_inf(M.inv_gj(Einv, LD), Einv).max()) <= 10.0


def test_dirichlet_and_layout_models():
    N = 41
    rp, ci, val = M.diag_inputs(N, 100, False, lens=(1, 8, 9, 33))
    A = dense_block_matrix(N, N, rp, ci, val)
    out = dense_block_matrix(N, N, rp, ci, M.zero_rows(N, rp, ci, val, [3, 3, -1, N, 7], 1, 2.5))
    want = A.copy()
    for node in (3, 7):
        want[3 * node + 1, :] = 0.0
        want[3 * node + 1, 3 * node + 1] = 2.5
    assert np.array_equal(out, want)
    out = dense_block_matrix(N, N, rp, ci, M.zero_scalar_rows(N, rp, ci, val, np.array([3 * 3 + 1, 3 * 7 + 1, -9, 3 * N]) - 4, 4, 2.5))
    assert np.array_equal(out, want)
    sval = val[: ci.size]
    S = sp.csr_matrix((sval, ci, rp), shape=(N, N)).toarray()
    got = sp.csr_matrix((M.csr_zero_row(sval, N, rp, ci, [5 - 2, N - 2, -1 - 2], 2, -1.5), ci, rp), shape=(N, N)).toarray()
    S[5, :] = 0.0
    S[5, 5] = -1.5
    assert np.array_equal(got, S)
    assert np.array_equal(M.dirichlet_vec(np.ones(12), [1, 3], 3, 2), np.where(np.isin(np.arange(12), [5, 11]), 0.0, 1.0))
    # export: sub-matrix (0,0) as a scalar CSR over node*3 + component holds the velocity part of the operator
    A00, A01, A10, A11 = M.export_fs(N, rp, val)
    srp, sci = M.expand_pattern(rp, ci, 3)
    assert np.array_equal(sp.csr_matrix((A00, sci, srp), shape=(3 * N, 3 * N)).toarray(), A[: 3 * N, : 3 * N])
    assert np.array_equal(sp.csr_matrix((A11, ci, rp), shape=(N, N)).toarray(), A[3 * N:, 3 * N:])
    r31 = np.concatenate([[0], np.cumsum(np.repeat(np.diff(rp), 3))])
    assert np.array_equal(sp.csr_matrix((A01, np.concatenate([np.tile(ci[rp[i]: rp[i + 1]], 3) for i in range(N)]), r31),
                                        shape=(3 * N, N)).toarray(), A[: 3 * N, 3 * N:])
    c13 = (ci[:, None].astype(I64) * 3 + np.arange(3)).ravel()
    assert np.array_equal(sp.csr_matrix((A10, c13, 3 * rp.astype(I64)), shape=(N, 3 * N)).toarray(), A[3 * N:, : 3 * N])


def test_scatter_models():
    ien, rp, ci, absent = M.elements_pattern(5, 4, 40, 130)
    assert np.unique(ien).size == 20 and absent[1] not in ci[rp[absent[0]]: rp[absent[0] + 1]]
    rng = np.random.default_rng(1)
    nnz = ci.size
    target, val = M.ints(rng, 16 * nnz), M.ints(rng, 4 * 16 * 27)
    bidx, mask = np.array([3, 0, 4, 1]), np.array([1, 1, 0, 1])
    got = M.elem_scatter(target, np.arange(16 * nnz).reshape(nnz, 4, 4), 2.0, 4, 4, bidx, ien, rp, ci, 4, 4, val, 6, 27, -3.0, mask)
    want = 2.0 * dense_block_matrix(40, 40, rp, ci, target)
    hit = np.zeros_like(want, bool)
    for slot in (0, 1, 3):
        nodes = ien[4 * bidx[slot]: 4 * bidx[slot] + 4]
        for a in range(4):
            for b in range(4):
                if (nodes[a], nodes[b]) != absent:
                    blk = val[(slot * 16 + a * 4 + b) * 27:][:24].reshape(4, 6)[:, :4]
                    ix = np.ix_(M.vec_idx([nodes[a]], 40)[0], M.vec_idx([nodes[b]], 40)[0])
                    want[ix] += -3.0 * blk
                    hit[ix] = True
    want = np.where(hit, want, want / 2.0)
    assert np.array_equal(dense_block_matrix(40, 40, rp, ci, got), want)
    # set-value and the element LHS on the scalar pattern
    t1, A1 = M.ints(rng, nnz), M.ints(rng, 3)
    k = np.array([0, 5, 9])
    got = M.csr_set_blocked(t1, -2.0, rp, ci, np.append(M.row_of_nnz(rp)[k], absent[0]), np.append(ci[k], absent[1]), 1, 1,
                            np.append(A1, 77.0), 3.0, 1, 1)
    w = t1.copy()
    w[k] = 3.0 * A1 - 2.0 * t1[k]
    assert np.array_equal(got, w)
    srp, sci = M.expand_pattern(rp, ci, 3)
    t3, v3 = M.ints(rng, sci.size), M.ints(rng, 2 * 144)
    got = M.csr_add_element_lhs(t3, 4, 3, srp, sci, 2, np.array([2, 0]), ien, v3)
    D = sp.csr_matrix((got - t3, sci, srp), shape=(120, 120)).toarray()
    dof = (ien[8:12, None].astype(I64) * 3 + np.arange(3)).ravel()
    assert np.array_equal(D[np.ix_(dof, dof)], v3[:144].reshape(12, 12))
    dof0 = (ien[0:4, None].astype(I64) * 3 + np.arange(3)).ravel()
    w0 = v3[144:].reshape(12, 12).copy()
    w0[3:6, 6:9] = 0.0  # the absent pair (node 1, node 2) of element 0
    assert np.array_equal(D[np.ix_(dof0, dof0)], w0)


# ---- DILU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nghost", [(3, 0), (4, 7)])
def test_dilu_generator_promises(seed, nghost):
    N, nown, rp, ci, target = M.dilu_pattern(seed, nghost=nghost)
    assert (nown < N) == (nghost > 0)
    A = sp.csr_matrix((np.ones(ci.size), ci, rp), shape=(N, N))
    assert (A != A.T).nnz == 0 and np.all(A.diagonal() == 1)  # (j, i) exists when (i, j) does; the diagonal is stored
    for i in range(N):
        assert np.all(np.diff(ci[rp[i]: rp[i + 1]]) > 0)
    color = M.greedy_colors(nown, N, rp, ci)
    assert np.array_equal(color, target) and np.all(color[nown:] == 255)
    r, c = M.row_of_nnz(rp), ci
    own = (r < nown) & (c < nown) & (r != c)
    assert np.all(color[r[own]] != color[c[own]])  # a valid colouring
    rows, coff, low, up = M.dilu_lists(nown, rp, ci, color)
    sizes = set(np.diff(coff).tolist())
    assert set(M.DILU_COLOR_SIZES) <= sizes and max(sizes) > 256
    assert np.all(np.diff(color[rows]) >= 0) and np.array_equal(np.sort(rows), np.arange(nown))
    nl, nu = np.diff(low[0]), np.diff(up[0])
    assert set(M.DILU_LIST_LENS) <= set(nl.tolist()) and set(M.DILU_LIST_LENS) <= set(nu.tolist())
    assert np.any((nl >= 9) & (nu >= 9)) and np.any((nl == 0) & (nu == 0))
    # the lists are what the host builds: per slot, the row's nonzeros in row order, split by colour, ghosts dropped
    for sl in (0, 40, nown - 1):
        i = rows[sl]
        k = np.arange(rp[i], rp[i + 1])
        k = k[(ci[k] < nown) & (ci[k] != i)]
        assert np.array_equal(low[1][low[0][sl]: low[0][sl + 1]], k[color[ci[k]] < color[i]])
        assert np.array_equal(up[2][up[0][sl]: up[0][sl + 1]], ci[k[color[ci[k]] > color[i]]])


def test_dilu_model_against_dense():
    N, nown, rp, ci, color = M.dilu_pattern(5, ncolors=12, sizes=[9, 8, 7, 12, 5, 4, 4, 5, 4, 4, 3, 1], nghost=4, nextra=60)
    assert np.array_equal(M.greedy_colors(nown, N, rp, ci), color)
    rows, coff, low, up = M.dilu_lists(nown, rp, ci, color)
    rng = np.random.default_rng(6)
    val = M.dilu_values(rng, N, rp, ci, False)
    r = rng.normal(size=4 * N)
    dt = LD if M.HAVE_EXTENDED else F64
    Einv = M.dilu_setup(N, nown, rp, ci, val, color, rows, coff, dt)
    z, zerr = M.dilu_apply(N, nown, rows, coff, low, up, val, Einv.astype(F64).reshape(-1), r, dt)
    zd, E = M.dilu_dense_apply(N, nown, rp, ci, val, color, r[M.vec_idx(np.arange(N), N)])
    assert np.abs(Einv[:nown].astype(F64) - np.linalg.inv(E)).max() < 1e-12
    assert np.abs(z[M.vec_idx(np.arange(nown), N)].astype(F64) - zd).max() < 1e-11 * np.abs(zd).max()
    assert np.all(zerr[:nown] > 0) and zerr.max() < 1e-12
    # the float64 run of the same sweeps stays inside the propagated bound
    z64, _ = M.dilu_apply(N, nown, rows, coff, low, up, val, Einv.astype(F64).reshape(-1), r, F64)
    if M.HAVE_EXTENDED:
        err = np.abs(z64.astype(LD) - z)[M.vec_idx(np.arange(nown), N)].astype(F64)
        assert np.all(err <= zerr[:nown])


def test_dilu_sweep_exact_tiers_agree():
    N, nown, rp, ci, color = M.dilu_pattern(3)
    rows, coff, low, up = M.dilu_lists(nown, rp, ci, color)
    rng = np.random.default_rng(173)
    val, Einv, r, z = M.ints(rng, 16 * ci.size), M.dyadic(rng, 16 * N), M.ints(rng, 4 * N), M.ints(rng, 4 * N)
    for fwd, t in ((1, low), (0, up)):
        for c in (0, 3, 9, coff.size - 2):
            args = (fwd, int(coff[c]), int(coff[c + 1] - coff[c]), rows, N, t[0], t[1], t[2], val, Einv, r, z)
            idx, a, _ = M.dilu_sweep(*args, I64, einv_shift=2)
            idx2, b, bound = M.dilu_sweep(*args, F64)
            assert np.array_equal(idx, idx2) and np.array_equal(a, b.astype(F64)) and np.all(bound >= 0)
            # mutation: the third and fourth entry of a list swapped between value and column changes the result
            q = int(t[0][coff[c]])
            if t[0][coff[c] + 1] - q >= 4:
                nz = t[1].copy()
                nz[[q + 2, q + 3]] = nz[[q + 3, q + 2]]
                _, m, _ = M.dilu_sweep(fwd, int(coff[c]), 1, rows, N, t[0], nz, t[2], val, Einv, r, z, I64, einv_shift=2)
                assert not np.array_equal(m, a[:1])


# ---- two-level ---------------------------------------------------------------------------------------------------------
def test_amg_models_and_generators():
    sizes = M.cycle_lens(M.AGG_SIZES, 11, 210)
    aoff, anode, agg = M.aggregates(sizes, 211)
    N, Nc = anode.size, sizes.size
    assert set(M.AGG_SIZES) <= set(sizes.tolist()) and {s % 16 for s in sizes} >= {0, 1, 2, 3, 15} and sizes.max() > 16
    assert np.array_equal(np.sort(anode), np.arange(N)) and np.array_equal(np.bincount(agg), sizes)
    rng = np.random.default_rng(212)
    r, sub, xc, z = M.ints(rng, 4 * N), M.ints(rng, 4 * N), M.ints(rng, 4 * Nc), M.ints(rng, 4 * N)
    P = sp.csr_matrix((np.ones(N), (np.arange(N), agg)), shape=(N, Nc))  # piecewise-constant prolongation
    idx, rc = M.restrict_diff(Nc, aoff, anode, N, r, sub, I64)
    d4 = (r - sub)[M.vec_idx(np.arange(N), N)]
    assert np.array_equal(rc, P.T @ d4) and np.array_equal(idx, M.vec_idx(np.arange(Nc), Nc))
    idx, zz = M.prolong_add(N - 40, N, agg, Nc, xc, z, I64)
    assert np.array_equal(zz, (z[M.vec_idx(np.arange(N), N)] + P @ xc[M.vec_idx(np.arange(Nc), Nc)])[: N - 40])
    lens = M.cycle_lens(M.COARSE_LENS, 23, 200)
    assert set(M.COARSE_LENS) <= set(lens.tolist()) and {n % 4 for n in lens} == {0, 1, 2, 3} and lens.max() > 4
    off, li = M.coarse_lists(lens, int(lens.sum()) + 11, 201)
    vf = M.ints(rng, 16 * (int(lens.sum()) + 11))
    vc = M.galerkin(lens.size, off, li, vf, I64)
    G = sp.csr_matrix((np.ones(li.size), li, off), shape=(lens.size, vf.size // 16))
    assert np.array_equal(vc, G @ vf.reshape(-1, 16)) and np.all(vc[lens == 0] == 0)
    if M.HAVE_EXTENDED:
        assert np.array_equal(M.galerkin(lens.size, off, li, vf, LD), vc)
        assert np.array_equal(M.restrict_diff(Nc, aoff, anode, N, r, sub, LD)[1], rc)


# ---- (3) generator promises, (6) mutations ---------------------------------------------------------------------------------
def test_pattern_generator_promises():
    hit, per = set(), set()
    for nrows, N in M.SPMV_CASES:
        rp, ci, val, x, y = M.spmv_inputs(nrows, N, 1000 + nrows, True)
        lens = np.diff(rp)
        hit |= set(lens.tolist())
        assert rp.size == nrows + 1 and ((ci.min() == 0 and ci.max() == N - 1) or nrows == 1)
        for i in range(nrows):
            assert np.all(np.diff(ci[rp[i]: rp[i + 1]]) > 0)
        if N > nrows:  # one row references ghost columns only
            assert any(lens[i] > 0 and ci[rp[i]] >= nrows for i in range(nrows))
        blocks = -(-nrows * 8 // 256)
        per.add((blocks + 7) // 8)
    assert set(M.SPMV_LENS) <= hit and {1, 2, 3} <= per
    assert {nr for nr, _ in M.SPMV_CASES} == set(M.ROW_COUNTS)
    for N in (33, 257, 513):
        rp, ci, val = M.diag_inputs(N, 60 + N, True)
        kd = M.diag_pos(rp, ci)
        first, last = kd == rp[:-1], kd == rp[1:] - 1
        assert np.any(first & ~last) and np.any(last & ~first) and np.any(~first & ~last)
        assert set(np.diff(rp).tolist()) >= {L for L in M.DIAG_LENS if L <= N}
    rp, ci = M.pattern(M.cycle_lens((1, 15, 16, 17, 33), 37, 120), 64, 121)
    assert set(np.diff(rp).tolist()) == {1, 15, 16, 17, 33}


def test_inputs_can_tell_mutations_apart():
    nrows, N = 257, 295
    rp, ci, val, x, y = M.spmv_inputs(nrows, N, 1000 + nrows, True)
    i = int(np.flatnonzero(np.diff(rp) == 17)[0])
    idx, good = M.bcsr_spmv([i], N, rp, ci, val, 1.0, x, 0.0, None, I64)
    dropped = val.copy()
    dropped[16 * (rp[i + 1] - 1): 16 * rp[i + 1]] = 0.0  # the last entry of a length-17 row
    assert np.all(M.bcsr_spmv([i], N, rp, ci, dropped, 1.0, x, 0.0, None, I64)[1] != good)
    swapped = val.reshape(-1, 4, 4).copy()
    swapped[:, :, [2, 3]] = swapped[:, :, [3, 2]]  # the (u2, p) pair of every block
    bad = M.bcsr_spmv(np.arange(nrows), N, rp, ci, swapped.reshape(-1), 1.0, x, 0.0, None, I64)[1]
    allgood = M.bcsr_spmv(np.arange(nrows), N, rp, ci, val, 1.0, x, 0.0, None, I64)[1]
    assert np.all((bad != allgood).any(axis=1)[np.diff(rp) > 0])
    # the export: dropping the second trip (entries from the 17th nonzero of a row on) leaves sentinels behind, and every
    # value is distinct, so a misplaced one cannot coincide
    rp, ci = M.pattern(M.cycle_lens((1, 15, 16, 17, 33), 37, 120), 64, 121)
    v = np.random.default_rng(122).permutation(16 * ci.size).astype(F64) + 0.25
    assert np.unique(np.concatenate(M.export_fs(37, rp, v))).size == v.size
