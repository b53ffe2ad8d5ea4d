"""Every matrix and preconditioner kernel of dedflow_amd/csrc/k_matrix.hip, k_dilu.hip and k_amg.hip alone, through its C
launcher, on synthetic patterns (tests/matrix_model.py), against the numpy model of the same file.

Tier A (exact): inputs are small integers stored as float64 (|a|, |x| <= 2**10; test_matrix_model_cpu.py shows from
the longest row and the largest magnitudes generated that every product and partial sum stays an integer below 2**53
in any order), unimodular velocity blocks, power-of-two A_pp and normalisation, dyadic E^-1: the expectation is BITWISE
equality with the int64 model, so a dropped, duplicated or misplaced entry of one short row cannot hide behind a
tolerance taken against the largest entry of an array.
Tier B (rounded): normal random data against the np.longdouble model with a-priori bounds that hold for every
summation order.  For a block row of `len` nodal nonzeros |err_i| <= gamma_k (|alpha| sum |a||x| + |beta||y_i|) with
gamma_k = k u / (1 - k u), k = 4 len + 3 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the
bounds of the other kernels are stated where they are used, the DILU sweep's (with the E^-1 product and the error the
input z already carries) in matrix_model.dilu_sweep.  For the _f32 kernels the float-rounded values are the model's
exact input.  The observed err / bound are appended to the file named by DFL_PARITY_OUT
(profiles/matrix_kernel_parity.jsonl is such a run).

Inverses (pc_setup, block3_invert, dilu_setup): compared with the longdouble inverse under the budget
c u kappa_inf(block) max|inverse|.  c is measured in the test itself on a float64 numpy restatement of the same closed
form (3x3: cofactors over the determinant; 4x4: Gauss-Jordan with partial pivoting through the same colour recurrence)
run on the same inputs, never on the kernel, with a factor 8 on the largest figure that restatement shows, for FMA
contraction and operand order.  Figures of the restatement on the committed cases (err / (u kappa max|inverse|)):
3x3 closed form 0.93 .. 1.97, i.e. c = 7.4 .. 15.8; 4x4 colour recurrence 3.22 and 3.34, i.e. c = 25.8 and 26.7 (the
blocks have kappa_inf of 2 .. 3, so u kappa max|inverse| is a small unit; both figures are written to the jsonl as `c`
and `restatement` with every record).

Every array sits inside a larger device buffer between guard bands of 64 sentinels (guarded_buffers.py).  After each
launch the bands, every const input and every output entry the operation must not write are compared bit for bit with
what was uploaded; outputs of overwrite-type kernels are preloaded with the NaN sentinel, so a read of y on a
beta == 0 path shows up as NaN.  Plain-layout vectors get a pointer offset of one double (8-byte aligned only);
buffers the kernels read as 16-byte vectors (val, x4 / y4, Einv, valf) stay 16-byte aligned, as in the solver.

Not here, on purpose: no case aims at a fault.  No null or out-of-range pointers (a NULL output is passed only where
the launcher documents it), no missing diagonal for the kernels that look one up without a guard, no unsorted rows,
no asymmetric pattern for DILU.
"""
import numpy as np
import pytest

import matrix_model as M
from guarded_buffers import F32, I32, U8, Pool, Recorder, assert_bits, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
U = M.U
record = Recorder("a")
TIERS = ["A", pytest.param("B", marks=pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON))]


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    _declare(A.lib())  # raises if the HIP library is missing: no fallback
    return A


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    record.write()


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def _declare(L):
    import ctypes as C
    i32, i64, f64, vp, ci = C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int
    sig = {
        "dfl_bcsr_spmv_range": [i32, i32, i32, vp, vp, vp, f64, vp, f64, vp, vp],
        "dfl_bcsr_spmv_rows": [i32, i32, vp, vp, vp, f64, vp, f64, vp, vp],
        "dfl_interleave4": [i32, i32, i32, vp, vp, vp],
        "dfl_bcsr_spmv_x4": [i32, i32, i32, vp, vp, vp, f64, vp, vp, vp],
        "dfl_bcsr_values_to_f32": [i64, vp, vp, vp],
        "dfl_bcsr_spmv_f32": [i32, i32, vp, vp, vp, vp, vp, vp],
        "dfl_csr_spmv": [i32, vp, vp, vp, f64, vp, f64, vp, vp],
        "PCJacobiDevice": [i32, i32, vp, vp, vp, vp, vp],
        "PCJacobiInplaceDevice": [i32, i32, vp, vp, vp, vp],
        "dfl_pc_jacobi_setup_rows": [i32, vp, vp, vp, vp, vp, vp],
        "dfl_pc_jacobi_apply_rows": [i32, i32, i32, vp, vp, vp, vp, vp],
        "dfl_pc_jacobi_apply_scaled_rows": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "dfl_pc_jacobi_apply_scaled_rows_x4": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "dfl_pc_jacobi_apply_scaled": [i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "dfl_block3_invert": [i32, vp, vp],
        "dfl_block3_apply": [i32, vp, vp, vp, vp],
        "dfl_bcsr_get_diag": [i32, vp, vp, vp, vp, vp, vp, vp],
        "MatrixCSRGetDiagGPU": [vp, vp, vp, vp, i32],
        "MatrixGetDiagBlockGPU": [vp, i32, i32, i32, vp, vp, vp, ci, ci],
        "dfl_bcsr_zero_rows": [i32, vp, vp, vp, i32, vp, i32, f64, vp],
        "dfl_bcsr_zero_scalar_rows": [i32, vp, vp, vp, i32, vp, i32, f64, vp],
        "MatrixCSRZeroRowGPU": [vp, i32, i32, vp, vp, i32, vp, i32, f64],
        "dfl_dirichlet_vec": [vp, i32, vp, i32, i32, vp],
        "ApplyBCVecNodalGPU": [vp, i32, vp, i32, i32],
        "GetRowFromNodeGPU": [i32, vp, i32, i32],
        "GetNodeFromRowGPU": [i32, vp, i32],
        "dfl_block_export_fs": [i32, vp, vp, vp, vp, vp, vp, vp],
        "dfl_block_import_fs": [i32, vp, vp, vp, vp, vp, vp, vp],
        "dfl_bcsr_add_elem_blocked": [vp, f64, i32, i32, vp, vp, vp, vp, vp, ci, ci, f64, vp, vp],
        "MatrixCSRAddElemValueBatchedGPU": [vp, f64, i32, vp, vp, i32, i32, i32, vp, vp, vp, f64, vp],
        "MatrixCSRAddElemValueBlockedBatchedGPU": [vp, f64, i32, vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, ci, ci, f64, vp],
        "MatrixCSRSetValueBatchedGPU": [vp, f64, i32, i32, vp, vp, i32, vp, vp, vp, f64],
        "MatrixCSRSetValueBlockedBatchedGPU": [vp, f64, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp, f64, ci, ci],
        "MatrixCSRAddElementLHSGPU": [vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, ci],
        "dfl_dilu_setup_color": [i32, vp, i32, vp, vp, vp, vp, vp, vp],
        "dfl_dilu_sweep_color": [ci, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "dfl_dilu_sweep_color_f32": [ci, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "dfl_copy_range": [i64, i64, vp, vp, vp],
        "dfl_amg_galerkin": [i32, vp, vp, vp, vp, vp],
        "dfl_amg_restrict_diff": [i32, vp, vp, i32, vp, vp, vp, vp],
        "dfl_amg_prolong_add_rows": [i32, i32, vp, i32, vp, vp, vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = None, args


# ======================================================================================================================
# helpers
# ======================================================================================================================
def verify(slot, idx, want, what, bound=None, kernel=None, case=None, dtype=F64, zero_sign=True, **extra):
    """the entries `idx` of the slot against `want` -- bit for bit (bound None) or within `bound` -- and every other
    entry, the bands included, against what was uploaded.  Returns the slot's data.  zero_sign False: the sign of an
    exact zero is not compared (the exact inverses: an integer model has no -0, and which sign a vanishing cofactor or
    an eliminated entry gets depends on the order of evaluation); every nonzero entry stays bitwise."""
    idx = np.asarray(idx, I64).ravel()
    mask = np.zeros(slot.n, bool)
    mask[idx] = True
    assert mask.sum() == idx.size, what + ": the model writes an entry twice"
    got = slot.check(what, mask)
    want = np.asarray(want)
    if bound is None:
        if zero_sign:
            assert_bits(got[idx], want.ravel(), what, dtype)
        else:
            assert_bits(got[idx] + 0.0, want.ravel().astype(F64) + 0.0, what, dtype)
        return got
    bound = np.broadcast_to(np.asarray(bound, F64), want.shape).ravel()
    want = want.ravel()
    assert np.all(np.isfinite(got[idx])), what + ": not finite"
    err = np.abs(got[idx].astype(LD) - want.astype(LD)).astype(F64)
    zero = bound == 0
    assert np.all(err[zero] == 0), what + ": an entry with a zero bound is not exact"
    ratio = float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0
    record(kernel or what, case or what, ratio, **extra)
    assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)
    return got


def untouched(what, *slots):
    for s in slots:
        s.check(what + ": an input or an unowned buffer changed")


def csr_slots(pool, rp, ci):
    return pool.slot(rp, 0, I32), pool.slot(ci, 0, I32)


def model_dtype(tier):
    return I64 if tier == "A" else LD


# ======================================================================================================================
# SpMV family
# ======================================================================================================================
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrows,N", M.SPMV_CASES, ids=lambda v: str(v))
def test_bcsr_spmv(nrows, N, tier, api, pool):
    """dfl_bcsr_spmv / _rows / _range: both beta paths (beta == 0 on a NaN-filled y), alpha != 1, nrows < N with a
    ghost-only row, empty rows, ranges with row0 in {1, 5, 31, 33} that write only their rows, row1 <= row0.
    256 / 257 / 513 rows run the XCD remap with 1, 2 and 3 blocks per XCD."""
    L = api.lib()
    exact = tier == "A"
    dt = model_dtype(tier)
    rp, ci, val, x, y = M.spmv_inputs(nrows, N, 1000 + nrows, exact)
    rps, cis = csr_slots(pool, rp, ci)
    vs, xs, ys = pool.slot(val), pool.slot(x, 1), pool.slot(y, 1)
    case = "nrows%d-N%d-%s" % (nrows, N, tier)

    def run(row0, row1, alpha, beta, entry):
        ys.reset(y if beta != 0 else sent(4 * N))
        if entry == "full":
            L.dfl_bcsr_spmv(N, rps.ptr, cis.ptr, vs.ptr, alpha, xs.ptr, beta, ys.ptr, None)
        elif entry == "rows":
            L.dfl_bcsr_spmv_rows(row1, N, rps.ptr, cis.ptr, vs.ptr, alpha, xs.ptr, beta, ys.ptr, None)
        else:
            L.dfl_bcsr_spmv_range(row0, row1, N, rps.ptr, cis.ptr, vs.ptr, alpha, xs.ptr, beta, ys.ptr, None)
        api.sync()
        rows = np.arange(row0, max(row0, row1))
        what = "spmv %s [%d,%d) alpha=%g beta=%g" % (entry, row0, row1, alpha, beta)
        idx, want = M.bcsr_spmv(rows, N, rp, ci, val, alpha, x, beta, y, dt)
        bound = None if exact else M.spmv_bound(rows, N, rp, ci, val, alpha, x, beta, y)
        verify(ys, idx, want, what, bound, "bcsr_spmv", case + " " + what)
        untouched(what, rps, cis, vs, xs)

    a2 = -2.0 if exact else -1.7
    entry = "full" if nrows == N else "rows"
    run(0, nrows, 1.0, 0.0, entry)
    run(0, nrows, a2, 0.0, entry)
    run(0, nrows, a2, 1.0, entry)
    run(0, nrows, 3.0 if exact else 0.3, -3.0, entry)
    for k, row0 in enumerate((1, 5, 31, 33)):
        if row0 < nrows:
            row1 = nrows if k & 1 else min(nrows, row0 + 3 + 40 * k)
            run(row0, row1, a2, 0.0, "range")
            run(row0, row1, a2, -3.0, "range")
    run(min(5, nrows), min(5, nrows), a2, 0.0, "range")  # row1 == row0: nothing is written
    run(nrows, nrows - 1, a2, 1.0, "range")


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrows,N", [(7, 139), (33, 33), (257, 295), (513, 513)], ids=lambda v: str(v))
def test_interleave4_and_spmv_x4(nrows, N, tier, api, pool):
    """dfl_interleave4 over [node0, node1) sub-ranges writes only its nodes; dfl_bcsr_spmv_x4 on the interleaved copy
    equals the model AND, bit for bit in both tiers, dfl_bcsr_spmv_range on the plain layout (the header's "bitwise the
    same y").  N is odd: the pressure part of the plain layout is only 8-byte aligned."""
    L = api.lib()
    exact = tier == "A"
    dt = model_dtype(tier)
    assert N & 1
    rp, ci, val, x, y = M.spmv_inputs(nrows, N, 2000 + nrows, exact)
    rps, cis = csr_slots(pool, rp, ci)
    vs, xs, x4s = pool.slot(val), pool.slot(x, 1), pool.slot(sent(4 * N))
    cut = [0, 1, min(N, 257), N]
    for a, b in zip(cut[:-1], cut[1:]):
        L.dfl_interleave4(a, b, N, xs.ptr, x4s.ptr, None)
        api.sync()
        idx, want = M.interleave4(0, b, N, x)  # the ranges so far; the nodes from b on still hold the sentinel
        verify(x4s, idx, want, "interleave4 [%d,%d)" % (a, b))
    L.dfl_interleave4(3, 3, N, xs.ptr, x4s.ptr, None)  # empty range
    api.sync()
    x4s.image[x4s.lo: x4s.lo + 4 * N] = x4s.get()  # from here on x4 is a const input
    untouched("interleave4", xs)
    alpha = -2.0 if exact else -1.7
    for row0, row1 in ((0, nrows), (1, nrows), (min(5, nrows), min(nrows, 40)), (min(33, nrows), nrows)):
        ya, yb = pool.slot(sent(4 * N), 1), pool.slot(sent(4 * N), 1)
        L.dfl_bcsr_spmv_x4(row0, row1, N, rps.ptr, cis.ptr, vs.ptr, alpha, x4s.ptr, ya.ptr, None)
        L.dfl_bcsr_spmv_range(row0, row1, N, rps.ptr, cis.ptr, vs.ptr, alpha, xs.ptr, 0.0, yb.ptr, None)
        api.sync()
        rows = np.arange(row0, max(row0, row1))
        what = "spmv_x4 [%d,%d)" % (row0, row1)
        idx, want = M.bcsr_spmv(rows, N, rp, ci, val, alpha, x, 0.0, None, dt)
        bound = None if exact else M.spmv_bound(rows, N, rp, ci, val, alpha, x, 0.0, None)
        got = verify(ya, idx, want, what, bound, "bcsr_spmv_x4", "nrows%d-N%d-%s %s" % (nrows, N, tier, what))
        assert_bits(got, yb.get(), what + ": bitwise the same y as the plain-layout kernel")
        untouched(what, rps, cis, vs, xs, x4s)


@pytest.mark.parametrize("tier", TIERS)
def test_values_to_f32(tier, api, pool):
    """n in {1..5, 1023, 1024, 1025}: the vector body, the scalar tail for n % 4 != 0 and both around a block edge"""
    L = api.lib()
    rng = np.random.default_rng(31)
    for n in (1, 2, 3, 4, 5, 1023, 1024, 1025):
        val = M.values(rng, n, tier == "A")
        vs, fs = pool.slot(val), pool.slot(sent(n, F32), 0, F32)
        L.dfl_bcsr_values_to_f32(n, vs.ptr, fs.ptr, None)
        api.sync()
        verify(fs, np.arange(n), M.values_to_f32(n, val), "values_to_f32 n=%d" % n, dtype=F32)
        untouched("values_to_f32", vs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrows,N", [(1, 139), (33, 33), (255, 293), (256, 256), (257, 295), (513, 551)], ids=lambda v: str(v))
def test_bcsr_spmv_f32(nrows, N, tier, api, pool):
    """dfl_bcsr_values_to_f32 with n = 16 nnz, then dfl_bcsr_spmv_f32 (8-wide trips need len >= 16, the 4-wide and the
    single tail every residue); the float-rounded values are the model's exact input"""
    L = api.lib()
    exact = tier == "A"
    rp, ci, val, x, _ = M.spmv_inputs(nrows, N, 3000 + nrows, exact)
    rps, cis = csr_slots(pool, rp, ci)
    vs, fs, xs, ys = pool.slot(val), pool.slot(sent(val.size, F32), 0, F32), pool.slot(x, 1), pool.slot(sent(4 * N), 1)
    L.dfl_bcsr_values_to_f32(val.size, vs.ptr, fs.ptr, None)
    api.sync()
    valf = M.values_to_f32(val.size, val)
    verify(fs, np.arange(val.size), valf, "values_to_f32 n=16 nnz", dtype=F32)
    fs.image[fs.lo: fs.lo + fs.n] = valf
    L.dfl_bcsr_spmv_f32(nrows, N, rps.ptr, cis.ptr, fs.ptr, xs.ptr, ys.ptr, None)
    api.sync()
    rows = np.arange(nrows)
    v64 = valf.astype(F64)
    idx, want = M.bcsr_spmv(rows, N, rp, ci, v64, 1.0, x, 0.0, None, model_dtype(tier))
    bound = None if exact else M.spmv_bound(rows, N, rp, ci, v64, 1.0, x, 0.0, None)
    verify(ys, idx, want, "spmv_f32", bound, "bcsr_spmv_f32", "nrows%d-N%d-%s" % (nrows, N, tier))
    untouched("spmv_f32", rps, cis, vs, fs, xs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrow,ncol", [(1, 120), (7, 101), (33, 150), (257, 257)])
def test_csr_spmv(nrow, ncol, tier, api, pool):
    """scalar CSR, row lengths {0, 1, 7, 8, 9, 17, 100}, both beta paths.  Bound: gamma_k (|alpha| sum |a||x| +
    |beta||y_i|), k = 2 len + 3 (len products, len - 1 additions, alpha, beta, the final addition)"""
    L = api.lib()
    exact = tier == "A"
    rp, ci = M.pattern(M.cycle_lens(M.CSR_LENS, nrow, 40 + nrow, cap=ncol), ncol, 41 + nrow)
    rng = np.random.default_rng(42 + nrow)
    val, x, y = (M.values(rng, n, exact) for n in (ci.size, ncol, nrow))
    rps, cis = csr_slots(pool, rp, ci)
    vs, xs, ys = pool.slot(val, 1), pool.slot(x, 1), pool.slot(y, 1)
    for alpha, beta in ((1.0, 0.0), (-2.0, 0.0), (-2.0, 1.0), (3.0, -3.0)):
        if not exact:
            alpha *= 0.85
        ys.reset(y if beta != 0 else sent(nrow))
        L.dfl_csr_spmv(nrow, rps.ptr, cis.ptr, vs.ptr, alpha, xs.ptr, beta, ys.ptr, None)
        api.sync()
        want = M.csr_spmv(nrow, rp, ci, val, alpha, x, beta, y, model_dtype(tier))
        bound = None
        if not exact:
            bound = M.gamma(2 * np.diff(rp) + 3) * M.csr_spmv(nrow, rp, ci, val, alpha, x, beta, y, LD, absolute=True).astype(F64)
        what = "csr_spmv alpha=%g beta=%g" % (alpha, beta)
        verify(ys, np.arange(nrow), want, what, bound, "csr_spmv", "nrow%d-%s %s" % (nrow, tier, what))
        untouched(what, rps, cis, vs, xs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n", [1, 33, 257])
def test_csr_point_jacobi(n, tier, api, pool):
    """PCJacobiDevice and PCJacobiInplaceDevice (x == y): rows without a stored diagonal, empty ones included, are left
    untouched.  One division: |err| <= u |y_i|"""
    L = api.lib()
    exact = tier == "A"
    ncol = max(n, 101)
    rp, ci = M.pattern(M.cycle_lens(M.CSR_LENS, n, 50 + n, cap=ncol), ncol, 51 + n)
    rng = np.random.default_rng(52 + n)
    data, x = M.values(rng, ci.size, exact), M.values(rng, n, exact)
    kd = np.flatnonzero(ci == M.row_of_nnz(rp))
    if n > 1:
        assert 0 < kd.size < n, "the case needs rows with and rows without a diagonal"
    data[kd] = rng.choice([-1.0, 1.0], kd.size) * (2.0 ** rng.integers(-3, 6, kd.size) if exact else 0.5 + rng.random(kd.size))
    rps, cis = csr_slots(pool, rp, ci)
    ds, xs, ys = pool.slot(data, 1), pool.slot(x, 1), pool.slot(sent(n), 1)
    rows, want = M.csr_jacobi(n, data, rp, ci, x, model_dtype(tier))
    bound = None if exact else U * np.abs(want).astype(F64)
    L.PCJacobiDevice(n, ci.size, ds.ptr, rps.ptr, cis.ptr, xs.ptr, ys.ptr)
    api.sync()
    verify(ys, rows, want, "PCJacobiDevice", bound, "csr_jacobi", "n%d-%s" % (n, tier))
    untouched("PCJacobiDevice", rps, cis, ds, xs)
    L.PCJacobiInplaceDevice(n, ci.size, ds.ptr, rps.ptr, cis.ptr, xs.ptr)
    api.sync()
    verify(xs, rows, want, "PCJacobiInplaceDevice", bound, "csr_jacobi_inplace", "n%d-%s" % (n, tier))
    untouched("PCJacobiInplaceDevice", rps, cis, ds)


# ======================================================================================================================
# Jacobi tree
# ======================================================================================================================
def inverse_check(slot, idx, blocks, m, what, kernel, case, restate):
    """device inverses of the [n,m,m] `blocks` against the longdouble inverse, budget c u kappa max|inverse| with
    c = 8 x the largest figure of the float64 restatement `restate` on the same blocks"""
    ref = M.inv_gj(blocks, LD)
    unit = M.inverse_budget(1.0, blocks, ref)
    fig = float((np.abs(restate.astype(LD) - ref).max(axis=(1, 2)).astype(F64) / unit).max())
    c = 8.0 * fig
    bound = np.repeat(c * unit, m * m)
    verify(slot, idx, ref.reshape(-1), what, bound, kernel, case, c=c, restatement=fig)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrows,N", [(1, 1), (33, 40), (257, 257), (513, 520)])
def test_pc_jacobi_setup(nrows, N, tier, api, pool):
    """dfl_pc_jacobi_setup[_rows]: memory image inv(D) row-major and 1 / A_pp; the diagonal is the first, the last or a
    middle entry of its row"""
    L = api.lib()
    rp, ci, val = M.diag_inputs(N, 60 + N, tier == "A")
    rps, cis = csr_slots(pool, rp, ci)
    vs, d33, d1 = pool.slot(val), pool.slot(sent(9 * N), 1), pool.slot(sent(N), 1)
    if nrows == N:
        L.dfl_pc_jacobi_setup(N, rps.ptr, cis.ptr, vs.ptr, d33.ptr, d1.ptr, None)
    else:
        L.dfl_pc_jacobi_setup_rows(nrows, rps.ptr, cis.ptr, vs.ptr, d33.ptr, d1.ptr, None)
    api.sync()
    case = "nrows%d-N%d-%s" % (nrows, N, tier)
    if tier == "A":
        w33, w1 = M.pc_setup(nrows, rp, ci, val, I64)
        verify(d33, np.arange(9 * nrows), w33, "dinv33", zero_sign=False)
        verify(d1, np.arange(nrows), w1, "dinv1")
    else:
        D = val.reshape(-1, 4, 4)[M.diag_pos(rp, ci)[:nrows]]
        inverse_check(d33, np.arange(9 * nrows), D[:, :3, :3], 3, "dinv33", "pc_jacobi_setup", case,
                      M.inv3_closed_f64(D[:, :3, :3]))
        w1 = 1.0 / D[:, 3, 3].astype(LD)
        verify(d1, np.arange(nrows), w1, "dinv1", U * np.abs(w1).astype(F64), "pc_jacobi_setup dinv1", case)
    untouched("pc_jacobi_setup", rps, cis, vs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("N", [1, 33, 257])
def test_block3_invert_and_apply(N, tier, api, pool):
    """dfl_block3_invert in place (row-major in, row-major out) and dfl_block3_apply, which reads the stored 9 numbers
    COLUMN-major.  Apply bound: gamma_5 |A||x| (3 products, 2 additions)"""
    L = api.lib()
    rng = np.random.default_rng(70 + N)
    exact = tier == "A"
    blocks = M.unimodular3(rng, N).astype(F64) if exact else M.dominant_blocks(rng, N, 3)
    ds = pool.slot(blocks.reshape(-1), 1)
    L.dfl_block3_invert(N, ds.ptr, None)
    api.sync()
    if exact:
        verify(ds, np.arange(9 * N), M.inv3(blocks, I64).reshape(-1), "block3_invert", zero_sign=False)
    else:
        inverse_check(ds, np.arange(9 * N), blocks, 3, "block3_invert", "block3_invert", "N%d" % N, M.inv3_closed_f64(blocks))
    img = M.values(rng, 9 * N, exact)  # an unsymmetric image: row- and column-major readings differ
    x = M.values(rng, 3 * N, exact)
    As, xs, ys = pool.slot(img, 1), pool.slot(x, 1), pool.slot(sent(3 * N), 1)
    L.dfl_block3_apply(N, As.ptr, xs.ptr, ys.ptr, None)
    api.sync()
    want = M.block3_apply(N, img, x, model_dtype(tier))
    bound = None if exact else M.gamma(5) * M.block3_apply(N, np.abs(img), np.abs(x), LD).astype(F64)
    verify(ys, np.arange(3 * N), want, "block3_apply", bound, "block3_apply", "N%d-%s" % (N, tier))
    untouched("block3_apply", As, xs)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("nrows,N", [(1, 1), (33, 33), (31, 40), (257, 257), (256, 261)])
def test_pc_jacobi_apply(nrows, N, tier, api, pool):
    """dfl_pc_jacobi_apply[_rows], _apply_scaled[_rows] and _apply_scaled_rows_x4 with n in {4N, 4N+1, 6N}: the tail
    copy starts at an odd offset for odd N; q_out written, d_nrm read from the device; y together with y4; y == NULL
    with n == 4N, where only y4 changes; nrows < N leaves the ghost rows alone.
    Bound: gamma_7 (|A||q|) -- three products and two additions on an input that carries the two roundings of
    x * (1 / nrm) -- and gamma_2 |q| for q_out and the tail"""
    L = api.lib()
    exact = tier == "A"
    dt = model_dtype(tier)
    rng = np.random.default_rng(80 + N)
    d33 = M.values(rng, 9 * N, exact)
    d1 = 2.0 ** rng.integers(-3, 4, N) * rng.choice([-1.0, 1.0], N) if exact else rng.normal(size=N)
    nrm = 8.0 if exact else 2.37
    x = M.values(rng, 6 * N, exact)
    d33s, d1s, xs, nrms = pool.slot(d33, 1), pool.slot(d1, 1), pool.slot(x, 1), pool.slot([nrm])
    qs, ys, y4s = pool.slot(sent(6 * N), 1), pool.slot(sent(6 * N), 1), pool.slot(sent(4 * N))
    case = "nrows%d-N%d-%s" % (nrows, N, tier)

    def check(what, n, scaled, want_y, want_y4):
        ref = M.pc_apply(nrows, N, n, d33, d1, x, nrm if scaled else None, dt)
        ab = None if exact else M.pc_apply(nrows, N, n, d33, d1, x, nrm if scaled else None, LD, absolute=True)
        nt = max(n - 4 * N, 0)
        gy = None if exact else np.concatenate([np.full(4 * nrows, M.gamma(7)), np.full(nt, M.gamma(2))])
        for name, slot, on in (("y", ys, want_y), ("y4", y4s, want_y4), ("q", qs, scaled)):
            if not on:
                untouched(what + " " + name, slot)
                continue
            idx, want = ref[name]
            bound = None
            if not exact:
                g = M.gamma(2) if name == "q" else gy[: idx.size]
                bound = g * np.abs(ab[name][1]).astype(F64)
            if name != "y4" and not want_y:  # y == NULL: the tail copy is skipped with it
                idx, want, bound = idx[: 4 * nrows], want[: 4 * nrows], None if exact else bound[: 4 * nrows]
            verify(slot, idx, want, what + " " + name, bound, "pc_jacobi_apply", case + " " + what + " " + name)
        untouched(what, d33s, d1s, xs, nrms)

    def reset():
        for s in (qs, ys, y4s):
            s.reset()

    for n in (4 * N, 4 * N + 1, 6 * N):
        reset()
        if nrows == N:
            L.dfl_pc_jacobi_apply(N, n, d33s.ptr, d1s.ptr, xs.ptr, ys.ptr, None)
        else:
            L.dfl_pc_jacobi_apply_rows(nrows, N, n, d33s.ptr, d1s.ptr, xs.ptr, ys.ptr, None)
        api.sync()
        check("apply n=%d" % n, n, False, True, False)
        reset()
        if nrows == N:
            L.dfl_pc_jacobi_apply_scaled(N, n, d33s.ptr, d1s.ptr, xs.ptr, nrms.ptr, qs.ptr, ys.ptr, None)
        else:
            L.dfl_pc_jacobi_apply_scaled_rows(nrows, N, n, d33s.ptr, d1s.ptr, xs.ptr, nrms.ptr, qs.ptr, ys.ptr, None)
        api.sync()
        check("apply_scaled n=%d" % n, n, True, True, False)
        for scaled in (True, False):
            reset()
            L.dfl_pc_jacobi_apply_scaled_rows_x4(nrows, N, n, d33s.ptr, d1s.ptr, xs.ptr, nrms.ptr if scaled else None,
                                                 qs.ptr if scaled else None, ys.ptr, y4s.ptr, None)
            api.sync()
            check("apply_x4 scaled=%d n=%d" % (scaled, n), n, scaled, True, True)
    reset()  # y == NULL, n == 4N, unscaled: only y4 changes
    L.dfl_pc_jacobi_apply_scaled_rows_x4(nrows, N, 4 * N, d33s.ptr, d1s.ptr, xs.ptr, None, None, None, y4s.ptr, None)
    api.sync()
    check("apply_x4 y=NULL", 4 * N, False, False, True)
    reset()  # y4 == NULL: only y
    L.dfl_pc_jacobi_apply_scaled_rows_x4(nrows, N, 6 * N, d33s.ptr, d1s.ptr, xs.ptr, None, None, ys.ptr, None, None)
    api.sync()
    check("apply_x4 y4=NULL", 6 * N, False, True, False)


@pytest.mark.parametrize("N", [1, 33, 257, 513])
def test_get_diag(N, api, pool):
    """dfl_bcsr_get_diag with each of its three outputs NULL in turn, MatrixCSRGetDiagGPU and MatrixGetDiagBlockGPU
    (bs in {1, 3}, lda > bs, stride > lda bs: the gaps stay untouched).  Pure copies: bitwise on normal data"""
    L = api.lib()
    rp, ci, val = M.diag_inputs(N, 90 + N, False)
    rps, cis = csr_slots(pool, rp, ci)
    vs = pool.slot(val)
    outs = [pool.slot(sent(9 * N), 1), pool.slot(sent(N), 1), pool.slot(sent(3 * N), 1)]
    want = M.get_diag(N, rp, ci, val)
    for skip in (None, 0, 1, 2):
        for s in outs:
            s.reset()
        L.dfl_bcsr_get_diag(N, rps.ptr, cis.ptr, vs.ptr, *[None if k == skip else s.ptr for k, s in enumerate(outs)], None)
        api.sync()
        for k, s in enumerate(outs):
            if k == skip:
                untouched("get_diag: the other outputs with output %d NULL" % k, s)
            else:
                verify(s, np.arange(s.n), want[k], "get_diag output %d (NULL: %s)" % (k, skip))
        untouched("get_diag", rps, cis, vs)
    rng = np.random.default_rng(91 + N)
    sv, ds = pool.slot(rng.normal(size=ci.size), 1), pool.slot(sent(N), 1)
    L.MatrixCSRGetDiagGPU(sv.ptr, rps.ptr, cis.ptr, ds.ptr, N)
    api.sync()
    verify(ds, np.arange(N), M.csr_get_diag(sv.host(), rp, ci, N), "MatrixCSRGetDiagGPU")
    untouched("MatrixCSRGetDiagGPU", rps, cis, sv)
    for bs in (1, 3):
        lda, stride = bs + 2, (bs + 2) * bs + 3
        mv, out = pool.slot(rng.normal(size=ci.size * bs * bs), 1), pool.slot(sent(N * stride), 1)
        L.MatrixGetDiagBlockGPU(mv.ptr, bs, N, N, rps.ptr, cis.ptr, out.ptr, lda, stride)
        api.sync()
        idx, w = M.get_diag_block(mv.host(), bs, N, rp, ci, lda, stride)
        verify(out, idx, w, "MatrixGetDiagBlockGPU bs=%d" % bs)
        untouched("MatrixGetDiagBlockGPU", rps, cis, mv)


# ======================================================================================================================
# Dirichlet
# ======================================================================================================================
def test_zero_rows(api, pool):
    """dfl_bcsr_zero_rows (comp 0..2) and dfl_bcsr_zero_scalar_rows (shift != 0) on node rows of length 1, 8, 9 and 33:
    duplicated boundary nodes, entries the kernels skip (node < 0, node >= N, scalar row outside [0, 3N)); only the
    `comp` row of the blocks of those node rows changes, every other double of val is bit-identical.
    MatrixCSRZeroRowGPU on a scalar matrix over the same pattern."""
    L = api.lib()
    N = 41
    rp, ci, val = M.diag_inputs(N, 100, False, lens=(1, 8, 9, 33))
    lens = np.diff(rp)
    pick = [int(np.flatnonzero(lens == k)[0]) for k in (1, 8, 9, 33)]
    rps, cis = csr_slots(pool, rp, ci)
    vs = pool.slot(val)
    bnode = np.array(pick + [pick[2], -1, N, N + 3, pick[0], 0, N - 1], I32)
    bs = pool.slot(bnode, 0, I32)
    everything = np.arange(val.size)
    for comp in range(3):
        vs.reset()
        L.dfl_bcsr_zero_rows(N, rps.ptr, cis.ptr, vs.ptr, bnode.size, bs.ptr, comp, 2.5, None)
        api.sync()
        verify(vs, everything, M.zero_rows(N, rp, ci, val, bnode, comp, 2.5), "zero_rows comp=%d" % comp)
        untouched("zero_rows", rps, cis, bs)
    for shift in (7, -5):
        scalar = [3 * n + (k % 3) for k, n in enumerate(pick * 2)] + [-1, 3 * N, 3 * N + 4, 3 * pick[3], 3 * pick[3], 0, 3 * N - 1]
        rows = np.array(scalar, I64) - shift  # the kernel adds the shift back
        rs = pool.slot(rows, 0, I32)
        vs.reset()
        L.dfl_bcsr_zero_scalar_rows(N, rps.ptr, cis.ptr, vs.ptr, rows.size, rs.ptr, shift, -1.5, None)
        api.sync()
        verify(vs, everything, M.zero_scalar_rows(N, rp, ci, val, rows, shift, -1.5), "zero_scalar_rows shift=%d" % shift)
        untouched("zero_scalar_rows", rps, cis, rs)
        sval = val[: ci.size].copy()
        ss = pool.slot(sval, 1)
        L.MatrixCSRZeroRowGPU(ss.ptr, N, N, rps.ptr, cis.ptr, rows.size, rs.ptr, shift, -1.5)
        api.sync()
        verify(ss, np.arange(ci.size), M.csr_zero_row(sval, N, rp, ci, rows, shift, -1.5), "MatrixCSRZeroRowGPU")
        untouched("MatrixCSRZeroRowGPU", rps, cis, rs)


def test_dirichlet_vec_and_row_maps(api, pool):
    """dfl_dirichlet_vec / ApplyBCVecNodalGPU zero b[node*shape + comp] only; GetRowFromNodeGPU / GetNodeFromRowGPU"""
    L = api.lib()
    rng = np.random.default_rng(110)
    for n, shape, comp in ((1, 1, 0), (33, 3, 2), (300, 3, 1), (257, 4, 3)):
        nn = 2 * n + 5
        b = rng.normal(size=nn * shape)
        bnode = rng.choice(nn, n, replace=False).astype(I32)
        bnode[n // 2] = bnode[0]  # one duplicate
        bsl, ns = pool.slot(b, 1), pool.slot(bnode, 0, I32)
        for fn in ("dfl_dirichlet_vec", "ApplyBCVecNodalGPU"):
            bsl.reset()
            if fn == "dfl_dirichlet_vec":
                L.dfl_dirichlet_vec(bsl.ptr, n, ns.ptr, shape, comp, None)
            else:
                L.ApplyBCVecNodalGPU(bsl.ptr, n, ns.ptr, shape, comp)
            api.sync()
            verify(bsl, np.arange(b.size), M.dirichlet_vec(b, bnode, shape, comp), fn)
            untouched(fn, ns)
        rows = pool.slot(bnode, 0, I32)
        L.GetRowFromNodeGPU(n, rows.ptr, shape, comp)
        api.sync()
        verify(rows, np.arange(n), bnode * shape + comp, "GetRowFromNodeGPU", dtype=I32)
        rows.image[rows.lo: rows.lo + n] = bnode * shape + comp
        L.GetNodeFromRowGPU(n, rows.ptr, shape)
        api.sync()
        verify(rows, np.arange(n), bnode, "GetNodeFromRowGPU", dtype=I32)


# ======================================================================================================================
# layout
# ======================================================================================================================
def test_block_export_import(api, pool):
    """dfl_block_export_fs against the numpy restatement of the row-expanded layout, row lengths {1, 15, 16, 17, 33}
    (len >= 17 takes the second trip of the 256-thread loop); dfl_block_import_fs of that export is the bitwise identity
    on val.  Every value is distinct, so a misplaced entry cannot coincide."""
    L = api.lib()
    N = 37
    rp, ci = M.pattern(M.cycle_lens((1, 15, 16, 17, 33), N, 120), 64, 121)
    val = np.random.default_rng(122).permutation(16 * ci.size).astype(F64) + 0.25
    rps = pool.slot(rp, 0, I32)
    vs = pool.slot(val)
    want = M.export_fs(N, rp, val)
    outs = [pool.slot(sent(w.size), k & 1) for k, w in enumerate(want)]
    L.dfl_block_export_fs(N, rps.ptr, vs.ptr, *[s.ptr for s in outs], None)
    api.sync()
    for s, w, name in zip(outs, want, ("A00", "A01", "A10", "A11")):
        verify(s, np.arange(w.size), w, "export " + name)
        s.image[s.lo: s.lo + s.n] = w
    untouched("export", rps, vs)
    v2 = pool.slot(sent(val.size))
    L.dfl_block_import_fs(N, rps.ptr, v2.ptr, *[s.ptr for s in outs], None)
    api.sync()
    verify(v2, np.arange(val.size), val, "import of the export")
    untouched("import", rps, *outs)


# ======================================================================================================================
# scatter launchers (exact tier)
# ======================================================================================================================
NSHL, NEL, NSC = 4, 5, 40


def scatter_setup(pool, seed):
    ien, rp, ci, absent = M.elements_pattern(NEL, NSHL, NSC, seed)
    rps, cis = csr_slots(pool, rp, ci)
    return ien, rp, ci, absent, rps, cis, pool.slot(ien, 0, I32)


BATCHES = [(None, None), (np.array([3, 0, 4, 1], I32), None), (None, np.array([1, 0, 1, 1], I32)),
           (np.array([2, 0, 1, 4], I32), np.array([1, 1, 0, 1], I32))]


@pytest.mark.parametrize("bk", range(len(BATCHES)))
def test_scatter_elem_launchers(bk, api, pool):
    """dfl_bcsr_add_elem_blocked, MatrixCSRAddElemValueBatchedGPU and MatrixCSRAddElemValueBlockedBatchedGPU ((br, bc) in
    {(3,3), (3,1), (1,3)}, lda larger than the block, stride larger than lda br) on conflict-free elements, nshl = 4:
    batch_index_ptr NULL and not, a mask with zeros, one (row, col) pair of element 0 absent from the pattern"""
    L = api.lib()
    bidx, mask = BATCHES[bk]
    nb = 4
    ien, rp, ci, absent, rps, cis, iens = scatter_setup(pool, 130)
    rng = np.random.default_rng(131 + bk)
    bs_ = pool.slot(bidx, 0, I32) if bidx is not None else None
    ms = pool.slot(mask, 0, I32) if mask is not None else None
    p = lambda s: s.ptr if s is not None else None
    consts = [rps, cis, iens] + [s for s in (bs_, ms) if s is not None]
    nnz = ci.size
    alpha, beta = 2.0, -3.0
    # 4x4 blocks of the block-CSR array
    lda, stride = 6, 27
    target, val = M.ints(rng, 16 * nnz), M.ints(rng, nb * 16 * stride)
    ts, vs = pool.slot(target), pool.slot(val, 1)
    L.dfl_bcsr_add_elem_blocked(ts.ptr, alpha, NSHL, nb, p(bs_), iens.ptr, rps.ptr, cis.ptr, vs.ptr, lda, stride, beta, p(ms), None)
    api.sync()
    want = M.elem_scatter(target, np.arange(16 * nnz).reshape(nnz, 4, 4), alpha, NSHL, nb, bidx, ien, rp, ci, 4, 4, val, lda,
                          stride, beta, mask)
    verify(ts, np.arange(target.size), want, "bcsr_add_elem_blocked")
    assert not np.array_equal(want, target)
    untouched("bcsr_add_elem_blocked", vs, *consts)
    # scalar
    target, val = M.ints(rng, nnz), M.ints(rng, nb * 16)
    ts, vs = pool.slot(target, 1), pool.slot(val, 1)
    L.MatrixCSRAddElemValueBatchedGPU(ts.ptr, alpha, nb, p(bs_), iens.ptr, NSHL, NSC, NSC, rps.ptr, cis.ptr, vs.ptr, beta, p(ms))
    api.sync()
    want = M.elem_scatter(target, M.expanded_index(rp, 1, 1), alpha, NSHL, nb, bidx, ien, rp, ci, 1, 1, val, 1, 1, beta, mask)
    verify(ts, np.arange(target.size), want, "MatrixCSRAddElemValueBatchedGPU")
    untouched("MatrixCSRAddElemValueBatchedGPU", vs, *consts)
    # row-expanded blocks
    for br, bc in ((3, 3), (3, 1), (1, 3)):
        lda = bc + 2
        stride = lda * br + 1
        target, val = M.ints(rng, nnz * br * bc), M.ints(rng, nb * 16 * stride)
        ts, vs = pool.slot(target, 1), pool.slot(val, 1)
        L.MatrixCSRAddElemValueBlockedBatchedGPU(ts.ptr, alpha, nb, p(bs_), iens.ptr, NSHL, NSC, NSC, rps.ptr, cis.ptr, br, bc,
                                                 vs.ptr, lda, stride, beta, p(ms))
        api.sync()
        want = M.elem_scatter(target, M.expanded_index(rp, br, bc), alpha, NSHL, nb, bidx, ien, rp, ci, br, bc, val, lda, stride,
                              beta, mask)
        what = "MatrixCSRAddElemValueBlockedBatchedGPU %dx%d" % (br, bc)
        verify(ts, np.arange(target.size), want, what)
        untouched(what, vs, *consts)


def test_scatter_set_value(api, pool):
    """MatrixCSRSetValueBatchedGPU and MatrixCSRSetValueBlockedBatchedGPU: distinct (row, col) pairs, one of them absent"""
    L = api.lib()
    ien, rp, ci, absent, rps, cis, _ = scatter_setup(pool, 140)
    rng = np.random.default_rng(141)
    nnz = ci.size
    k = rng.choice(nnz, 9, replace=False)
    brow = np.concatenate([M.row_of_nnz(rp)[k], [absent[0]]]).astype(I32)
    bcol = np.concatenate([ci[k], [absent[1]]]).astype(I32)
    rs, cs = pool.slot(brow, 0, I32), pool.slot(bcol, 0, I32)
    alpha, beta = -2.0, 3.0
    target, A = M.ints(rng, nnz), M.ints(rng, brow.size)
    ts, As = pool.slot(target, 1), pool.slot(A, 1)
    L.MatrixCSRSetValueBatchedGPU(ts.ptr, alpha, NSC, NSC, rps.ptr, cis.ptr, brow.size, rs.ptr, cs.ptr, As.ptr, beta)
    api.sync()
    want = M.csr_set_blocked(target, alpha, rp, ci, brow, bcol, 1, 1, A, beta, 1, 1)
    verify(ts, np.arange(nnz), want, "MatrixCSRSetValueBatchedGPU")
    untouched("MatrixCSRSetValueBatchedGPU", rps, cis, rs, cs, As)
    for br, bc in ((3, 3), (3, 1), (1, 3)):
        lda = bc + 2
        stride = lda * br + 1
        target, A = M.ints(rng, nnz * br * bc), M.ints(rng, brow.size * stride)
        ts, As = pool.slot(target, 1), pool.slot(A, 1)
        L.MatrixCSRSetValueBlockedBatchedGPU(ts.ptr, alpha, NSC, NSC, rps.ptr, cis.ptr, brow.size, rs.ptr, cs.ptr, br, bc,
                                             As.ptr, beta, lda, stride)
        api.sync()
        want = M.csr_set_blocked(target, alpha, rp, ci, brow, bcol, br, bc, A, beta, lda, stride)
        what = "MatrixCSRSetValueBlockedBatchedGPU %dx%d" % (br, bc)
        verify(ts, np.arange(target.size), want, what)
        untouched(what, rps, cis, rs, cs, As)


@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("with_ptr", [False, True])
def test_scatter_add_element_lhs(bs, with_ptr, api, pool):
    """MatrixCSRAddElementLHSGPU: scalar CSR over node*bs + component, one dense (nshl bs)^2 block per element"""
    L = api.lib()
    ien, rp, ci, absent = M.elements_pattern(NEL, NSHL, NSC, 150)
    srp, sci = M.expand_pattern(rp, ci, bs)
    rps, cis = csr_slots(pool, srp, sci)
    iens = pool.slot(ien, 0, I32)
    rng = np.random.default_rng(151 + bs)
    bptr = np.array([4, 0, 2], I32) if with_ptr else None
    nb = 3
    m = NSHL * bs
    target, val = M.ints(rng, sci.size), M.ints(rng, nb * m * m)
    ts, vs = pool.slot(target, 1), pool.slot(val, 1)
    bp = pool.slot(bptr, 0, I32) if with_ptr else None
    L.MatrixCSRAddElementLHSGPU(ts.ptr, NSHL, bs, NSC * bs, rps.ptr, NSC * bs, cis.ptr, nb, bp.ptr if bp else None, iens.ptr,
                                vs.ptr, m)
    api.sync()
    want = M.csr_add_element_lhs(target, NSHL, bs, srp, sci, nb, bptr, ien, val)
    verify(ts, np.arange(target.size), want, "MatrixCSRAddElementLHSGPU")
    assert not np.array_equal(want, target)
    untouched("MatrixCSRAddElementLHSGPU", rps, cis, iens, vs, *([bp] if bp else []))


# ======================================================================================================================
# DILU
# ======================================================================================================================
DILU_CASES = [(3, 0), (4, 7)]  # (seed, ghost nodes)
_dilu_cache = {}


def dilu_case(seed, nghost):
    """pattern, colouring and lists of a DILU case, built once"""
    key = (seed, nghost)
    if key not in _dilu_cache:
        N, nown, rp, ci, target = M.dilu_pattern(seed, nghost=nghost)
        color = M.greedy_colors(nown, N, rp, ci)
        assert np.array_equal(color, target)
        _dilu_cache[key] = (N, nown, rp, ci, color) + M.dilu_lists(nown, rp, ci, color)
    return _dilu_cache[key]


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("seed,nghost", DILU_CASES)
def test_dilu_setup(seed, nghost, tier, api, pool):
    """dfl_dilu_setup_color colour by colour in order.  Tier A: the rows without lower neighbours (colour 0, signed
    permutation times power-of-two diagonal blocks) have an exact inverse; only colour 0 is launched and only its rows
    of Einv change.  Tier B: all colours against the longdouble recurrence, budget c u kappa_inf(E) max|E^-1|, c from
    the float64 restatement of the whole recurrence (Gauss-Jordan with partial pivoting)"""
    L = api.lib()
    N, nown, rp, ci, color, rows, coff, low, up = dilu_case(seed, nghost)
    exact = tier == "A"
    val = M.dilu_values(np.random.default_rng(160 + seed), N, rp, ci, exact)
    rps, cis = csr_slots(pool, rp, ci)
    vs, cs, rs, Es = pool.slot(val), pool.slot(color, 0, U8), pool.slot(rows, 0, I32), pool.slot(sent(16 * N))
    blk = lambda r: (16 * np.asarray(r, I64)[:, None] + np.arange(16)).ravel()
    if exact:
        r0 = rows[coff[0]: coff[1]]
        L.dfl_dilu_setup_color(r0.size, rs.ptr, nown, rps.ptr, cis.ptr, vs.ptr, cs.ptr, Es.ptr, None)
        api.sync()
        want = M.exact_inverse_perm4(val.reshape(-1, 4, 4)[M.diag_pos(rp, ci)[r0]])
        verify(Es, blk(r0), want.reshape(-1), "dilu_setup colour 0", zero_sign=False)
    else:
        ref = M.dilu_setup(N, nown, rp, ci, val, color, rows, coff, LD)
        f64 = M.dilu_setup(N, nown, rp, ci, val, color, rows, coff, F64)
        for c in range(coff.size - 1):
            L.dfl_dilu_setup_color(coff[c + 1] - coff[c], rs.ptr + 4 * int(coff[c]), nown, rps.ptr, cis.ptr, vs.ptr, cs.ptr,
                                   Es.ptr, None)
            api.sync()
            done = rows[: coff[c + 1]]
            mask = np.zeros(16 * N, bool)
            mask[blk(done)] = True
            Es.check("dilu_setup colour %d: only the rows of the colours launched so far change" % c, mask)
        own = rows[:nown]
        E = M.inv_gj(ref[own], LD)  # the blocks that were inverted
        unit = M.inverse_budget(1.0, E, ref[own])
        fig = float((np.abs(f64[own].astype(LD) - ref[own]).max(axis=(1, 2)).astype(F64) / unit).max())
        verify(Es, blk(own), ref[own].reshape(-1), "dilu_setup", np.repeat(8.0 * fig * unit, 16), "dilu_setup",
               "seed%d-ghost%d" % (seed, nghost), c=8.0 * fig, restatement=fig)
        assert float(M.kappa_inf(E, ref[own]).max()) <= 10.0
    untouched("dilu_setup", rps, cis, vs, cs, rs)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("seed,nghost", DILU_CASES)
def test_dilu_sweep_exact(seed, nghost, f32, api, pool):
    """dfl_dilu_sweep_color[_f32], every colour alone, forward and backward, Tier A: integer blocks, r and z, E^-1 =
    integers / 4.  slot0 > 0 for every colour but the first; colours of 1, 31, 32, 33 and 257 rows; lists of 0 .. 13
    and more neighbours (the four-wide trip twice and every tail); only the rows of the launched colour change in z,
    whose own entries are NaN sentinels on the forward sweep (it must not read them)"""
    L = api.lib()
    N, nown, rp, ci, color, rows, coff, low, up = dilu_case(seed, nghost)
    rng = np.random.default_rng(170 + seed)
    val = M.ints(rng, 16 * ci.size)
    Einv = M.dyadic(rng, 16 * N)
    r, z = M.ints(rng, 4 * N), M.ints(rng, 4 * N)
    rs = pool.slot(rows, 0, I32)
    vs = pool.slot(val.astype(F32), 0, F32) if f32 else pool.slot(val)
    Es, rr, zs = pool.slot(Einv), pool.slot(r, 1), pool.slot(z, 1)
    fn = L.dfl_dilu_sweep_color_f32 if f32 else L.dfl_dilu_sweep_color
    for fwd, (ptr, nz, col) in ((1, low), (0, up)):
        ps, ns, cs = pool.slot(ptr, 0, I32), pool.slot(nz, 0, I32), pool.slot(col, 0, I32)
        for c in range(coff.size - 1):
            nrc = int(coff[c + 1] - coff[c])
            zin = z.copy()
            if fwd:
                zin[M.vec_idx(rows[coff[c]: coff[c + 1]], N)] = sent(1)[0]
            zs.reset(zin)
            fn(fwd, int(coff[c]), nrc, rs.ptr, N, ps.ptr, ns.ptr, cs.ptr, vs.ptr, Es.ptr, rr.ptr, zs.ptr, None)
            api.sync()
            idx, want, _ = M.dilu_sweep(fwd, int(coff[c]), nrc, rows, N, ptr, nz, col, val, Einv, r, zin, I64, einv_shift=2)
            what = "dilu_sweep%s fwd=%d colour %d" % ("_f32" if f32 else "", fwd, c)
            verify(zs, idx, want, what)
            untouched(what, rs, ps, ns, cs, vs, Es, rr)


@pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("seed,nghost", DILU_CASES)
def test_dilu_apply_rounded(seed, nghost, f32, api, pool):
    """the full application -- forward over the colours ascending, backward descending -- equals the model's M^-1 r
    within the bound of matrix_model.dilu_sweep propagated through the colours (dilu_apply); ghost rows of z untouched"""
    L = api.lib()
    N, nown, rp, ci, color, rows, coff, low, up = dilu_case(seed, nghost)
    rng = np.random.default_rng(180 + seed)
    val = M.dilu_values(rng, N, rp, ci, False)
    Einv = M.dilu_setup(N, nown, rp, ci, val, color, rows, coff, F64).reshape(-1)
    r = rng.normal(size=4 * N)
    valf = val.astype(F32)
    rs = pool.slot(rows, 0, I32)
    vs = pool.slot(valf, 0, F32) if f32 else pool.slot(val)
    Es, rr, zs = pool.slot(Einv), pool.slot(r, 1), pool.slot(sent(4 * N), 1)
    fn = L.dfl_dilu_sweep_color_f32 if f32 else L.dfl_dilu_sweep_color
    lists = [[pool.slot(a, 0, I32) for a in t] for t in (low, up)]
    nc = coff.size - 1
    for fwd, t, order in ((1, lists[0], range(nc)), (0, lists[1], range(nc - 1, -1, -1))):
        for c in order:
            fn(fwd, int(coff[c]), int(coff[c + 1] - coff[c]), rs.ptr, N, t[0].ptr, t[1].ptr, t[2].ptr, vs.ptr, Es.ptr, rr.ptr,
               zs.ptr, None)
    api.sync()
    zref, zerr = M.dilu_apply(N, nown, rows, coff, low, up, val, Einv, r, LD, valf=valf if f32 else None)
    idx = M.vec_idx(rows, N)
    verify(zs, idx, zref[idx], "dilu apply", zerr[rows], "dilu_apply" + ("_f32" if f32 else ""), "seed%d-ghost%d" % (seed, nghost))
    untouched("dilu apply", rs, vs, Es, rr, *lists[0], *lists[1])


def test_copy_range(api, pool):
    """dfl_copy_range with odd begin and end, more than one block, and an empty range"""
    L = api.lib()
    x = np.random.default_rng(190).normal(size=700)
    xs, ys = pool.slot(x, 1), pool.slot(sent(700), 1)
    for b, e in ((1, 2), (3, 263), (255, 699), (5, 5), (9, 3)):
        ys.reset()
        L.dfl_copy_range(b, e, xs.ptr, ys.ptr, None)
        api.sync()
        idx = np.arange(b, max(b, e))
        verify(ys, idx, x[idx], "copy_range [%d,%d)" % (b, e))
        untouched("copy_range", xs)


# ======================================================================================================================
# two-level transfer
# ======================================================================================================================
@pytest.mark.parametrize("tier", TIERS)
def test_amg_galerkin(tier, api, pool):
    """dfl_amg_galerkin: lists of {0, 1, 2, 3, 4, 5, 7, 8, 9, 40} fine nonzeros (every residue of the four-way stride,
    more than one trip), several blocks; empty lists give exact +0.  Bound (any association): gamma_len sum |v|"""
    L = api.lib()
    exact = tier == "A"
    lens = M.cycle_lens(M.COARSE_LENS, 23, 200)
    nnzf = int(lens.sum()) + 11
    off, idx = M.coarse_lists(lens, nnzf, 201)
    vf = M.values(np.random.default_rng(202), 16 * nnzf, exact)
    offs, idxs, vfs, vcs = pool.slot(off, 0, I32), pool.slot(idx, 0, I32), pool.slot(vf), pool.slot(sent(16 * lens.size))
    L.dfl_amg_galerkin(lens.size, offs.ptr, idxs.ptr, vfs.ptr, vcs.ptr, None)
    api.sync()
    want = M.galerkin(lens.size, off, idx, vf, model_dtype(tier))
    bound = None if exact else M.gamma(lens)[:, None] * M.galerkin(lens.size, off, idx, vf, LD, absolute=True).astype(F64)
    got = verify(vcs, np.arange(16 * lens.size), want, "galerkin", bound, "amg_galerkin", tier)
    empty = np.flatnonzero(lens == 0)
    assert empty.size and np.all(got.reshape(-1, 16)[empty].view(np.uint64) == 0), "empty lists give +0"
    untouched("galerkin", offs, idxs, vfs)


@pytest.mark.parametrize("tier", TIERS)
def test_amg_restrict_and_prolong(tier, api, pool):
    """dfl_amg_restrict_diff over aggregates of {1, 2, 3, 15, 16, 17, 33, 70} nodes (every residue of the 16-way stride
    and more than one trip), odd N and Nc; dfl_amg_prolong_add_rows with nrows < N accumulates into z on the owned rows
    only.  Bounds: gamma_len sum |r - sub| (one subtraction per term, len - 1 additions in any order); u |z_i| for the
    single addition of the prolongation"""
    L = api.lib()
    exact = tier == "A"
    dt = model_dtype(tier)
    sizes = M.cycle_lens(M.AGG_SIZES, 11, 210)
    aoff, anode, agg = M.aggregates(sizes, 211)
    N, Nc = anode.size, sizes.size
    assert N & 1 and Nc & 1
    rng = np.random.default_rng(212)
    r, sub = M.values(rng, 4 * N, exact), M.values(rng, 4 * N, exact)
    aos, ans, rs, ss, rcs = (pool.slot(aoff, 0, I32), pool.slot(anode, 0, I32), pool.slot(r, 1), pool.slot(sub, 1),
                             pool.slot(sent(4 * Nc), 1))
    L.dfl_amg_restrict_diff(Nc, aos.ptr, ans.ptr, N, rs.ptr, ss.ptr, rcs.ptr, None)
    api.sync()
    idx, want = M.restrict_diff(Nc, aoff, anode, N, r, sub, dt)
    bound = None
    if not exact:
        bound = M.gamma(sizes)[:, None] * M.restrict_diff(Nc, aoff, anode, N, r, sub, LD, absolute=True)[1].astype(F64)
    verify(rcs, idx, want, "restrict_diff", bound, "amg_restrict_diff", tier)
    untouched("restrict_diff", aos, ans, rs, ss)
    xc, z = M.values(rng, 4 * Nc, exact), M.values(rng, 4 * N, exact)
    ags, xcs, zs = pool.slot(agg, 0, I32), pool.slot(xc, 1), pool.slot(z, 1)
    for nrows in (N, N - 40, 1):
        zs.reset()
        L.dfl_amg_prolong_add_rows(nrows, N, ags.ptr, Nc, xcs.ptr, zs.ptr, None)
        api.sync()
        idx, want = M.prolong_add(nrows, N, agg, Nc, xc, z, dt)
        bound = None if exact else U * np.abs(want).astype(F64)
        verify(zs, idx, want, "prolong_add nrows=%d" % nrows, bound, "amg_prolong_add_rows", "%s nrows=%d" % (tier, nrows))
        untouched("prolong_add", ags, xcs)


# ======================================================================================================================
# n == 0
# ======================================================================================================================
def test_zero_rows_launch_nothing(api, pool):
    """every launcher that guards n <= 0 (dfl_block3_invert, dfl_block3_apply, dfl_bcsr_get_diag, dfl_block_export_fs,
    dfl_block_import_fs, MatrixCSRGetDiagGPU and MatrixGetDiagBlockGPU among them) returns without a launch: all buffers
    stay bit-identical"""
    L = api.lib()
    N = 9
    rp, ci, val = M.diag_inputs(N, 220, False)
    rps, cis = csr_slots(pool, rp, ci)
    rng = np.random.default_rng(221)
    a, b, c, d = (pool.slot(rng.normal(size=16 * ci.size)) for _ in range(4))
    ia, ib, ic = (pool.slot(np.arange(N), 0, I32) for _ in range(3))
    f = pool.slot(rng.normal(size=64).astype(F32), 0, F32)
    u8 = pool.slot(np.zeros(N), 0, U8)
    z = None
    L.dfl_bcsr_spmv(0, rps.ptr, cis.ptr, a.ptr, 1.0, b.ptr, 0.0, c.ptr, z)
    L.dfl_bcsr_spmv_rows(0, N, rps.ptr, cis.ptr, a.ptr, 1.0, b.ptr, 1.0, c.ptr, z)
    L.dfl_bcsr_spmv_range(0, 0, N, rps.ptr, cis.ptr, a.ptr, 1.0, b.ptr, 0.0, c.ptr, z)
    L.dfl_interleave4(0, 0, N, b.ptr, c.ptr, z)
    L.dfl_bcsr_spmv_x4(0, 0, N, rps.ptr, cis.ptr, a.ptr, 1.0, b.ptr, c.ptr, z)
    L.dfl_bcsr_values_to_f32(0, a.ptr, f.ptr, z)
    L.dfl_bcsr_spmv_f32(0, N, rps.ptr, cis.ptr, f.ptr, b.ptr, c.ptr, z)
    L.dfl_csr_spmv(0, rps.ptr, cis.ptr, a.ptr, 1.0, b.ptr, 0.0, c.ptr, z)
    L.PCJacobiDevice(0, 0, a.ptr, rps.ptr, cis.ptr, b.ptr, c.ptr)
    L.PCJacobiInplaceDevice(0, 0, a.ptr, rps.ptr, cis.ptr, b.ptr)
    L.dfl_pc_jacobi_setup(0, rps.ptr, cis.ptr, a.ptr, b.ptr, c.ptr, z)
    L.dfl_pc_jacobi_setup_rows(0, rps.ptr, cis.ptr, a.ptr, b.ptr, c.ptr, z)
    L.dfl_pc_jacobi_apply(0, 0, a.ptr, b.ptr, c.ptr, d.ptr, z)
    L.dfl_pc_jacobi_apply_rows(0, 0, 0, a.ptr, b.ptr, c.ptr, d.ptr, z)
    L.dfl_pc_jacobi_apply_scaled(0, 0, a.ptr, b.ptr, c.ptr, a.ptr, d.ptr, d.ptr, z)
    L.dfl_pc_jacobi_apply_scaled_rows(0, 0, 0, a.ptr, b.ptr, c.ptr, a.ptr, d.ptr, d.ptr, z)
    L.dfl_pc_jacobi_apply_scaled_rows_x4(0, 0, 0, a.ptr, b.ptr, c.ptr, a.ptr, d.ptr, d.ptr, d.ptr, z)
    L.dfl_block3_invert(0, a.ptr, z)
    L.dfl_block3_apply(0, a.ptr, b.ptr, c.ptr, z)
    L.dfl_bcsr_get_diag(0, rps.ptr, cis.ptr, a.ptr, b.ptr, c.ptr, d.ptr, z)
    L.MatrixCSRGetDiagGPU(a.ptr, rps.ptr, cis.ptr, b.ptr, 0)
    L.MatrixGetDiagBlockGPU(a.ptr, 3, 0, 0, rps.ptr, cis.ptr, b.ptr, 3, 9)
    L.dfl_bcsr_zero_rows(N, rps.ptr, cis.ptr, a.ptr, 0, ia.ptr, 0, 1.0, z)
    L.dfl_bcsr_zero_scalar_rows(N, rps.ptr, cis.ptr, a.ptr, 0, ia.ptr, 1, 1.0, z)
    L.MatrixCSRZeroRowGPU(a.ptr, N, N, rps.ptr, cis.ptr, 0, ia.ptr, 0, 1.0)
    L.dfl_dirichlet_vec(a.ptr, 0, ia.ptr, 3, 0, z)
    L.ApplyBCVecNodalGPU(a.ptr, 0, ia.ptr, 3, 0)
    L.GetRowFromNodeGPU(0, ia.ptr, 3, 1)
    L.GetNodeFromRowGPU(0, ia.ptr, 3)
    L.dfl_block_export_fs(0, rps.ptr, a.ptr, b.ptr, c.ptr, d.ptr, d.ptr, z)
    L.dfl_block_import_fs(0, rps.ptr, a.ptr, b.ptr, c.ptr, d.ptr, d.ptr, z)
    L.dfl_bcsr_add_elem_blocked(a.ptr, 1.0, 4, 0, None, ia.ptr, rps.ptr, cis.ptr, b.ptr, 4, 16, 1.0, None, z)
    L.MatrixCSRAddElemValueBatchedGPU(a.ptr, 1.0, 0, None, ia.ptr, 4, N, N, rps.ptr, cis.ptr, b.ptr, 1.0, None)
    L.MatrixCSRAddElemValueBlockedBatchedGPU(a.ptr, 1.0, 0, None, ia.ptr, 4, N, N, rps.ptr, cis.ptr, 3, 3, b.ptr, 3, 9, 1.0, None)
    L.MatrixCSRSetValueBatchedGPU(a.ptr, 1.0, N, N, rps.ptr, cis.ptr, 0, ia.ptr, ib.ptr, b.ptr, 1.0)
    L.MatrixCSRSetValueBlockedBatchedGPU(a.ptr, 1.0, N, N, rps.ptr, cis.ptr, 0, ia.ptr, ib.ptr, 3, 3, b.ptr, 1.0, 3, 9)
    L.MatrixCSRAddElementLHSGPU(a.ptr, 4, 1, N, rps.ptr, N, cis.ptr, 0, None, ia.ptr, b.ptr, 4)
    L.dfl_dilu_setup_color(0, ia.ptr, N, rps.ptr, cis.ptr, a.ptr, u8.ptr, b.ptr, z)
    L.dfl_dilu_sweep_color(1, 0, 0, ia.ptr, N, ia.ptr, ib.ptr, ic.ptr, a.ptr, b.ptr, c.ptr, d.ptr, z)
    L.dfl_dilu_sweep_color_f32(0, 0, 0, ia.ptr, N, ia.ptr, ib.ptr, ic.ptr, f.ptr, b.ptr, c.ptr, d.ptr, z)
    L.dfl_copy_range(0, 0, a.ptr, b.ptr, z)
    L.dfl_amg_galerkin(0, ia.ptr, ib.ptr, a.ptr, b.ptr, z)
    L.dfl_amg_restrict_diff(0, ia.ptr, ib.ptr, N, a.ptr, b.ptr, c.ptr, z)
    L.dfl_amg_prolong_add_rows(0, N, ia.ptr, 1, a.ptr, b.ptr, z)
    api.sync()
    untouched("n == 0", rps, cis, a, b, c, d, ia, ib, ic, f, u8)
