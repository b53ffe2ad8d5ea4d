"""dfl_bcsr_spmv_x4_pc and dfl_bcsr_spmv_x4_scaled_pc alone (csrc/k_matrix.hip): the interleaved block-CSR product whose row
groups also write z4_out[row][4] = M^-1 y_row of the block-Jacobi tree, on the synthetic patterns of tests/matrix_model.py.

Shapes: N in {1, 7, 33, 257, 513} -- one partial workgroup, then 1, 2 and 3 workgroups per XCD slab of the remapped grid;
row lengths cycling through 1 (the diagonal alone), 2, 3, 4, 5, 7, 8, 9, so that every tail length of the 4-wide trip occurs;
the diagonal is the first, the last or a middle entry of its row in turn (matrix_model.pattern, with_diag).

Per shape, for the plain and the scaled launcher:
  * y is bit for bit what dfl_bcsr_spmv_x4 / _scaled writes from the same inputs;
  * tier A: integer values with velocity diagonal blocks that are triangular with power-of-two diagonals and a power-of-two
    A_pp, whose closed-form inverse (integer cofactors over a power-of-two determinant) is exact in float64: z4_out is bit for
    bit the int64 / dyadic model.  Every product and sum stays an integer below 2**53 over a power of two: |y| <= 9 * 4 * 2**20,
    cofactors <= 2 * 8 * 8, so numerators stay below 2**35.  (The sign of an exact zero is not compared, as for the inverses
    of test_gpu_matrix_kernels.py: an integer model has no -0.)
  * tier B: normal data with diagonally dominant velocity blocks (kappa_inf <= 10, matrix_model.dominant_blocks).  The model
    is the longdouble inverse of the diagonal block applied in longdouble to the device's own y (bitwise the plain kernel's);
    the bound is the one the separate kernels are held to:
        |err z_c| <= gamma_7 sum_r |inv[r][c]| |y_r|  +  c u kappa_inf(D) max|inv(D)| sum_r |y_r|,
    the application bound of test_pc_jacobi_apply plus the inverse budget of test_pc_jacobi_setup (c = 8 x the largest
    figure of the float64 numpy restatement of the closed form on the same blocks), and gamma_2 |y_p / A_pp| for the pressure;
  * the deviation from dfl_pc_jacobi_setup + dfl_pc_jacobi_apply_scaled_rows_x4 of the same build on the same y is printed
    and recorded (DFL_PARITY_OUT; profiles/product_pc_fold_parity.jsonl is such a run);
  * x4, the values, rp, ci, diag_pos and d_nrm are untouched and every guard band is intact;
  * z4_out == x4 is refused: -1, nothing launched, nothing written.
dfl_bcsr_diag_pos is checked against matrix_model.diag_pos on the same patterns.
"""
import ctypes as C

import numpy as np
import pytest

import matrix_model as M
from guarded_buffers import I32, Pool, Recorder, assert_bits, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
U = M.U
LENS = (1, 2, 3, 4, 5, 7, 8, 9)
SIZES = (1, 7, 33, 257, 513)
NRM = {"A": 8.0, "B": 2.37}
record = Recorder("a")
TIERS = ["A", pytest.param("B", marks=pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON))]


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    L = A.lib()  # raises if the HIP library is missing: no fallback
    i32, f64, vp = C.c_int32, C.c_double, C.c_void_p
    for name, res, args in (("dfl_bcsr_spmv_x4", None, [i32, i32, i32, vp, vp, vp, f64, vp, vp, vp]),
                            ("dfl_bcsr_spmv_x4_scaled", None, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
                            ("dfl_bcsr_spmv_x4_pc", C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp]),
                            ("dfl_bcsr_spmv_x4_scaled_pc", C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                            ("dfl_bcsr_diag_pos", None, [i32, vp, vp, vp, vp]),
                            ("dfl_pc_jacobi_setup", None, [i32, vp, vp, vp, vp, vp, vp]),
                            ("dfl_pc_jacobi_apply_scaled_rows_x4", None, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
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


def triangular_pow2(rng, n):
    """n integer 3x3 blocks, upper or lower triangular in turn, diagonal +-2**k (k = 0..3), other entries in [-8, 8]"""
    b = rng.integers(-8, 9, (n, 3, 3)).astype(F64)
    up = (np.arange(n) % 2 == 0)[:, None, None]
    r, c = np.arange(3)[:, None], np.arange(3)[None, :]
    b = np.where(up & (r > c), 0.0, b)
    b = np.where(~up & (r < c), 0.0, b)
    d = np.arange(3)
    b[:, d, d] = rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.integers(0, 4, (n, 3))
    return b


def inputs(N, tier):
    """rp, ci, diag_pos, val [16 nnz], x [4N] (plain layout)"""
    seed = 400 + N
    rp, ci = M.pattern(M.cycle_lens(LENS, N, seed, cap=N), N, seed + 1, with_diag=True)
    rng = np.random.default_rng(seed + 2)
    kd = M.diag_pos(rp, ci)
    if tier == "A":
        val = M.ints(rng, 16 * ci.size).reshape(-1, 4, 4)
        val[kd, :3, :3] = triangular_pow2(rng, N)
        val[kd, 3, 3] = rng.choice([-1.0, 1.0], N) * 2.0 ** rng.integers(0, 6, N)  # (an integer: y stays one for the int64 model)
        val = val.reshape(-1)
    else:
        val = M.tier_b_blocks(rng, rp, ci, True)
    return rp, ci, kd.astype(I32), val, M.values(rng, 4 * N, tier == "A")


def model_z4(tier, N, D, y4, c_budget=None):
    """z4 [N,4] from the stored (already scaled) y4 [N,4] and the diagonal blocks D [N,4,4]; tier B: and its bound"""
    if tier == "A":
        D3 = D[:, :3, :3].astype(I64)
        adj = M.adjugate3(D3)
        det = (D3[:, 0] * adj[:, :, 0]).sum(axis=1)
        assert np.all(np.frexp(np.abs(det).astype(F64))[0] == 0.5) and np.all(np.frexp(np.abs(D[:, 3, 3]))[0] == 0.5)
        # y is an integer over a power of two (the scaled launcher: over 8): numerators in int64, the scalings in float64
        sh = 8.0
        yi = y4 * sh
        assert np.array_equal(yi, np.rint(yi)) and np.abs(yi).max(initial=0) < 2.0 ** 40
        num = np.einsum("nrc,nr->nc", adj, yi[:, :3].astype(I64))
        assert np.abs(num).max(initial=0) < 2 ** 53
        zu = num.astype(F64) / det.astype(F64)[:, None] / sh
        zp = y4[:, 3] / D[:, 3, 3]
        return np.concatenate([zu, zp[:, None]], axis=1), None
    inv = M.inv_gj(D[:, :3, :3], LD)
    y = y4.astype(LD)
    zu = np.einsum("nrc,nr->nc", inv, y[:, :3])
    zp = y[:, 3] / D[:, 3, 3].astype(LD)
    ay = np.abs(y4)
    budget = M.inverse_budget(c_budget, D[:, :3, :3], inv)
    bu = M.gamma(7) * np.einsum("nrc,nr->nc", np.abs(inv).astype(F64), ay[:, :3]) + budget[:, None] * ay[:, :3].sum(axis=1)[:, None]
    bp = M.gamma(2) * np.abs(zp).astype(F64)
    return np.concatenate([zu, zp[:, None]], axis=1), np.concatenate([bu, bp[:, None]], axis=1)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("N", SIZES)
def test_product_pc_fold(N, tier, api, pool):
    L = api.lib()
    rp, ci, dpos, val, x = inputs(N, tier)
    lens = np.diff(rp)
    if N >= 33:  # every length, and the diagonal first, last and in the middle of a row
        where = dpos - rp[:-1]
        assert set(LENS) <= set(int(v) for v in lens)
        assert np.any((where == 0) & (lens > 2)) and np.any((where == lens - 1) & (lens > 2)) and np.any((where > 0) & (where < lens - 1))
    D = val.reshape(-1, 4, 4)[dpos]
    x4 = M.interleave4(0, N, N, x)[1]
    rps, cis, dps = pool.slot(rp, 0, I32), pool.slot(ci, 0, I32), pool.slot(sent(N, I32), 0, I32)
    vs, x4s, nrms = pool.slot(val), pool.slot(x4), pool.slot([NRM[tier]])
    L.dfl_bcsr_diag_pos(N, rps.ptr, cis.ptr, dps.ptr, None)
    api.sync()
    assert_bits(dps.check("diag_pos", True), dpos, "dfl_bcsr_diag_pos", I32)
    dps.reset(dpos)  # from here on a const input
    c_budget = None
    if tier == "B":
        ref = M.inv_gj(D[:, :3, :3], LD)
        assert float(M.kappa_inf(D[:, :3, :3], ref).max()) <= 10.0
        unit = M.inverse_budget(1.0, D[:, :3, :3], ref)
        c_budget = 8.0 * float((np.abs(M.inv3_closed_f64(D[:, :3, :3]).astype(LD) - ref).max(axis=(1, 2)).astype(F64) / unit).max())
    idx4 = M.vec_idx(np.arange(N), N)
    inputs_const = (rps, cis, dps, vs, x4s, nrms)
    for scaled in (False, True):
        what = "N%d-%s %s" % (N, tier, "scaled_pc" if scaled else "pc")
        ys, yr, z4s = pool.slot(sent(4 * N), 1), pool.slot(sent(4 * N), 1), pool.slot(sent(4 * N))
        if scaled:
            rc = L.dfl_bcsr_spmv_x4_scaled_pc(N, rps.ptr, cis.ptr, dps.ptr, vs.ptr, nrms.ptr, x4s.ptr, ys.ptr, z4s.ptr, None)
            L.dfl_bcsr_spmv_x4_scaled(0, N, N, rps.ptr, cis.ptr, vs.ptr, nrms.ptr, x4s.ptr, yr.ptr, None)
        else:
            rc = L.dfl_bcsr_spmv_x4_pc(N, rps.ptr, cis.ptr, dps.ptr, vs.ptr, x4s.ptr, ys.ptr, z4s.ptr, None)
            L.dfl_bcsr_spmv_x4(0, N, N, rps.ptr, cis.ptr, vs.ptr, 1.0, x4s.ptr, yr.ptr, None)
        api.sync()
        assert rc == 0
        y = ys.check(what + " y", True)
        assert_bits(y, yr.check(what + " y of the plain kernel", True), what + ": y bitwise the product without the fold")
        z4 = z4s.check(what + " z4", True).reshape(N, 4)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(z4)), what + ": an entry was not written"
        if tier == "A":  # y itself against the integer model
            s = 1.0 / NRM[tier] if scaled else 1.0
            _, yi = M.bcsr_spmv(np.arange(N), N, rp, ci, val, 1.0, x, 0.0, None, I64)
            assert_bits(y[idx4], yi * s, what + ": y against the int64 model")
        want, bound = model_z4(tier, N, D, y[idx4], c_budget)
        if tier == "A":
            assert_bits(z4 + 0.0, want + 0.0, what + ": z4 against the int64 / dyadic model")
        else:
            err = np.abs(z4.astype(LD) - want).astype(F64)
            ratio = float((err / bound).max())
            print("%s: z4 err / bound %.3g (c = %.3g)" % (what, ratio, c_budget))
            record("bcsr_spmv_x4_pc", what, ratio, c=c_budget)
            assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)
        # the separate kernels of the same build on the same y
        d33, d1, zsep = pool.slot(sent(9 * N), 1), pool.slot(sent(N), 1), pool.slot(sent(4 * N))
        L.dfl_pc_jacobi_setup(N, rps.ptr, cis.ptr, vs.ptr, d33.ptr, d1.ptr, None)
        L.dfl_pc_jacobi_apply_scaled_rows_x4(N, N, 4 * N, d33.ptr, d1.ptr, ys.ptr, None, None, None, zsep.ptr, None)
        api.sync()
        sep = zsep.get().reshape(N, 4)
        dev = float(np.abs(z4 - sep).max() / np.abs(sep).max())
        print("%s: deviation from setup + apply of the same build: %.3g of max|z4|, %d of %d entries differ in bits"
              % (what, dev, int((z4 != sep).sum()), 4 * N))
        record("bcsr_spmv_x4_pc against pc_setup + pc_apply", what, 0.0, rel_dev=dev, entries_differ=int((z4 != sep).sum()))
        for s_ in inputs_const:
            s_.check(what + ": an input changed")
        # the gathered buffer as the output: refused, nothing launched
        ys.reset()
        if scaled:
            rc = L.dfl_bcsr_spmv_x4_scaled_pc(N, rps.ptr, cis.ptr, dps.ptr, vs.ptr, nrms.ptr, x4s.ptr, ys.ptr, x4s.ptr, None)
        else:
            rc = L.dfl_bcsr_spmv_x4_pc(N, rps.ptr, cis.ptr, dps.ptr, vs.ptr, x4s.ptr, ys.ptr, x4s.ptr, None)
        api.sync()
        assert rc == -1, what + ": z4_out == x4 was not refused"
        ys.check(what + ": a refused call wrote y")
        x4s.check(what + ": a refused call wrote x4")
