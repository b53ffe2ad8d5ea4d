"""Every Krylov kernel of dedflow_amd/csrc (k_blas.hip, k_cgs.hip, k_cgs_block.hip) alone, through its C launcher, against
tests/krylov_model.py.

Tier A (exact): inputs are small integers stored as float64 (generators of krylov_model.py; test_krylov_model_cpu.py
shows that every product and partial sum stays an integer below 2**53 in any order), so the expectation is BITWISE
equality with the int64 model: a dropped, duplicated or misplaced element cannot hide behind a tolerance.
Tier B (rounded): normal random data against the np.longdouble model with a-priori bounds that hold for every
summation order (Higham, Accuracy and Stability of Numerical Algorithms: section 3.1 for sums and dots, Lemmas
19.7-19.9 for rotations, Theorem 8.5 for the triangular solve).  They are loose on purpose: Tier A catches indexing,
Tier B lost precision (a float intermediate, an approximate square root), which shows orders of magnitude above them.
The observed err / bound go to the file named by DFL_PARITY_OUT (profiles/krylov_kernel_parity.jsonl is such a run).

Every array sits inside a larger device buffer between guard bands of 64 sentinel doubles (a NaN with a recognisable
payload), and in the gap [n, ldq) of every basis column where ldq > n.  After each launch the bands, the gaps, every
const input and every entry an output must not touch are compared bit for bit with what was uploaded.  A pointer
offset of one double gives the 8-byte-aligned-only case the solver produces for odd row counts.

Not here, on purpose: no case aims at a fault.  No null or out-of-range pointers, no ncol beyond a launcher's own guard
(dfl_cgs_update_pc_givens_x4 aborts above 1025 columns), and no n <= 0 for the launchers that do not guard it
(dfl_cgs_update, dfl_gemv_n, dfl_ddot, dfl_dnrm2 would ask for an empty grid).
"""
import numpy as np
import pytest

import krylov_model as M
from guarded_buffers import ALL, SENT, Pool, Recorder, assert_bits, bits, sent

pytestmark = pytest.mark.gpu

U = M.U
F64, LD, I64 = np.float64, np.longdouble, np.int64
needs_extended = pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON)
record = Recorder()


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()  # raises if the HIP library is missing: no fallback
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


def with_gaps(Q, n, ncol, ldq):
    Q = Q.copy()
    for j in range(ncol):
        Q[j * ldq + n: (j + 1) * ldq] = SENT
    return Q


def givens_state(pool, it, ldh, hcol, beta_it, gv_prev=None):
    """device state for the Givens step of column `it`: only column `it` of H and beta[it] hold numbers"""
    H = sent((it + 1) * ldh)
    H[it * ldh: it * ldh + it + 1] = hcol
    gv = sent(2 * (it + 1))
    gv[:2 * it] = np.tile([1.0, 0.0], it) if gv_prev is None else gv_prev
    beta = sent(it + 2)
    beta[it] = beta_it
    return pool.slot(H), pool.slot(gv), pool.slot(beta), pool.slot(sent(it + 1))


def check_givens(it, ldh, Hs, gvs, betas, hists, nrm, what, ref=None, beta0=None):
    """the state after the step against the model: `ref` = (H, gv, beta, res_hist) of a model run of its own, or (None)
    one model step from the uploaded state.  Bounds: 12 (iter + 1) u ||column||_2 per column entry (a rotation is at
    most 6 rounded operations, Higham Lemmas 19.7-19.9, twice because the rotation itself is computed) and
    12 (iter + 1) u |beta0| for beta / res_hist.  Written: column `it` rows 0..it+1, gv[2it..2it+1], beta[it..it+1],
    res_hist[it]; everything else must be untouched."""
    m = np.zeros(Hs.n, bool)
    m[it * ldh: it * ldh + it + 2] = True
    H = Hs.check(what + " H", m)
    m = np.zeros(gvs.n, bool)
    m[2 * it: 2 * it + 2] = True
    gv = gvs.check(what + " gv", m)
    m = np.zeros(betas.n, bool)
    m[it: it + 2] = True
    beta = betas.check(what + " beta", m)
    m = np.zeros(hists.n, bool)
    m[it] = True
    hist = hists.check(what + " res_hist", m)
    dt = LD if M.HAVE_EXTENDED else F64
    img = lambda s: s.image[s.lo: s.lo + s.n].astype(dt)
    col0 = np.concatenate([Hs.image[Hs.lo + it * ldh: Hs.lo + it * ldh + it + 1], [nrm]])
    if ref is None:
        rH, rgv, rbeta, rhist = img(Hs), img(gvs), img(betas), img(hists)
        M.givens_step(it, dt(nrm), rH, ldh, rgv, rbeta, rhist, dt)
    else:
        rH, rgv, rbeta, rhist = ref
    big = np.abs(col0).max()  # scaled: the squares of 1e-200 underflow
    bcol = 12 * (it + 1) * U * (big * np.linalg.norm(col0 / big) if big > 0 else 0.0)
    bbeta = 12 * (it + 1) * U * abs(betas.image[betas.lo + it] if beta0 is None else beta0)
    c = slice(it * ldh, it * ldh + it + 1)
    ratio = 0.0
    if bcol > 0:
        ratio = float(np.abs(H[c] - rH[c]).max() / bcol)
    else:
        assert np.all(H[c] == 0)
    assert H[it * ldh + it + 1] == 0.0 and not np.signbit(H[it * ldh + it + 1])
    r = abs(float(rH[it * ldh + it]))
    if r > 0:  # gv = (a / r, b / r): the column error over r, twice (a and r), plus the divisions
        bgv = 2 * bcol / r + 4 * U
        ratio = max(ratio, float(np.abs(gv[2 * it: 2 * it + 2] - rgv[2 * it: 2 * it + 2]).max() / bgv))
    else:
        assert gv[2 * it] == 1.0 and gv[2 * it + 1] == 0.0
    if bbeta > 0:
        ratio = max(ratio, float(np.abs(beta[it: it + 2] - rbeta[it: it + 2]).max() / bbeta),
                    float(abs(hist[it] - rhist[it]) / bbeta))
    assert hist[it] == abs(beta[it + 1])
    assert np.all(np.isfinite(H[c])) and np.all(np.isfinite(gv[2 * it: 2 * it + 2])) and np.all(np.isfinite(beta[it: it + 2]))
    assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)
    return ratio


# ======================================================================================================================
# Tier A
# ======================================================================================================================
@pytest.mark.parametrize("case", M.cgs_cases(), ids=lambda c: "n%d-c%d-pad%d-off%d" % c)
def test_exact_cgs_family(case, api, pool):
    L = api.lib()
    n, ncol, pad, off = case
    ldq = n + pad
    Q, w, h = M.gen_cgs(n * 31 + ncol, n, ncol, ldq)
    ex_d = M.cgs_dots(n, ncol, Q, ldq, w, I64)
    ex_w, ex_s = M.cgs_update(n, ncol, Q, ldq, h, w, I64)
    ex_y = M.gemv_n(n, ncol, Q, ldq, h, I64)
    qs, ws, hs = pool.slot(with_gaps(Q, n, ncol, ldq), off), pool.slot(w, off), pool.slot(h, off)
    nwork = int(L.dfl_cgs_work_size(n, ncol))
    work, out, nrm = pool.slot(sent(nwork)), pool.slot(sent(ncol), off), pool.slot(sent(1))

    def consts(what):  # (Q is never re-uploaded: it is compared after the dots and once more at the very end)
        hs.check(what + ": coefficients")
        work.check(what + ": work", ALL)

    # dots
    L.dfl_cgs_dots(n, ncol, qs.ptr, ldq, ws.ptr, out.ptr, work.ptr, None)
    api.sync()
    assert_bits(out.check("cgs_dots h", ALL), ex_d, "cgs_dots")
    ws.check("cgs_dots: w")
    qs.check("cgs_dots: Q")
    consts("cgs_dots")
    # update, three norm modes
    for take_sqrt, want in ((0, F64(ex_s)), (1, np.sqrt(F64(ex_s))), (None, None)):
        ws.reset()
        nrm.reset()
        work.reset()
        L.dfl_cgs_update(n, ncol, qs.ptr, ldq, hs.ptr, ws.ptr, nrm.ptr if want is not None else None, take_sqrt or 0,
                         work.ptr, None)
        api.sync()
        what = "cgs_update take_sqrt=%s" % take_sqrt
        assert_bits(ws.check(what + " w", ALL), ex_w, what + " w")
        if want is None:
            nrm.check(what + ": d_nrm")
            work.check(what + ": work is not used without a norm")
        else:
            assert_bits(nrm.check(what + " d_nrm", ALL), [want], what + " d_nrm")
            consts(what)
    # update + norm + Givens in two launches
    ws.reset()
    nrm.reset()
    Hs, gvs, betas, hists = givens_state(pool, 0, 4, [2.0], 1.5)
    L.dfl_cgs_update_givens(n, ncol, qs.ptr, ldq, hs.ptr, ws.ptr, nrm.ptr, work.ptr, 0, Hs.ptr, 4, gvs.ptr, betas.ptr,
                            hists.ptr, None)
    api.sync()
    assert_bits(ws.check("cgs_update_givens w", ALL), ex_w, "cgs_update_givens w")
    assert_bits(nrm.check("cgs_update_givens d_nrm", ALL), [np.sqrt(F64(ex_s))], "cgs_update_givens d_nrm")
    consts("cgs_update_givens")
    check_givens(0, 4, Hs, gvs, betas, hists, np.sqrt(F64(ex_s)), "cgs_update_givens")
    # y = Q c: y is output only
    ys = pool.slot(sent(n), off)
    L.dfl_gemv_n(n, ncol, qs.ptr, ldq, hs.ptr, ys.ptr, None)
    api.sync()
    assert_bits(ys.check("gemv_n y", ALL), ex_y, "gemv_n")
    hs.check("gemv_n: c")
    # the plain reductions on column 0 and w
    ws.reset()
    rw = pool.slot(sent(int(L.dfl_reduce_work_size())))
    L.dfl_ddot(n, qs.ptr, ws.ptr, nrm.ptr, rw.ptr, None)
    api.sync()
    assert_bits(nrm.check("ddot", ALL), [M.ddot(n, Q, w, I64)], "ddot")
    L.dfl_dnrm2(n, ws.ptr, nrm.ptr, rw.ptr, None)
    api.sync()
    assert_bits(nrm.check("dnrm2", ALL), [np.sqrt(F64(M.dnrm2_sq(n, w, I64)))], "dnrm2")
    rw.check("reduction work", ALL)
    qs.check("reductions: Q")
    ws.check("reductions: w")


PC_CASES = [(nrows, ncol, (a + b) & 1, (a + 2 * b) % 3) for a, nrows in enumerate((1, 255, 256, 257, 5000))
            for b, ncol in enumerate((1, 4, 5, 41, 130))]


@pytest.mark.parametrize("nrows,ncol,use_z4,ghost", PC_CASES)
def test_exact_update_pc_givens(nrows, ncol, use_z4, ghost, api, pool):
    """ghost = 0: N == nrows; 1, 2: N = nrows + 3 / + 4 (odd and even N, the pressure segment starts at 3N)"""
    L = api.lib()
    N = nrows + (0, 3, 4)[ghost]
    ldq = 6 * N + (ncol & 1)
    k = (nrows + ncol) % 4
    it, ldh = ncol - 1, ncol + 2 + (nrows & 1)
    rows, Qv, wv, hraw, d33, d1 = M.gen_pc(nrows * 7 + ncol, nrows, N, ncol, ldq, k)
    Q = sent(ncol * ldq)
    for j in range(ncol):
        Q[j * ldq + rows] = Qv[j]
    w = sent(6 * N)
    w[rows] = wv
    owned = np.zeros(6 * N, bool)
    owned[rows] = True
    qs, ws, hr = pool.slot(Q), pool.slot(w), pool.slot(hraw)
    d33s, d1s, zs, z4s = pool.slot(d33), pool.slot(d1), pool.slot(sent(6 * N)), pool.slot(sent(4 * N))
    Hs, gvs, betas, hists = givens_state(pool, it, ldh, sent(it + 1), 1.5)
    nrm, flag = pool.slot(sent(1)), pool.slot([0], 0, np.int32)
    if use_z4:
        L.dfl_cgs_update_pc_givens_x4(nrows, N, ncol, qs.ptr, ldq, hr.ptr, ws.ptr, d33s.ptr, d1s.ptr, zs.ptr, z4s.ptr, it,
                                      Hs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, nrm.ptr, flag.ptr, None)
    else:
        L.dfl_cgs_update_pc_givens(nrows, N, ncol, qs.ptr, ldq, hr.ptr, ws.ptr, d33s.ptr, d1s.ptr, zs.ptr, it, Hs.ptr, ldh,
                                   gvs.ptr, betas.ptr, hists.ptr, nrm.ptr, flag.ptr, None)
    api.sync()
    # the model on the same images (sentinels included: ghost rows must come back as they went in)
    mw, mz, mz4 = w.copy(), sent(6 * N), sent(4 * N)
    mH, mgv = Hs.image[Hs.lo: Hs.lo + Hs.n].copy(), gvs.image[gvs.lo: gvs.lo + gvs.n].copy()
    mbeta, mhist = betas.image[betas.lo: betas.lo + betas.n].copy(), sent(it + 1)
    mnrm, mflag = M.update_pc_givens(nrows, N, ncol, Q, ldq, hraw, mw, d33, d1, mz, mz4 if use_z4 else None, it, mH, ldh,
                                     mgv, mbeta, mhist, I64)
    assert mnrm == 2.0 ** k and mflag == 0
    assert_bits(ws.check("w", owned), mw, "w (owned rows updated and scaled, ghost rows untouched)")
    assert_bits(zs.check("z", owned), mz, "z")
    m4 = np.arange(4 * N) < 4 * nrows
    assert_bits(z4s.check("z4", m4 if use_z4 else None), mz4, "z4")
    assert_bits(nrm.check("d_nrm", ALL), [mnrm], "d_nrm")
    assert flag.check("d_flag")[0] == 0
    for s, what in ((qs, "Q"), (hr, "hraw"), (d33s, "dinv33"), (d1s, "dinv1")):
        s.check(what)
    # the copied column: rows 0..it-1 pass the identity rotations unchanged
    assert_bits(Hs.get()[it * ldh: it * ldh + it], hraw[:it], "H[0:iter, iter]")
    Hs.image[Hs.lo + it * ldh: Hs.lo + it * ldh + it + 1] = hraw[:ncol]  # what the step started from
    check_givens(it, ldh, Hs, gvs, betas, hists, mnrm, "update_pc_givens")


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 20015])
@pytest.mark.parametrize("off", [0, 1])
def test_exact_dscal_inv_dev(n, off, api, pool):
    L = api.lib()
    x = np.random.default_rng(n).integers(-100, 101, size=n).astype(F64)
    xs, sc = pool.slot(x, off), pool.slot([8.0])
    L.dfl_dscal_inv_dev(n, sc.ptr, xs.ptr, None)
    api.sync()
    assert_bits(xs.check("x", ALL), M.scal_inv(n, 8.0, x, I64), "dscal_inv_dev")
    sc.check("scale")


def test_exact_dsqrt_dev(api, pool):
    v = pool.slot([1234321.0])  # 1111**2
    api.lib().dfl_dsqrt_dev(v.ptr, None)
    api.sync()
    assert_bits(v.check("value", ALL), [1111.0], "dsqrt_dev")


@pytest.mark.parametrize("N", [1, 2, 255, 257, 70001])
@pytest.mark.parametrize("take_sqrt", [0, 1])
def test_exact_norms4(N, take_sqrt, api, pool):
    L = api.lib()
    F = M.gen_states(N, N, 1)[0]
    fs, out, work = pool.slot(F), pool.slot(sent(4)), pool.slot(sent(int(L.dfl_reduce_work_size())))
    L.dfl_norms4(N, fs.ptr, out.ptr, take_sqrt, work.ptr, None)
    api.sync()
    want = M.norms4(N, F, I64).astype(F64)
    assert_bits(out.check("out", ALL), np.sqrt(want) if take_sqrt else want, "norms4")
    fs.check("F")
    work.check("work", ALL)


ALPHA_N = [1, 255, 256, 257, 10001]


@pytest.mark.parametrize("N", ALPHA_N)
@pytest.mark.parametrize("mode", ["plain", "nodep", "nodep+nodexu", "states1", "states1+nodep"])
def test_exact_alpha_states(N, mode, api, pool):
    L = api.lib()
    wgold, dwgold, dwg, xg = M.gen_states(N + 5, N, 4)
    f = (0.5, 0.25, 2.0, 0.5)
    want_p, want_x = "nodep" in mode, "nodexu" in mode
    ew, ed, enp, enx = M.alpha_states(N, wgold, dwgold, dwg, *f, xg, I64, want_p, want_x)
    ins = [pool.slot(a) for a in (wgold, dwgold, dwg, xg[:3 * N])]
    wa, da, ps, xs = pool.slot(sent(6 * N)), pool.slot(sent(6 * N)), pool.slot(sent(16 * N)), pool.slot(sent(8 * N))
    pp, xp = ps.ptr if want_p else None, xs.ptr if want_x else None
    if mode.startswith("states1"):
        L.dfl_alpha_states(N, ins[0].ptr, ins[1].ptr, ins[2].ptr, *f, ins[3].ptr, wa.ptr, da.ptr, pp, None)
    else:
        L.dfl_alpha_states2(N, ins[0].ptr, ins[1].ptr, ins[2].ptr, *f, ins[3].ptr, wa.ptr, da.ptr, pp, xp, None)
    api.sync()
    assert_bits(wa.check("wgalpha", ALL), ew, "wgalpha (pressure slot 0)")
    assert_bits(da.check("dwgalpha", ALL), ed, "dwgalpha (pressure slot = dwg)")
    assert np.all(ew[3 * N: 4 * N] == 0) and np.array_equal(ed[3 * N: 4 * N], dwg[3 * N: 4 * N])
    if want_p:
        got = ps.check("nodep", ALL)
        assert_bits(got, enp, "nodep")
        assert np.all(bits(got.reshape(N, 16)[:, 14:]) == 0)  # both pad slots are +0
    else:
        ps.check("nodep not asked for")
    if want_x:
        assert_bits(xs.check("nodexu", ALL), enx, "nodexu")
    else:
        xs.check("nodexu not asked for")
    for s, what in zip(ins, ("wgold", "dwgold", "dwg", "xg")):
        s.check(what)


@pytest.mark.parametrize("N", ALPHA_N)
def test_exact_alpha_predict_and_correct(N, api, pool):
    L = api.lib()
    wgold, dwgold, dwg = M.gen_states(N + 9, N, 3)
    ds = pool.slot(dwg)
    L.dfl_alpha_predict(N, 0.25, ds.ptr, None)
    api.sync()
    want = M.alpha_predict(N, 0.25, dwg, I64)
    assert np.array_equal(want[3 * N: 4 * N], dwg[3 * N: 4 * N])
    assert_bits(ds.check("dwg", ALL), want, "alpha_predict (the pressure slot [3N, 4N) is left alone)")
    ds.reset()
    wo, do = pool.slot(wgold), pool.slot(dwgold)
    L.dfl_alpha_correct(N, 0.5, 2.0, wo.ptr, do.ptr, ds.ptr, None)
    api.sync()
    ew, ed = M.alpha_correct(N, 0.5, 2.0, wgold, dwgold, dwg, I64)
    assert np.array_equal(ew[3 * N: 4 * N], wgold[3 * N: 4 * N])
    assert_bits(wo.check("wgold", ALL), ew, "alpha_correct wgold (pressure slot kept)")
    assert_bits(do.check("dwgold", ALL), ed, "alpha_correct dwgold = dwg on all slots")
    ds.check("dwg")


H_LO = np.array([999.0, 30, 9, 3, 3])    # sum of squares 999000
H_HI = np.array([1000.0, 30, 10, 0, 0])  # 1001000
PYTH = {
    "kept-above-1e-6": (H_LO, 999000.0 + 1.0),    # r = 1 >= 1e-6 ww: flag 0
    "kept-below-1e-6": (H_HI, 1001000.0 + 1.0),   # r = 1 <  1e-6 ww: flag 1, nrm still exact
    "kept-16": (H_LO, 999000.0 + 16.0),
    "kept-large": (np.array([3.0, -2, 1, 0, 2]), 18.0 + 4.0 ** 9),
    "equal": (H_LO, 999000.0),                    # nrm = 0, flag 1
    "negative": (H_LO, 998000.0),                 # clamped to 0, flag 1
}


@pytest.mark.parametrize("name", list(PYTH))
@pytest.mark.parametrize("null_flag", [False, True])
def test_exact_givens_pythagoras(name, null_flag, api, pool):
    L = api.lib()
    h, ww = PYTH[name]
    it, ldh = h.size - 1, h.size + 3
    mnrm, mflag = M.pythagoras_norm(h, ww, I64)
    Hs, gvs, betas, hists = givens_state(pool, it, ldh, h, 1.5)
    Hs.image[Hs.lo + it * ldh + it + 1] = ww
    Hs.reset()
    nrm, flag = pool.slot(sent(1)), pool.slot([0], 0, np.int32)
    L.dfl_gmres_givens_pythagoras(it, nrm.ptr, Hs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, None if null_flag else flag.ptr,
                                  None)
    api.sync()
    assert_bits(nrm.check("d_nrm", ALL), [mnrm], "pythagoras d_nrm")
    assert flag.check("d_flag", ALL)[0] == (0 if null_flag else mflag)
    check_givens(it, ldh, Hs, gvs, betas, hists, mnrm, "givens_pythagoras " + name)
    if mnrm > 0 and not null_flag:  # the fused kernel takes the same norm from the same hraw, bit for bit
        nrows = N = 3
        hraw = np.concatenate([h, [ww]])
        q = pool.slot(np.ones(h.size * 6 * N))
        w, z = pool.slot(np.ones(6 * N)), pool.slot(sent(6 * N))
        d33, d1, hr = pool.slot(np.ones(9 * nrows)), pool.slot(np.ones(nrows)), pool.slot(hraw)
        H2, gv2, beta2, hist2 = givens_state(pool, it, ldh, sent(it + 1), 1.5)
        nrm2, flag2 = pool.slot(sent(1)), pool.slot([0], 0, np.int32)
        L.dfl_cgs_update_pc_givens(nrows, N, h.size, q.ptr, 6 * N, hr.ptr, w.ptr, d33.ptr, d1.ptr, z.ptr, it, H2.ptr, ldh,
                                   gv2.ptr, beta2.ptr, hist2.ptr, nrm2.ptr, flag2.ptr, None)
        api.sync()
        assert_bits(nrm2.get(), nrm.get(), "fused norm against the wrapper's")
        assert flag2.get()[0] == mflag
        for a, b, what in ((H2, Hs, "H"), (gv2, gvs, "gv"), (beta2, betas, "beta"), (hist2, hists, "res_hist")):
            assert_bits(a.get(), b.get(), "fused kernel against givens_pythagoras: " + what)


def test_fused_norm_equals_wrapper_on_random_data(api, pool):
    """cgs_update_pc_kernel recomputes the norm in every block in the order of gmres_givens_pythagoras_kernel: equal bits
    on rounded data too"""
    L = api.lib()
    rng = np.random.default_rng(41)
    ncol, nrows, N = 41, 700, 703
    it, ldh = ncol - 1, ncol + 2
    h = rng.normal(size=ncol)
    ww = float(np.sum(h * h) * 1.37)
    Hs, gvs, betas, hists = givens_state(pool, it, ldh, h, 0.8)
    Hs.image[Hs.lo + it * ldh + it + 1] = ww
    Hs.reset()
    nrm, flag = pool.slot(sent(1)), pool.slot([0], 0, np.int32)
    L.dfl_gmres_givens_pythagoras(it, nrm.ptr, Hs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, flag.ptr, None)
    i = np.arange(nrows)
    rows = np.concatenate([3 * i, 3 * i + 1, 3 * i + 2, 3 * N + i])
    Q, w = sent(ncol * 6 * N), sent(6 * N)
    for j in range(ncol):
        Q[j * 6 * N + rows] = rng.normal(size=rows.size)
    w[rows] = rng.normal(size=rows.size)
    q, ws, z = pool.slot(Q), pool.slot(w), pool.slot(sent(6 * N))
    d33, d1, hr = pool.slot(rng.normal(size=9 * nrows)), pool.slot(rng.normal(size=nrows)), pool.slot(np.concatenate([h, [ww]]))
    H2, gv2, beta2, hist2 = givens_state(pool, it, ldh, sent(it + 1), 0.8)
    nrm2, flag2 = pool.slot(sent(1)), pool.slot([0], 0, np.int32)
    L.dfl_cgs_update_pc_givens(nrows, N, ncol, q.ptr, 6 * N, hr.ptr, ws.ptr, d33.ptr, d1.ptr, z.ptr, it, H2.ptr, ldh,
                               gv2.ptr, beta2.ptr, hist2.ptr, nrm2.ptr, flag2.ptr, None)
    api.sync()
    assert_bits(nrm2.get(), nrm.get(), "fused norm against the wrapper's")
    assert flag.get()[0] == 0 and flag2.get()[0] == 0
    for a, b, what in ((H2, Hs, "H"), (gv2, gvs, "gv"), (beta2, betas, "beta"), (hist2, hists, "res_hist")):
        assert_bits(a.get(), b.get(), "fused kernel against givens_pythagoras: " + what)
    # all blocks scaled by the same bits: w_out * nrm reproduces one common factor (checked against the model in
    # extended precision, (ncol + 2) roundings per entry)
    if M.HAVE_EXTENDED:
        mw, mz = w.astype(LD), sent(6 * N).astype(LD)
        hraw = np.concatenate([h, [ww]])
        M.update_pc_givens(nrows, N, ncol, Q, 6 * N, hraw, mw, d33.get(), d1.get(), mz, None, it,
                           sent((it + 1) * ldh).astype(LD), ldh, np.tile([1.0, 0.0], it + 1).astype(LD),
                           np.full(it + 2, 0.8, LD), None, LD)
        s = 1 / np.sqrt(LD(ww) - np.sum(h.astype(LD) ** 2))
        mag = (np.abs(w[rows]) + np.abs(Q.reshape(ncol, -1)[:, rows] * h[:, None]).sum(axis=0)).astype(LD) * s
        bound = (ncol + 3) * U * mag + (ncol + 40) * U * np.abs(mw[rows])  # the norm itself carries ncol + O(1) roundings
        ratio = float((np.abs(ws.get()[rows] - mw[rows]) / bound).max())
        record("cgs_update_pc_givens w", "nrows700-ncol41", ratio)
        assert ratio <= 1.0
    owned = np.zeros(6 * N, bool)
    owned[rows] = True
    ws.check("w ghost rows", owned)
    z.check("z ghost rows", owned)


# ======================================================================================================================
# Tier B
# ======================================================================================================================
TIER_B_CGS = [(20015, 37, 1, 1), (2049, 129, 0, 0), (256 * 2048 + 7, 9, 5, 1), (1025, 8, 0, 1), (20014, 200, 1, 0)]


@needs_extended
@pytest.mark.parametrize("case", TIER_B_CGS, ids=lambda c: "n%d-c%d-pad%d-off%d" % c)
def test_rounded_cgs_family(case, api, pool):
    """|err| <= n_terms u sum_i |x_i y_i| for every summation order (Higham 3.1); n_terms = ncol + 1 per entry of an
    update.  Norms: the same bound on the sum of squares (plus the error the entries themselves carry), through the
    square root: d sqrt(s) = ds / (2 sqrt(s)), plus the rounding of the root (2u covers it and the second-order terms)."""
    L = api.lib()
    n, ncol, pad, off = case
    ldq = n + pad
    rng = np.random.default_rng(n + ncol)
    Q = np.zeros(ncol * ldq)
    for j in range(ncol):
        Q[j * ldq: j * ldq + n] = rng.normal(size=n)
    w, h = rng.normal(size=n), rng.normal(size=ncol)
    Qm = np.stack([Q[j * ldq: j * ldq + n] for j in range(ncol)])
    cid = "n%d-c%d-pad%d-off%d" % case
    qs, ws, hs = pool.slot(with_gaps(Q, n, ncol, ldq), off), pool.slot(w, off), pool.slot(h, off)
    work, out, nrm = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol)))), pool.slot(sent(ncol), off), pool.slot(sent(1))
    # dots, twice on the same buffers
    runs = []
    for _ in range(2):
        out.reset()
        L.dfl_cgs_dots(n, ncol, qs.ptr, ldq, ws.ptr, out.ptr, work.ptr, None)
        api.sync()
        runs.append(out.check("h", ALL).copy())
    assert_bits(runs[1], runs[0], "cgs_dots is reproducible")
    ref = M.cgs_dots(n, ncol, Q, ldq, w, LD)
    bound = n * U * (np.abs(Qm) * np.abs(w)).sum(axis=1)
    ratio = float((np.abs(runs[0] - ref) / bound).max())
    record("cgs_dots", cid, ratio)
    assert ratio <= 1.0
    # update with the norm, twice
    ref_w, ref_ss = M.cgs_update(n, ncol, Q, ldq, h, w, LD)
    bw = (ncol + 1) * U * (np.abs(w) + (np.abs(Qm) * np.abs(h)[:, None]).sum(axis=0))
    ref_nrm = np.sqrt(ref_ss)
    bss = float(np.sum(2 * np.abs(ref_w) * bw + bw * bw) + (n + 1) * U * ref_ss)
    bnrm = bss / (2 * float(ref_nrm)) + 2 * U * float(ref_nrm)
    runs = []
    for _ in range(2):
        ws.reset()
        nrm.reset()
        L.dfl_cgs_update(n, ncol, qs.ptr, ldq, hs.ptr, ws.ptr, nrm.ptr, 1, work.ptr, None)
        api.sync()
        runs.append((ws.check("w", ALL).copy(), nrm.check("nrm", ALL).copy()))
    assert_bits(runs[1][0], runs[0][0], "cgs_update w is reproducible")
    assert_bits(runs[1][1], runs[0][1], "cgs_update norm is reproducible")
    ratio = float((np.abs(runs[0][0] - ref_w) / bw).max())
    record("cgs_update w", cid, ratio)
    assert ratio <= 1.0
    ratio = float(abs(runs[0][1][0] - ref_nrm) / bnrm)
    record("cgs_update d_nrm", cid, ratio)
    assert ratio <= 1.0
    # gemv_n
    ys = pool.slot(sent(n), off)
    L.dfl_gemv_n(n, ncol, qs.ptr, ldq, hs.ptr, ys.ptr, None)
    api.sync()
    ref = M.gemv_n(n, ncol, Q, ldq, h, LD)
    ratio = float((np.abs(ys.check("y", ALL) - ref) / (ncol * U * (np.abs(Qm) * np.abs(h)[:, None]).sum(axis=0))).max())
    record("gemv_n", cid, ratio)
    assert ratio <= 1.0
    # ddot, dnrm2
    ws.reset()
    rw = pool.slot(sent(int(L.dfl_reduce_work_size())))
    got = []
    for _ in range(2):
        L.dfl_ddot(n, qs.ptr, ws.ptr, nrm.ptr, rw.ptr, None)
        api.sync()
        got.append(nrm.get().copy())
        L.dfl_dnrm2(n, ws.ptr, nrm.ptr, rw.ptr, None)
        api.sync()
        got.append(nrm.get().copy())
    assert_bits(got[2], got[0], "ddot is reproducible")
    assert_bits(got[3], got[1], "dnrm2 is reproducible")
    ratio = float(abs(got[0][0] - M.ddot(n, Q, w, LD)) / (n * U * np.sum(np.abs(Qm[0] * w))))
    record("ddot", cid, ratio)
    assert ratio <= 1.0
    rn = np.sqrt(M.dnrm2_sq(n, w, LD))
    ratio = float(abs(got[1][0] - rn) / (n * U * float(rn) / 2 + 2 * U * float(rn)))
    record("dnrm2", cid, ratio)
    assert ratio <= 1.0
    qs.check("Q")
    hs.check("coefficients")
    ws.check("w")


def _hessenberg(rng, m):
    """columns h[0..it] normal, subdiagonal 3 s with s in 1..5: the norm every wrapper can receive exactly"""
    return [rng.normal(size=it + 1) for it in range(m)], 3.0 * rng.integers(1, 6, size=m)


def _run_givens_variant(api, pool, variant, it, ldh, hcol, nrmv, beta_it, gv_prev):
    """one step through one wrapper from the given state; returns the slots"""
    L = api.lib()
    Hs, gvs, betas, hists = givens_state(pool, it, ldh, hcol, beta_it, gv_prev)
    nrm = pool.slot(sent(1))
    if variant == "givens":
        nrm.reset([nrmv])
        L.dfl_gmres_givens(it, nrm.ptr, Hs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, None)
        api.sync()
        assert_bits(nrm.check("d_nrm is const"), [nrmv], "gmres_givens d_nrm")
    elif variant == "sq":
        nrm.reset([nrmv * nrmv])
        L.dfl_gmres_givens_sq(it, nrm.ptr, Hs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, None)
        api.sync()
        assert_bits(nrm.check("d_nrm", ALL), [nrmv], "gmres_givens_sq leaves the square root in d_nrm")
    else:  # update + norm + Givens: w - Q h = s (2, 1, 2, 0, 0), integer partial sums, 9 s^2 in all
        s = nrmv / 3.0
        n, ncol = 5, 2
        Q = np.array([1.0, -2, 3, 0, 1, 2, 0, -1, 1, 3])
        h = np.array([2.0, -1.0])
        w = s * np.array([2.0, 1, 2, 0, 0]) + Q[:5] * h[0] + Q[5:] * h[1]
        qs, hs, ws = pool.slot(Q), pool.slot(h), pool.slot(w)
        work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
        L.dfl_cgs_update_givens(n, ncol, qs.ptr, n, hs.ptr, ws.ptr, nrm.ptr, work.ptr, it, Hs.ptr, ldh, gvs.ptr, betas.ptr,
                                hists.ptr, None)
        api.sync()
        assert_bits(nrm.check("d_nrm", ALL), [nrmv], "cgs_update_givens d_nrm")
    return Hs, gvs, betas, hists


@needs_extended
@pytest.mark.parametrize("m", [1, 2, 40, 200])
def test_rounded_givens_wrappers(m, api, pool):
    """iter = 0..m-1 on a random upper-Hessenberg matrix through the three wrappers, the device carrying its own
    rotations and beta forward as a solve does, against ONE extended-precision model run of all m steps; the three
    wrappers must agree bit for bit (they share givens_step_block)."""
    rng = np.random.default_rng(500 + m)
    cols, sub = _hessenberg(rng, m)
    ldh = m + 3
    gv, beta = np.zeros(2 * m), np.zeros(m + 1)
    beta[0] = 2.5
    worst = 0.0
    mH, mgv, mbeta, mhist = np.zeros(m * ldh, LD), np.zeros(2 * m, LD), np.zeros(m + 1, LD), np.zeros(m, LD)
    mbeta[0] = 2.5
    for it in range(m):
        mH[it * ldh: it * ldh + it + 1] = cols[it]
        M.givens_step(it, LD(sub[it]), mH, ldh, mgv, mbeta, mhist, LD)
        res = [_run_givens_variant(api, pool, v, it, ldh, cols[it], sub[it], beta[it], gv[:2 * it])
               for v in ("givens", "sq", "update")]
        for v, r in zip(("gmres_givens", "gmres_givens_sq", "cgs_update_givens"), res):
            ratio = check_givens(it, ldh, *r, sub[it], "%s m=%d iter=%d" % (v, m, it),
                                 ref=(mH, mgv, mbeta, mhist), beta0=2.5)
            worst = max(worst, ratio)
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert_bits(b.get(), a.get(), "the wrappers agree bit for bit, iter=%d" % it)
        # carry the device's own float64 state forward, as a solve does
        gv[2 * it: 2 * it + 2] = res[0][1].get()[2 * it: 2 * it + 2]
        beta[it: it + 2] = res[0][2].get()[it: it + 2]
        pool.free()
    record("givens wrappers", "m%d" % m, worst)


@needs_extended
def test_rounded_givens_staging_boundary(api, pool):
    """iter = 1021, 1022 (the last staged steps) and 1023, 1024 (the first that walk global memory), ldh = 1030, from a
    precomputed state of random rotations"""
    rng = np.random.default_rng(77)
    ldh = 1030
    worst = 0.0
    for it in (1021, 1022, 1023, 1024):
        ang = rng.uniform(0, 2 * np.pi, size=it)
        gv_prev = np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(-1)
        hcol, nrmv = rng.normal(size=it + 1), 3.0 * rng.integers(1, 6)
        res = [_run_givens_variant(api, pool, v, it, ldh, hcol, nrmv, 0.37, gv_prev) for v in ("givens", "sq", "update")]
        for v, r in zip(("gmres_givens", "gmres_givens_sq", "cgs_update_givens"), res):
            worst = max(worst, check_givens(it, ldh, *r, nrmv, "%s iter=%d" % (v, it)))
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert_bits(b.get(), a.get(), "the wrappers agree bit for bit, iter=%d" % it)
        pool.free()
    record("givens wrappers", "iter1021-1024", worst)


DROTG = [(3, 4), (4, 3), (-3, 4), (-4, 3), (3, 0), (0, 4), (0, 0), (1e-200, 1e-200), (1e200, 1e200)]


@needs_extended
@pytest.mark.parametrize("pair", DROTG, ids=lambda p: "%g_%g" % p)
def test_drotg_branches(pair, api, pool):
    L = api.lib()
    a, b = float(pair[0]), float(pair[1])
    Hs, gvs, betas, hists = givens_state(pool, 0, 5, [a], 1.5)
    nrm = pool.slot([b])
    L.dfl_gmres_givens(0, nrm.ptr, Hs.ptr, 5, gvs.ptr, betas.ptr, hists.ptr, None)
    api.sync()
    ratio = check_givens(0, 5, Hs, gvs, betas, hists, b, "drotg %r" % (pair,))
    record("drotg", "%g_%g" % pair, ratio)
    H, gv = Hs.get(), gvs.get()
    c, s = gv[0], gv[1]
    assert bits(H[1:2])[0] == 0, "H[1, 0] is exactly +0 afterwards"
    if pair == (0, 0):
        assert (c, s, H[0]) == (1.0, 0.0, 0.0)
    else:
        assert abs(c * c + s * s - 1.0) <= 4 * U
        roe = a if abs(a) > abs(b) else b
        assert np.sign(H[0]) == np.sign(roe)  # r takes the sign of the larger entry
        if b == 0:
            assert (c, s) == (1.0, 0.0) and H[0] == a
        if a == 0:
            assert (c, s) == (0.0, 1.0) and H[0] == b


@needs_extended
@pytest.mark.parametrize("m", [1, 2, 40, 87, 88, 129, 300])
@pytest.mark.parametrize("pad", [1, 7])
def test_rounded_trsv(m, pad, api, pool):
    """|y - y_ref| <= 2 m u |U^-1| |U| |y_ref| componentwise (Higham Theorem 8.5, margin 2); m = 87 is the last size
    staged in LDS, 88 the first that reads H from global memory.  The strict lower triangle and the rows >= m hold the
    sentinel: the result must not depend on them."""
    L = api.lib()
    ldh = m + pad
    rng = np.random.default_rng(900 + m)
    Ud = np.triu(rng.normal(size=(m, m)) / np.sqrt(m), 1) + np.diag(rng.uniform(1, 2, size=m))
    H = sent(m * ldh)
    for j in range(m):
        H[j * ldh: j * ldh + j + 1] = Ud[:j + 1, j]
    b = rng.normal(size=m)
    Hs, bs = pool.slot(H), pool.slot(np.concatenate([b, sent(3)]))
    runs = []
    for _ in range(2):
        bs.reset()
        L.dfl_gmres_trsv(m, Hs.ptr, ldh, bs.ptr, None)
        api.sync()
        runs.append(bs.check("beta", np.arange(m + 3) < m)[:m].copy())
    Hs.check("H")
    assert_bits(runs[1], runs[0], "trsv is reproducible")
    y = M.trsv_upper(m, H, ldh, b, LD)
    Ul = Ud.astype(LD)
    assert float(np.abs(Ul @ y - b).max()) < 1e-15  # the reference solves the system
    Uinv = np.zeros((m, m), LD)  # back substitution on the identity
    for i in range(m - 1, -1, -1):
        e = np.zeros(m, LD)
        e[i] = 1
        Uinv[i] = (e - Ul[i, i + 1:] @ Uinv[i + 1:]) / Ul[i, i]
    bound = 2 * m * U * (np.abs(Uinv) @ (np.abs(Ul) @ np.abs(y)))
    ratio = float((np.abs(runs[0] - y) / bound).max())
    record("gmres_trsv", "m%d-ldh%d" % (m, ldh), ratio)
    assert ratio <= 1.0


@needs_extended
@pytest.mark.parametrize("N", [257, 70001])
def test_rounded_norms4(N, api, pool):
    L = api.lib()
    F = np.random.default_rng(N).normal(size=6 * N)
    fs, out, work = pool.slot(F), pool.slot(sent(4)), pool.slot(sent(int(L.dfl_reduce_work_size())))
    runs = []
    for _ in range(2):
        out.reset()
        L.dfl_norms4(N, fs.ptr, out.ptr, 1, work.ptr, None)
        api.sync()
        runs.append(out.check("out", ALL).copy())
    assert_bits(runs[1], runs[0], "norms4 is reproducible")
    ref = np.sqrt(M.norms4(N, F, LD))
    lens = np.array([3 * N, N, N, N])
    ratio = float((np.abs(runs[0] - ref) / ((lens / 2 + 2) * U * ref.astype(F64))).max())
    record("norms4", "N%d" % N, ratio)
    assert ratio <= 1.0
    fs.check("F")
