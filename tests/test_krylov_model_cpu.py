"""CPU checks of tests/krylov_model.py, the numpy model the Krylov kernel tests (tests/test_gpu_krylov_kernels.py)
compare the device with:

  (1) run as a GMRES loop in float64 it reproduces the oracle's history and solution on cube_M4 within the tolerances
      test_gpu_parity.py applies to the device: model and oracle agree on what GMRES is;
  (2) independent of the recurrence: after k Givens steps |beta[k]| is the least-squares residual of
      min ||beta0 e1 - H y|| and trsv_upper returns its minimiser (numpy.linalg.lstsq, 1e-12 relative);
  (3) every Tier A (exact-integer) input generator gives identical float64 bits in three summation orders, equal to the
      int64 model, with every intermediate below 2**53: the condition under which the device tests may demand bitwise
      equality whatever the kernel's reduction order or FMA contraction.
"""
import numpy as np
import pytest

import krylov_model as M
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields

F64 = np.float64
LIMIT = 2.0 ** 53


def test_model_gmres_matches_oracle(oracle_lib):
    m = kuhn_cube(4, jitter=0.2)
    S = oracle_lib.System(m)
    wg, dwg = synthetic_fields(m)
    b, vals = S.assemble_system(wg, dwg, True, True)
    xo, ho, r0o, ito = S.gmres(vals, b)
    d33, d1 = S.pc_setup(vals)
    n, maxit = 6 * S.N, 120
    ldq, ldh = n, maxit + 1
    Q, H = np.zeros((maxit + 1) * ldq), np.zeros(maxit * ldh)
    gv, beta, hist = np.zeros(2 * maxit), np.zeros(maxit + 1), np.zeros(maxit)
    r0 = np.sqrt(M.dnrm2_sq(n, b, F64))
    Q[:n] = M.scal_inv(n, r0, b, F64)
    beta[0] = r0
    it, conv = 0, False
    while not conv and it < maxit:
        w = S.matvec(vals, S.pc_apply(d33, d1, Q[it * ldq: it * ldq + n]))
        h = M.cgs_dots(n, it + 1, Q, ldq, w, F64)
        H[it * ldh: it * ldh + it + 1] = h
        w, ss = M.cgs_update(n, it + 1, Q, ldq, h, w, F64)
        nrm = np.sqrt(ss)
        Q[(it + 1) * ldq: (it + 1) * ldq + n] = M.scal_inv(n, nrm, w, F64)
        M.givens_step(it, nrm, H, ldh, gv, beta, hist, F64)
        if (it + 1) % 20 == 0:
            r = abs(beta[it + 1])
            conv = r < 1e-12 or r < (r0 + 1e-16) * 1e-4
        it += 1
    y = M.trsv_upper(it, H, ldh, beta, F64)
    x = S.pc_apply(d33, d1, M.gemv_n(n, it, Q, ldq, y, F64))
    assert it == ito
    assert abs(r0 - r0o) <= 1e-12 * r0o
    k = np.arange(1, it + 1)
    assert np.all(np.abs(hist[:it] - ho) <= 1e-10 * r0o * np.maximum(1.0, k / 10.0)), np.abs(hist[:it] - ho).max() / r0o
    N4 = 4 * S.N
    assert np.abs(x[:N4] - xo[:N4]).max() <= 1e-8 * np.abs(xo[:N4]).max()


@pytest.mark.parametrize("k", [1, 2, 7, 40])
def test_givens_steps_solve_the_least_squares_problem(k):
    rng = np.random.default_rng(100 + k)
    ldh = k + 3
    Hd = np.triu(rng.normal(size=(k + 1, k)), -1)  # upper Hessenberg, (k+1) x k
    Hd[np.arange(1, k + 1), np.arange(k)] = np.abs(Hd[np.arange(1, k + 1), np.arange(k)]) + 0.5
    beta0 = 1.7
    H = np.zeros(k * ldh)
    gv, beta, hist = np.zeros(2 * k), np.zeros(k + 1), np.zeros(k)
    beta[0] = beta0
    for it in range(k):
        H[it * ldh: it * ldh + it + 1] = Hd[:it + 1, it]
        M.givens_step(it, Hd[it + 1, it], H, ldh, gv, beta, hist, F64)
    y = M.trsv_upper(k, H, ldh, beta, F64)
    rhs = np.zeros(k + 1)
    rhs[0] = beta0
    yl = np.linalg.lstsq(Hd, rhs, rcond=None)[0]
    res = np.linalg.norm(rhs - Hd @ yl)
    assert abs(abs(beta[k]) - res) <= 1e-12 * beta0
    assert hist[k - 1] == abs(beta[k])
    assert np.abs(y - yl).max() <= 1e-12 * np.linalg.cond(Hd) * np.abs(yl).max()


@pytest.mark.parametrize("pair", [(3, 4), (4, 3), (-3, 4), (-4, 3), (3, 0), (0, 4), (0, 0)])
def test_drotg_model_known_answers(pair):
    a, b = F64(pair[0]), F64(pair[1])
    r, z, c, s = M.drotg(a, b, F64)
    if pair == (0, 0):
        assert (r, z, c, s) == (0.0, 0.0, 1.0, 0.0)
        return
    assert abs(abs(r) - np.hypot(a, b)) <= 4 * M.U * np.hypot(a, b)
    assert np.sign(r) == np.sign(a if abs(a) > abs(b) else b)  # the sign of the larger entry
    assert abs(c * a + s * b - r) <= 8 * M.U * abs(r) and abs(c * b - s * a) <= 8 * M.U * abs(r)


# ---- (3) the exactness of every Tier A generator -----------------------------------------------------------------------
def _orders():
    fwd = lambda n: np.arange(n)
    rev = lambda n: np.arange(n)[::-1]
    perm = lambda n: np.random.default_rng(977).permutation(n)
    return (fwd, rev, perm)


def _same_bits(results, exact):
    for r in results:
        r = np.asarray(r, F64)
        assert np.array_equal(r.view(np.uint64), np.asarray(exact).astype(F64).view(np.uint64))


@pytest.mark.parametrize("case", M.cgs_cases(), ids=lambda c: "n%d-c%d-pad%d-off%d" % c)
def test_tier_a_cgs_generator_is_exact_in_every_order(case):
    n, ncol, pad, _ = case
    ldq = n + pad
    Q, w, h = M.gen_cgs(n * 31 + ncol, n, ncol, ldq)
    peak = [0.0]
    ex_d = M.cgs_dots(n, ncol, Q, ldq, w, np.int64)
    ex_w, ex_s = M.cgs_update(n, ncol, Q, ldq, h, w, np.int64)
    ex_y = M.gemv_n(n, ncol, Q, ldq, h, np.int64)
    ex_dot, ex_nn = M.ddot(n, Q, w, np.int64), M.dnrm2_sq(n, w, np.int64)
    for o in _orders():
        _same_bits([M.cgs_dots(n, ncol, Q, ldq, w, F64, order=o, peak=peak)], ex_d)
        gw, gs = M.cgs_update(n, ncol, Q, ldq, h, w, F64, order=o, col_order=o, peak=peak)
        _same_bits([gw], ex_w)
        _same_bits([gs], ex_s)
        _same_bits([M.gemv_n(n, ncol, Q, ldq, h, F64, col_order=o, peak=peak)], ex_y)
        _same_bits([M.ddot(n, Q, w, F64, order=o, peak=peak)], ex_dot)
        _same_bits([M.dnrm2_sq(n, w, F64, order=o, peak=peak)], ex_nn)
    assert peak[0] < LIMIT
    # sufficient for ANY order (trees included): the sum of the magnitudes of the terms stays below 2**53
    assert n * 3 * 4 < LIMIT and int(np.sum(ex_w.astype(object) ** 2)) < LIMIT


PC_CASES = [(nrows, ncol) for nrows in (1, 255, 256, 257, 5000) for ncol in (1, 4, 5, 41, 130)]


@pytest.mark.parametrize("nrows,ncol", PC_CASES)
def test_tier_a_pc_generator_is_exact(nrows, ncol):
    N = nrows + 3
    rows, Qv, wv, hraw, d33, d1 = M.gen_pc(nrows * 7 + ncol, nrows, N, ncol, 6 * N, 2)
    a = wv.astype(np.int64) - (Qv.astype(np.int64) * hraw[:ncol].astype(np.int64)[:, None]).sum(axis=0)
    peak = [0.0]
    for o in _orders():
        acc = wv.copy()
        for j in o(ncol):
            acc -= Qv[j] * hraw[j]
            M._note(peak, acc)
        assert np.array_equal(acc, a)
    nrm, flag = M.pythagoras_norm(hraw[:ncol], hraw[ncol], np.int64)
    assert (nrm, flag) == (4.0, 0)
    assert M.pythagoras_norm(hraw[:ncol], hraw[ncol], F64) == (4.0, 0)
    s = a.astype(F64) / 4.0
    assert np.array_equal(s * 4.0, a)  # the scaling is exact
    A = d33.reshape(nrows, 9)
    t = [A[:, k] * s[q * nrows:(q + 1) * nrows] for k, q in ((0, 0), (3, 1), (6, 2))]
    assert np.array_equal((t[0] + t[1]) + t[2], t[0] + (t[1] + t[2]))  # multiples of 1/4, far below 2**53
    assert np.array_equal((t[0] + t[1]) + t[2], (t[2] + t[0]) + t[1])
    assert peak[0] < LIMIT and np.abs(np.stack(t)).max() * 3 * 4 < LIMIT


@pytest.mark.parametrize("N", [1, 2, 255, 257, 70001])
def test_tier_a_norms4_generator_is_exact_in_every_order(N):
    F = M.gen_states(N, N, 1)[0]
    ex = M.norms4(N, F, np.int64)
    peak = [0.0]
    for o in _orders():
        _same_bits([M.norms4(N, F, F64, order=o, peak=peak)], ex)
    assert peak[0] < LIMIT and 6 * N * 64 < LIMIT


@pytest.mark.parametrize("N", [1, 255, 256, 257, 10001])
def test_tier_a_alpha_generators_are_exact(N):
    """the state kernels reduce nothing; what has to hold is that every fused multiply-add and every separately rounded
    product-then-sum of the dyadic coefficients gives the same float64: compare the float64 model with the int64 one"""
    wgold, dwgold, dwg, xg = M.gen_states(N + 5, N, 4)
    ew, ed, enp, enx = M.alpha_states(N, wgold, dwgold, dwg, 0.5, 0.25, 2.0, 0.5, xg, np.int64, True, True)
    fw, fd, fnp, fnx = M.alpha_states(N, wgold, dwgold, dwg, 0.5, 0.25, 2.0, 0.5, xg, F64, True, True)
    for e, f in ((ew, fw), (ed, fd), (enp, fnp), (enx, fnx)):
        _same_bits([f], e)
    _same_bits([M.alpha_predict(N, 0.25, dwg, F64)], M.alpha_predict(N, 0.25, dwg, np.int64))
    e0, e1 = M.alpha_correct(N, 0.5, 2.0, wgold, dwgold, dwg, np.int64)
    f0, f1 = M.alpha_correct(N, 0.5, 2.0, wgold, dwgold, dwg, F64)
    _same_bits([f0], e0)
    _same_bits([f1], e1)
    assert 8 * (2 + 0.5 + 1) * 4 < LIMIT


def test_scal_inv_power_of_two_is_exact():
    x = np.arange(-8, 9, dtype=F64)
    assert np.array_equal(M.scal_inv(17, 8.0, x, np.int64), x / 8.0)
    assert np.array_equal(M.scal_inv(17, 8.0, x, F64), x / 8.0)


def test_pythagoras_flag_cases():
    """the four regimes the device test uses, decided by the int64 model: each side of 1e-6 ww, ww == hh, ww < hh"""
    lo = np.array([999.0, 30, 9, 3, 3])    # hh = 999000
    hi = np.array([1000.0, 30, 10, 0, 0])  # hh = 1001000
    assert int(np.sum(lo * lo)) == 999000 and int(np.sum(hi * hi)) == 1001000
    assert M.pythagoras_norm(lo, 999000.0 + 1, np.int64) == (1.0, 0)
    assert M.pythagoras_norm(hi, 1001000.0 + 1, np.int64) == (1.0, 1)
    assert M.pythagoras_norm(lo, 999000.0 + 16, np.int64) == (4.0, 0)
    assert M.pythagoras_norm(lo, 999000.0, np.int64) == (0.0, 1)
    assert M.pythagoras_norm(lo, 998000.0, np.int64) == (0.0, 1)
    for h, ww in ((lo, 999001.0), (hi, 1001001.0), (lo, 999000.0), (lo, 998000.0)):
        assert M.pythagoras_norm(h, ww, F64) == M.pythagoras_norm(h, ww, np.int64)


def test_covering_list_covers():
    cs = M.cgs_cases()
    for ax, vals in ((0, M.CGS_N), (1, M.CGS_NCOL), (2, M.CGS_PAD)):
        for v in vals:
            assert len({(c[3], (c[0] + c[2]) & 1) for c in cs if c[ax] == v}) == 4, (ax, v)
    assert all(c[1] <= 9 for c in cs if c[0] > 100000)
    assert max((c[0] + c[2]) * c[1] * 8 for c in cs) <= 256 * 2 ** 20


def test_extended_precision_is_available_or_reported():
    assert M.HAVE_EXTENDED or "64-bit significand" in M.EXTENDED_REASON
