"""The paired raw-basis Arnoldi step (GmresPlan.pair, host/gmres.c: two products, then one dots pass and one update pass over the
Krylov basis for both new vectors): its kernels alone through their C launchers, its two scalar kernels against the numpy
recurrences of two_step_model.py, and the solver against the CPU oracle and against DFL_GMRES_TWO_STEP=0.

Kernel tier, exact as in test_gpu_krylov_kernels.py: integer-valued columns, vectors and coefficients, power-of-two norms and
inverse diagonals; every product and partial sum is an integer multiple of 2**-4 below 2**53, so any summation order and any
fused multiply-add gives the same bits and the expectation is bitwise equality with numpy.  n in {1, 2, 3, 2047, 2048, 2049,
4097} (one entry, a partial double2 slot, the edges of the 2048-row dots block and the 1024-row update block, more than one
block), ncol in {1, 7, 8, 9, 41} (the edge of the 8-column tile), each with ldq = n and with ldq > n and a basis pointer that
is only 8-byte aligned.  The fix-up launch (one column) with N odd and N < 256.

Scalars: pair_first / pair_second alone on synthetic dots and partials for k = 0, 1, 8 against the numpy recurrence, 1e-14
relative to the magnitude of the terms of each entry (the partials are positive: their sums do not cancel).

Solver tier, in child processes (tests/two_step_worker.py) so that DFL_SPMV_X4_MIN=1 is in place when the library first reads
it: Kuhn cubes M = 6 and 8, tolerances 0 unless stated.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import two_step_model as TM
from guarded_buffers import ALL, Pool, assert_bits, sent

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = np.float64
STEP_REFERENCE, STEP_RAW_BASIS = 0, 4

NS = [1, 2, 3, 2047, 2048, 2049, 4097]
NCOLS = [1, 7, 8, 9, 41]
LAYOUTS = [(0, 0), (3, 1)]  # (ldq - n, offset of the basis pointer in doubles)


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    L = A.lib()  # raises if the HIP library is missing: no fallback
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.dfl_cgs_update2_parts.restype, L.dfl_cgs_update2_parts.argtypes = C.c_int, [i32]
    L.dfl_cgs_dots2_raw.restype, L.dfl_cgs_dots2_raw.argtypes = None, [i32, i32, vp, i64] + [vp] * 10
    L.dfl_cgs_update2.restype, L.dfl_cgs_update2.argtypes = None, [i32, i32, vp, i64] + [vp] * 6
    L.dfl_gmres_pair_first.restype, L.dfl_gmres_pair_first.argtypes = None, [C.c_int, vp, i32, vp, vp, vp, i32] + [vp] * 5
    L.dfl_cgs_update_jacobi.restype, L.dfl_cgs_update_jacobi.argtypes = None, [i32, i32, vp, i64] + [vp] * 7
    L.dfl_gmres_pair_second.restype, L.dfl_gmres_pair_second.argtypes = None, [C.c_int, vp, i32, vp, vp, vp, i32] + [vp] * 7
    return A


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def basis(rng, n, ncol, ldq):
    """integer columns, sentinels in the gap [n, ldq) of every column"""
    Q = sent(ncol * ldq)
    Qm = rng.integers(-3, 4, size=(ncol, n)).astype(F64)
    for j in range(ncol):
        Q[j * ldq: j * ldq + n] = Qm[j]
    return Q, Qm


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("n", NS)
def test_exact_dots2(n, ncol, api, pool):
    L = api.lib()
    for pad, off in LAYOUTS:
        ldq = n + pad
        rng = np.random.default_rng(100 * n + ncol + pad)
        Q, Qm = basis(rng, n, ncol, ldq)
        w1, w2 = rng.integers(-50, 51, size=n).astype(F64), rng.integers(-50, 51, size=n).astype(F64)
        nu = (2.0 ** rng.integers(-1, 3, size=ncol)).astype(F64)
        g1 = (Qm.astype(np.int64) * w1.astype(np.int64)).sum(axis=1).astype(F64)
        g2 = (Qm.astype(np.int64) * w2.astype(np.int64)).sum(axis=1).astype(F64)
        qs, w1s, w2s, nus = pool.slot(Q, off), pool.slot(w1), pool.slot(w2), pool.slot(nu)
        outs = [pool.slot(sent(ncol)) for _ in range(5)]  # h1, its copy, c1, e, c2
        work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
        runs = []
        for _ in range(2):
            for o in outs:
                o.reset()
            work.reset()
            L.dfl_cgs_dots2_raw(n, ncol, qs.ptr, ldq, w1s.ptr, w2s.ptr, nus.ptr, *[o.ptr for o in outs], work.ptr, None)
            api.sync()
            runs.append([o.check("output", ALL).copy() for o in outs])
            nrb = (n + 2047) // 2048
            m = np.zeros(work.n, bool)
            m[:2 * ncol * nrb] = True
            work.check("work: one partial per vector, column and block of 2048 rows", m)
            for s, what in ((qs, "Q"), (w1s, "w1"), (w2s, "w2"), (nus, "nu")):
                s.check(what)
        for a, b in zip(runs[0], runs[1]):
            assert_bits(b, a, "run-to-run")
        h1, h1c, c1, e, c2 = runs[0]
        assert_bits(h1, g1 / nu, "h1_j = <r_j, w1> / nu_j")
        assert_bits(h1c, g1 / nu, "the copy of h1")
        assert_bits(c1, g1 / nu / nu, "c1_j = h1_j / nu_j")
        assert_bits(e, g2 / nu, "e_j = <r_j, w2> / nu_j")
        assert_bits(c2, g2 / nu / nu, "c2_j = e_j / nu_j")
        # the single-vector kernel on the same operands: the same bits
        L.dfl_cgs_dots_raw(n, ncol, qs.ptr, ldq, w2s.ptr, nus.ptr, outs[0].ptr, outs[2].ptr, work.ptr, None)
        api.sync()
        assert_bits(outs[0].get(), e, "dfl_cgs_dots_raw on w2")
        pool.free()


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("n", NS)
def test_exact_update2(n, ncol, api, pool):
    L = api.lib()
    for pad, off in LAYOUTS:
        ldq = n + pad
        rng = np.random.default_rng(200 * n + ncol + pad)
        Q, Qm = basis(rng, n, ncol, ldq)
        w1, w2 = rng.integers(-50, 51, size=n).astype(F64), rng.integers(-50, 51, size=n).astype(F64)
        c1, c2 = rng.integers(-2, 3, size=ncol).astype(F64), rng.integers(-2, 3, size=ncol).astype(F64)
        ex1, ex2 = w1 - c1 @ Qm, w2 - c2 @ Qm  # integers: exact in any order
        g = int(L.dfl_cgs_update2_parts(n))
        assert g == (n + 1023) // 1024
        i1, i2 = np.zeros(g * 1024, np.int64), np.zeros(g * 1024, np.int64)
        i1[:n], i2[:n] = ex1.astype(np.int64), ex2.astype(np.int64)
        ex_part = np.concatenate([(a * b).reshape(g, 1024).sum(axis=1) for a, b in ((i1, i1), (i1, i2), (i2, i2))]).astype(F64)
        qs, w1s, w2s, c1s, c2s = pool.slot(Q, off), pool.slot(w1), pool.slot(w2), pool.slot(c1), pool.slot(c2)
        work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
        runs = []
        for _ in range(2):
            w1s.reset()
            w2s.reset()
            work.reset()
            L.dfl_cgs_update2(n, ncol, qs.ptr, ldq, c1s.ptr, c2s.ptr, w1s.ptr, w2s.ptr, work.ptr, None)
            api.sync()
            m = np.zeros(work.n, bool)
            m[:3 * g] = True
            runs.append([w1s.check("w1", ALL).copy(), w2s.check("w2", ALL).copy(), work.check("work: 3 partials per block", m)[:3 * g].copy()])
            for s, what in ((qs, "Q"), (c1s, "c1"), (c2s, "c2")):
                s.check(what)
        for a, b in zip(runs[0], runs[1]):
            assert_bits(b, a, "run-to-run")
        assert_bits(runs[0][0], ex1, "w1' = w1 - Q c1")
        assert_bits(runs[0][1], ex2, "w2' = w2 - Q c2")
        assert_bits(runs[0][2], ex_part, "partials of s11, s12, s22")
        # the single-vector kernel gives the same w1'
        w1s.reset()
        L.dfl_cgs_update(n, ncol, qs.ptr, ldq, c1s.ptr, w1s.ptr, None, 0, work.ptr, None)
        api.sync()
        assert_bits(w1s.get(), ex1, "dfl_cgs_update on w1")
        pool.free()


def jacobi(N, w, d33, d1):
    A, x = d33.reshape(N, 9), w[:3 * N].reshape(N, 3)
    z = np.empty((N, 4))
    for r in range(3):
        z[:, r] = A[:, r] * x[:, 0] + A[:, r + 3] * x[:, 1] + A[:, r + 6] * x[:, 2]
    z[:, 3] = w[3 * N:4 * N] * d1
    return z.reshape(-1)


@pytest.mark.parametrize("use_z4", [True, False], ids=["z4", "noz4"])
@pytest.mark.parametrize("N", [1, 3, 255, 257])
def test_exact_fixup(N, use_z4, api, pool):
    """q = w2' - c w1' with one column and the coefficient in device memory, ||q||^2 partials, z4 = M^-1 q"""
    L = api.lib()
    n = 4 * N
    rng = np.random.default_rng(300 + N)
    p1, p2 = rng.integers(-3, 4, size=n).astype(F64), rng.integers(-50, 51, size=n).astype(F64)
    sc = np.array([float(rng.integers(1, 3)), 7.0, 9.0, 11.0])  # only sc[0] is read
    d33 = (rng.choice([-1.0, 1.0], size=9 * N) * 2.0 ** rng.integers(-2, 3, size=9 * N)).astype(F64)
    d1 = (2.0 ** rng.integers(-2, 3, size=N)).astype(F64)
    ex_q = p2 - sc[0] * p1
    g = (N + 255) // 256
    sq = np.zeros((g, 256, 4))
    node = np.arange(N)
    sq[node // 256, node % 256, :3] = (ex_q[:3 * N] ** 2).reshape(N, 3)
    sq[node // 256, node % 256, 3] = ex_q[3 * N:] ** 2
    ex_part = sq.reshape(g, -1).sum(axis=1)
    p1s, p2s, scs, d33s, d1s = pool.slot(p1), pool.slot(p2), pool.slot(sc), pool.slot(d33), pool.slot(d1)
    z4s = pool.slot(sent(4 * N)) if use_z4 else None
    work = pool.slot(sent(int(L.dfl_cgs_work_size(n, 1))))
    L.dfl_cgs_update_jacobi(N, 1, p1s.ptr, n, scs.ptr, p2s.ptr, d33s.ptr, d1s.ptr, z4s.ptr if z4s else None, work.ptr, None)
    api.sync()
    m = np.zeros(work.n, bool)
    m[:g] = True
    assert_bits(p2s.check("q", ALL), ex_q, "q = w2' - c w1'")
    assert_bits(work.check("work: one partial per block of 256 nodes", m)[:g], ex_part, "partials of ||q||^2")
    if use_z4:
        assert_bits(z4s.check("z4", ALL), jacobi(N, ex_q, d33, d1), "z4 = M^-1 q")
    for s, what in ((p1s, "w1'"), (scs, "sc"), (d33s, "dinv33"), (d1s, "dinv1")):
        s.check(what)


def close(got, want, scale, what):
    err = np.abs(np.asarray(got) - np.asarray(want)) / scale
    print("%s: worst err / (1e-14 scale) %.3g" % (what, np.max(err) / 1e-14))
    assert np.all(err <= 1e-14), what


@pytest.mark.parametrize("k", [0, 1, 8])
def test_pair_scalars(k, api, pool):
    L = api.lib()
    rng = np.random.default_rng(400 + k)
    ldh, ncolH = 32, k + 2
    npart1, npart2 = 37, 300  # fewer and more partials than the 256 threads of the workgroup
    # state at entry: un-rotated columns 0..k-1 (upper Hessenberg), rotations 0..k-1, h1 in column k, beta[k]
    Hraw = sent(ldh * ncolH)
    H = sent(ldh * ncolH)
    for j in range(k):
        Hraw[j * ldh: j * ldh + j + 2] = rng.uniform(0.5, 2.0, size=j + 2) * rng.choice([-1.0, 1.0], size=j + 2)
    h1 = rng.uniform(0.5, 2.0, size=k + 1) * rng.choice([-1.0, 1.0], size=k + 1)
    H[k * ldh: k * ldh + k + 1] = h1
    Hraw[k * ldh: k * ldh + k + 1] = h1
    H[(k + 1) * ldh: (k + 1) * ldh + k + 2] = 0.0
    ang = rng.uniform(0.0, 2 * np.pi, size=k)
    gv = sent(2 * (k + 2))
    gv[0:2 * k:2], gv[1:2 * k:2] = np.cos(ang), np.sin(ang)
    beta = sent(k + 3)
    beta[k] = 1.5
    nu = sent(k + 3)
    nu[:k + 1] = rng.uniform(0.5, 3.0, size=k + 1)
    hist = sent(k + 2)
    e = rng.uniform(0.5, 2.0, size=k + 1) * rng.choice([-1.0, 1.0], size=k + 1)
    part1 = rng.uniform(0.1, 1.0, size=3 * npart1)
    part1[npart1:2 * npart1] *= 0.3  # s12: |s12| < sqrt(s11 s22)
    part2 = rng.uniform(0.1, 1.0, size=npart2)
    # the model
    mH, mHraw, mgv, mbeta, mnu, mhist = H.copy(), Hraw.copy(), gv.copy(), beta.copy(), nu.copy(), hist.copy()
    s11, s12, s22 = (part1[i * npart1:(i + 1) * npart1].sum() for i in range(3))
    msc = TM.pair_first(s11, s12, s22, k, mnu, mH, mHraw, ldh, mgv, mbeta, mhist)
    first = [a.copy() for a in (mH, mHraw, mgv, mbeta, mnu, mhist)]
    mflag = TM.pair_second(part2.sum(), k, mnu, mH, mHraw, ldh, e, msc, mgv, mbeta, mhist)
    # the device
    Hs, Hrs, gvs, betas, nus, hists = (pool.slot(a) for a in (H, Hraw, gv, beta, nu, hist))
    scs, es, p1s, p2s, flag = pool.slot(sent(4)), pool.slot(e), pool.slot(part1), pool.slot(part2), pool.slot(np.zeros(4, np.int32), 0, np.int32)
    L.dfl_gmres_pair_first(npart1, p1s.ptr, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, scs.ptr, None)
    api.sync()
    colk = slice(k * ldh, k * ldh + k + 2)
    hmag = np.abs(np.concatenate([h1, [np.sqrt(s11)]])).max() * (k + 2)  # every rotated entry is a combination of k + 2 of them
    close(scs.get(), msc, np.abs(msc), "sc = [c, d, s22, nu1]")
    close(nus.get()[k + 1], first[4][k + 1], first[4][k + 1], "nu1")
    close(Hs.get()[colk], first[0][colk], hmag, "column k of H, rotated")
    assert_bits(Hrs.get()[k * ldh: k * ldh + k + 1], h1, "un-rotated column k keeps h1")
    close(Hrs.get()[k * ldh + k + 1], first[1][k * ldh + k + 1], first[4][k + 1], "un-rotated H[k+1, k] = nu1")
    close(gvs.get()[2 * k: 2 * k + 2], first[2][2 * k: 2 * k + 2], 1.0, "rotation k")
    close(betas.get()[k: k + 2], first[3][k: k + 2], 1.5, "beta[k], beta[k+1]")
    close(hists.get()[k], first[5][k], 1.5, "res_hist[k]")
    L.dfl_gmres_pair_second(npart2, p2s.ptr, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, es.ptr, scs.ptr, gvs.ptr, betas.ptr, hists.ptr,
                            flag.ptr, None)
    api.sync()
    nu1 = msc[3]
    # magnitude of the terms of row i of the new column
    mag = np.zeros(k + 3)
    for i in range(k + 1):
        mag[i] = (abs(e[i]) + sum(abs(h1[j] * mHraw[j * ldh + i]) for j in range(max(i - 1, 0), k)) + abs(h1[k] * h1[i])) / nu1
    mag[k + 1] = (abs(msc[1]) + abs(h1[k] * nu1)) / nu1
    mag[k + 2] = np.sqrt(part2.sum()) / nu1
    col1 = slice((k + 1) * ldh, (k + 1) * ldh + k + 3)
    close(nus.get()[k + 2], mnu[k + 2], mnu[k + 2], "nu_q")
    close(Hrs.get()[col1], mHraw[col1], mag, "un-rotated column k+1")
    close(Hs.get()[col1][:k + 3], mH[col1][:k + 3], mag.max() * (k + 3), "column k+1 of H, rotated")
    close(gvs.get()[2 * k + 2: 2 * k + 4], mgv[2 * k + 2: 2 * k + 4], 1.0, "rotation k+1")
    close(betas.get()[k: k + 3], mbeta[k: k + 3], 1.5, "beta[k..k+2]")
    close(hists.get()[k: k + 2], mhist[k: k + 2], 1.5, "res_hist[k], res_hist[k+1]")
    assert int(flag.get()[0]) == mflag == 0
    # what a pair must not touch: earlier columns, earlier rotations, the norms before k + 1
    assert_bits(Hrs.get()[:k * ldh], Hraw[:k * ldh], "earlier un-rotated columns")
    assert_bits(Hs.get()[:k * ldh], H[:k * ldh], "earlier columns of H")
    assert_bits(gvs.get()[:2 * k], gv[:2 * k], "earlier rotations")
    assert_bits(nus.get()[:k + 1], nu[:k + 1], "earlier norms")
    for s, what in ((es, "e"), (p1s, "partials of the update"), (p2s, "partials of the fix-up")):
        s.check(what)
    for s, what in ((Hs, "H"), (Hrs, "Hraw"), (gvs, "gv"), (betas, "beta"), (nus, "nu"), (hists, "res_hist"), (scs, "sc")):
        s.check(what + " (guard bands)", ALL)
    # heavy cancellation in the second vector raises the flag: nu_q = 1e-5 sqrt(s22)
    tiny = pool.slot(np.full(npart2, 1e-10 * s22 / npart2))
    L.dfl_gmres_pair_second(npart2, tiny.ptr, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, es.ptr, scs.ptr, gvs.ptr, betas.ptr, hists.ptr,
                            flag.ptr, None)
    api.sync()
    assert int(flag.get()[0]) == 1


# ======================================================================================================================
# solver level
# ======================================================================================================================
SIZES = (6, 8)
CASES = ["default", "it41", "restart15", "x0", "tail", "check5", "conv"]
# (pairs, single steps) of each case: 40 iterations as 20 pairs; 41 with a single-step tail; restart 15 as cycles of 7 pairs + 1,
# 2 pairs + 1 (the check after iteration 20) + 5 pairs, 5 pairs; a check every 5 iterations as 8 x (2 pairs + 1); convergence
# at the first check: 10 pairs counted, the 11th already enqueued and dropped
STEPS = {"default": (20, 0), "it41": (20, 1), "restart15": (19, 2), "x0": (20, 0), "check5": (16, 8), "conv": (10, 0)}


def _child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    env = dict(os.environ)
    env.pop("DFL_GMRES_RAW_BASIS", None)
    env.pop("DFL_GMRES_TWO_STEP", None)
    env["DFL_SPMV_X4_MIN"] = "1"
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "two_step_worker.py"), out] + [str(M) for M in SIZES], env=env,
                       timeout=180, capture_output=True, text=True)
    assert r.returncode == 0, "worker %s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solves(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("two_step")
    return {"pair": _child(tmp, "pair", {}), "single": _child(tmp, "single", {"DFL_GMRES_TWO_STEP": "0"})}


@pytest.fixture(scope="module")
def oracle(oracle_lib, solves):
    """the CPU oracle's solves of the same systems, computed once"""
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    from raw_basis_worker import operands
    ref = {}
    for M in SIZES:
        m = kuhn_cube(M, jitter=0.2)
        wg, dwg = synthetic_fields(m)
        S = oracle_lib.System(m)
        F, vals = S.assemble_system(wg, dwg, True, True)
        b, x0, b_tail = operands(S.N, F)
        kw = dict(atol=0.0, rtol=0.0)
        ref[M, "default"] = S.gmres(vals, b, maxit=40, **kw)
        ref[M, "check5"] = ref[M, "default"]  # how often the host looks does not change the arithmetic
        ref[M, "it41"] = S.gmres(vals, b, maxit=41, **kw)
        ref[M, "x0"] = S.gmres(vals, b, x0=x0, maxit=40, **kw)
        ref[M, "tail"] = S.gmres(vals, b_tail, maxit=40, **kw)
        ref[M, "restart15"] = S.gmres_restarted(vals, b, 15, 40)
        rtol = float(solves["pair"]["M%d/conv/0/scalars" % M][7])
        ref[M, "conv"] = S.gmres(vals, b, maxit=40, atol=0.0, rtol=rtol)
        ref[M, "N"] = S.N
    return ref


def _against_oracle(run, M, case, ref):
    xo, ho, r0o, ito = ref[M, case]
    N = ref[M, "N"]
    pre = "M%d/%s/0/" % (M, case)
    it, r0 = int(run[pre + "scalars"][0]), run[pre + "scalars"][1]
    hist, x = run[pre + "hist"], run[pre + "x"]
    assert it == ito and abs(r0 - r0o) <= 1e-12 * r0o
    ho = np.asarray(ho)[:it]
    k = np.arange(1, it + 1)
    dev = np.abs(hist - ho) / (1e-10 * r0o * np.maximum(1.0, k / 10.0))
    print("M=%d %s: history against the oracle, worst err/bar %.3g" % (M, case, dev.max()))
    assert dev.max() <= 1.0
    na = 6 * N if case == "tail" else 4 * N
    errx = np.abs(x[:na] - xo[:na]).max() / np.abs(xo[:na]).max()
    print("M=%d %s: x against the oracle, rel err %.3g" % (M, case, errx))
    assert errx <= 1e-8


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", SIZES)
def test_solver_matches_oracle_and_single_steps(M, case, solves, oracle):
    pair, single = solves["pair"], solves["single"]
    pre = "M%d/%s/0/" % (M, case)
    sp, ss = pair[pre + "scalars"], single[pre + "scalars"]
    it = int(sp[0])
    assert int(ss[0]) == it
    # which step ran and how it advanced; a non-zero tail of b means vectors of 6N and the reference step, one at a time
    assert int(sp[2]) == int(ss[2]) == (STEP_REFERENCE if case == "tail" else STEP_RAW_BASIS)
    assert (int(ss[3]), int(ss[4])) == (0, it)
    assert (int(sp[3]), int(sp[4])) == ((0, it) if case == "tail" else STEPS[case])
    assert int(sp[5]) == 0 and int(ss[5]) == 0, "cancellation flag"
    if case == "conv":
        assert it == 20 and int(sp[6]) == 1 and int(ss[6]) == 1
    _against_oracle(pair, M, case, oracle)
    _against_oracle(single, M, case, oracle)
    r0 = sp[1]
    assert_bits([r0], [ss[1]], "r0 does not depend on the step")
    dh = np.abs(pair[pre + "hist"] - single[pre + "hist"]).max() / r0
    dx = np.abs(pair[pre + "x"] - single[pre + "x"]).max() / np.abs(single[pre + "x"]).max()
    print("M=%d %s: pairs against DFL_GMRES_TWO_STEP=0: history %.3g r0, x %.3g relative" % (M, case, dh, dx))
    if case == "tail":  # the same code ran
        assert_bits(pair[pre + "hist"], single[pre + "hist"], "fall-back history")
        assert_bits(pair[pre + "x"], single[pre + "x"], "fall-back x")
    else:  # twice the bar each of them holds against the oracle
        k = np.arange(1, it + 1)
        assert np.all(np.abs(pair[pre + "hist"] - single[pre + "hist"]) <= 2e-10 * r0 * np.maximum(1.0, k / 10.0))


@pytest.mark.parametrize("M", SIZES)
def test_two_consecutive_solves_are_bitwise_equal(M, solves):
    for name in ("pair", "single"):
        run = solves[name]
        for what in ("x", "hist", "scalars"):
            assert_bits(run["M%d/default/1/%s" % (M, what)], run["M%d/default/0/%s" % (M, what)], "%s: second solve, %s" % (name, what))
