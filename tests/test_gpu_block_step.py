"""The raw-basis Arnoldi step that takes three or four iterations per pass over the Krylov basis (host/gmres.c: gmres_block): its
kernels alone through their C launchers, its two scalar kernels against the numpy recurrences of block_step_model.py, and the
solver against the CPU oracle for DFL_GMRES_BLOCK = 4, 3, 2, 1.

Kernel tier, the two tiers of test_gpu_two_step.py, each launcher with S = 3 and 4.  Exact: integer-valued columns, vectors and
coefficients, power-of-two norms and inverse diagonals; every product and partial sum is an integer multiple of 2**-4 below
2**53, so any summation order and any fused multiply-add gives the same bits: bitwise equality with numpy.  Rounded: random
data against numpy, 1e-14 of the sum of the magnitudes of the terms of each entry (at most 2049 + 129 terms of unit roundoff
1.1e-16 each, in a pairwise-like order: far inside).  n in {1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049} (one entry, a partial
double2 slot, the edges of the 1024-row blocks, more than one block), ncol in {1, 2, 41, 129} (129: past the 128-entry LDS
coefficient table), each with ldq = n, ldw = n and with gaps and pointers that are only 8-byte aligned.  The fix-up with
N in {1, 255, 256, 257, 513} nodes, with and without z4.  Two launches on the same input give equal bits.

Solver tier, in child processes (tests/block_step_worker.py) so that DFL_SPMV_X4_MIN=1 is in place when the library first reads
it: Kuhn cubes M = 6 and 8.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import block_step_model as BM
from guarded_buffers import ALL, Pool, assert_bits, sent

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = np.float64
STEP_REFERENCE, STEP_RAW_BASIS = 0, 4

NS = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049]
NCOLS = [1, 2, 41, 129]
LAYOUTS = [(0, 0), (3, 1)]  # (gap after every column of Q and of w, offset of both pointers in doubles)


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    L = A.lib()  # raises if the HIP library is missing: no fallback
    vp, i32 = C.c_void_p, C.c_int32
    L.dfl_pc_jacobi_apply_scaled_rows_x4.restype = None
    L.dfl_pc_jacobi_apply_scaled_rows_x4.argtypes = [i32, i32, i32] + [vp] * 8
    return A


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def columns(rng, n, ncol, ld, integer, lo=-3, hi=4):
    """ncol columns of length n with leading dimension ld, sentinels in the gaps"""
    A = sent(ncol * ld)
    Am = rng.integers(lo, hi, size=(ncol, n)).astype(F64) if integer else rng.uniform(-1.0, 1.0, size=(ncol, n))
    for j in range(ncol):
        A[j * ld: j * ld + n] = Am[j]
    return A, Am


def gap_mask(ncol, ld, n):
    m = np.zeros(ncol * ld, bool)
    for j in range(ncol):
        m[j * ld: j * ld + n] = True
    return m


def close(got, want, scale, what):
    err = np.abs(np.asarray(got) - np.asarray(want)) / np.maximum(scale, 1e-300)
    print("%s: worst err / (1e-14 scale) %.3g" % (what, np.max(err) / 1e-14))
    assert np.all(err <= 1e-14), what


def blocked_sums(prod, rows):
    """sums of a vector over consecutive blocks of `rows` entries"""
    g = (prod.size + rows - 1) // rows
    full = np.zeros(g * rows, prod.dtype)
    full[:prod.size] = prod
    return full.reshape(g, rows).sum(axis=1)


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("n", NS)
def test_dots_block(n, ncol, S, api, pool):
    L = api.lib()
    nrb = int(L.dfl_cgs_dots_block_parts(n, S))
    assert nrb * 4096 >= n and 1 <= nrb <= (n + 511) // 512
    for integer in (True, False):
        for pad, off in LAYOUTS:
            ldq, ldw, lde = n + pad, n + pad, ncol + pad
            rng = np.random.default_rng(1000 * n + 10 * ncol + S + pad)
            Q, Qm = columns(rng, n, ncol, ldq, integer)
            W, Wm = columns(rng, n, S, ldw, integer, -50, 51)
            nu = (2.0 ** rng.integers(-1, 3, size=ncol)).astype(F64) if integer else rng.uniform(0.5, 3.0, size=ncol)
            if integer:
                g = (Qm.astype(np.int64)[None, :, :] * Wm.astype(np.int64)[:, None, :]).sum(axis=2).astype(F64)
            else:
                g = np.einsum("jn,in->ij", Qm, Wm)
            mag = np.einsum("jn,in->ij", np.abs(Qm), np.abs(Wm))  # sum of the magnitudes of the terms
            qs, ws, nus = pool.slot(Q, off), pool.slot(W, off), pool.slot(nu)
            h, hraw, e, c = pool.slot(sent(ncol)), pool.slot(sent(ncol)), pool.slot(sent(S * lde)), pool.slot(sent(S * lde))
            work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
            wm = np.zeros(work.n, bool)
            wm[:S * ncol * nrb] = True
            em = gap_mask(S, lde, ncol)
            runs = []
            for _ in range(2):
                for o in (h, hraw, e, c, work):
                    o.reset()
                L.dfl_cgs_dots_block(n, ncol, S, qs.ptr, ldq, ws.ptr, ldw, nus.ptr, h.ptr, hraw.ptr, e.ptr, c.ptr, lde, work.ptr, None)
                api.sync()
                runs.append([h.check("h", ALL).copy(), hraw.check("h_raw", ALL).copy(), e.check("e", em).copy(), c.check("c", em).copy()])
                work.check("work: one partial per vector, column and row block", wm)
                for s, what in ((qs, "Q"), (ws, "w"), (nus, "nu")):
                    s.check(what)
            for a, b in zip(runs[0], runs[1]):
                assert_bits(b, a, "run-to-run")
            hh, hr, ee, cc = runs[0]
            assert_bits(hr, hh, "the copy of e_0")
            assert_bits(ee[:ncol], hh, "e_0 is column k of H")
            for i in range(S):
                ei, ci = ee[i * lde: i * lde + ncol], cc[i * lde: i * lde + ncol]
                if integer:
                    assert_bits(ei, g[i] / nu, "e_%d[j] = <r_j, p_%d> / nu_j" % (i, i))
                    assert_bits(ci, g[i] / nu / nu, "c_%d = e_%d / nu" % (i, i))
                else:
                    close(ei, g[i] / nu, mag[i] / nu, "e_%d" % i)
                    close(ci, g[i] / nu / nu, mag[i] / nu / nu, "c_%d" % i)
            pool.free()


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("n", NS)
def test_update_block(n, ncol, S, api, pool):
    L = api.lib()
    gp = int(L.dfl_cgs_update_block_parts(n, S))
    rows = 1024
    assert gp == (n + rows - 1) // rows
    NG = S * (S + 1) // 2
    for integer in (True, False):
        for pad, off in LAYOUTS:
            ldq, ldw, lde = n + pad, n + pad, ncol + pad
            rng = np.random.default_rng(2000 * n + 10 * ncol + S + pad)
            Q, Qm = columns(rng, n, ncol, ldq, integer, -2, 3)
            W, Wm = columns(rng, n, S, ldw, integer, -20, 21)
            # (integers: |w'| <= 20 + 129 * 2 * 2, the block sums of products stay below 2**53 by far)
            Cc, Cm = columns(rng, ncol, S, lde, integer, -2, 3)
            ex = Wm - Cm @ Qm
            mag = np.abs(Wm) + np.abs(Cm) @ np.abs(Qm)
            pairs = [(a, b) for a in range(S) for b in range(a, S)]
            if integer:
                exi = ex.astype(np.int64)
                ex_part = np.concatenate([blocked_sums(exi[a] * exi[b], rows) for a, b in pairs]).astype(F64)
            else:
                ex_part = np.concatenate([blocked_sums(ex[a] * ex[b], rows) for a, b in pairs])
            # an error of 1e-14 mag in each factor, and the rounding of the sum itself
            mag_part = np.concatenate([blocked_sums(3.0 * mag[a] * mag[b], rows) for a, b in pairs])
            qs, ws, cs = pool.slot(Q, off), pool.slot(W, off), pool.slot(Cc)
            work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
            wm = np.zeros(work.n, bool)
            wm[:NG * gp] = True
            wmask = gap_mask(S, ldw, n)
            runs = []
            for _ in range(2):
                ws.reset()
                work.reset()
                L.dfl_cgs_update_block(n, ncol, S, qs.ptr, ldq, cs.ptr, lde, ws.ptr, ldw, work.ptr, None)
                api.sync()
                runs.append([ws.check("w: the gaps", wmask).copy(), work.check("work: S (S + 1) / 2 partials per block", wm)[:NG * gp].copy()])
                for s, what in ((qs, "Q"), (cs, "c")):
                    s.check(what)
            for a, b in zip(runs[0], runs[1]):
                assert_bits(b, a, "run-to-run")
            got = np.stack([runs[0][0][i * ldw: i * ldw + n] for i in range(S)])
            if integer:
                assert_bits(got, ex, "p_i' = p_i - Q c_i")
                assert_bits(runs[0][1], ex_part, "partials of G, upper triangle row-major")
            else:
                close(got, ex, mag, "p_i'")
                close(runs[0][1], ex_part, mag_part, "partials of G")
            pool.free()


def jacobi(N, w, d33, d1):
    A, x = d33.reshape(N, 9), w[:3 * N].reshape(N, 3)
    z = np.empty((N, 4))
    for r in range(3):
        z[:, r] = A[:, r] * x[:, 0] + A[:, r + 3] * x[:, 1] + A[:, r + 6] * x[:, 2]
    z[:, 3] = w[3 * N:4 * N] * d1
    return z.reshape(-1)


def node_block_sums(N, v):
    """sums of a 4N-vector ([u AoS | p]) over blocks of 256 nodes"""
    g = (N + 255) // 256
    sq = np.zeros((g, 256, 4), v.dtype)
    node = np.arange(N)
    sq[node // 256, node % 256, :3] = v[:3 * N].reshape(N, 3)
    sq[node // 256, node % 256, 3] = v[3 * N:]
    return sq.reshape(g, -1).sum(axis=1)


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("use_z4", [True, False], ids=["z4", "noz4"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_fixup_block(N, use_z4, S, api, pool):
    """q_i = sum_{l<=i} C[i,l] p_l' in place for i >= 1, partials of ||q_i||^2, z4 = M^-1 q_{S-1} (against the existing pc_apply)"""
    L = api.lib()
    n, g = 4 * N, (N + 255) // 256
    for integer in (True, False):
        for pad, off in LAYOUTS:
            ldw = n + pad
            rng = np.random.default_rng(3000 + 10 * N + S + pad)
            W, Wm = columns(rng, n, S, ldw, integer)
            sc = sent(48)
            Cm = np.eye(4)
            for a in range(1, S):
                Cm[a, :a] = rng.integers(-2, 3, size=a) if integer else rng.uniform(-1.0, 1.0, size=a)
            sc[BM.SC_C:BM.SC_C + 16] = Cm.reshape(-1)  # only C is read
            if integer:
                d33 = (rng.choice([-1.0, 1.0], size=9 * N) * 2.0 ** rng.integers(-2, 3, size=9 * N)).astype(F64)
                d1 = (2.0 ** rng.integers(-2, 3, size=N)).astype(F64)
            else:
                d33, d1 = rng.uniform(-1.0, 1.0, size=9 * N), rng.uniform(0.5, 2.0, size=N)
            ex = BM.fixup(Wm, sc)
            mag = np.abs(Wm)
            for a in range(1, S):
                mag[a] = np.abs(Wm[a]) + np.abs(Cm[a, :a]) @ np.abs(Wm[:a])
            ws, scs, d33s, d1s = pool.slot(W, off), pool.slot(sc), pool.slot(d33), pool.slot(d1)
            z4s = pool.slot(sent(4 * N)) if use_z4 else None
            work = pool.slot(sent(int(L.dfl_cgs_work_size(n, 1))))
            wm = np.zeros(work.n, bool)
            wm[:(S - 1) * g] = True
            wmask = gap_mask(S, ldw, n)
            wmask[:ldw] = False  # p_0' = q_0 is not written
            runs = []
            for _ in range(2):
                ws.reset()
                work.reset()
                if z4s:
                    z4s.reset()
                L.dfl_cgs_fixup_block(N, S, ws.ptr, ldw, scs.ptr, d33s.ptr, d1s.ptr, z4s.ptr if z4s else None, work.ptr, None)
                api.sync()
                runs.append([ws.check("w: q_0 and the gaps", wmask).copy(), work.check("work: S - 1 partials per block", wm)[:(S - 1) * g].copy(),
                             z4s.check("z4", ALL).copy() if z4s else np.zeros(1)])
                for s, what in ((scs, "sc"), (d33s, "dinv33"), (d1s, "dinv1")):
                    s.check(what)
            for a, b in zip(runs[0], runs[1]):
                assert_bits(b, a, "run-to-run")
            got = np.stack([runs[0][0][i * ldw: i * ldw + n] for i in range(S)])
            if integer:
                assert_bits(got, ex, "q_i")
                ex_part = np.concatenate([node_block_sums(N, ex[a].astype(np.int64) ** 2) for a in range(1, S)]).astype(F64)
                assert_bits(runs[0][1], ex_part, "partials of ||q_i||^2")
            else:
                close(got, ex, mag, "q_i")
                close(runs[0][1], np.concatenate([node_block_sums(N, ex[a] ** 2) for a in range(1, S)]),
                      np.concatenate([node_block_sums(N, 3.0 * mag[a] ** 2) for a in range(1, S)]), "partials of ||q_i||^2")
            if use_z4:
                # M^-1 of the q_{S-1} the kernel left, by the preconditioner kernel the solver applies between the products
                qd, ref = pool.slot(got[S - 1]), pool.slot(sent(4 * N))
                L.dfl_pc_jacobi_apply_scaled_rows_x4(N, N, n, d33s.ptr, d1s.ptr, qd.ptr, None, None, None, ref.ptr, None)
                api.sync()
                zref = ref.check("z4 of pc_apply", ALL)
                if integer:
                    assert_bits(runs[0][2], zref, "z4 = M^-1 q_{S-1}, pc_apply")
                    assert_bits(runs[0][2], jacobi(N, ex[S - 1], d33, d1), "z4 = M^-1 q_{S-1}, numpy")
                else:
                    zmag = jacobi(N, np.abs(got[S - 1]), np.abs(d33), np.abs(d1))
                    close(runs[0][2], zref, zmag, "z4 against pc_apply")
            pool.free()


def gram_partials(rng, S, npart):
    """partials of the Gram matrix of S random vectors cut into npart pieces: [t][piece], upper triangle row-major; and the
    sums of the magnitudes of their terms"""
    X = rng.normal(size=(S, npart, 6))
    pairs = [(a, b) for a in range(S) for b in range(a, S)]
    part = np.stack([(X[a] * X[b]).sum(axis=1) for a, b in pairs])
    mag = np.stack([np.abs(X[a] * X[b]).sum(axis=1) for a, b in pairs])
    return part, mag.sum(axis=1)


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("k", [0, 1, 7, 36])
def test_block_scalars(k, S, api, pool):
    L = api.lib()
    rng = np.random.default_rng(500 + 10 * k + S)
    ldh, lde, ncolH = 64, 64, k + S + 1
    npart1, npart2 = 37, 300  # fewer and more partials than the 256 threads of the workgroup
    NG = S * (S + 1) // 2
    # state at entry: un-rotated columns 0..k-1 (upper Hessenberg), rotations 0..k-1, e_0 in column k, beta[k]
    Hraw, H = sent(ldh * ncolH), sent(ldh * ncolH)
    for j in range(k):
        Hraw[j * ldh: j * ldh + j + 2] = rng.uniform(0.5, 2.0, size=j + 2) * rng.choice([-1.0, 1.0], size=j + 2)
    e = sent(S * lde)
    for i in range(S):
        e[i * lde: i * lde + k + 1] = rng.uniform(0.5, 2.0, size=k + 1) * rng.choice([-1.0, 1.0], size=k + 1)
    H[k * ldh: k * ldh + k + 1] = e[:k + 1]
    Hraw[k * ldh: k * ldh + k + 1] = e[:k + 1]
    for i in range(1, S):
        H[(k + i) * ldh: (k + i) * ldh + k + i + 2] = 0.0
    ang = rng.uniform(0.0, 2 * np.pi, size=k)
    gv = sent(2 * (k + S))
    gv[0:2 * k:2], gv[1:2 * k:2] = np.cos(ang), np.sin(ang)
    beta = sent(k + S + 1)
    beta[k] = 1.5
    nu = sent(k + S + 1)
    nu[:k + 1] = rng.uniform(0.5, 3.0, size=k + 1)
    hist = sent(k + S)
    part1, gmag = gram_partials(rng, S, npart1)
    part2 = rng.uniform(0.1, 1.0, size=(S - 1, npart2))
    # the model
    mH, mHraw, mgv, mbeta, mnu, mhist = H.copy(), Hraw.copy(), gv.copy(), beta.copy(), nu.copy(), hist.copy()
    G = np.zeros((S, S))
    t = 0
    for a in range(S):
        for b in range(a, S):
            G[a, b] = G[b, a] = part1[t].sum()
            t += 1
    msc = BM.block_first(G, k, mnu, mH, mHraw, ldh, mgv, mbeta, mhist)
    first = [a.copy() for a in (mH, mHraw, mgv, mbeta, mnu, mhist)]
    mflag = BM.block_second(part2.sum(axis=1), k, mnu, mH, mHraw, ldh, e, lde, msc, mgv, mbeta, mhist)
    # the device
    Hs, Hrs, gvs, betas, nus, hists = (pool.slot(a) for a in (H, Hraw, gv, beta, nu, hist))
    scs, es, p1s, p2s = pool.slot(sent(48)), pool.slot(e), pool.slot(part1.reshape(-1)), pool.slot(part2.reshape(-1))
    flag = pool.slot(np.zeros(4, np.int32), 0, np.int32)
    state = (Hs, Hrs, gvs, betas, nus, hists, scs)
    runs = []
    for _ in range(2):  # the same input twice: the second stage of the Gram sums and the Givens step give equal bits
        for s in state:
            s.reset()
        L.dfl_gmres_block_first(npart1, p1s.ptr, S, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, gvs.ptr, betas.ptr, hists.ptr, scs.ptr, None)
        api.sync()
        runs.append([s.dev.numpy().copy() for s in state])
    for a, b, what in zip(runs[0], runs[1], ("H", "Hraw", "gv", "beta", "nu", "res_hist", "sc")):
        assert_bits(b, a, "block_first run-to-run: " + what)
    sc = scs.check("sc", ALL).copy()
    d = np.sqrt(np.diag(G))
    gsc = np.zeros((4, 4))
    gsc[:S, :S] = np.outer(d, d)  # |G_ab| <= d_a d_b; C[i,l] and U[l,i] / (d_l d_i) are of order one here (the vectors are random)
    Gm = np.zeros((4, 4))
    t = 0
    for a in range(S):
        for b in range(a, S):
            Gm[a, b] = Gm[b, a] = gmag[t]
            t += 1
    close(sc[:16], msc[:16], np.maximum(Gm, 1.0).reshape(-1), "G")
    close(sc[16:32], msc[16:32], np.ones(16) * max(1.0, np.abs(msc[16:32]).max()) * (d.max() / d.min()), "C")
    close(sc[32:48], msc[32:48], np.maximum(gsc, 1.0).reshape(-1) * S, "U")
    colk = slice(k * ldh, k * ldh + k + 2)
    hmag = np.abs(np.concatenate([e[:k + 1], [d[0]]])).max() * (k + 2)
    close(nus.get()[k + 1], first[4][k + 1], first[4][k + 1], "nu[k+1]")
    close(Hs.get()[colk], first[0][colk], hmag, "column k of H, rotated")
    assert_bits(Hrs.get()[k * ldh: k * ldh + k + 1], e[:k + 1], "un-rotated column k keeps e_0")
    close(Hrs.get()[k * ldh + k + 1], first[1][k * ldh + k + 1], d[0], "un-rotated H[k+1, k] = nu[k+1]")
    close(gvs.get()[2 * k: 2 * k + 2], first[2][2 * k: 2 * k + 2], 1.0, "rotation k")
    close(betas.get()[k: k + 2], first[3][k: k + 2], 1.5, "beta[k], beta[k+1]")
    close(hists.get()[k], first[5][k], 1.5, "res_hist[k]")
    runs = []
    after_first = [s.dev.numpy().copy() for s in (Hs, Hrs, gvs, betas, nus, hists)]
    for _ in range(2):
        for s, img in zip((Hs, Hrs, gvs, betas, nus, hists), after_first):
            s.dev.upload(img)
        L.dfl_gmres_block_second(npart2, p2s.ptr, S, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, es.ptr, lde, scs.ptr, gvs.ptr, betas.ptr,
                                 hists.ptr, flag.ptr, None)
        api.sync()
        runs.append([s.get().copy() for s in (Hs, Hrs, gvs, betas, nus, hists)])
    for a, b in zip(runs[0], runs[1]):
        assert_bits(b, a, "run-to-run")
    gH, gHraw, ggv, gbeta, gnu, ghist = runs[0]
    # magnitude of the terms of every entry of the new columns, from the model's values
    tt = np.zeros((S, S))
    Um = msc[32:48].reshape(4, 4)
    for l in range(S):
        for i in range(l + 1, S):
            tt[l, i] = Um[l, i] / mnu[k + 1 + l]

    def rho(i, r):
        if r <= k:
            return e[i * lde + r]
        return tt[r - k - 1, i] if r - k - 1 < i else mnu[k + 1 + i]

    worst = 0.0
    for i in range(1, S):
        c = k + i
        mag = np.zeros(c + 2)
        for r in range(c + 2):
            mag[r] = (abs(rho(i, r)) + sum(abs(rho(i - 1, j) * mHraw[j * ldh + r]) for j in range(max(r - 1, 0), c))) / mnu[k + i]
        # the columns before it inside the block carry their own error into this one, times |rho_{i-1}[j]| / nu[k+i]
        mag = np.maximum(mag, worst * np.abs([rho(i - 1, j) for j in range(c)]).max() / mnu[k + i])
        worst = mag.max()
        col = slice(c * ldh, c * ldh + c + 2)
        close(gnu[k + 1 + i], mnu[k + 1 + i], mnu[k + 1 + i], "nu[k+1+%d]" % i)
        close(gHraw[col], mHraw[col], mag, "un-rotated column k+%d" % i)
        close(gH[col], mH[col], mag.max() * (c + 2), "column k+%d of H, rotated" % i)
        close(ggv[2 * c: 2 * c + 2], mgv[2 * c: 2 * c + 2], 1.0, "rotation k+%d" % i)
    close(gbeta[k: k + S + 1], mbeta[k: k + S + 1], 1.5, "beta[k..k+S]")
    close(ghist[k: k + S], mhist[k: k + S], 1.5, "res_hist[k..k+S-1]")
    assert int(flag.get()[0]) == mflag == 0
    # what a block must not touch: earlier columns, earlier rotations, the norms before k + 1
    assert_bits(gHraw[:k * ldh], Hraw[:k * ldh], "earlier un-rotated columns")
    assert_bits(gH[:k * ldh], H[:k * ldh], "earlier columns of H")
    assert_bits(ggv[:2 * k], gv[:2 * k], "earlier rotations")
    assert_bits(gnu[:k + 1], nu[:k + 1], "earlier norms")
    for s, what in ((es, "e"), (p1s, "partials of the update"), (p2s, "partials of the fix-up")):
        s.check(what)
    assert_bits(scs.get(), sc, "sc is read only after block_first")
    for s, what in ((Hs, "H"), (Hrs, "Hraw"), (gvs, "gv"), (betas, "beta"), (nus, "nu"), (hists, "res_hist"), (scs, "sc")):
        s.check(what + " (guard bands)", ALL)
    # heavy cancellation in the last vector raises the flag: ||q_{S-1}|| = 1e-5 sqrt(G_{S-1,S-1}); constructed partials, no solve
    tiny = part2.copy()
    tiny[S - 2] = 1e-10 * G[S - 1, S - 1] / npart2
    ts = pool.slot(tiny.reshape(-1))
    L.dfl_gmres_block_second(npart2, ts.ptr, S, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, es.ptr, lde, scs.ptr, gvs.ptr, betas.ptr, hists.ptr,
                             flag.ptr, None)
    api.sync()
    assert int(flag.get()[0]) == 1


# ======================================================================================================================
# solver level
# ======================================================================================================================
SIZES = (6, 8)
BLOCKS = (4, 3, 2, 1)
CASES = ["it40", "it41", "it42", "it43", "restart15", "check5", "check3", "x0", "tail", "conv"]
# (iteration cap, restart length or 0, check interval, iterations counted)
SHAPE = {"it40": (40, 0, 20, 40), "it41": (41, 0, 20, 41), "it42": (42, 0, 20, 42), "it43": (43, 0, 20, 43), "restart15": (40, 15, 20, 40),
         "check5": (40, 0, 5, 40), "check3": (40, 0, 3, 40), "x0": (40, 0, 20, 40), "conv": (40, 0, 20, 20)}
# the histograms [steps of 1, 2, 3, 4 iterations] at the default block 4, by hand: 40 = 10 x 4; tails of 1, 2, 3; restart 15 as
# 4+4+4+3 | 4+1 (the check after 20) +4+4+2 | 4+4+2; a check every 5 as 8 x (4+1), every 3 as 13 x 3 + 1; convergence at the
# first check: five blocks counted, the sixth already enqueued and dropped
BY_HAND = {"it40": [0, 0, 0, 10], "it41": [1, 0, 0, 10], "it42": [0, 1, 0, 10], "it43": [0, 0, 1, 10], "restart15": [1, 2, 1, 8],
           "check5": [8, 0, 0, 8], "check3": [1, 0, 13, 0], "x0": [0, 0, 0, 10], "conv": [0, 0, 0, 5]}


def histogram(block, case):
    """the driver's rule: s = min(block, m - iter, maxit - total, ci - total % ci) at every trip"""
    maxit, restart, ci, stop = SHAPE[case]
    m = restart if restart else maxit
    counts, total = [0, 0, 0, 0], 0
    while total < stop:
        it = 0
        while it < m and total < stop:
            s = min(block, m - it, maxit - total, ci - total % ci)
            counts[s - 1] += 1
            it += s
            total += s
    assert total == stop
    return counts


def test_histogram_rule_by_hand():
    for case, want in BY_HAND.items():
        assert histogram(4, case) == want, case
    assert histogram(3, "it40") == [0, 2, 12, 0] and histogram(2, "it41") == [1, 20, 0, 0] and histogram(1, "check3") == [40, 0, 0, 0]
    assert histogram(3, "conv") == [0, 1, 6, 0]


def _child(tmp, name, extra_env, sizes=SIZES):
    out = os.path.join(str(tmp), name + ".npz")
    env = dict(os.environ)
    for v in ("DFL_GMRES_RAW_BASIS", "DFL_GMRES_TWO_STEP", "DFL_GMRES_BLOCK"):
        env.pop(v, None)
    env["DFL_SPMV_X4_MIN"] = "1"
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "block_step_worker.py"), out] + [str(M) for M in sizes], env=env,
                       timeout=180, capture_output=True, text=True)
    assert r.returncode == 0, "worker %s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    res["stderr"] = r.stderr
    return res


@pytest.fixture(scope="module")
def solves(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block_step")
    runs = {b: _child(tmp, "block%d" % b, {"DFL_GMRES_BLOCK": str(b)}) for b in BLOCKS}
    runs["unset"] = _child(tmp, "unset", {})
    runs["two_step_0"] = _child(tmp, "two_step_0", {"DFL_GMRES_TWO_STEP": "0"})
    return runs


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
        for it in (40, 41, 42, 43):
            ref[M, "it%d" % it] = S.gmres(vals, b, maxit=it, **kw)
        ref[M, "check5"] = ref[M, "check3"] = ref[M, "it40"]  # how often the host looks does not change the arithmetic
        ref[M, "x0"] = S.gmres(vals, b, x0=x0, maxit=40, **kw)
        ref[M, "tail"] = S.gmres(vals, b_tail, maxit=40, **kw)
        ref[M, "restart15"] = S.gmres_restarted(vals, b, 15, 40)
        rtol = float(solves[4]["M%d/conv/0/scalars" % M][5])
        ref[M, "conv"] = S.gmres(vals, b, maxit=40, atol=0.0, rtol=rtol)
        ref[M, "N"] = S.N
    return ref


def _against_oracle(run, M, case, ref, name):
    xo, ho, r0o, ito = ref[M, case]
    N = ref[M, "N"]
    pre = "M%d/%s/0/" % (M, case)
    it, r0 = int(run[pre + "scalars"][0]), run[pre + "scalars"][1]
    hist, x = run[pre + "hist"], run[pre + "x"]
    assert it == ito and abs(r0 - r0o) <= 1e-12 * r0o
    ho = np.asarray(ho)[:it]
    k = np.arange(1, it + 1)
    dev = np.abs(hist - ho) / (1e-10 * r0o * np.maximum(1.0, k / 10.0))
    na = 6 * N if case == "tail" else 4 * N
    errx = np.abs(x[:na] - xo[:na]).max() / np.abs(xo[:na]).max()
    print("M=%d %s block %s: history against the oracle, worst err/bar %.3g; x rel err %.3g" % (M, case, name, dev.max(), errx))
    assert dev.max() <= 1.0
    assert errx <= 1e-8


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", SIZES)
def test_solver_matches_oracle_in_every_block_setting(M, case, solves, oracle):
    pre = "M%d/%s/0/" % (M, case)
    it = int(solves[4][pre + "scalars"][0])
    for b in BLOCKS:
        run = solves[b]
        sc, counts = run[pre + "scalars"], [int(c) for c in run[pre + "counts"]]
        assert int(sc[0]) == it
        # which step ran and how it advanced; a non-zero tail of b means vectors of 6N and the reference step, one at a time
        assert int(sc[2]) == (STEP_REFERENCE if case == "tail" else STEP_RAW_BASIS)
        want = [it, 0, 0, 0] if case == "tail" else histogram(b, case)
        assert counts[0] == 0 and counts[1:] == want, "block %d: histogram %r, want %r" % (b, counts[1:], want)
        assert (int(sc[6]), int(sc[7])) == (want[1] + want[2] + 2 * want[3], want[0] + want[2]), "pairs and singles"
        assert int(sc[3]) == 0, "cancellation flag"
        if case == "conv":
            assert it == 20 and int(sc[4]) == 1
        _against_oracle(run, M, case, oracle, str(b))
    r0 = solves[4][pre + "scalars"][1]
    k = np.arange(1, it + 1)
    for i, a in enumerate(BLOCKS):
        assert_bits([solves[a][pre + "scalars"][1]], [r0], "r0 does not depend on the block size")
        for b in BLOCKS[i + 1:]:
            dh = np.abs(solves[a][pre + "hist"] - solves[b][pre + "hist"])
            if case == "tail":  # the same code ran
                assert_bits(solves[a][pre + "hist"], solves[b][pre + "hist"], "fall-back history, blocks %d and %d" % (a, b))
                assert_bits(solves[a][pre + "x"], solves[b][pre + "x"], "fall-back x, blocks %d and %d" % (a, b))
            else:  # twice the bar each of them holds against the oracle
                assert np.all(dh <= 2e-10 * r0 * np.maximum(1.0, k / 10.0)), "blocks %d and %d" % (a, b)
    # the default is block 4
    for what in ("hist", "x", "counts"):
        assert_bits(solves["unset"][pre + what], solves[4][pre + what], "DFL_GMRES_BLOCK unset against 4: " + what,
                    np.int64 if what == "counts" else F64)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", SIZES)
def test_two_consecutive_solves_are_bitwise_equal(M, case, solves):
    """every case is solved twice on the same Krylov object: nothing a solve leaves behind (coefficient and scalar buffers, the
    un-rotated H, z4, the assumed operand probes) reaches the next one"""
    for b in BLOCKS:
        run = solves[b]
        for what in ("x", "hist", "scalars", "counts"):
            assert_bits(run["M%d/%s/1/%s" % (M, case, what)], run["M%d/%s/0/%s" % (M, case, what)],
                        "block %d, %s: second solve, %s" % (b, case, what), np.int64 if what == "counts" else F64)


@pytest.mark.parametrize("M", SIZES)
def test_block_one_is_two_step_off(M, solves):
    """DFL_GMRES_BLOCK=1 and DFL_GMRES_TWO_STEP=0 are the same setting: equal bits in every case"""
    for case in CASES:
        for what in ("x", "hist", "scalars", "counts"):
            key = "M%d/%s/0/%s" % (M, case, what)
            assert_bits(solves[1][key], solves["two_step_0"][key], "%s: block 1 against DFL_GMRES_TWO_STEP=0, %s" % (case, what),
                        np.int64 if what == "counts" else F64)


@pytest.mark.parametrize("M", SIZES)
def test_block_two_takes_pairs_and_single_steps_only(M, solves):
    """DFL_GMRES_BLOCK=2 is the paired step as it was: no counted step of three or four iterations in any case"""
    for case in CASES:
        counts = solves[2]["M%d/%s/0/counts" % (M, case)]
        assert int(counts[3]) == 0 and int(counts[4]) == 0, case
        c1 = solves[1]["M%d/%s/0/counts" % (M, case)]
        assert int(c1[2]) == 0 and int(c1[3]) == 0 and int(c1[4]) == 0, case


def test_block_out_of_range_is_clamped_and_named(tmp_path_factory, solves):
    """DFL_GMRES_BLOCK=9 runs as block 4 and says so once on stderr; the valid settings say nothing"""
    run = _child(tmp_path_factory.mktemp("block_step_clamp"), "block9", {"DFL_GMRES_BLOCK": "9"}, sizes=(6,))
    assert run["stderr"].count("DFL_GMRES_BLOCK=9 is not one of 1, 2, 3, 4: using 4") == 1
    for case in CASES:
        for what in ("hist", "counts"):
            key = "M6/%s/0/%s" % (case, what)
            assert_bits(run[key], solves[4][key], "%s: block 9 against block 4, %s" % (case, what), np.int64 if what == "counts" else F64)
    for b in BLOCKS:
        assert "DFL_GMRES_BLOCK" not in solves[b]["stderr"]
