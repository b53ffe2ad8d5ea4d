"""Blocks of three and four Arnoldi steps whose update and fix-up are one pass (host/gmres.c: gmres_block with GmresPlan.fuse_fixup):
the three new launchers alone, then the solver against the CPU oracle and against DFL_GMRES_FUSE_FIXUP=0.

Kernel tier, as tests/test_gpu_block_step.py.  Exact: integer-valued data, power-of-two norms and inverse diagonals, every sum an
integer multiple of 2**-4 below 2**53: bitwise equality with numpy in any order.  Rounded: random data, 1e-14 of the sum of the
magnitudes of the terms.
  dfl_cgs_dots_block_gram     n = 4N, N in {1, 255, 257, 1029} (odd n / 4, more than one row block of 1024 rows), ncol in {1, 5, 65}
                              (65: a second column tile), S = 3, 4.  e, c, h, h_raw bitwise those of dfl_cgs_dots_block.
  dfl_cgs_update_fixup_block  N in {1, 255, 256, 257, 513}, ncol in {1, 4, 130} (130: past the LDS coefficient table), S = 3, 4, with
                              and without z4, aligned and only 8-byte aligned (odd N: the p rows take the scalar path).  q and z4
                              bitwise those of dfl_cgs_update_block + dfl_cgs_fixup_block with the same tables.
  dfl_gmres_block_fused       against fused_block_model.block_fused on integer partials, both flag bits.
Solver tier in child processes (tests/fused_block_worker.py), Kuhn cubes M = 6 and 8, the cases of test_gpu_block_step.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import block_step_model as BM
import fused_block_model as FM
from guarded_buffers import ALL, Pool, assert_bits, sent
from test_gpu_block_step import CASES, STEP_RAW_BASIS, STEP_REFERENCE, close, columns, gap_mask, histogram, jacobi, node_block_sums

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = np.float64
LAYOUTS = [(0, 0), (3, 1)]  # (gap after every column, offset of the pointers in doubles)
SC_GD, SC_GR = 48, 64


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()  # raises if the HIP library is missing: no fallback
    return A


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def pairs(S):
    return [(a, b) for a in range(S) for b in range(a, S)]


# ======================================================================================================================
# the dots pass that also sums <p_a, p_b>, and C from the derived Gram matrix
# ======================================================================================================================
@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("ncol", [1, 5, 65])
@pytest.mark.parametrize("N", [1, 255, 257, 1029])
def test_dots_block_gram(N, ncol, S, api, pool):
    L = api.lib()
    n = 4 * N
    nrb = int(L.dfl_cgs_dots_block_parts(n, S))
    NG = S * (S + 1) // 2
    for integer in (True, False):
        for pad, off in LAYOUTS:
            ldq, ldw, lde = n + pad, n + pad, ncol + pad
            rng = np.random.default_rng(7000 * N + 10 * ncol + S + pad)
            Q, Qm = columns(rng, n, ncol, ldq, integer)
            W, Wm = columns(rng, n, S, ldw, integer, -5, 6)
            for a in range(S):  # vector a dominates in its own rows: the Gram matrix is well conditioned at every n, n = 4 included
                sl = slice(a, n, 4)
                Wm[a, sl] += 8.0 if integer else 3.0
                W[a * ldw: a * ldw + n] = Wm[a]
            # nu_j >= 2 sqrt(ncol) ||r_j||: sum_j e_a[j] e_b[j] stays below a quarter of ||p_a|| ||p_b||, the derived G positive definite
            big = 2.0 * np.sqrt(ncol) * np.linalg.norm(Qm, axis=1)
            nu = 2.0 ** np.ceil(np.log2(np.maximum(big, 1.0))) if integer else np.maximum(big, 0.5) * rng.uniform(1.0, 1.5, size=ncol)
            if integer:
                Wi = Wm.astype(np.int64)
                graw = (Wi[:, None, :] * Wi[None, :, :]).sum(axis=2).astype(F64)
            else:
                graw = Wm @ Wm.T
            gmag = np.abs(Wm) @ np.abs(Wm).T
            qs, ws, nus = pool.slot(Q, off), pool.slot(W, off), pool.slot(nu)
            outs = []
            for gram in (False, True):
                h, hraw, e, c = pool.slot(sent(ncol)), pool.slot(sent(ncol)), pool.slot(sent(S * lde)), pool.slot(sent(S * lde))
                work, sc = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol)))), pool.slot(sent(80))
                wm = np.zeros(work.n, bool)
                wm[:S * ncol * nrb + (NG * nrb if gram else 0)] = True
                if gram:
                    L.dfl_cgs_dots_block_gram(n, ncol, S, qs.ptr, ldq, ws.ptr, ldw, nus.ptr, h.ptr, hraw.ptr, e.ptr, c.ptr, lde, sc.ptr,
                                              work.ptr, None)
                else:
                    L.dfl_cgs_dots_block(n, ncol, S, qs.ptr, ldq, ws.ptr, ldw, nus.ptr, h.ptr, hraw.ptr, e.ptr, c.ptr, lde, work.ptr, None)
                api.sync()
                em = gap_mask(S, lde, ncol)
                outs.append([h.check("h", ALL).copy(), hraw.check("h_raw", ALL).copy(), e.check("e", em).copy(), c.check("c", em).copy()])
                work.check("work: the dots partials, then the Gram partials", wm)
                scm = np.zeros(80, bool)
                scm[BM.SC_C:BM.SC_C + 16] = scm[SC_GD:SC_GD + 32] = gram
                scv = sc.check("sc: C, the derived G and the raw sums only", scm).copy()
                for s, what in ((qs, "Q"), (ws, "w"), (nus, "nu")):
                    s.check(what)
            for a, b, what in zip(outs[1], outs[0], ("h", "h_raw", "e", "c")):
                assert_bits(a, b, what + ": the pass with the Gram sums against dfl_cgs_dots_block")
            ee = outs[1][2]
            Gr, Gd, Cd = (scv[o:o + 16].reshape(4, 4) for o in (SC_GR, SC_GD, BM.SC_C))
            assert not Gr[S:].any() and not Gr[:, S:].any() and not Gd[S:].any() and not Gd[:, S:].any()
            assert_bits(Gr, Gr.T, "raw sums symmetric")
            if integer:
                assert_bits(Gr[:S, :S], graw, "<p_a, p_b>")
            else:
                close(Gr[:S, :S], graw, gmag, "<p_a, p_b>")
            want = FM.derived_gram(Gr[:S, :S], ee, lde, ncol)
            emag = np.array([[np.abs(ee[a * lde: a * lde + ncol] * ee[b * lde: b * lde + ncol]).sum() for b in range(S)] for a in range(S)])
            close(Gd[:S, :S], want, gmag + emag, "derived G = raw sums - sum_j e_a[j] e_b[j]")
            Cm = BM.gram_coefficients(Gd[:S, :S])[0]
            errC = np.abs(Cd - Cm).max()
            print("C against the model's C from the same G: %.3g" % errC)
            assert errC <= 1e-13 * max(1.0, np.abs(Cm).max())
            pool.free()


# ======================================================================================================================
# update and fix-up in one pass
# ======================================================================================================================
@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("use_z4", [True, False], ids=["z4", "noz4"])
@pytest.mark.parametrize("ncol", [1, 4, 130])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_update_fixup_block(N, ncol, use_z4, S, api, pool):
    L = api.lib()
    n, g = 4 * N, (N + 255) // 256
    assert int(L.dfl_cgs_update_fixup_block_parts(N)) == g
    NG = S * (S + 1) // 2
    gu = int(L.dfl_cgs_update_block_parts(n, S))
    for integer in (True, False):
        for pad, off in LAYOUTS:
            ldq, ldw, lde = n + pad, n + pad, ncol + pad
            rng = np.random.default_rng(9000 * N + 10 * ncol + S + pad)
            Q, Qm = columns(rng, n, ncol, ldq, integer, -2, 3)
            # S columns of the block between two columns that belong to somebody else
            W, Wm = columns(rng, n, S + 2, ldw, integer, -20, 21)
            Cc, Ccm = columns(rng, ncol, S, lde, integer, -2, 3)
            sc = sent(80)
            Cm = np.eye(4)
            for a in range(1, S):
                Cm[a, :a] = rng.integers(-2, 3, size=a) if integer else rng.uniform(-1.0, 1.0, size=a)
            sc[BM.SC_C:BM.SC_C + 16] = Cm.reshape(-1)  # only C is read
            if integer:
                d33 = (rng.choice([-1.0, 1.0], size=9 * N) * 2.0 ** rng.integers(-2, 3, size=9 * N)).astype(F64)
                d1 = (2.0 ** rng.integers(-2, 3, size=N)).astype(F64)
            else:
                d33, d1 = rng.uniform(-1.0, 1.0, size=9 * N), rng.uniform(0.5, 2.0, size=N)
            pu = Wm[1:S + 1] - Ccm @ Qm                      # p_i'
            pmag = np.abs(Wm[1:S + 1]) + np.abs(Ccm) @ np.abs(Qm)
            ex = BM.fixup(pu, sc)
            qmag = pmag.copy()
            for a in range(1, S):
                qmag[a] = pmag[a] + np.abs(Cm[a, :a]) @ pmag[:a]
            qs, cs, scs, d33s, d1s = pool.slot(Q, off), pool.slot(Cc), pool.slot(sc), pool.slot(d33), pool.slot(d1)
            wmask = gap_mask(S + 2, ldw, n)
            wmask[:ldw] = False
            wmask[(S + 1) * ldw:] = False  # the columns next to the block are not touched

            def launch(fused):
                ws = pool.slot(W, off)
                z4s = pool.slot(sent(4 * N)) if use_z4 else None
                work = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
                w1 = ws.ptr + 8 * ldw
                zp = z4s.ptr if z4s else None
                if fused:
                    L.dfl_cgs_update_fixup_block(N, ncol, S, qs.ptr, ldq, cs.ptr, lde, w1, ldw, scs.ptr, d33s.ptr, d1s.ptr, zp, work.ptr, None)
                    nw = (NG + S - 1) * g
                else:
                    L.dfl_cgs_update_block(n, ncol, S, qs.ptr, ldq, cs.ptr, lde, w1, ldw, work.ptr, None)
                    L.dfl_cgs_fixup_block(N, S, w1, ldw, scs.ptr, d33s.ptr, d1s.ptr, zp, work.ptr, None)
                    nw = max(NG * gu, (S - 1) * g)
                api.sync()
                wm = np.zeros(work.n, bool)
                wm[:nw] = True
                out = [ws.check("w: the neighbouring columns and the gaps", wmask).copy(), work.check("work", wm)[:nw].copy(),
                       z4s.check("z4", ALL).copy() if z4s else np.zeros(1)]
                for s, what in ((qs, "Q"), (cs, "c"), (scs, "sc"), (d33s, "dinv33"), (d1s, "dinv1")):
                    s.check(what)
                return out

            two = launch(False)
            one = launch(True)
            again = launch(True)
            for a, b in zip(one, again):
                assert_bits(b, a, "run-to-run")
            assert_bits(one[0], two[0], "q_0..q_{S-1} against dfl_cgs_update_block + dfl_cgs_fixup_block")
            if use_z4:
                assert_bits(one[2], two[2], "z4 against dfl_cgs_update_block + dfl_cgs_fixup_block")
            got = np.stack([one[0][(i + 1) * ldw: (i + 1) * ldw + n] for i in range(S)])
            parts = one[1]
            if integer:
                assert_bits(got, ex, "q_i")
                pi, qi = pu.astype(np.int64), ex.astype(np.int64)
                ex_part = np.concatenate([node_block_sums(N, pi[a] * pi[b]) for a, b in pairs(S)]
                                         + [node_block_sums(N, qi[a] ** 2) for a in range(1, S)]).astype(F64)
                assert_bits(parts, ex_part, "partials of the measured G, then of ||q_i||^2")
                if use_z4:
                    assert_bits(one[2], jacobi(N, ex[S - 1], d33, d1), "z4 = M^-1 q_{S-1}, numpy")
            else:
                close(got, ex, qmag, "q_i")
                ex_part = np.concatenate([node_block_sums(N, pu[a] * pu[b]) for a, b in pairs(S)]
                                         + [node_block_sums(N, ex[a] ** 2) for a in range(1, S)])
                # an error of 1e-14 mag in each factor, and the rounding of the sum itself
                mag_part = np.concatenate([node_block_sums(N, 3.0 * pmag[a] * pmag[b]) for a, b in pairs(S)]
                                          + [node_block_sums(N, 3.0 * qmag[a] ** 2) for a in range(1, S)])
                close(parts, ex_part, mag_part, "partials of the measured G, then of ||q_i||^2")
            pool.free()


# ======================================================================================================================
# the scalars of a fused block
# ======================================================================================================================
@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("k", [0, 1, 7, 36])
def test_block_fused_scalars(k, S, api, pool):
    L = api.lib()
    rng = np.random.default_rng(800 + 10 * k + S)
    ldh, lde, ncolH = 64, 64, k + S + 1
    npart = 300  # more partials than the 256 threads of the workgroup
    NG = S * (S + 1) // 2
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
    # integer partials of the Gram matrix of S integer vectors cut into npart pieces: every sum is exact in any order
    X = rng.integers(-3, 4, size=(S, npart, 6))
    gpart = np.stack([(X[a] * X[b]).sum(axis=1) for a, b in pairs(S)]).astype(F64)
    G = np.zeros((S, S))
    for t, (a, b) in enumerate(pairs(S)):
        G[a, b] = G[b, a] = gpart[t].sum()
    Cgood = BM.gram_coefficients(G)[0]
    dgood = np.array([Cgood[i, :S] @ G @ Cgood[i, :S] for i in range(S)])  # ||q_i||^2 as G has it

    def integer_partials(total):
        """npart non-negative integers that add up to round(total)"""
        t = int(round(total))
        p = np.full(npart, t // npart, np.int64)
        p[:t % npart] += 1
        return p.astype(F64)

    Cskew = Cgood.copy()
    Cskew[S - 1, 0] += 1e-3  # q_{S-1} keeps 1e-3 ||p_0'|| along q_0: far over tau
    cases = [("clean", Cgood, [dgood[i] for i in range(1, S)], 0),
             ("cancelled", Cgood, [dgood[i] for i in range(1, S - 1)] + [1e-10 * G[S - 1, S - 1]], 1),
             ("skew", Cskew, [dgood[i] for i in range(1, S)], 2)]
    Hs, Hrs, gvs, betas, nus, hists = (pool.slot(a) for a in (H, Hraw, gv, beta, nu, hist))
    es = pool.slot(e)
    for name, Cm, qq_want, want_flag in cases:
        if name == "cancelled":
            qpart = np.stack([integer_partials(q) if q >= 1.0 else np.full(npart, q / npart) for q in qq_want])
        else:
            qpart = np.stack([integer_partials(q) for q in qq_want])
        qq = qpart.sum(axis=1)
        part = np.concatenate([gpart.reshape(-1), qpart.reshape(-1)])
        sc0 = sent(80)
        sc0[BM.SC_C:BM.SC_C + 16] = Cm.reshape(-1)
        mH, mHraw, mgv, mbeta, mnu, mhist = H.copy(), Hraw.copy(), gv.copy(), beta.copy(), nu.copy(), hist.copy()
        msc, mflag, mskew = FM.block_fused(G, Cm, qq, k, mnu, mH, mHraw, ldh, e, lde, mgv, mbeta, mhist)
        assert mflag == want_flag, "%s: the model's flag bits %d, skew %.3g" % (name, mflag, mskew)
        ps, scs = pool.slot(part), pool.slot(sc0)
        flag = pool.slot(np.zeros(4, np.int32), 0, np.int32)
        runs = []
        for _ in range(2):
            for s in (Hs, Hrs, gvs, betas, nus, hists, scs, flag):
                s.reset()
            L.dfl_gmres_block_fused(npart, ps.ptr, S, k, nus.ptr, Hs.ptr, Hrs.ptr, ldh, es.ptr, lde, scs.ptr, gvs.ptr, betas.ptr, hists.ptr,
                                    flag.ptr, FM.TAU, None)
            api.sync()
            runs.append([s.get().copy() for s in (Hs, Hrs, gvs, betas, nus, hists, scs)])
        for a, b in zip(runs[0], runs[1]):
            assert_bits(b, a, name + ": run-to-run")
        gH, gHraw, ggv, gbeta, gnu, ghist, gsc = runs[0]
        fl = flag.get()
        assert (int(fl[0]) | 2 * int(fl[1])) == want_flag and int(fl[2]) == 0 and int(fl[3]) == 0, name
        scm = np.zeros(80, bool)
        scm[:16] = scm[32:48] = True
        scs.check("sc: G and U written, C kept", scm)
        assert_bits(gsc[:16], msc[:16], name + ": G, exact sums")
        d = np.sqrt(np.diag(G))
        gsc4 = np.zeros((4, 4))
        gsc4[:S, :S] = np.outer(d, d)
        cmax = max(1.0, np.abs(Cm).max())
        close(gsc[32:48], msc[32:48], np.maximum(gsc4, 1.0).reshape(-1) * S * cmax, name + ": U")
        for i in range(S):
            close(gnu[k + 1 + i], mnu[k + 1 + i], mnu[k + 1 + i], name + ": nu[k+1+%d]" % i)
        assert_bits(gHraw[k * ldh: k * ldh + k + 1], e[:k + 1], "un-rotated column k keeps e_0")
        close(gHraw[k * ldh + k + 1], mHraw[k * ldh + k + 1], d[0], name + ": un-rotated H[k+1, k]")
        # magnitude of the terms of every entry of the new columns, from the model's values (test_gpu_block_step.py)
        tt = np.zeros((S, S))
        Um = msc[32:48].reshape(4, 4)
        for l in range(S):
            for i in range(l + 1, S):
                tt[l, i] = Um[l, i] / mnu[k + 1 + l]

        def rho(i, r):
            if r <= k:
                return e[i * lde + r]
            return tt[r - k - 1, i] if r - k - 1 < i else mnu[k + 1 + i]

        worst = np.abs(np.concatenate([e[:k + 1], [d[0]]])).max() * (k + 2)
        close(gH[k * ldh: k * ldh + k + 2], mH[k * ldh: k * ldh + k + 2], worst, name + ": column k of H, rotated")
        worst = 0.0
        for i in range(1, S):
            c = k + i
            mag = np.zeros(c + 2)
            for r in range(c + 2):
                mag[r] = (abs(rho(i, r)) + sum(abs(rho(i - 1, j) * mHraw[j * ldh + r]) for j in range(max(r - 1, 0), c))) / mnu[k + i]
            mag = np.maximum(mag, worst * np.abs([rho(i - 1, j) for j in range(c)]).max() / mnu[k + i])
            worst = mag.max()
            col = slice(c * ldh, c * ldh + c + 2)
            close(gHraw[col], mHraw[col], mag, name + ": un-rotated column k+%d" % i)
            close(gH[col], mH[col], mag.max() * (c + 2), name + ": column k+%d of H, rotated" % i)
            close(ggv[2 * c: 2 * c + 2], mgv[2 * c: 2 * c + 2], 1.0, name + ": rotation k+%d" % i)
        bmag = 1.5  # |beta[k]|
        close(ggv[2 * k: 2 * k + 2], mgv[2 * k: 2 * k + 2], 1.0, name + ": rotation k")
        close(gbeta[k: k + S + 1], mbeta[k: k + S + 1], bmag, name + ": beta[k..k+S]")
        close(ghist[k: k + S], mhist[k: k + S], bmag, name + ": res_hist[k..k+S-1]")
        assert_bits(gHraw[:k * ldh], Hraw[:k * ldh], "earlier un-rotated columns")
        assert_bits(gH[:k * ldh], H[:k * ldh], "earlier columns of H")
        assert_bits(ggv[:2 * k], gv[:2 * k], "earlier rotations")
        assert_bits(gnu[:k + 1], nu[:k + 1], "earlier norms")
        for s, what in ((es, "e"), (ps, "partials")):
            s.check(what)
        for s, what in ((Hs, "H"), (Hrs, "Hraw"), (gvs, "gv"), (betas, "beta"), (nus, "nu"), (hists, "res_hist")):
            s.check(what + " (guard bands)", ALL)


# ======================================================================================================================
# solver level
# ======================================================================================================================
SIZES = (6, 8)


def _child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    env = dict(os.environ)
    for v in ("DFL_GMRES_RAW_BASIS", "DFL_GMRES_TWO_STEP", "DFL_GMRES_BLOCK", "DFL_GMRES_FUSE_FIXUP", "DFL_GMRES_FOLD_PC"):
        env.pop(v, None)
    env["DFL_SPMV_X4_MIN"] = "1"
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "fused_block_worker.py"), out] + [str(M) for M in SIZES], env=env,
                       timeout=180, capture_output=True, text=True)
    assert r.returncode == 0, "worker %s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solves(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_block")
    runs = {}
    for b in (4, 3, 2):
        runs[b, "on"] = _child(tmp, "block%d_on" % b, {"DFL_GMRES_BLOCK": str(b)})
        runs[b, "off"] = _child(tmp, "block%d_off" % b, {"DFL_GMRES_BLOCK": str(b), "DFL_GMRES_FUSE_FIXUP": "0"})
    return runs


@pytest.fixture(scope="module")
def oracle(oracle_lib, solves):
    """the CPU oracle's solves of the same systems, computed once (as in test_gpu_block_step.py)"""
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
        ref[M, "check5"] = ref[M, "check3"] = ref[M, "it40"]
        ref[M, "x0"] = S.gmres(vals, b, x0=x0, maxit=40, **kw)
        ref[M, "tail"] = S.gmres(vals, b_tail, maxit=40, **kw)
        ref[M, "restart15"] = S.gmres_restarted(vals, b, 15, 40)
        rtol = float(solves[4, "on"]["M%d/conv/0/scalars" % M][5])
        ref[M, "conv"] = S.gmres(vals, b, maxit=40, atol=0.0, rtol=rtol)
        ref[M, "N"] = S.N
    return ref


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", SIZES)
def test_fused_solver_matches_oracle(M, case, solves, oracle):
    pre = "M%d/%s/0/" % (M, case)
    xo, ho, r0o, ito = oracle[M, case]
    N = oracle[M, "N"]
    na = 6 * N if case == "tail" else 4 * N
    for b in (4, 3):
        hists = {}
        for mode in ("on", "off"):
            run = solves[b, mode]
            sc, counts = run[pre + "scalars"], [int(c) for c in run[pre + "counts"]]
            it, r0 = int(sc[0]), sc[1]
            assert it == ito and abs(r0 - r0o) <= 1e-12 * r0o
            assert int(sc[2]) == (STEP_REFERENCE if case == "tail" else STEP_RAW_BASIS)
            want = [it, 0, 0, 0] if case == "tail" else histogram(b, case)
            assert counts[0] == 0 and counts[1:] == want
            assert int(sc[3]) == 0, "flag bits"
            assert int(sc[6]) == (want[2] + want[3] if mode == "on" else 0), "blocks that ran update and fix-up as one pass"
            k = np.arange(1, it + 1)
            bar = 1e-10 * r0o * np.maximum(1.0, k / 10.0)
            dev = np.abs(run[pre + "hist"] - np.asarray(ho)[:it]) / bar
            errx = np.abs(run[pre + "x"][:na] - xo[:na]).max() / np.abs(xo[:na]).max()
            print("M=%d %s block %d fused %s: history against the oracle, worst err/bar %.3g; x rel err %.3g" % (M, case, b, mode, dev.max(), errx))
            assert dev.max() <= 1.0
            assert errx <= 1e-8
            hists[mode] = run[pre + "hist"]
        dh = np.abs(hists["on"] - hists["off"]) / bar
        print("M=%d %s block %d: fused on against off, worst difference / bar %.3g" % (M, case, b, dh.max()))
        assert dh.max() <= 2.0
        if case == "tail":  # the reference step ran: the switch has no say
            for what in ("hist", "x"):
                assert_bits(solves[b, "on"][pre + what], solves[b, "off"][pre + what], "non-zero tail, block %d: %s" % (b, what))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", SIZES)
def test_two_fused_solves_are_bitwise_equal(M, case, solves):
    for b in (4, 3):
        run = solves[b, "on"]
        for what in ("x", "hist", "scalars", "counts"):
            assert_bits(run["M%d/%s/1/%s" % (M, case, what)], run["M%d/%s/0/%s" % (M, case, what)],
                        "block %d, %s: second solve, %s" % (b, case, what), np.int64 if what == "counts" else F64)


@pytest.mark.parametrize("M", SIZES)
def test_pairs_do_not_depend_on_the_switch(M, solves):
    """DFL_GMRES_BLOCK=2 runs pairs and single steps only: what it ran before, bit for bit, and no block counted as fused"""
    for case in CASES:
        for what in ("x", "hist", "counts"):
            key = "M%d/%s/0/%s" % (M, case, what)
            assert_bits(solves[2, "on"][key], solves[2, "off"][key], "%s: block 2, %s" % (case, what), np.int64 if what == "counts" else F64)
        assert int(solves[2, "on"]["M%d/%s/0/scalars" % (M, case)][6]) == 0
