"""The raw-basis Arnoldi step of the one-GPU Jacobi-GMRES (GMRES_STEP_RAW_BASIS, host/gmres.c): its kernels alone through
their C launchers against numpy, and the solver against the CPU oracle and against the step it replaces.

Kernel level, two tiers as in test_gpu_krylov_kernels.py.  Exact: integer-valued columns, w and coefficients, power-of-two
norms and inverse diagonals; every product and partial sum is an integer multiple of 2**-4 below 2**53, so any summation order
and any fused multiply-add gives the same bits and the expectation is bitwise equality -- with the numpy model and with
dfl_cgs_update_givens, which the new launcher must reproduce entry for entry.  Rounded: normal random data against
np.longdouble with the a-priori bounds of that file (Higham 3.1: n_terms u sum |x_i y_i| for every order of summation).
Shapes: N in {1, 2, 255, 256, 257, 513} (a partial block, a full one, a block plus one node, odd N with its 8-byte-aligned
pressure section), ncol in {1, 8, 9, 41, 129} (129 passes the 128 coefficients staged in LDS), with and without z4.

Solver level, in child processes (tests/raw_basis_worker.py) so that DFL_SPMV_X4_MIN=1 is in place when the library first
reads it: Kuhn cubes M = 6 and 8, 40 iterations, tolerances 0, with the raw basis and with DFL_GMRES_RAW_BASIS=0.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded_buffers import ALL, Pool, assert_bits, sent

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64, LD = np.float64, np.longdouble
U = 2.0 ** -53
STEP_REFERENCE, STEP_RAW_BASIS = 0, 4

NS = [1, 2, 255, 256, 257, 513]
NCOLS = [1, 8, 9, 41, 129]


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


def jacobi(N, w, d33, d1, dt):
    """z4[node] = (inv(D)^T r_u, r_p dinv1): the column-major image of pc_apply_kernel (Q7), products summed left to right"""
    A = d33.astype(dt).reshape(N, 9)
    x = w[:3 * N].astype(dt).reshape(N, 3)
    z = np.empty((N, 4), dt)
    for r in range(3):
        z[:, r] = A[:, r] * x[:, 0] + A[:, r + 3] * x[:, 1] + A[:, r + 6] * x[:, 2]
    z[:, 3] = w[3 * N:4 * N].astype(dt) * d1.astype(dt)
    return z.reshape(-1)


def givens_slots(pool, it, ldh):
    """column `it` of H zero above the subdiagonal, identity rotations before it, beta[it] = 1.5"""
    H = sent((it + 1) * ldh)
    H[it * ldh: it * ldh + it + 1] = 0.0
    gv = sent(2 * (it + 1))
    gv[:2 * it] = np.tile([1.0, 0.0], it)
    beta = sent(it + 2)
    beta[it] = 1.5
    return pool.slot(H), pool.slot(gv), pool.slot(beta), pool.slot(sent(it + 1))


def run_update(L, api, N, ncol, qs, ldq, cs, ws, d33s, d1s, z4s, nrm, work, g):
    it = ncol - 1
    L.dfl_cgs_update_jacobi_givens(N, ncol, qs.ptr, ldq, cs.ptr, ws.ptr, d33s.ptr, d1s.ptr, z4s.ptr if z4s else None, nrm.ptr,
                                   work.ptr, it, g[0].ptr, ncol + 2, g[1].ptr, g[2].ptr, g[3].ptr, None)
    api.sync()


@pytest.mark.parametrize("use_z4", [True, False], ids=["z4", "noz4"])
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("N", NS)
def test_exact_update_jacobi(N, ncol, use_z4, api, pool):
    L = api.lib()
    n, ldq, it, ldh = 4 * N, 4 * N, ncol - 1, ncol + 2
    rng = np.random.default_rng(1000 * N + ncol)
    Q = rng.integers(-3, 4, size=ncol * ldq).astype(F64)
    w = rng.integers(-50, 51, size=n).astype(F64)
    c = rng.integers(-2, 3, size=ncol).astype(F64)
    d33 = (rng.choice([-1.0, 1.0], size=9 * N) * 2.0 ** rng.integers(-2, 3, size=9 * N)).astype(F64)
    d1 = (2.0 ** rng.integers(-2, 3, size=N)).astype(F64)
    ex_w = w - (Q.reshape(ncol, ldq)[:, :n] * c[:, None]).sum(axis=0)   # integers: exact in any order
    ex_nrm = np.sqrt(F64(np.sum(ex_w.astype(np.int64) ** 2)))
    ex_z4 = jacobi(N, ex_w, d33, d1, F64)
    qs, cs, ws = pool.slot(Q), pool.slot(c), pool.slot(w)
    d33s, d1s = pool.slot(d33), pool.slot(d1)
    z4s = pool.slot(sent(4 * N)) if use_z4 else None
    nwork = int(L.dfl_cgs_work_size(n, ncol))
    work, nrm = pool.slot(sent(nwork)), pool.slot(sent(1))
    # the step it replaces, on the same operands: every output must agree bit for bit
    g0 = givens_slots(pool, it, ldh)
    L.dfl_cgs_update_givens(n, ncol, qs.ptr, ldq, cs.ptr, ws.ptr, nrm.ptr, work.ptr, it, g0[0].ptr, ldh, g0[1].ptr, g0[2].ptr,
                            g0[3].ptr, None)
    api.sync()
    old = [ws.get().copy(), nrm.get().copy()] + [s.get().copy() for s in g0]
    assert_bits(old[0], ex_w, "dfl_cgs_update_givens w (the model)")
    runs = []
    for _ in range(2):
        ws.reset()
        nrm.reset()
        work.reset()
        if z4s:
            z4s.reset()
        g = givens_slots(pool, it, ldh)
        run_update(L, api, N, ncol, qs, ldq, cs, ws, d33s, d1s, z4s, nrm, work, g)
        runs.append([ws.check("w", ALL).copy(), nrm.check("d_nrm", ALL).copy()] + [s.get().copy() for s in g]
                    + ([z4s.check("z4", ALL).copy()] if z4s else []))
        for s, what in ((qs, "Q"), (cs, "c"), (d33s, "dinv33"), (d1s, "dinv1")):
            s.check(what)
        m = np.zeros(nwork, bool)
        m[:(N + 255) // 256] = True
        work.check("work: one partial per block of 256 nodes", m)
    for a, b in zip(runs[0], runs[1]):
        assert_bits(b, a, "run-to-run")
    assert_bits(runs[0][0], ex_w, "w' = w - Q c")
    assert_bits(runs[0][1], [ex_nrm], "||w'||")
    for a, b, what in zip(runs[0][2:6], old[2:], ("H", "gv", "beta", "res_hist")):
        assert_bits(a, b, "Givens step against dfl_cgs_update_givens: " + what)
    if use_z4:
        assert_bits(runs[0][6], ex_z4, "z4 = M^-1 w'")


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("N", NS)
def test_exact_dots_raw_and_scale(N, ncol, api, pool):
    L = api.lib()
    n = ldq = 4 * N
    rng = np.random.default_rng(2000 * N + ncol)
    Q = rng.integers(-3, 4, size=ncol * ldq).astype(F64)
    w = rng.integers(-50, 51, size=n).astype(F64)
    nu = (2.0 ** rng.integers(-1, 3, size=ncol)).astype(F64)
    g = (Q.reshape(ncol, ldq).astype(np.int64) * w.astype(np.int64)).sum(axis=1).astype(F64)
    qs, ws, nus = pool.slot(Q), pool.slot(w), pool.slot(nu)
    hs, cs, work = pool.slot(sent(ncol)), pool.slot(sent(ncol)), pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol))))
    runs = []
    for _ in range(2):
        hs.reset()
        cs.reset()
        L.dfl_cgs_dots_raw(n, ncol, qs.ptr, ldq, ws.ptr, nus.ptr, hs.ptr, cs.ptr, work.ptr, None)
        api.sync()
        runs.append((hs.check("h", ALL).copy(), cs.check("c", ALL).copy()))
    assert_bits(runs[1][0], runs[0][0], "h run-to-run")
    assert_bits(runs[1][1], runs[0][1], "c run-to-run")
    assert_bits(runs[0][0], g / nu, "h_j = <r_j, w> / nu_j")
    assert_bits(runs[0][1], g / nu / nu, "c_j = h_j / nu_j")
    for s, what in ((qs, "Q"), (ws, "w"), (nus, "nu")):
        s.check(what)
    # the plain dots on the same operands: the same partial sums
    L.dfl_cgs_dots(n, ncol, qs.ptr, ldq, ws.ptr, hs.ptr, work.ptr, None)
    api.sync()
    assert_bits(hs.get(), g, "dfl_cgs_dots")
    # y_j / nu_j
    y = rng.integers(-100, 101, size=ncol).astype(F64)
    ys = pool.slot(np.concatenate([y, sent(3)]))
    L.dfl_gmres_scale_inv(ncol, nus.ptr, ys.ptr, None)
    api.sync()
    assert_bits(ys.check("y", np.arange(ncol + 3) < ncol)[:ncol], y / nu, "y_j / nu_j")
    nus.check("nu")


@pytest.mark.parametrize("use_z4", [True, False], ids=["z4", "noz4"])
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("N", NS)
def test_rounded_update_jacobi_and_dots(N, ncol, use_z4, api, pool):
    """w': (ncol + 1) u (|w| + sum |c_j| |r_j|) per entry.  Norm: that error carried through the sum of squares, plus
    (n + 1) u of the sum, through the square root, plus 2u for the root.  z4 against M^-1 of the DEVICE's w' (so that only the
    3-term products are judged): 3 u sum |A| |x|.  h, c: n u sum |r_j| |w| / nu_j (+ 2u, 4u |value| for the divisions)."""
    L = api.lib()
    n = ldq = 4 * N
    it, ldh = ncol - 1, ncol + 2
    rng = np.random.default_rng(3000 * N + ncol)
    Q, w, c = rng.normal(size=ncol * ldq), rng.normal(size=n), rng.normal(size=ncol)
    d33, d1 = rng.normal(size=9 * N), rng.normal(size=N)
    nu = rng.uniform(0.5, 3.0, size=ncol)
    Qm = Q.reshape(ncol, ldq)
    qs, cs, ws = pool.slot(Q), pool.slot(c), pool.slot(w)
    d33s, d1s = pool.slot(d33), pool.slot(d1)
    z4s = pool.slot(sent(4 * N)) if use_z4 else None
    work, nrm = pool.slot(sent(int(L.dfl_cgs_work_size(n, ncol)))), pool.slot(sent(1))
    runs = []
    for _ in range(2):
        ws.reset()
        g = givens_slots(pool, it, ldh)
        run_update(L, api, N, ncol, qs, ldq, cs, ws, d33s, d1s, z4s, nrm, work, g)
        runs.append([ws.check("w", ALL).copy(), nrm.check("d_nrm", ALL).copy()] + [s.get().copy() for s in g]
                    + ([z4s.check("z4", ALL).copy()] if z4s else []))
    for a, b in zip(runs[0], runs[1]):
        assert_bits(b, a, "run-to-run")
    got_w, got_nrm = runs[0][0], runs[0][1][0]
    ref_w = w.astype(LD) - (Qm.astype(LD) * c.astype(LD)[:, None]).sum(axis=0)
    bw = (ncol + 1) * U * (np.abs(w) + (np.abs(Qm) * np.abs(c)[:, None]).sum(axis=0))
    ratio = float((np.abs(got_w - ref_w) / bw).max())
    print("update_jacobi w err/bound %.3g" % ratio)
    assert ratio <= 1.0
    ref_ss = float(np.sum(ref_w * ref_w))
    bss = float(np.sum(2 * np.abs(ref_w) * bw + bw * bw)) + (n + 1) * U * ref_ss
    ref_nrm = float(np.sqrt(ref_ss))
    ratio = abs(got_nrm - ref_nrm) / (bss / (2 * ref_nrm) + 2 * U * ref_nrm)
    print("update_jacobi nrm err/bound %.3g" % ratio)
    assert ratio <= 1.0
    assert runs[0][2][it * ldh + it] != 0.0 and np.isfinite(runs[0][2][it * ldh: it * ldh + it + 2]).all()  # the Givens step ran
    if use_z4:
        ref_z = jacobi(N, got_w, d33, d1, LD)
        bz = 3 * U * jacobi(N, np.abs(got_w), np.abs(d33), np.abs(d1), LD).astype(F64)
        ratio = float((np.abs(runs[0][6] - ref_z) / bz).max())
        print("update_jacobi z4 err/bound %.3g" % ratio)
        assert ratio <= 1.0
    if use_z4:  # (the dots do not depend on z4: once per shape)
        hs, cs2, nus = pool.slot(sent(ncol)), pool.slot(sent(ncol)), pool.slot(nu)
        L.dfl_cgs_dots_raw(n, ncol, qs.ptr, ldq, ws.ptr, nus.ptr, hs.ptr, cs2.ptr, work.ptr, None)
        api.sync()
        ref_h = (Qm.astype(LD) * got_w.astype(LD)).sum(axis=1) / nu
        bh = n * U * (np.abs(Qm) * np.abs(got_w)).sum(axis=1) / nu
        ratio = float(max((np.abs(hs.get() - ref_h) / (bh + 2 * U * np.abs(ref_h))).max(),
                          (np.abs(cs2.get() - ref_h / nu) / (bh / nu + 4 * U * np.abs(ref_h / nu))).max()))
        print("dots_raw h, c err/bound %.3g" % ratio)
        assert ratio <= 1.0
        qs.check("Q")


@pytest.mark.parametrize("nu", [1.0, 4.0, 0.37, 1234.5])
def test_scaled_spmv_is_the_unscaled_one_times_s(nu, api, pool):
    """y_scaled = tot * (1.0 / nu) where the unscaled kernel stores alpha * tot = tot: one more rounding, the same bits as
    numpy's product; whole matrix and a row range (rows outside keep what they held)"""
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    L = api.lib()
    m = kuhn_cube(5, jitter=0.2)
    wg, dwg = synthetic_fields(m)
    P = api.Problem(m)
    try:
        N = P.N
        wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
        P.assemble_system(wg_d, dwg_d, None, want_J=True)
        api.sync()
        a = P.spy1x1.contents
        val = L.MatrixFSBlockValues(P.J)
        x4 = pool.slot(np.random.default_rng(5).normal(size=4 * N))
        nus = pool.slot([nu])
        y0, y1 = pool.slot(sent(4 * N)), pool.slot(sent(4 * N))
        for row0, row1 in ((0, N), (17, 150)):
            y0.reset()
            y1.reset()
            L.dfl_bcsr_spmv_x4(row0, row1, N, a.row_ptr, a.col_ind, val, 1.0, x4.ptr, y0.ptr, None)
            L.dfl_bcsr_spmv_x4_scaled(row0, row1, N, a.row_ptr, a.col_ind, val, nus.ptr, x4.ptr, y1.ptr, None)
            api.sync()
            i = np.arange(row0, row1)
            rows = np.zeros(4 * N, bool)
            rows[np.concatenate([3 * i, 3 * i + 1, 3 * i + 2, 3 * N + i])] = True
            plain, scaled = y0.check("y", rows), y1.check("y scaled", rows)
            assert np.isfinite(plain[rows]).all() and np.abs(plain[rows]).max() > 0
            assert_bits(scaled[rows], plain[rows] * (1.0 / nu), "scaled SpMV")
            first = scaled.copy()
            y1.reset()
            L.dfl_bcsr_spmv_x4_scaled(row0, row1, N, a.row_ptr, a.col_ind, val, nus.ptr, x4.ptr, y1.ptr, None)
            api.sync()
            assert_bits(y1.get(), first, "run-to-run")
        x4.check("x4")
        nus.check("nu")
    finally:
        P.close()


# ======================================================================================================================
# solver level
# ======================================================================================================================
SIZES = (6, 8)


def _child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    env = dict(os.environ)
    env.pop("DFL_GMRES_RAW_BASIS", None)
    env["DFL_SPMV_X4_MIN"] = "1"
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "raw_basis_worker.py"), out] + [str(M) for M in SIZES], env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, "worker %s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solves(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("raw_basis")
    return {"raw": _child(tmp, "raw", {}), "old": _child(tmp, "old", {"DFL_GMRES_RAW_BASIS": "0"})}


@pytest.fixture(scope="module")
def oracle(oracle_lib):
    """the CPU oracle's solves of the same systems, computed once"""
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    from raw_basis_worker import MAXIT, operands
    ref = {}
    for M in SIZES:
        m = kuhn_cube(M, jitter=0.2)
        wg, dwg = synthetic_fields(m)
        S = oracle_lib.System(m)
        F, vals = S.assemble_system(wg, dwg, True, True)
        b, x0, b_tail = operands(S.N, F)
        kw = dict(maxit=MAXIT, atol=0.0, rtol=0.0)
        ref[M, "default"] = S.gmres(vals, b, **kw)[:3]
        ref[M, "x0"] = S.gmres(vals, b, x0=x0, **kw)[:3]
        ref[M, "tail"] = S.gmres(vals, b_tail, **kw)[:3]
        ref[M, "restart15"] = S.gmres_restarted(vals, b, 15, MAXIT)[:3]
        ref[M, "N"] = S.N
    return ref


def _against_oracle(run, M, case, ref):
    xo, ho, r0o = ref[M, case]
    N = ref[M, "N"]
    pre = "M%d/%s/0/" % (M, case)
    it, r0 = int(run[pre + "scalars"][0]), run[pre + "scalars"][1]
    hist, x = run[pre + "hist"], run[pre + "x"]
    ho = np.asarray(ho)[:it]
    assert it == 40 and abs(r0 - r0o) <= 1e-12 * r0o
    k = np.arange(1, it + 1)
    dev = np.abs(hist - ho) / (1e-10 * r0o * np.maximum(1.0, k / 10.0))
    print("M=%d %s: history against the oracle, worst err/bar %.3g" % (M, case, dev.max()))
    assert dev.max() <= 1.0
    na = 6 * N if case == "tail" else 4 * N
    errx = np.abs(x[:na] - xo[:na]).max() / np.abs(xo[:na]).max()
    print("M=%d %s: x against the oracle, rel err %.3g" % (M, case, errx))
    assert errx <= 1e-8


@pytest.mark.parametrize("case", ["default", "restart15", "x0", "tail"])
@pytest.mark.parametrize("M", SIZES)
def test_solver_matches_oracle_and_old_step(M, case, solves, oracle):
    raw, old = solves["raw"], solves["old"]
    pre = "M%d/%s/0/" % (M, case)
    # which step ran: the raw basis wherever the plan allows it; a non-zero tail of b means vectors of 6N and the old step
    want = STEP_REFERENCE if case == "tail" else STEP_RAW_BASIS
    assert int(raw[pre + "scalars"][2]) == want
    assert int(old[pre + "scalars"][2]) == STEP_REFERENCE
    _against_oracle(raw, M, case, oracle)
    _against_oracle(old, M, case, oracle)
    r0 = raw[pre + "scalars"][1]
    assert_bits([r0], [old[pre + "scalars"][1]], "r0 does not depend on the step")
    dh = np.abs(raw[pre + "hist"] - old[pre + "hist"]).max() / r0
    dx = np.abs(raw[pre + "x"] - old[pre + "x"]).max() / np.abs(old[pre + "x"]).max()
    print("M=%d %s: raw basis against DFL_GMRES_RAW_BASIS=0: history %.3g r0, x %.3g relative" % (M, case, dh, dx))
    if case == "tail":  # the same code ran
        assert_bits(raw[pre + "hist"], old[pre + "hist"], "fall-back history")
        assert_bits(raw[pre + "x"], old[pre + "x"], "fall-back x")
    else:  # twice the bar each of them holds against the oracle
        k = np.arange(1, 41)
        assert np.all(np.abs(raw[pre + "hist"] - old[pre + "hist"]) <= 2e-10 * r0 * np.maximum(1.0, k / 10.0))


@pytest.mark.parametrize("M", SIZES)
def test_two_consecutive_solves_are_bitwise_equal(M, solves):
    for name in ("raw", "old"):
        run = solves[name]
        for what in ("x", "hist", "scalars"):
            assert_bits(run["M%d/default/1/%s" % (M, what)], run["M%d/default/0/%s" % (M, what)], "%s: second solve, %s" % (name, what))
