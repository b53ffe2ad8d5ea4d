"""PC_AMGX on the device: the hierarchy (aggregates, Galerkin matrices, colourings) and PCApply against the numpy model
(tests/amgx_model.py) on a stand-alone CSR matrix and on the pressure view of the assembled (u,p) system, the reference's
tree with AMG on A11 (krylov.c:450) through KrylovSetPCType, the mesh-size behaviour on Poisson, and the options."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
from tests import amgx_model as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _csr_on_pattern(api, P, A):
    """MAT_TYPE_CSR matrix over the Problem's nodal pattern holding the values of scipy A (same pattern)."""
    L = api.lib()
    rp, ci = P.pattern()
    A = A.tocsr()
    A.sort_indices()
    assert np.array_equal(rp, A.indptr) and np.array_equal(ci, A.indices)
    M = L.MatrixCreateTypeCSR(P.spy1x1, None)
    L.MatrixZero(M)
    csr = C.cast(M.contents.data, C.POINTER(api.MatrixCSR)).contents
    vals = api.DeviceArray(ci.size, np.float64, ptr=csr.val, owner=False)
    vals.upload(A.data.astype(np.float64))
    return M, vals


def _dirichlet_poisson(M):
    m = kuhn_cube(M, jitter=0.2)
    A = am.p1_stiffness(m)
    return m, am.dirichlet_identity(A, np.unique(m.bound_node))


def _level_csr(api, pc, l):
    L = api.lib()
    mat = L.PCAMGXLevelMatrix(pc, l)
    csr = C.cast(mat.contents.data, C.POINTER(api.MatrixCSR)).contents
    at = csr.attr.contents
    n, nnz = at.num_row, at.nnz
    rp = api.d2h(at.row_ptr, n + 1, np.int32)
    ci = api.d2h(at.col_ind, nnz, np.int32)
    v = api.d2h(csr.val, nnz, np.float64)
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def _hierarchy(api, pc):
    L = api.lib()
    nl = L.PCAMGXNumLevels(pc)
    mats = [_level_csr(api, pc, l) for l in range(nl)]
    aggs = [api.d2h(L.PCAMGXLevelAggregates(pc, l), mats[l].shape[0], np.int32).astype(np.int64) for l in range(nl - 1)]
    cols = [api.d2h(L.PCAMGXLevelColors(pc, l), mats[l].shape[0], np.int32).astype(np.int64) for l in range(nl)]
    return mats, aggs, cols


def _check_structure(mats, aggs, cols, passes=1):
    for l in range(len(mats)):
        A = mats[l]
        assert np.array_equal(cols[l], am.greedy_colors(A.indptr, A.indices)), l
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        off = rows != A.indices
        assert np.all(cols[l][rows[off]] != cols[l][A.indices[off]]), l     # a valid colouring
        if l + 1 < len(mats):
            agg, nc = am.aggregate(A, passes)                                   # one pass: am.pairwise
            assert nc == mats[l + 1].shape[0] and np.array_equal(aggs[l], agg), l
            Ac = am.galerkin(A, aggs[l], nc)
            D = (mats[l + 1] - Ac).tocsr()
            assert abs(D).max() <= 1e-12 * abs(Ac).max(), l


def _cfg(smoother, max_iters):
    return (f"config_version=2, solver:preconditioner:smoother={smoother}, solver:preconditioner:max_iters={max_iters}, "
            "solver:solver=FGMRES")


def _apply(api, pc, r):
    r_d, z_d = api.DeviceArray.from_numpy(r), api.DeviceArray(r.size)
    api.lib().PCApply(pc, r_d.ptr, z_d.ptr)
    api.sync()
    return z_d.numpy()


# tail_rows 0: every level but the coarsest runs the per-colour grid kernels; 8192 (default): all in the one-workgroup tail
@pytest.mark.parametrize("tail_rows", [8192, 0])
@pytest.mark.parametrize("smoother,max_iters", [("MULTICOLOR_DILU", 1), ("MULTICOLOR_DILU", 2), ("BLOCK_JACOBI", 1),
                                                ("BLOCK_JACOBI", 2)])
def test_standalone_hierarchy_apply_and_new_values(api, monkeypatch, smoother, max_iters, tail_rows):
    m, A = _dirichlet_poisson(12)
    P = api.Problem(m)
    L = api.lib()
    try:
        M, vals = _csr_on_pattern(api, P, A)
        monkeypatch.setenv("DFL_AMGX_TAIL_ROWS", str(tail_rows))
        pc = L.PCCreateAMGX(M, _cfg(smoother, max_iters).encode())
        monkeypatch.delenv("DFL_AMGX_TAIL_ROWS")
        tail = C.c_int32(-1)
        L.PCAMGXInfo(pc, None, None, None, None, C.byref(tail), None, None)
        assert tail.value == (0 if tail_rows else L.PCAMGXNumLevels(pc) - 1)
        assert pc
        L.PCSetup(pc)
        api.sync()
        mats, aggs, cols = _hierarchy(api, pc)
        # the identity rows have no strong neighbour and stay singletons: coarsening stops at the 90 % rule
        assert len(mats) >= 3 and mats[-1].shape[0] <= 2048
        assert np.array_equal(mats[0].toarray(), A.toarray())
        _check_structure(mats, aggs, cols)
        model = am.Model(mats, aggs, cols, smoother="JACOBI" if smoother == "BLOCK_JACOBI" else "DILU", max_iters=max_iters)
        rng = np.random.default_rng(3)
        for _ in range(2):
            r = rng.normal(size=A.shape[0])
            z = _apply(api, pc, r)
            zm = model.apply(r)
            assert np.all(np.isfinite(z)) and np.abs(z - zm).max() <= 1e-12 * np.abs(zm).max()
            assert np.array_equal(z, _apply(api, pc, r))                       # bitwise reproducible
        # new values, same structure: scale every row differently (a symmetric diagonal scaling), PCSetup
        s = 1.0 + rng.random(A.shape[0])
        A2 = A.copy()                                                         # same stored pattern, zeros included
        A2.data = A.data * s[np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))] * s[A.indices]
        vals.upload(A2.data)
        L.PCSetup(pc)
        api.sync()
        mats2, aggs2, cols2 = _hierarchy(api, pc)
        assert [a.shape for a in mats2] == [a.shape for a in mats]
        assert all(np.array_equal(a, b) for a, b in zip(aggs, aggs2))
        for l in range(1, len(mats2)):
            Ac = am.galerkin(mats2[l - 1], aggs2[l - 1], mats2[l].shape[0])
            assert abs(mats2[l] - Ac).max() <= 1e-12 * abs(Ac).max()
        model2 = am.Model(mats2, aggs2, cols2, smoother="JACOBI" if smoother == "BLOCK_JACOBI" else "DILU", max_iters=max_iters)
        r = rng.normal(size=A.shape[0])
        z, zm = _apply(api, pc, r), model2.apply(r)
        assert np.abs(z - zm).max() <= 1e-12 * np.abs(zm).max()
        L.PCDestroy(pc)
        L.MatrixDestroy(M)
    finally:
        P.close()


def _setup_up(api, M, maxit=400, rtol=1e-8):
    m = kuhn_cube(M, jitter=0.2)
    wg, dwg = synthetic_fields(m)
    N = m.num_node
    wg[3 * N:4 * N] = 0.0
    P = api.Problem(m, maxit=maxit, atol=0.0, rtol=rtol)
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(0.1 * dwg)
    F_d = api.DeviceArray(6 * N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=False)
    P.assemble_system(wg_d, dwg_d, None, want_J=True)
    return m, P, F_d


def test_pressure_view_singular_coarsest(api):
    m, P, F_d = _setup_up(api, 10)
    L = api.lib()
    try:
        pc = L.PCCreateAMGX(P.fs.mat[5], None)
        assert pc
        L.PCSetup(pc)
        api.sync()
        mats, aggs, cols = _hierarchy(api, pc)
        A11 = P.export_values()[3]
        assert np.array_equal(mats[0].data, A11)                                # the gathered [3][3] entries, bitwise
        _check_structure(mats, aggs, cols)
        Ac = mats[-1].toarray()
        nC = Ac.shape[0]
        piv = api.d2h(L.PCAMGXCoarsePivots(pc), 2 * nC, np.int32)
        fac = am.lu_factor(Ac)
        assert np.array_equal(piv[:nC], fac[1]) and np.array_equal(piv[nC:].astype(bool), fac[2])
        assert np.linalg.svd(Ac, compute_uv=False)[-1] <= 1e-10 * np.abs(Ac).max()   # singular (constants in the null space)
        assert fac[2].any()
        model = am.Model(mats, aggs, cols)
        rng = np.random.default_rng(5)
        r = rng.normal(size=P.N)
        z = _apply(api, pc, r)
        zm = model.apply(r)
        assert np.all(np.isfinite(z)) and np.abs(z - zm).max() <= 1e-10 * np.abs(zm).max()
        L.PCDestroy(pc)
    finally:
        P.close()


def test_reference_tree_with_amg_on_a11(api):
    import scipy.sparse.linalg as spl
    m, P, F_d = _setup_up(api, 10, rtol=1e-6)
    L = api.lib()
    N = P.N
    try:
        L.KrylovSetPCType(P.ksp, api.PC_AMGX)
        x_d = api.DeviceArray(6 * N)
        it, r0, hist, conv = P.solve(x_d, F_d)
        pc = L.KrylovGetPC(P.ksp)
        assert C.cast(pc, C.POINTER(C.c_int)).contents.value == api.PC_DECOMPOSITION
        # PCDecomposition { n_sec; offset*; pc**; } -> pc[1]->type
        class _Dec(C.Structure):
            _fields_ = [("n_sec", C.c_int32), ("offset", C.c_void_p), ("pc", C.POINTER(C.c_void_p))]
        pcdata = C.cast(pc, C.POINTER(C.c_void_p * 6)).contents[5]        # struct PC: type, mat, op[3], data
        dec = C.cast(pcdata, C.POINTER(_Dec)).contents
        assert dec.n_sec == 4 and C.cast(dec.pc[1], C.POINTER(C.c_int)).contents.value == api.PC_AMGX
        assert conv, (it, hist[-3:] if len(hist) else None)
        # direct solution of the same 4N system (node-block order -> [u: 3N AoS | p: N])
        rp, ci = P.pattern()
        blocks = P.block_values().numpy().reshape(-1, 4, 4)
        Ab = sp.bsr_matrix((blocks, ci, rp), shape=(4 * N, 4 * N)).tocsr()
        nodes = np.arange(N)
        perm = np.concatenate([(nodes[:, None] * 4 + np.arange(3)).reshape(-1), nodes * 4 + 3])
        A = Ab[perm][:, perm].tocsc()
        F = F_d.numpy()[:4 * N]
        x = x_d.numpy()
        ref = spl.spsolve(A, F)
        print(f"tree with AMG on A11: {it} iterations to rtol 1e-6, |r0| = {r0:.3e}")
        assert np.linalg.norm(x[:4 * N] - ref) <= 1e-4 * np.linalg.norm(ref)
        assert np.all(x[4 * N:] == 0.0)
        # the true residual meets the tolerance up to a small factor.  It does not equal the recurrence residual here (measured
        # at kuhn_cube(10): 7.7e-7 r0 true against 2.0e-7 r0 recurrence): the truncated coarse solve leaves the constant
        # pressure, a near-null vector of the coupled operator, out of the preconditioner's reach (DESIGN.md "PC_AMGX")
        true_res = np.linalg.norm(F - A @ x[:4 * N])
        assert hist[-1] <= 1e-6 * r0 and true_res <= 5e-6 * r0, (true_res / r0, hist[-1] / r0)
    finally:
        P.close()


class _OwnCSR:
    """MAT_TYPE_CSR matrix over a pattern of its own (device row_ptr / col_ind kept alive here)."""

    def __init__(self, api, A):
        A = A.tocsr()
        A.sort_indices()
        L = api.lib()
        self.rp = api.DeviceArray.from_numpy(A.indptr.astype(np.int32))
        self.ci = api.DeviceArray.from_numpy(A.indices.astype(np.int32))
        self.attr = api.CSRAttr(A.shape[0], A.shape[1], A.nnz, self.rp.ptr, self.ci.ptr, None)
        self.M = L.MatrixCreateTypeCSR(C.pointer(self.attr), None)
        L.MatrixZero(self.M)
        csr = C.cast(self.M.contents.data, C.POINTER(api.MatrixCSR)).contents
        api.DeviceArray(A.nnz, np.float64, ptr=csr.val).upload(A.data.astype(np.float64))

    def close(self, api):
        api.lib().MatrixDestroy(self.M)


def _gmres_count(api, M, A, pc_type, cfg=None, maxit=1500):
    L = api.lib()
    ksp = L.KrylovCreateGMRES(maxit, 0.0, 1e-8, None)
    L.KrylovSetVerbose(ksp, 0)
    L.KrylovSetCheckInterval(ksp, 1)
    L.KrylovSetPCType(ksp, pc_type)
    if cfg is not None:
        L.KrylovSetAMGXConfig(ksp, cfg.encode())
    b = np.random.default_rng(7).normal(size=A.shape[0])
    b_d, x_d = api.DeviceArray.from_numpy(b), api.DeviceArray(A.shape[0])
    L.KrylovSolve(ksp, M, x_d.ptr, b_d.ptr)
    api.sync()
    st = L.KrylovGetStats(ksp).contents
    it, conv = int(st.iterations), bool(st.converged)
    pc_kind = C.cast(L.KrylovGetPC(ksp), C.POINTER(C.c_int)).contents.value
    x = x_d.numpy()
    L.KrylovDestroy(ksp)
    assert conv, (pc_type, it)
    assert pc_kind == (api.PC_AMGX if pc_type == api.PC_AMGX else 0)
    assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
    return it


def _interior_poisson(M):
    """Dirichlet P1 Poisson matrix: the stiffness matrix on the interior nodes (boundary unknowns eliminated)."""
    m = kuhn_cube(M, jitter=0.2)
    A = am.p1_stiffness(m)
    inner = np.setdiff1d(np.arange(m.num_node), np.unique(m.bound_node))
    return A[inner][:, inner].tocsr()


def test_poisson_iterations_do_not_follow_the_mesh(api):
    counts = {}
    for M in (16, 32):
        A = _interior_poisson(M)
        own = _OwnCSR(api, A)
        try:
            counts[("amg", M)] = _gmres_count(api, own.M, A, api.PC_AMGX)
            if M == 32:
                counts[("none", M)] = _gmres_count(api, own.M, A, api.PC_DECOMPOSITION)
        finally:
            own.close(api)
    print("GMRES iterations to 1e-8:", counts)
    assert counts[("amg", 32)] <= 2 * counts[("amg", 16)]
    assert 4 * counts[("amg", 32)] <= counts[("none", 32)]


def test_options_forms_and_pool(api, tmp_path):
    m, A = _dirichlet_poisson(8)
    P = api.Problem(m)
    L = api.lib()
    try:
        M, vals = _csr_on_pattern(api, P, A)
        f = tmp_path / "AMGX.json"
        f.write_text(am.REFERENCE_JSON)

        def hier(opt):
            pc = L.PCCreateAMGX(M, opt)
            assert pc
            L.PCSetup(pc)
            api.sync()
            h = _hierarchy(api, pc)
            L.PCDestroy(pc)
            return h

        ref = hier(None)
        for opt in (am.REFERENCE_INLINE.encode(), str(f).encode()):
            h = hier(opt)
            assert len(h[0]) == len(ref[0])
            assert all(np.array_equal(a.toarray(), b.toarray()) for a, b in zip(h[0], ref[0]))
            assert all(np.array_equal(a, b) for a, b in zip(h[1], ref[1]))
        assert not L.PCCreateAMGX(M, b"config_version=2, solver:preconditioner:cycle=W")
        assert not L.PCCreateAMGX(M, b"config_version=2, solver:preconditioner:algorithm=CLASSICAL")
        # BLOCK_JACOBI works as a preconditioner
        it_j = _gmres_count(api, M, A, api.PC_AMGX, "config_version=2, solver:preconditioner:smoother=BLOCK_JACOBI")
        it_d = _gmres_count(api, M, A, api.PC_AMGX)
        print("GMRES iterations, BLOCK_JACOBI / MULTICOLOR_DILU:", it_j, it_d)
        assert it_d <= it_j < 100
        # create / destroy cycles return the device pool to where it started
        api.sync()
        res0, use0 = C.c_int64(0), C.c_int64(0)
        L.DflDevicePoolStats(C.byref(res0), C.byref(use0))
        for _ in range(3):
            pc = L.PCCreateAMGX(M, None)
            L.PCSetup(pc)
            L.PCDestroy(pc)
        api.sync()
        res1, use1 = C.c_int64(0), C.c_int64(0)
        L.DflDevicePoolStats(C.byref(res1), C.byref(use1))
        assert use1.value == use0.value
        L.MatrixDestroy(M)
    finally:
        P.close()


# SIZE_4: every level's map is two pairwise passes composed, the second on the Galerkin graph of the first
@pytest.mark.parametrize("tail_rows", [8192, 0])
@pytest.mark.parametrize("smoother", ["MULTICOLOR_DILU", "BLOCK_JACOBI"])
def test_multipass_selector_hierarchy_and_apply(api, monkeypatch, smoother, tail_rows):
    m, A = _dirichlet_poisson(8)
    P = api.Problem(m)
    L = api.lib()
    try:
        M, vals = _csr_on_pattern(api, P, A)
        monkeypatch.setenv("DFL_AMGX_TAIL_ROWS", str(tail_rows))
        pc = L.PCCreateAMGX(M, f"config_version=2, solver:preconditioner:selector=SIZE_4, "
                               f"solver:preconditioner:smoother={smoother}".encode())
        monkeypatch.delenv("DFL_AMGX_TAIL_ROWS")
        assert pc
        L.PCSetup(pc)
        api.sync()
        mats, aggs, cols = _hierarchy(api, pc)
        assert len(mats) >= 3                                                  # two coarse levels at least
        assert np.array_equal(mats[0].toarray(), A.toarray())
        _check_structure(mats, aggs, cols, passes=2)
        model = am.Model(mats, aggs, cols, smoother="JACOBI" if smoother == "BLOCK_JACOBI" else "DILU")
        r = np.random.default_rng(13).normal(size=A.shape[0])
        z, zm = _apply(api, pc, r), model.apply(r)
        assert np.all(np.isfinite(z)) and np.abs(z - zm).max() <= 1e-12 * np.abs(zm).max()
        assert np.array_equal(z, _apply(api, pc, r))                           # bitwise reproducible
        L.PCDestroy(pc)
        L.MatrixDestroy(M)
    finally:
        P.close()


def test_rebuild_equals_a_fresh_preconditioner(api):
    m, A = _dirichlet_poisson(8)
    P = api.Problem(m)
    L = api.lib()
    try:
        M, vals = _csr_on_pattern(api, P, A)
        api.sync()
        res0, use0 = C.c_int64(0), C.c_int64(0)
        L.DflDevicePoolStats(C.byref(res0), C.byref(use0))

        def state(pc, r):
            L.PCSetup(pc)
            api.sync()
            mats, aggs, cols = _hierarchy(api, pc)
            piv = api.d2h(L.PCAMGXCoarsePivots(pc), 2 * mats[-1].shape[0], np.int32)
            arrays = [a for A_l in mats for a in (A_l.indptr, A_l.indices, A_l.data)] + aggs + cols + [piv, _apply(api, pc, r)]
            return aggs, arrays

        rng = np.random.default_rng(17)
        r = rng.normal(size=A.shape[0])
        pc = L.PCCreateAMGX(M, None)
        assert pc
        aggs0, _ = state(pc, r)
        # new values with other strengths: rows and columns scaled by different vectors.  (Scaling rows alone would not do:
        # the strength |a_ij| / |a_ii| does not see it.)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        A2 = A.copy()
        A2.data = A.data * (1.0 + rng.random(A.shape[0]))[rows] * (1.0 + rng.random(A.shape[0]))[A.indices]
        vals.upload(A2.data)
        L.PCAMGXRebuild(pc)
        aggs1, rebuilt = state(pc, r)
        assert len(aggs1) != len(aggs0) or any(not np.array_equal(a, b) for a, b in zip(aggs0, aggs1))
        fresh_pc = L.PCCreateAMGX(M, None)
        assert fresh_pc
        _, fresh = state(fresh_pc, r)
        assert len(rebuilt) == len(fresh)
        for a, b in zip(rebuilt, fresh):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        L.PCDestroy(pc)
        L.PCDestroy(fresh_pc)
        api.sync()
        res1, use1 = C.c_int64(0), C.c_int64(0)
        L.DflDevicePoolStats(C.byref(res1), C.byref(use1))
        assert use1.value == use0.value
        L.MatrixDestroy(M)
    finally:
        P.close()
