"""Every assembly kernel of dedflow_amd/csrc/k_assemble.hip and k_assemble2.hip alone, through its C launcher, against the
numpy model of tests/assembly_model.py, judged ENTRY BY ENTRY against the entry's own abs-sum -- never against the largest
magnitude of an array (the continuity rows of F are 1e-4 of its maximum, A11 is 1e-6 of A00).

Tier A (bitwise): the data-movement kernels (node records, packed residual, ordered sums, gathers, the nonzero search) on
small integers stored as float64 against the int64 model.
Tier B (rounded): geometry, element residual, element Jacobian, face terms against the np.longdouble model with
|err| <= 8 c u K a: a = the entry's abs-sum, c = what the float64 numpy restatement of the same formulas shows against u a
on the 129-tet soup of the same geometry family and field regime (measured here on the restatement, never on a kernel; the
factor 8 is for FMA contraction and operand order, as in test_gpu_matrix_kernels.py), K = kappa_inf(J) of the tet on the
stretched family, whose c is the unit family's (test_assembly_model_cpu.py checks that the restatement itself stays inside
that bound).  The Newton-seeded kernels of schedule 4 get 2.2e-14 |term| more for every term that carries a stabilisation
parameter ((3/2) 2^-46: one Newton step from the 2^-23 seed asm_device.hpp quotes) and nothing for their reciprocals.
Entries with a zero abs-sum must be exactly 0.0.  The observed err / bound, c and, for schedule 4, err against the Newton
term alone are appended to the file named by DFL_PARITY_OUT (profiles/assembly_kernel_parity.jsonl is such a run).

Inputs of the colour-batch kernels are a tet SOUP: B disjoint tets on 4 B distinct nodes in shuffled order, race-free by
construction, in six geometry families (unit, 1e-5, 1e+3, stretched 1:1:1e-3, translated by 1e3 at cell size 1e-2, negative
orientation) and four field regimes (synthetic_fields, u = 0, |u| = 1e3, dwg = 0).  The two schedule-4 kernels read records
built by host/slotpatch.c and host/patch.c and are run through AssembleSystemTet / DflAssembleSystemTetBeta on real meshes,
with schedules 0 and 1 on the same meshes against the same model.

Every array of a directly launched kernel sits between guard bands (guarded_buffers.py); after each launch the bands, every
const input and every output entry the operation must not write are compared bit for bit.  Overwrite-type outputs are
preloaded with the NaN sentinel.  No case aims at a fault: no NULL where the header does not document one, no index out of
range, no degenerate tet (the nonzero search, which reads no coordinates, gets tets with repeated nodes for its short rows).
"""
import ctypes as C

import numpy as np
import pytest

import assembly_model as A
from guarded_buffers import I32, Pool, Recorder, assert_bits, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
U = A.U
record = Recorder("a")
needs_ld = pytest.mark.skipif(not A.HAVE_EXTENDED, reason=A.EXTENDED_REASON)
C_SOUP = 129   # the soup the constant c of a (family, regime) is measured on


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as Ap
    _declare(Ap.lib())  # raises if the HIP library is missing: no fallback
    return Ap


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    record.write()


class FlatPool(Pool):
    def slot(self, data, off=0, dtype=F64):
        return super().slot(np.ravel(data), off, dtype)


@pytest.fixture
def pool(api):
    p = FlatPool(api)
    yield p
    p.free()


def _declare(L):
    i32, f64, vp = C.c_int32, C.c_double, C.c_void_p
    sig = {
        "dfl_elem_geometry": [i32, vp, vp, vp, vp],
        "dfl_assemble_tet_lhs": [i32, vp, vp, vp, vp, vp, vp],
        "dfl_assemble_tet_rhs": [i32, vp, vp, vp, vp],
        "dfl_rhs_node_sum": [i32, vp, vp, vp, vp, vp],
        "dfl_pack_nodes": [i32, vp, vp, vp, vp, vp],
        "dfl_pack_nodes2": [i32, vp, vp, vp, vp, vp, vp],
        "dfl_unpack_rhs": [i32, vp, vp, vp],
        "dfl_assemble_face": [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "dfl_assemble_face_park": [i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp],
        "dfl_face_sum_F": [i32, vp, vp, vp, vp, i32, vp, vp],
        "dfl_face_sum_J": [i32, vp, vp, vp, vp, vp, vp],
        "dfl_elem_nzmap": [i32, vp, vp, vp, vp, vp],
        "dfl_gather_ien": [i32, vp, vp, vp, vp],
        "dfl_set_rhs_lane_grid_cap": [C.c_int],
        "DflSetSlotPatchParameters": [i32, i32, i32],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = None, args
    from dedflow_amd.api import Matrix, Mesh3D
    L.DflAsmDefaults.restype, L.DflAsmDefaults.argtypes = C.POINTER(C.c_int32 * 5), []   # sched, face group, leaf, cap, tets
    L.DflAssembleSystemTetBeta.restype = None
    L.DflAssembleSystemTetBeta.argtypes = [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix), f64]


# ======================================================================================================================
# helpers
# ======================================================================================================================
def exact(slot, idx, want, what, dtype=F64):
    """entries idx == want bit for bit; every other entry and the bands as uploaded"""
    idx = np.asarray(idx, I64).ravel()
    mask = np.zeros(slot.n, bool)
    mask[idx] = True
    assert mask.sum() == idx.size, what + ": the model writes an entry twice"
    got = slot.check(what, mask)
    assert_bits(got[idx], np.asarray(want).ravel(), what, dtype)
    return got


def judge(got, model, c, K, what, kernel, case, newton=False, **extra):
    """got against the longdouble model under 8 c u K a (+ 2.2e-14 t); zero abs-sum: exactly 0.0.  Records the ratio."""
    got = np.asarray(got, F64)
    assert got.shape == model.v.shape, what
    assert np.all(np.isfinite(got)), what + ": not finite"
    b = A.bound(model, c, K, newton)
    err = np.abs(got.astype(LD) - model.v).astype(F64)
    zero = np.asarray(model.a == 0)
    assert np.all(got[zero] == 0.0), what + ": an entry with a zero abs-sum is not exactly 0.0"
    ratio = float((err[~zero] / b[~zero]).max()) if np.any(~zero) else 0.0
    if newton:   # the observed ratio where the Newton allowance is the larger part of the bound (nobody measured the seed)
        nt = np.asarray(A.NEWTON * model.t, F64)
        dom = nt > A.bound(model, c, K, False)
        extra["max_err_over_newton_term"] = float((err[dom] / nt[dom]).max()) if np.any(dom) else None
        extra["newton_dominated_entries"] = int(dom.sum())
    record(kernel, case, ratio, c=float(c), **extra)
    print("%s %s: err / bound = %.3g (c = %.3g)" % (kernel, case, ratio, c))
    assert ratio <= 1.0, "%s: err / bound = %.3g at entry %d" % (what, ratio, int(np.argmax(np.where(zero, 0, err / np.where(zero, 1, b)))))
    return ratio


def bounded(slot, idx, model, c, K, what, kernel, case, **kw):
    idx = np.asarray(idx, I64).ravel()
    mask = np.zeros(slot.n, bool)
    mask[idx] = True
    assert mask.sum() == idx.size, what + ": the model writes an entry twice"
    got = slot.check(what, mask)
    judge(got[idx].reshape(model.v.shape), model, c, K, what, kernel, case, **kw)
    return got


def untouched(what, *slots):
    for s in slots:
        s.check(what + ": an input changed")


def ints(rng, n, lo=-1000, hi=1000):
    return rng.integers(lo, hi + 1, int(n)).astype(F64)


class Soup:
    """B disjoint tets of one geometry family with the fields of one regime"""

    def __init__(self, B, family, regime, extra=0):
        self.B, self.family, self.regime = B, family, regime
        self.xg, ien = A.tet_soup(B + extra, family)
        self.N = 4 * (B + extra)
        self.ien_all = ien
        self.ien = np.ascontiguousarray(ien[:4 * B])
        self.wg, self.dwg = A.fields(self.xg, regime)
        self.X = A.mesh_vertices(self.xg, self.ien)
        self.W, self.D = A.element_fields(self.ien, self.N, self.wg, self.dwg)
        self.K = A.kappa_inf(self.X) if family in A.KAPPA_FAMILIES else np.ones(B)
        self.case = "B%d-%s-%s" % (B, family, regime)

    def Kfor(self, model):
        return self.K.reshape((-1,) + (1,) * (model.v.ndim - 1))


_C = {}


def constant(kind, family, regime, fn):
    """c of a kernel family: the float64 restatement of fn against its longdouble evaluation, on the C_SOUP-tet soup of
    the geometry family (the unit family for the families whose bound carries kappa) and the regime"""
    fam = "unit" if family in A.KAPPA_FAMILIES else family
    key = (kind, fam, regime)
    if key not in _C:
        s = Soup(C_SOUP, fam, regime)
        mod, rest = fn(s, LD), fn(s, F64)
        _C[key] = A.ratio_c(A.restatement_error(mod, rest), mod.a)
    return _C[key]


SIZES_RHS = (1, 63, 64, 65, 129)
SIZES_LHS = (1, 15, 16, 17, 33)
SIZES_FACE = (1, 63, 64, 65)
SIZES_GEO = (1, 255, 256, 257)


def soup_cases(sizes):
    big = sizes[-1]
    out = [(B, "unit", "synthetic") for B in sizes]
    out += [(big, f, "synthetic") for f in A.FAMILIES[1:]]
    out += [(big, "unit", r) for r in A.REGIMES[1:]]
    out += [(big, "stretched", "convective"), (big, "scale1e-5", "u0"), (big, "negative", "dwg0")]
    return out


def case_id(v):
    return "%d-%s-%s" % v if isinstance(v, tuple) else str(v)


# ======================================================================================================================
# Tier A: bitwise
# ======================================================================================================================
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 321])
def test_pack_nodes(N, api, pool):
    """dfl_pack_nodes2 / dfl_pack_nodes: full records only, compact (x, u) records only, both; dwg NULL zeroes the rate
    slots; the pressure slot [11] comes from dwg; the pad slots are +0.0; N around the 64 nodes a wave stages through LDS"""
    L = api.lib()
    rng = np.random.default_rng(100 + N)
    xg, wg, dwg = ints(rng, 3 * N), ints(rng, 6 * N), ints(rng, 6 * N)
    xs, ws, ds = pool.slot(xg, 1), pool.slot(wg, 1), pool.slot(dwg, 1)
    ps, us = pool.slot(sent(16 * N)), pool.slot(sent(8 * N))
    for rate in (True, False):
        want_p, want_u = A.pack_nodes(N, xg, wg, dwg if rate else None, I64)
        assert np.array_equal(want_p[:, 11], dwg[3 * N:4 * N] if rate else np.zeros(N))
        dp = ds.ptr if rate else None
        for mode in ("full", "full-legacy", "compact", "both"):
            ps.reset(sent(16 * N))
            us.reset(sent(8 * N))
            if mode == "full-legacy":
                L.dfl_pack_nodes(N, xs.ptr, ws.ptr, dp, ps.ptr, None)
            else:
                L.dfl_pack_nodes2(N, xs.ptr, ws.ptr, dp, ps.ptr if mode != "compact" else None,
                                  us.ptr if mode in ("compact", "both") else None, None)
            api.sync()
            what = "pack_nodes N=%d %s rate=%s" % (N, mode, rate)
            if mode != "compact":
                exact(ps, np.arange(16 * N), want_p, what + " nodep")
            else:
                ps.check(what + ": nodep was not asked for")
            if mode in ("compact", "both"):
                exact(us, np.arange(8 * N), want_u, what + " nodexu")
            else:
                us.check(what + ": nodexu was not asked for")
            untouched(what, xs, ws, ds)


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_unpack_rhs(N, api, pool):
    """F += the six live slots of every packed record, which are then cleared; the two pad slots are not touched"""
    L = api.lib()
    rng = np.random.default_rng(200 + N)
    Fp, F = ints(rng, 8 * N), ints(rng, 6 * N)
    fps, fs = pool.slot(Fp), pool.slot(F, 1)
    L.dfl_unpack_rhs(N, fps.ptr, fs.ptr, None)
    api.sync()
    exact(fs, np.arange(6 * N), A.unpack_rhs(N, Fp.astype(I64), F.astype(I64)), "unpack_rhs F")
    live = (np.arange(N)[:, None] * 8 + np.arange(6)).ravel()
    exact(fps, live, np.zeros(6 * N), "unpack_rhs: packed buffer cleared, pads kept")


@pytest.mark.parametrize("N", [1, 256, 257])
def test_rhs_node_sum(N, api, pool):
    """nodes with 0, 1, 3, 4, 5, 8 and 9 partial records (the unrolled-by-four loop and its tail), records referenced out of
    order, some never referenced"""
    L = api.lib()
    rng = np.random.default_rng(300 + N)
    counts = np.array([(0, 1, 3, 4, 5, 8, 9)[(i + N) % 7] for i in range(N)])
    if N == 1:
        counts[:] = 9
    goff = np.concatenate([[0], np.cumsum(counts)]).astype(I32)
    R = int(goff[-1]) + 5
    gidx = rng.permutation(R)[:goff[-1]].astype(I32)
    partial, F = ints(rng, 6 * R), ints(rng, 6 * N)
    gs, xs, ps, fs = pool.slot(goff, 0, I32), pool.slot(gidx, 0, I32), pool.slot(partial), pool.slot(F, 1)
    L.dfl_rhs_node_sum(N, gs.ptr, xs.ptr, ps.ptr, fs.ptr, None)
    api.sync()
    exact(fs, np.arange(6 * N), A.rhs_node_sum(N, goff, gidx, partial.astype(I64), F.astype(I64)), "rhs_node_sum")
    untouched("rhs_node_sum", gs, xs, ps)


def _lists(rng, nkeys, nent_total_extra=3):
    counts = np.array([(0, 1, 5)[k % 3] for k in range(nkeys)])
    if nkeys == 1:
        counts[:] = 5
    off = np.concatenate([[0], np.cumsum(counts)]).astype(I32)
    nrec = int(off[-1]) + nent_total_extra
    ent = rng.permutation(nrec)[:off[-1]].astype(I32)
    return off, ent, nrec


@pytest.mark.parametrize("nn", [1, 63, 64, 65, 100])
def test_face_sum_F(nn, api, pool):
    """4 lanes per node, 0 / 1 / 5 parked entries per node, nn ending inside a 64-node workgroup; only the u and p rows of
    the listed nodes are written"""
    L = api.lib()
    rng = np.random.default_rng(400 + nn)
    N = nn + 9
    fnode = rng.permutation(N)[:nn].astype(I32)
    off, ent, nrec = _lists(rng, nn)
    pF, F = ints(rng, 4 * nrec), ints(rng, 6 * N)
    ns, os_, es, ps, fs = (pool.slot(fnode, 0, I32), pool.slot(off, 0, I32), pool.slot(ent, 0, I32), pool.slot(pF, 1),
                           pool.slot(F, 1))
    L.dfl_face_sum_F(nn, ns.ptr, os_.ptr, es.ptr, ps.ptr, N, fs.ptr, None)
    api.sync()
    index_of = lambda n, j: 3 * n + j if j < 3 else 3 * N + n   # noqa: E731
    want = A.face_sum(fnode, off, ent, pF.astype(I64), 4, F.astype(I64), index_of)
    idx = np.array([index_of(int(n), j) for n in fnode for j in range(4)])
    exact(fs, idx, want[idx], "face_sum_F")
    untouched("face_sum_F", ns, os_, es, ps)


@pytest.mark.parametrize("nz", [1, 15, 16, 17, 40])
def test_face_sum_J(nz, api, pool):
    """16 lanes per nodal nonzero, 0 / 1 / 5 parked blocks per nonzero, nz ending inside a 16-nonzero workgroup"""
    L = api.lib()
    rng = np.random.default_rng(500 + nz)
    nnz = nz + 7
    fnz = rng.permutation(nnz)[:nz].astype(I32)
    off, ent, nrec = _lists(rng, nz)
    pJ, val = ints(rng, 16 * nrec), ints(rng, 16 * nnz)
    ns, os_, es, ps, vs = (pool.slot(fnz, 0, I32), pool.slot(off, 0, I32), pool.slot(ent, 0, I32), pool.slot(pJ, 1),
                           pool.slot(val))
    L.dfl_face_sum_J(nz, ns.ptr, os_.ptr, es.ptr, ps.ptr, vs.ptr, None)
    api.sync()
    want = A.face_sum(fnz, off, ent, pJ.astype(I64), 16, val.astype(I64), lambda k, c: k * 16 + c)
    idx = (fnz.astype(I64)[:, None] * 16 + np.arange(16)).ravel()
    exact(vs, idx, want[idx], "face_sum_J")
    untouched("face_sum_J", ns, os_, es, ps)


@pytest.mark.parametrize("T", [1, 63, 64, 65])
def test_gather_ien(T, api, pool):
    L = api.lib()
    rng = np.random.default_rng(600 + T)
    Tall = T + 11
    ien = rng.integers(0, 500, 4 * Tall).astype(I32)
    ind = rng.permutation(Tall)[:T].astype(I32)
    is_, bs, outs = pool.slot(ien, 0, I32), pool.slot(ind, 0, I32), pool.slot(sent(4 * T, I32), 0, I32)
    L.dfl_gather_ien(T, is_.ptr, bs.ptr, outs.ptr, None)
    api.sync()
    exact(outs, np.arange(4 * T), A.gather_ien(ien, ind), "gather_ien", I32)
    untouched("gather_ien", is_, bs)


@pytest.mark.parametrize("T", [1, 15, 16, 17])
def test_elem_nzmap(T, api, pool):
    """The binary search of nzmap_kernel against the model's linear search.  Pattern: the fan mesh (centre row of 41 nonzeros;
    the wanted column is its first, its last and middle ones) plus two extra nodes whose rows have 1 and 2 nonzeros, reached
    through connectivity entries with repeated nodes -- the search reads no coordinates."""
    from dedflow_amd.meshgen import fan_mesh
    L = api.lib()
    m = fan_mesh()
    Nf = m.num_node
    fan = m.ien.reshape(-1, 4)
    assert Nf == 41
    last = fan[np.any(fan == Nf - 1, axis=1)][:1]                       # a tet with the centre row's LAST column
    short = np.array([[Nf, Nf, Nf, Nf], [Nf + 1, Nf + 2, Nf + 1, Nf + 2]], np.int32)
    tets = np.concatenate([last, short, fan])[:T] if T > 1 else last
    rp, ci = A.nodal_pattern(np.concatenate([fan, short]).reshape(-1), Nf + 3)
    lens = np.diff(rp)
    assert lens[0] == 41 and lens[Nf] == 1 and lens[Nf + 1] == 2 and lens[Nf + 2] == 2
    ien_b = np.ascontiguousarray(tets.reshape(-1).astype(np.int32))
    es, rs, cs, outs = (pool.slot(ien_b, 0, I32), pool.slot(rp, 0, I32), pool.slot(ci, 0, I32),
                        pool.slot(sent(16 * T, I32), 0, I32))
    L.dfl_elem_nzmap(T, es.ptr, rs.ptr, cs.ptr, outs.ptr, None)
    api.sync()
    want = A.elem_nzmap(ien_b, rp, ci)
    assert rp[0] in want and rp[1] - 1 in want                          # first and last column of the centre row
    exact(outs, np.arange(16 * T), want, "elem_nzmap", I32)
    untouched("elem_nzmap", es, rs, cs)


# ======================================================================================================================
# Tier B: rounded
# ======================================================================================================================
def m_geometry(s, dt):
    return A.geometry_record(A.geometry(s.X, dt))


@needs_ld
@pytest.mark.parametrize("case", soup_cases(SIZES_GEO)[:len(SIZES_GEO) + len(A.FAMILIES) - 1], ids=case_id)
def test_elem_geometry(case, api, pool):
    """the cached record shg[12], |det J|, sum G_ij^2, 1 / tr G, pad (exactly 0.0) of every tet"""
    L = api.lib()
    s = Soup(*case)
    T = s.B
    es, xs, gs = pool.slot(s.ien, 0, I32), pool.slot(s.xg, 1), pool.slot(sent(16 * T))
    L.dfl_elem_geometry(T, es.ptr, xs.ptr, gs.ptr, None)
    api.sync()
    mod = m_geometry(s, LD)
    bounded(gs, np.arange(16 * T), mod, constant("geometry", s.family, s.regime, m_geometry), s.Kfor(mod), "elem_geometry",
            "elem_geometry", s.case, family=s.family, regime=s.regime, shape=T)
    untouched("elem_geometry", es, xs)


def scaled_normals(seed, ab):
    """a preload of every entry's own size (its abs-sum times a standard normal), so that neither side of the addition
    hides the other in any geometry family"""
    return np.random.default_rng(seed).normal(size=ab.shape) * np.asarray(np.maximum(ab, 1e-300), F64)


def m_residual(s, dt, preload=True):
    """preload + the six rows of every (tet, node)"""
    r = A.tet_residual(s.X, s.W, s.D, dt)
    if not preload:
        return r
    if not hasattr(s, "rhs_preload"):
        s.rhs_preload = scaled_normals(11, r.a if dt == LD else A.tet_residual(s.X, s.W, s.D, LD).a)
    return A.AV(s.rhs_preload.astype(dt)) + r


@needs_ld
@pytest.mark.parametrize("case", soup_cases(SIZES_RHS), ids=case_id)
def test_assemble_tet_rhs(case, api, pool):
    """tet_rhs_kernel, 64 tets per block: the six rows of every node are ADDED to a preloaded packed record, pads untouched"""
    L = api.lib()
    s = Soup(*case)
    nodep, _ = A.pack_nodes(s.N, s.xg, s.wg, s.dwg)
    mod = m_residual(s, LD)
    idx = s.ien.astype(I64).reshape(-1, 4)[:, :, None] * 8 + np.arange(6)
    pre = np.random.default_rng(10).normal(size=8 * s.N)
    pre[idx] = s.rhs_preload
    es, ns, fs = pool.slot(s.ien, 0, I32), pool.slot(nodep), pool.slot(pre)
    L.dfl_assemble_tet_rhs(s.B, es.ptr, ns.ptr, fs.ptr, None)
    api.sync()
    bounded(fs, idx, mod, constant("residual", s.family, s.regime, m_residual), s.Kfor(mod), "assemble_tet_rhs", "assemble_tet_rhs",
            s.case, family=s.family, regime=s.regime, shape=s.B)
    untouched("assemble_tet_rhs", es, ns)


def m_jacobian(s, dt):
    """preload + the blocks tet_lhs_kernel adds, from the cached geometry record it reads (float64, the restatement's)"""
    if not hasattr(s, "egeo"):
        s.egeo = m_geometry(s, F64).v
    j = A.tet_jacobian(A.geometry_from_record(s.egeo, dt), s.W[:, :, :3], dt)
    if not hasattr(s, "lhs_preload"):
        s.lhs_preload = scaled_normals(12, j.a if dt == LD else A.tet_jacobian(A.geometry_from_record(s.egeo, LD), s.W[:, :, :3], LD).a)
    return A.AV(s.lhs_preload.astype(dt)) + j


@needs_ld
@pytest.mark.parametrize("case", soup_cases(SIZES_LHS), ids=case_id)
def test_assemble_tet_lhs(case, api, pool):
    """tet_lhs_kernel, 16 tets per block: the sixteen blocks of every tet are ADDED to a non-zero val; the nonzeros of three
    more tets of the pattern, which the batch does not hold, stay bit-identical.  The kernel reads the cached geometry
    record, so the model starts from that record (no inverse inside: K = 1 in every family)."""
    L = api.lib()
    s = Soup(*case, extra=3)
    rp, ci = A.nodal_pattern(s.ien_all, s.N)
    nz = A.nzmap_fast(s.ien, rp, ci)
    assert np.array_equal(nz.ravel(), A.elem_nzmap(s.ien, rp, ci))
    nodep, _ = A.pack_nodes(s.N, s.xg, s.wg, s.dwg)
    mod = m_jacobian(s, LD)
    egeo = s.egeo
    val0 = np.random.default_rng(9).normal(size=(ci.size, 16))
    val0[nz] = s.lhs_preload
    es, zs, gs, ns, vs = (pool.slot(s.ien, 0, I32), pool.slot(nz.astype(np.int32), 0, I32), pool.slot(egeo), pool.slot(nodep),
                          pool.slot(val0))
    L.dfl_assemble_tet_lhs(s.B, es.ptr, zs.ptr, gs.ptr, ns.ptr, vs.ptr, None)
    api.sync()
    idx = nz[:, :, :, None] * 16 + np.arange(16)
    assert idx.size < val0.size
    bounded(vs, idx, mod, constant("jacobian", s.family, s.regime, m_jacobian), 1.0, "assemble_tet_lhs", "assemble_tet_lhs", s.case,
            family=s.family, regime=s.regime, shape=s.B)
    untouched("assemble_tet_lhs", es, zs, gs, ns)


def m_face(s, dt):
    W4 = np.concatenate([s.W[:, :, :3], s.W[:, :, 3:4]], axis=2)
    eF, eJ = A.face_terms(s.X, W4, np.arange(s.B) % 4, dt)
    return A.AV(np.concatenate([eF.v.reshape(s.B, -1), eJ.v.reshape(s.B, -1)], 1), np.concatenate([eF.a.reshape(s.B, -1), eJ.a.reshape(s.B, -1)], 1))


@needs_ld
@pytest.mark.parametrize("case", soup_cases(SIZES_FACE), ids=case_id)
def test_assemble_face(case, api, pool):
    """face_kernel, 64 faces per block, one face per soup tet, orientation = tet % 4: the direct form with and without a
    face_list (F only, val only, both), the parked form, and the parked form summed by dfl_face_sum_F / dfl_face_sum_J against
    the same model under the same bound as the direct form"""
    L = api.lib()
    s = Soup(*case, extra=2)
    nf, N = s.B, s.N
    rng = np.random.default_rng(13)
    order = rng.permutation(nf + 2)                                   # face f of the group sits on tet order[f]
    f2e = order.astype(np.int32)
    forn = (order % 4).astype(np.int32)
    pick = np.flatnonzero(order < nf)                                 # the faces on the first nf tets, in group order
    face_list = rng.permutation(pick).astype(np.int32)
    rp, ci = A.nodal_pattern(s.ien_all, N)
    mod = m_face(s, LD)
    c = constant("face", s.family, s.regime, m_face)
    K = s.Kfor(mod)
    eF, eJ = mod[:, :16].reshape(nf, 4, 4), mod[:, 16:].reshape(nf, 4, 4, 16)
    ien64 = s.ien.astype(I64).reshape(-1, 4)
    nz = A.nzmap_fast(s.ien, rp, ci)
    iF = np.stack([3 * ien64, 3 * ien64 + 1, 3 * ien64 + 2, 3 * N + ien64], axis=2)
    iJ = nz[:, :, :, None] * 16 + np.arange(16)
    F0, val0 = rng.normal(size=6 * N), rng.normal(size=16 * ci.size)
    F0[iF], val0[iJ] = scaled_normals(15, eF.a), scaled_normals(16, eJ.a)
    consts = [pool.slot(a, 0, I32) for a in (f2e, forn, s.ien_all, rp, ci, face_list)]
    fes, frs, ies, rps, cis, fls = consts
    xs, ws, ds = pool.slot(s.xg, 1), pool.slot(s.wg, 1), pool.slot(s.dwg, 1)
    Fs, vs = pool.slot(F0, 1), pool.slot(val0)
    consts += [xs, ws, ds]
    rec = dict(family=s.family, regime=s.regime, shape=nf)
    K3, K4 = K.reshape(-1, 1, 1), K.reshape(-1, 1, 1, 1)
    mF, mJ = A.AV(F0[iF].astype(LD)) + eF, A.AV(val0[iJ].astype(LD)) + eJ

    def check(what, wantF, wantJ):
        if wantF:
            bounded(Fs, iF, mF, c, K3, what + " F", "assemble_face", s.case + " " + what + " F", **rec)
        else:
            Fs.check(what + ": F was not asked for")
        if wantJ:
            bounded(vs, iJ, mJ, c, K4, what + " val", "assemble_face", s.case + " " + what + " val", **rec)
        else:
            vs.check(what + ": val was not asked for")
        untouched(what, *consts)
        Fs.reset()
        vs.reset()

    # direct form with a face list (nf of the nf + 2 faces of the group), every combination of outputs
    for wantF, wantJ in ((True, True), (True, False), (False, True)):
        L.dfl_assemble_face(nf, fls.ptr, fes.ptr, frs.ptr, ies.ptr, N, xs.ptr, ws.ptr, ds.ptr, Fs.ptr if wantF else None, rps.ptr,
                            cis.ptr, vs.ptr if wantJ else None, None)
        api.sync()
        check("direct list F=%d J=%d" % (wantF, wantJ), wantF, wantJ)
    # direct form without a list: the first nf faces of a group that is the soup's first nf tets in order
    f2e2, forn2 = pool.slot(np.arange(nf, dtype=np.int32), 0, I32), pool.slot((np.arange(nf) % 4).astype(np.int32), 0, I32)
    consts += [f2e2, forn2]
    L.dfl_assemble_face(nf, None, f2e2.ptr, forn2.ptr, ies.ptr, N, xs.ptr, ws.ptr, ds.ptr, Fs.ptr, rps.ptr, cis.ptr, vs.ptr, None)
    api.sync()
    check("direct", True, True)
    # parked form, then the ordered sums
    pFs, pJs = pool.slot(sent(16 * nf)), pool.slot(sent(256 * nf))
    for wantF, wantJ in ((True, False), (False, True), (True, True)):
        pFs.reset()
        pJs.reset()
        L.dfl_assemble_face_park(nf, f2e2.ptr, forn2.ptr, ies.ptr, N, xs.ptr, ws.ptr, ds.ptr, pFs.ptr if wantF else None,
                                 pJs.ptr if wantJ else None, None)
        api.sync()
        what = "park F=%d J=%d" % (wantF, wantJ)
        if wantF:
            bounded(pFs, np.arange(16 * nf), eF, c, K3, what + " pF", "assemble_face_park", s.case + " " + what + " pF", **rec)
        else:
            pFs.check(what + ": pF was not asked for")
        if wantJ:
            bounded(pJs, np.arange(256 * nf), eJ, c, K4, what + " pJ", "assemble_face_park", s.case + " " + what + " pJ", **rec)
        else:
            pJs.check(what + ": pJ was not asked for")
        untouched(what, *consts)
    nodes = rng.permutation(4 * nf)                                   # (face, a) pairs in shuffled order, one entry each
    fnode = ien64.ravel()[nodes].astype(np.int32)
    slots = [pool.slot(a, 0, I32) for a in (fnode, np.arange(4 * nf + 1, dtype=np.int32), nodes.astype(np.int32))]
    L.dfl_face_sum_F(4 * nf, slots[0].ptr, slots[1].ptr, slots[2].ptr, pFs.ptr, N, Fs.ptr, None)
    blocks = rng.permutation(16 * nf)
    fnz = nz.ravel()[blocks].astype(np.int32)
    slots += [pool.slot(a, 0, I32) for a in (fnz, np.arange(16 * nf + 1, dtype=np.int32), blocks.astype(np.int32))]
    L.dfl_face_sum_J(16 * nf, slots[3].ptr, slots[4].ptr, slots[5].ptr, pJs.ptr, vs.ptr, None)
    api.sync()
    consts += slots
    pFs.image[:] = pFs.dev.numpy()                                    # the parked values are inputs of the sums
    pJs.image[:] = pJs.dev.numpy()
    consts += [pFs, pJs]
    check("parked + sums", True, True)


# ======================================================================================================================
# schedules 0, 1 and 4 on real meshes: dfl_assemble_tet_lhs_slot, dfl_assemble_tet_rhs_lane (and the colour-batch chain)
# ======================================================================================================================
def _mesh(name):
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet
    return {"tet": single_tet, "fan": fan_mesh, "cube2": lambda: kuhn_cube(2), "cube6j": lambda: kuhn_cube(6, jitter=0.2)}[name]()


_MODELS = {}


def mesh_model(name, family, regime):
    """(mesh, wg, dwg, rp, ci, F, blocks, F restated, blocks restated, K) -- computed once per case, never modified"""
    key = (name, family, regime)
    if key not in _MODELS:
        m = A.scaled_mesh(_mesh(name), family)
        N = m.num_node
        wg, dwg = A.fields(m.xg, regime)
        rp, ci = A.nodal_pattern(m.ien, N)
        F, blk = A.assemble_tet(m.xg, m.ien, N, wg, dwg, rp, ci, LD)
        Fr, blkr = A.assemble_tet(m.xg, m.ien, N, wg, dwg, rp, ci, F64)
        K = float(A.kappa_inf(A.mesh_vertices(m.xg, m.ien)).max()) if family in A.KAPPA_FAMILIES else 1.0
        _MODELS[key] = (m, wg, dwg, rp, ci, F, blk, Fr, blkr, K)
    return _MODELS[key]


def preloads(F, blk):
    """what F and the block values hold before the call: of every entry's own size, so that neither side of the addition
    hides the other"""
    rng = np.random.default_rng(14)
    F0 = rng.normal(size=F.v.size) * np.asarray(np.maximum(F.a, 1e-300), F64)
    val0 = rng.normal(size=blk.v.shape) * np.asarray(np.maximum(blk.a, 1e-300), F64)
    return F0, val0


def mesh_constants(name, family, regime, beta):
    """c of preload + F and of beta * preload + blocks on this mesh, from the float64 restatement (the unit copy of the mesh
    for the families whose bound carries kappa)"""
    fam = "unit" if family in A.KAPPA_FAMILIES else family
    _, _, _, _, _, F, blk, Fr, blkr, _ = mesh_model(name, fam, regime)
    F0, val0 = preloads(F, blk)
    mF, mJ = A.AV(F0.astype(LD)) + F, A.AV(val0.astype(LD)) * beta + blk
    return (A.ratio_c(np.abs((F0 + Fr.v).astype(LD) - mF.v), mF.a), A.ratio_c(np.abs((beta * val0 + blkr.v).astype(LD) - mJ.v), mJ.a))


MESH_CASES = [("tet", "unit", "synthetic"), ("fan", "unit", "synthetic"), ("cube2", "unit", "synthetic"),
              ("cube6j", "unit", "synthetic")]
MESH_CASES += [("fan", f, "synthetic") for f in A.FAMILIES[1:5]] + [("cube6j", f, "synthetic") for f in A.FAMILIES[1:5]]
MESH_CASES += [("cube6j", "unit", r) for r in A.REGIMES[1:]] + [("cube6j", "stretched", "convective")]


def run_mesh(api, name, family, regime, schedule, *, beta=1.0, params=None, cap=None, want_F=True, want_J=True):
    """AssembleSystemTet / DflAssembleSystemTetBeta into a preloaded F and preloaded block values; judged entry by entry
    against beta * preload + model, and the continuity identity on the device's F_p rows"""
    L = api.lib()
    m, wg, dwg, rp, ci, F, blk, _, _, K = mesh_model(name, family, regime)
    cF, cJ = mesh_constants(name, family, regime, beta)
    N = m.num_node
    newton = schedule == 4
    rec = dict(family=family, regime=regime, shape="%s N%d T%d" % (name, N, m.num_tet), schedule=schedule)
    tag = "%s-%s-%s sched%d beta%g params%s cap%s" % (name, family, regime, schedule, beta, params, cap)
    saved = tuple(L.DflAsmDefaults().contents[2:5])
    try:
        if params:
            L.DflSetSlotPatchParameters(*params)
        if cap is not None:
            L.dfl_set_rhs_lane_grid_cap(cap)
        P = api.Problem(m, schedule=schedule, bcs=[])
        try:
            prp, pci = P.pattern()
            assert np.array_equal(prp, rp) and np.array_equal(pci, ci)
            F0, val0 = preloads(F, blk)
            wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
            F_d = api.DeviceArray.from_numpy(F0)
            P.block_values().upload(val0.ravel())
            L.DflAssembleSystemTetBeta(P.mesh, wg_d.ptr, dwg_d.ptr, F_d.ptr if want_F else None, P.J if want_J else None, beta)
            api.sync()
            if want_F:
                got = F_d.numpy()
                mod = A.AV(F0.astype(LD)) + F
                judge(got, mod, cF, K, tag + " F", "assemble_system_tet_F", tag, newton, **rec)
                # identity on the device: sum of the F_p rows against sum_tets |det J| / 6 div u_h from the mesh alone
                rows = slice(3 * N, 4 * N)
                lhs = (got[rows].astype(LD) - F0[rows].astype(LD)).sum()
                ident = A.continuity_identity(m.xg, m.ien, wg)
                b = A.bound(mod[rows], cF, K, newton).astype(LD).sum() + 2e-15 * F.a[rows].sum()
                r = float(abs(lhs - ident.v) / b) if b > 0 else 0.0
                record("continuity_identity", tag, r, c=float(cF), **rec)
                assert (r <= 1.0) if b > 0 else (lhs == 0), "%s: sum F_p - sum |detJ|/6 div u = %.3g of its bound" % (tag, r)
            else:
                assert np.array_equal(F_d.numpy().view(np.uint64), F0.view(np.uint64)), tag + ": F was not asked for"
            gotv = P.block_values().numpy().reshape(-1, 16)
            if want_J:
                judge(gotv, A.AV(val0.astype(LD)) * beta + blk, cJ, K, tag + " blocks", "assemble_system_tet_J", tag, newton, **rec)
            else:
                assert np.array_equal(gotv.view(np.uint64), val0.view(np.uint64)), tag + ": J was not asked for"
        finally:
            P.close()
    finally:
        L.DflSetSlotPatchParameters(*saved)
        L.dfl_set_rhs_lane_grid_cap(0)


@needs_ld
@pytest.mark.parametrize("schedule", [0, 1, 4])
@pytest.mark.parametrize("name,family,regime", MESH_CASES, ids=lambda v: str(v))
def test_schedules_on_meshes(name, family, regime, schedule, api):
    """schedule 4 runs dfl_pack_nodes2 + dfl_assemble_tet_lhs_slot + dfl_assemble_tet_rhs_lane + dfl_rhs_node_sum; schedules 0
    and 1 run dfl_elem_nzmap + dfl_elem_geometry + dfl_assemble_tet_rhs / _lhs per colour + dfl_unpack_rhs.  All three are
    judged entry by entry against the same model."""
    run_mesh(api, name, family, regime, schedule)


@needs_ld
@pytest.mark.parametrize("params", [(16, 255, 208), (1, 40, 64), (5, 60, 40)], ids=str)
@pytest.mark.parametrize("name", ["tet", "fan", "cube2", "cube6j"])
def test_slot_owner_patch_shapes_and_beta(name, params, api):
    """dfl_assemble_tet_lhs_slot with patches of 16 / 1 / 5 leaf nodes and beta_J in {0, 1, -0.5} against beta * preload +
    model (beta = 0 must not read the preload's sign or size: it is judged against the model alone)"""
    for beta in (0.0, 1.0, -0.5):
        run_mesh(api, name, "unit", "synthetic", 4, beta=beta, params=params, want_F=False)


@needs_ld
@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("name", ["tet", "fan", "cube2", "cube6j"])
def test_lane_residual_grid_cap(name, cap, api):
    """dfl_assemble_tet_rhs_lane on the resident grid and capped (8 workgroups: every wave walks several patches of
    kuhn_cube(6) through the pipelined loop); the block values are not touched"""
    run_mesh(api, name, "unit", "synthetic", 4, cap=cap, want_J=False)
