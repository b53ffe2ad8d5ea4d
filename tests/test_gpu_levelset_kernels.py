"""Every launcher of the level-set redistancing and volume correction (csrc/k_redistance.hip, csrc/k_volume.hip; the per-tet
closed forms of csrc/level_facets.hpp and the reductions of csrc/block_ops.hpp) alone, through ctypes, against
tests/levelset_kernel_model.py.

Tier A (bitwise, integers): blk_count, cell_count, cell_fill, the band list, ncand; list and the entries of a cell as sets.
Tier E (bitwise, floats): facets, part, out, new phi and chg against the float64 restatement plus the tree model; the per-tet
volumes and ||g| - 1| through the isolation deck, where a workgroup holds one live tet and the tree adds zeros.
Tier B (rounded, independent): per tet |v - closed form| <= 4 c_vol u V K against the divided-difference form, per node
|d^2 - region method| <= 4 c_dist u max_v |p - v|^2 on the well-shaped family, both references in np.longdouble; c_vol and
c_dist are what the float64 restatement shows on the CPU (test_levelset_kernel_model_cpu.py), 4 is the margin
test_gpu_redistance.py grants the device over the model's own deviation.  In the node test level = 0 and old > 0, so phi is the
distance itself; the rounding of its square root (u d^2) lies inside the bound.

Every array sits between guard bands (guarded_buffers.py); overwrite outputs are preloaded with the sentinel, accumulate
outputs with known nonzero values; after each launch the bands, every const input and every entry the call must not write
are compared bit for bit.  Index arrays a launcher reads are the model's or a device output verified earlier in the same
test.  The caps are short by a few entries only, far inside the guard bands.  No case aims at a fault.  err / bound go to the
file named by DFL_PARITY_OUT (profiles/levelset_kernel_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import levelset_kernel_model as M
import redistance_model as rm
from guarded_buffers import ALL, I32, U8, Pool, Recorder, assert_bits, raw, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
U = M.U
record = Recorder("a")
needs_ld = pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON)
vp, f64, i32 = C.c_void_p, C.c_double, C.c_int32
ISENT = int(sent(1, I32)[0])


class Grid(C.Structure):
    _fields_ = [("lo", f64 * 3), ("inv_h", f64), ("n", i32 * 3)]


def _declare(L):
    gp = C.POINTER(Grid)
    sig = {
        "dfl_scan_counts": (None, [i32, vp, vp, vp, vp]),
        "dfl_scan_num_chunks": (i32, [i32]),
        "dfl_tets_per_block": (i32, []),
        "dfl_node_reduce_max_part": (i32, []),
        "dfl_redistance_cut": (None, [i32, vp, vp, vp, i32, f64, gp, vp, vp, vp, vp]),
        "dfl_redistance_emit": (None, [i32, vp, vp, vp, i32, f64, gp, vp, vp, vp, vp, i32, vp, i32, vp]),
        "dfl_redistance_nodes": (None, [i32, vp, vp, f64, f64, gp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "dfl_redistance_node_stats": (None, [i32, vp, vp, vp, vp]),
        "dfl_redistance_reduce": (None, [i32, vp, vp, vp]),
        "dfl_volume_classify": (None, [i32, vp, vp, vp, i32, f64, f64, f64, vp, vp, vp, vp]),
        "dfl_volume_emit": (None, [i32, vp, vp, i32, f64, f64, vp, vp, i32, vp]),
        "dfl_volume_eval": (None, [i32, vp, vp, vp, vp, i32, C.POINTER(f64), vp, vp, vp]),
        "dfl_volume_shift": (None, [i32, vp, f64, vp]),
        "dfl_volume_node_sum": (None, [i32, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args


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

    def ints(self, data):
        return self.slot(np.asarray(data).astype(I32), 0, I32)


@pytest.fixture
def pool(api):
    p = FlatPool(api)
    yield p
    p.free()


def exact(slot, want, what, dtype=F64):
    """the whole array == want bit for bit, the bands as uploaded"""
    got = slot.check(what, ALL)
    assert_bits(got, np.ravel(want), what, dtype)
    return got


def untouched(what, *slots):
    for s in slots:
        if s is not None:
            s.check(what + ": an array the call must not write changed")


def settle(*slots):
    """what the device holds now is what a later check compares with"""
    for s in slots:
        s.image[s.lo: s.lo + s.n] = s.get()


def same_numbers(got, want, what):
    """bit for bit where the model has a number; a NaN where it has a NaN (the payload of a computed NaN is not modelled)"""
    got, want = np.ravel(got), np.ravel(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs in other places"
    assert_bits(got[~nan], want[~nan], what)


def cgrid(g):
    return Grid((f64 * 3)(*g.lo), g.inv_h, (i32 * 3)(*g.n))


def test_constants_and_struct(api):
    L = api.lib()
    assert L.dfl_tets_per_block() == M.BLK == 256 and L.dfl_node_reduce_max_part() == M.MAX_PART == 1024
    assert C.sizeof(Grid) == 48 and M.K == 15


# ======================================================================================================================
# decks, grids and the model's answers, computed once
# ======================================================================================================================
BUILDERS = {"orbit": M.orbit, "orbit-shared": M.orbit_shared, "swapped-cube": M.swapped_cube, "on-level": M.on_level,
            "dyadic": M.dyadic}
SLICES = [("on-level", n) for n in (1, 255, 256, 257, 384, 512, 3 * 256 + 1)]
DECKS = [(k, None) for k in BUILDERS] + SLICES
_cache = {}


def deck(name, nt=None):
    if (name, nt) not in _cache:
        d = BUILDERS[name]() if name in BUILDERS else getattr(M, name)()
        _cache[(name, nt)] = d if nt is None else d.first(nt)
    return _cache[(name, nt)]


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def grids(d, name):
    """the grids of a deck: 1 x 1 x 1; 5 x 1 x 3; one smaller than the mesh (vertices clamp into its edge cells); and for the
    small decks a cell edge of a quarter of a facet; for the dyadic deck cells of 2^-2 whose boundaries the vertices sit on"""
    lo, hi = d.xg.min(axis=0), d.xg.max(axis=0)
    ext = float((hi - lo).max())
    out = {"1x1x1": M.make_grid(lo, 1.0 / ext, (1, 1, 1)), "5x1x3": M.make_grid(lo, 5.0 / ext, (5, 1, 3)),
           "smaller": M.make_grid(lo + 0.3 * (hi - lo), 4.0 / (0.4 * ext), (4, 3, 4))}
    if name in ("orbit-shared", "swapped-cube"):
        h = 0.125 if name == "orbit-shared" else 0.0625
        out["quarter"] = M.make_grid(lo, 1.0 / h, tuple(int(np.ceil(q / h)) + 1 for q in hi - lo))
    if name == "dyadic":
        out["on-boundaries"] = M.make_grid([0.0, 0.0, 0.0], 4.0, (13, 13, 13))
    return out


class Bufs:
    """the guarded mesh and state of one deck"""

    def __init__(self, pool, d):
        self.d = d
        self.ien, self.xg, self.w = pool.slot(d.ien, 0, I32), pool.slot(d.xg), pool.slot(d.w())
        self.nblk = -(-d.NT // M.BLK)

    def const(self, what):
        untouched(what, self.ien, self.xg, self.w)


# ======================================================================================================================
# dfl_redistance_cut
# ======================================================================================================================
@pytest.mark.parametrize("name,nt", DECKS)
def test_cut(name, nt, api, pool):
    """part [nblk][2] bit for bit (E), blk_count and cell_count (A, cell_count += on a nonzero preload) on every grid; without
    blk_count, with and without a grid, the same part and nothing else written"""
    L, d = api.lib(), deck(name, nt)
    ref = cached(("cut", name, nt), lambda: M.cut(d.xg, d.ien, d.phi, d.level))
    b = Bufs(pool, d)
    for gname, g in grids(d, name).items():
        what = "cut %s/%s %s" % (name, nt, gname)
        count, start, sets = cached(("cells", name, nt, gname), lambda: M.cell_lists(ref["facets"], g))
        pre = (np.arange(g.ncell) * 7 + 3) % 11
        part, blk, cc = pool.slot(sent(2 * b.nblk)), pool.slot(sent(b.nblk, I32), 0, I32), pool.ints(pre)
        gs = cgrid(g)
        L.dfl_redistance_cut(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(gs), blk.ptr, cc.ptr, part.ptr, None)
        api.sync()
        exact(part, ref["part"], what + " part")
        exact(blk, ref["blk_count"], what + " blk_count", I32)
        exact(cc, pre + count, what + " cell_count", I32)
        b.const(what)
        settle(blk, cc)
        for gp in (C.byref(gs), None):
            part.reset(sent(2 * b.nblk))
            L.dfl_redistance_cut(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, gp, None, None, part.ptr, None)
            api.sync()
            exact(part, ref["part"], what + " part, statistics alone")
            untouched(what + " statistics alone", blk, cc)
        b.const(what)
        for s in (part, blk, cc):
            s.dev.free()
            pool.slots.remove(s)
    nan_tets = int(np.isnan(d.phi[d.ien]).any(axis=1).sum())
    record("dfl_redistance_cut", "%s/%s" % (name, nt or d.NT), 0.0, exact=True, tets=d.NT, facets=len(ref["facets"]), nan_tets=nan_tets)


def test_cut_counts_a_facet_without_a_finite_vertex(api, pool):
    """a NaN at the lone node that is not positive: no vertex of the facet is finite, it enters no cell and is still counted; a NaN at one
    of the others: the facet enters the cells of its two finite vertices"""
    L = api.lib()
    x, f3 = M._orbit_values(M.PERMS[7], 0b0111)
    _, f1 = M._orbit_values(M.PERMS[7], 0b0010)
    phi = np.r_[f3, f1]
    phi[3] = np.nan            # the one node of the first tet that is not positive: every crossing point is a NaN
    phi[4 + 2] = np.nan        # one of the three that are not, of the second: one crossing point is
    d = M.Deck("nan-facets", np.r_[x, x + 0.5], np.arange(8).reshape(2, 4), phi, M.ORBIT_LEVEL)
    F, _ = rm.facets(d.xg, d.ien, d.phi, d.level)
    assert len(F) == 2 and np.isnan(F[0].reshape(3, 3)).any(axis=1).all() and np.isnan(F[1].reshape(3, 3)).any(axis=1).sum() == 1
    g = M.make_grid(d.xg.min(axis=0), 8.0, (14, 14, 14))
    count, _, sets = M.cell_lists(F, g)
    assert count.sum() > 1 and all(s <= {1} for s in sets)
    b = Bufs(pool, d)
    part, blk, cc = pool.slot(sent(2)), pool.slot(sent(1, I32), 0, I32), pool.ints(np.zeros(g.ncell))
    L.dfl_redistance_cut(2, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(cgrid(g)), blk.ptr, cc.ptr, part.ptr, None)
    api.sync()
    exact(blk, [2], "blk_count", I32)
    exact(cc, count, "cell_count", I32)
    assert part.check("part", ALL)[0] == 0.0       # a NaN volume adds nothing
    record("dfl_redistance_cut", "facets with NaN vertices", 0.0, exact=True)


@needs_ld
def test_cut_isolation(api, pool):
    """one live tet per workgroup: part[b] is that tet's own volume and ||g| - 1|, bit for bit against the restatement (E) and
    within 4 c_vol u V K of the closed form (B), for the 384 orbit cases at the thread positions 0, 1, 63, 64, 127, 128, 255"""
    L, d = api.lib(), deck("isolation")
    live = d.info["live"]
    ref = cached(("cut", "isolation", None), lambda: M.cut(d.xg, d.ien, d.phi, d.level))
    b = Bufs(pool, d)
    part, blk, cc = pool.slot(sent(2 * b.nblk)), pool.slot(sent(b.nblk, I32), 0, I32), pool.ints([5])
    g = M.make_grid(d.xg.min(axis=0), 0.01, (1, 1, 1))
    L.dfl_redistance_cut(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(cgrid(g)), blk.ptr, cc.ptr, part.ptr, None)
    api.sync()
    got = exact(part, ref["part"], "isolation part").reshape(-1, 2)
    assert_bits(got[:, 0], ref["vol"][live], "the live tet's volume")
    assert_bits(got[:, 1], ref["dev"][live], "the live tet's | |g| - 1 |")
    exact(blk, M.facet_counts(M.tet_masks(d.ien[live], d.phi, d.level)), "blk_count", I32)
    exact(cc, [5 + len(ref["facets"])], "cell_count", I32)
    b.const("isolation")
    cv = M.c_vol()[0]
    want, V, K = M.closed_form_volume(d.xg, d.ien[live], d.phi, d.level)
    bound = 4.0 * cv * LD(U) * V * K
    err = np.abs(got[:, 0].astype(LD) - want)
    assert (err[K == 0] == 0).all()
    ratio = float((err[K > 0] / bound[K > 0]).max())
    print(f"cut isolation: worst err / bound {ratio:.3f} with c_vol = {cv:.2f}")
    record("dfl_redistance_cut", "isolation, per tet against the closed form", ratio, c_vol=cv, tets=len(live))
    assert ratio <= 1.0


def test_nothing_to_do_writes_nothing(api, pool):
    """T <= 0, N <= 0, nband <= 0 and npart <= 0"""
    L = api.lib()
    s = [pool.slot(sent(32)) for _ in range(4)]
    q = [pool.slot(sent(32, I32), 0, I32) for _ in range(5)]
    gs = cgrid(M.make_grid([0.0, 0.0, 0.0], 1.0, (1, 1, 1)))
    cand = (f64 * M.K)(*([0.0] * M.K))
    for n in (0, -1):
        L.dfl_redistance_cut(n, q[0].ptr, s[0].ptr, s[1].ptr, 4, 0.0, C.byref(gs), q[1].ptr, q[2].ptr, s[2].ptr, None)
        L.dfl_redistance_emit(n, q[0].ptr, s[0].ptr, s[1].ptr, 4, 0.0, C.byref(gs), q[1].ptr, q[2].ptr, q[3].ptr, s[2].ptr, 3, q[4].ptr, 3, None)
        L.dfl_redistance_nodes(n, s[0].ptr, s[1].ptr, 0.0, 1.0, C.byref(gs), q[0].ptr, q[1].ptr, s[2].ptr, 3, None, q[2].ptr, q[3].ptr, s[3].ptr, None)
        L.dfl_redistance_node_stats(n, s[0].ptr, s[1].ptr, s[2].ptr, None)
        L.dfl_redistance_reduce(n, s[0].ptr, s[1].ptr, None)
        L.dfl_volume_classify(n, q[0].ptr, s[0].ptr, s[1].ptr, 4, 0.0, -1.0, 1.0, q[1].ptr, s[2].ptr, s[3].ptr, None)
        L.dfl_volume_emit(n, q[0].ptr, s[1].ptr, 4, -1.0, 1.0, q[1].ptr, q[2].ptr, 3, None)
        L.dfl_volume_eval(n, q[0].ptr, q[1].ptr, s[0].ptr, s[1].ptr, 4, cand, s[2].ptr, s[3].ptr, None)
        L.dfl_volume_shift(n, s[0].ptr, 1.0, None)
        L.dfl_volume_node_sum(n, s[0].ptr, s[1].ptr, s[2].ptr, None)
        api.sync()
        untouched("n = %d" % n, *(s + q))


# ======================================================================================================================
# dfl_redistance_emit
# ======================================================================================================================
def check_entries(ent, start, fill, sets, what):
    for c, s in enumerate(sets):
        got = ent[start[c]:start[c] + fill[c]].tolist()
        assert len(got) == len(s) and set(got) == s, "%s: cell %d holds %r, want %r" % (what, c, sorted(got), sorted(s))


@pytest.mark.parametrize("name,nt", [(k, None) for k in BUILDERS] + [("on-level", 257), ("on-level", 512)])
def test_emit(name, nt, api, pool):
    """the facets in ascending tet order bit for bit, cell_fill == cell_count, the entries of every cell as sets; then with
    cap_facets short by 1, 2, 3 and cap_entries short by 1, 3, 8: nothing at or past a cap, a clipped facet in no cell"""
    L, d = api.lib(), deck(name, nt)
    ref = cached(("cut", name, nt), lambda: M.cut(d.xg, d.ien, d.phi, d.level))
    F = ref["facets"]
    nf = len(F)
    b = Bufs(pool, d)
    base = pool.ints(M.exclusive_scan(ref["blk_count"]))
    gl = grids(d, name)
    for gname in [k for k in gl if k != "1x1x1"][:3] + ["1x1x1"]:
        g = gl[gname]
        count, start, sets = cached(("cells", name, nt, gname), lambda: M.cell_lists(F, g))
        ne = int(start[-1])
        cs, gs = pool.ints(start), cgrid(g)
        caps = [(nf, ne)] if gname != "5x1x3" else [(nf, ne)] + [(nf - s, ne) for s in (1, 2, 3)] + [(nf, ne - r) for r in (1, 3, 8)]
        for cap_f, cap_e in caps:
            what = "emit %s/%s %s caps %d/%d %d/%d" % (name, nt, gname, cap_f, nf, cap_e, ne)
            assert cap_f > 0 and cap_e > 0
            fill, fac, ent = pool.ints(np.zeros(g.ncell)), pool.slot(sent(9 * cap_f)), pool.slot(sent(cap_e, I32), 0, I32)
            L.dfl_redistance_emit(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(gs), base.ptr, cs.ptr, fill.ptr, fac.ptr,
                                  cap_f, ent.ptr, cap_e, None)
            api.sync()
            same_numbers(fac.check(what + " facets", ALL), F[:cap_f], what + " facets")
            got_fill = fill.check(what + " cell_fill", ALL).astype(I64)
            got_ent = ent.check(what + " entries", ALL).astype(I64)
            if cap_f == nf:
                assert np.array_equal(got_fill, count), what + ": cell_fill != cell_count"
                want_sets = sets
            else:
                want_sets = [{i for i in s if i < cap_f} for s in sets]
                assert np.array_equal(got_fill, [len(s) for s in want_sets]), what + ": a clipped facet entered a cell"
            if cap_e == ne:
                check_entries(got_ent, start, got_fill, want_sets, what)
                assert (got_ent == ISENT).sum() == ne - got_fill.sum(), what + ": entries outside the cells' fills were written"
            else:                      # the positions below the cap are all written, each with a facet of its cell
                for c, s in enumerate(sets):
                    got = got_ent[start[c]:min(start[c] + count[c], cap_e)].tolist()
                    assert len(set(got)) == len(got) and set(got) <= s, what + ": cell %d" % c
            untouched(what, base, cs)
            b.const(what)
            for s in (fill, fac, ent):
                s.dev.free()
                pool.slots.remove(s)
    record("dfl_redistance_emit", "%s/%s" % (name, nt or d.NT), 0.0, exact=True, facets=nf)


# ======================================================================================================================
# dfl_redistance_nodes
# ======================================================================================================================
class NodeCase:
    """the inputs of one dfl_redistance_nodes call on the first N nodes: x [N, 3], old phi [N], grid, per cell the list of entries
    (ids, also ids the kernel must pass over), facets [nf, 9], cap_facets, hold or None"""

    def __init__(self, x, old, level, band, g, cells, F, cap_facets=None, hold=None):
        self.x, self.old, self.level, self.band, self.g = np.asarray(x, F64), np.asarray(old, F64), level, band, g
        self.F = np.asarray(F, F64).reshape(-1, 9)
        self.cap = len(self.F) if cap_facets is None else cap_facets
        self.start = M.exclusive_scan([len(c) for c in cells])
        self.entries = np.array([i for c in cells for i in c], I64)
        self.hold = hold

    def model(self):
        return M.nodes(self.x, self.old, self.level, self.band, self.g, self.start, self.entries, self.F, self.cap, self.hold)


def run_nodes(api, pool, case, want=None, what="nodes", again=None):
    """one call on guarded buffers, everything compared; `again`: a second case on the same state, output and list buffers"""
    L, N = api.lib(), len(case.x)
    w = np.random.default_rng(5).uniform(-2.0, 2.0, 6 * N)
    w[4 * N:5 * N] = case.old
    xs, ws = pool.slot(case.x), pool.slot(w)
    ncand, lst, chg = pool.ints([0]), pool.slot(sent(N, I32), 0, I32), pool.slot(sent(N))
    phi_slot = np.zeros(6 * N, bool)
    phi_slot[4 * N:5 * N] = True
    out = None
    for k, cs in enumerate([case] + ([again] if again is not None else [])):
        tag = what + (" (second call)" if k else "")
        new, cg, listed = want if (want is not None and k == 0) else cs.model()
        start, ent = pool.ints(cs.start), pool.ints(cs.entries if len(cs.entries) else [0])
        fac = pool.slot(cs.F if len(cs.F) else np.zeros(9))
        hold = None if cs.hold is None else pool.slot(cs.hold.astype(U8), 0, U8)
        if k:
            ncand.reset([0])
            lst.reset(sent(N, I32))
            ws.image[ws.lo: ws.lo + ws.n] = ws.get()      # the state as the first call left it
            new, cg, listed = M.nodes(cs.x, ws.host()[4 * N:5 * N], cs.level, cs.band, cs.g, cs.start, cs.entries, cs.F, cs.cap, cs.hold)
        L.dfl_redistance_nodes(N, xs.ptr, ws.ptr, cs.level, cs.band, C.byref(cgrid(cs.g)), start.ptr, ent.ptr, fac.ptr, cs.cap,
                               None if hold is None else hold.ptr, ncand.ptr, lst.ptr, chg.ptr, None)
        api.sync()
        got_w = ws.check(tag + " w: only the phi slot may change", written=phi_slot)
        assert_bits(got_w[4 * N:5 * N], new, tag + " phi")
        exact(chg, cg, tag + " chg")
        exact(ncand, [len(listed)], tag + " ncand", I32)
        got_list = lst.check(tag + " list", ALL).astype(I64)
        assert set(got_list[:len(listed)].tolist()) == set(listed) and (got_list[len(listed):] == ISENT).all(), tag + " list"
        untouched(tag, xs, start, ent, fac, hold)
        out = (got_w[4 * N:5 * N].copy(), cg, listed)
    return out


def mesh_node_case(d, N, level, band, cell, hold=None):
    """the first N nodes of a deck against the facets of the whole deck at `level`, the grid over its bounding box"""
    F, _ = rm.facets(d.xg, d.ien, d.phi, level)
    lo, hi = d.xg.min(axis=0), d.xg.max(axis=0)
    g = M.make_grid(lo, 1.0 / cell, tuple(int(np.floor(q / cell)) + 1 for q in hi - lo))
    _, start, sets = M.cell_lists(F, g)
    return NodeCase(d.xg[:N], d.phi[:N], level, band, g, [sorted(s) for s in sets], F, hold=hold)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 125, 255, 256, 257])
def test_nodes_on_a_mesh(N, api, pool):
    """the first N nodes of the swapped cube (6^3 cells for N > 125) against its own facets, hold NULL and a mask; then a second
    call on the result with the lists of a larger facet set"""
    d = deck("swapped-cube") if N <= 125 else cached("cube6", lambda: M.swapped_cube(6))
    h = 0.25 if N <= 125 else 1.0 / 6.0
    case = mesh_node_case(d, N, d.level, 1.2 * h, 1.2 * h)
    hold = (np.arange(N) % 3 == 1)
    held = mesh_node_case(d, N, d.level, 1.2 * h, 1.2 * h, hold=hold)
    more = mesh_node_case(d, N, d.level - 0.21, 0.8 * h, 0.8 * h)
    assert len(more.F) != len(case.F) and len(case.F) > 50
    _, cg, listed = run_nodes(api, pool, case, what="nodes N=%d" % N, again=more)
    pool.free()
    new_h, cg_h, _ = run_nodes(api, pool, held, what="nodes N=%d held" % N)
    assert_bits(new_h[hold], case.old[hold], "held nodes keep their bits")
    assert N < 100 or ((cg >= 0).any() and (cg < 0).any() and 0 < len(listed))
    record("dfl_redistance_nodes", "swapped cube N=%d" % N, 0.0, exact=True, listed=len(listed), band_nodes=int((cg >= 0).sum()))


def special_node_case():
    """a 4 x 4 x 4 grid of unit cells over [0, 4)^3 with hand-made facets: a right triangle of legs 3/4 in z = 1 of cell (1, 1, 1), 70
    small facets in cell (3, 3, 3) and 20 in cell (0, 3, 0), an entry -1 and an entry == cap_facets among those of cell (1, 1, 1)"""
    g = M.make_grid([0.0, 0.0, 0.0], 1.0, (4, 4, 4))
    rng = np.random.default_rng(8)
    F = [np.array([1.0, 1.0, 1.0, 1.75, 1.0, 1.0, 1.0, 1.75, 1.0])]     # (inside cell (1, 1, 1) alone, boundaries included)
    for org, n in (((3.0, 3.0, 3.0), 70), ((0.0, 3.0, 0.0), 20)):
        for _ in range(n):
            F.append((np.array(org) + rng.uniform(0.1, 0.9, (3, 3))).ravel())
    F = np.array(F)
    _, _, sets = M.cell_lists(F, g)
    cells = [sorted(s) for s in sets]
    c111 = 1 + 4 * (1 + 4 * 1)
    assert cells[c111] == [0] and len(cells[63]) == 70 and len(cells[12]) == 20
    cells[c111] = [-1, 0, len(F)]
    level, band = 0.0, 0.5
    x = [[1.25, 1.25, 1.5],      # 0: above the interior at height 1/2: d == band exactly, chg -1, phi = level + band
         [1.25, 1.25, 0.5],      # 1: the same below, old negative: phi = level - band
         [1.25, 1.25, 1.25],     # 2: d = 1/4 inside the band
         [1.25, 1.25, 0.75],     # 3: old == level exactly: the negative side
         [1.25, 1.25, 1.125],    # 4: NaN old: keeps its bits, chg 0 (inside the band)
         [1.25, 1.25, 1.75],     # 5: NaN old outside the band: chg -1
         [2.5, 0.5, 2.5],        # 6: cell (2, 0, 2): the facet's cell is in exactly one of its nine runs
         [0.5, 3.5, 3.5],        # 7: no entry at all
         [3.5, 3.5, 3.5],        # 8: the corner cell with 70 entries in one run
         [3.95, 3.95, 3.95],     # 9: the same corner
         [9.0, 9.0, 9.0],        # 10: outside the box, clamped into that corner
         [0.5, 3.5, 0.5],        # 11: the cell with 20 entries
         [-3.0, 7.0, -2.0],      # 12: outside, clamped into it
         [0.5, 0.5, 3.5],        # 13: a corner cell without entries
         [1.25, 1.25, 1.0],      # 14: on the facet: d = 0
         [3.5, 3.5, 3.5]]        # 15: NaN old among 70 entries
    old = np.array([2.0, -2.0, 2.0, level, np.nan, np.nan, 1.0, 3.0, 0.3, -0.3, 5.0, 0.2, -4.0, -1.0, 0.7, np.nan])
    old[4] = np.array([0x7FF8000000000ABC], np.uint64).view(F64)[0]
    return NodeCase(x, old, level, band, g, cells, F, cap_facets=len(F))


def test_nodes_special_cases(api, pool):
    case = special_node_case()
    new, chg, listed = case.model()
    # the model's answers are the header's
    assert (new[0], chg[0]) == (0.5, -1.0) and (new[1], chg[1]) == (-0.5, -1.0) and (new[2], chg[2]) == (0.25, 1.75)
    assert (new[3], chg[3]) == (-0.25, 0.25) and raw(new[4:5])[0] == 0x7FF8000000000ABC and chg[4] == 0.0 and chg[5] == -1.0
    assert 6 in listed and 7 not in listed and 13 not in listed and (new[7], chg[7]) == (0.5, -1.0) and new[13] == -0.5
    assert sum(hi > lo for lo, hi in M.node_runs(case.x[6], case.g, case.start)) == 1
    assert max(hi - lo for lo, hi in M.node_runs(case.x[8], case.g, case.start)) == 70
    assert 16 < max(hi - lo for lo, hi in M.node_runs(case.x[11], case.g, case.start)) <= 64
    assert chg[8] >= 0 and chg[14] == 0.7 and new[14] == 0.0 and np.isnan(new[15])
    for N in (16, 13):
        sub = NodeCase(case.x[:N], case.old[:N], case.level, case.band, case.g, [[]], case.F, case.cap)
        sub.start, sub.entries = case.start, case.entries
        run_nodes(api, pool, sub, what="special nodes N=%d" % N)
        pool.free()
        hold = np.zeros(N, bool)
        hold[[2, 7, 8]] = True
        sub.hold = hold
        got, cg, _ = run_nodes(api, pool, sub, what="special nodes N=%d held" % N)
        assert_bits(got[hold], sub.old[hold], "held nodes keep their bits")
        assert cg[2] == 0.0 and cg[7] == -1.0
        pool.free()
    record("dfl_redistance_nodes", "hand-made cells", 0.0, exact=True)


@pytest.mark.parametrize("N", [32768 + 16 * 3 + 5, 2 * 32768 + 16 + 5])
def test_nodes_group_loop(N, api, pool):
    """every node is a candidate (one cell, two facets), so the 16-lane groups go round their loop a second (and, for the larger
    N, a third) time: 2048 workgroups of 16 groups take 32768 nodes per trip"""
    rng = np.random.default_rng(N)
    x = rng.uniform(-1.0, 1.0, (N, 3))
    old = rng.uniform(-1.0, 1.0, N)
    F = np.array([[-0.5, -0.4, 0.1, 0.6, -0.3, 0.0, 0.1, 0.7, -0.1], [0.9, 0.9, 0.9, 0.8, 0.95, 0.7, 0.7, 0.9, 0.95]])
    g = M.make_grid([-1.0, -1.0, -1.0], 0.5, (1, 1, 1))
    case = NodeCase(x, old, 0.1, 0.75, g, [[0, 1]], F)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.fmin(rm.dist2(x, F[0]), rm.dist2(x, F[1])))
    m = np.where(d < 0.75, d, 0.75)
    new = 0.1 + np.where(old - 0.1 > 0.0, m, -m)
    chg = np.where(d < 0.75, np.abs(new - old), -1.0)
    for a in (0, 1, N // 2, N - 1):                        # the vectorised answer is the model's
        one = M.nodes(x[a:a + 1], old[a:a + 1], 0.1, 0.75, g, case.start, case.entries, F, 2)
        assert one[0][0] == new[a] and one[1][0] == chg[a]
    assert N > M.MAX_GROUP_BLOCKS * (M.BLK // M.LANES) and (chg >= 0).any() and (chg < 0).any()
    run_nodes(api, pool, case, want=(new, chg, set(range(N))), what="nodes N=%d" % N)
    record("dfl_redistance_nodes", "group loop N=%d" % N, 0.0, exact=True, trips=-(-N // 32768))


@needs_ld
def test_nodes_against_the_region_method(api, pool):
    """64 well-shaped triangles and 64 points in one cell, level 0, old > 0, the band beyond every distance: phi is the distance
    to the nearest triangle; its square against the Voronoi-region method under 4 c_dist u max_v |p - v|^2"""
    F, P = M.well_shaped(64, seed=21)
    g = M.make_grid([-9.0, -9.0, -9.0], 0.01, (1, 1, 1))
    case = NodeCase(P, np.ones(len(P)), 0.0, 100.0, g, [list(range(len(F)))], F)
    new, _, _ = run_nodes(api, pool, case, what="well-shaped")
    cd = M.c_dist()[0]
    worst = 0.0
    for a in range(len(P)):
        ref = [M.region_dist2(P[a], F[i]) for i in range(len(F))]
        i = int(np.argmin(ref))
        bound = 4.0 * cd * LD(U) * LD(M.dist_scale(P[a:a + 1], F[i:i + 1])[0])
        worst = max(worst, float(abs(LD(new[a]) ** 2 - ref[i]) / bound))
    print(f"nodes against the region method: worst err / bound {worst:.3f} with c_dist = {cd:.2f}")
    record("dfl_redistance_nodes", "well-shaped family against the region method", worst, c_dist=cd, nodes=len(P))
    assert worst <= 1.0


# ======================================================================================================================
# the two-stage reductions
# ======================================================================================================================
NODE_SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 2 ** 21 - 1, 2 ** 21 + 2049]


@pytest.mark.parametrize("N", NODE_SIZES)
def test_node_stats_and_node_sum(N, api, pool):
    """exact integers (any order gives these bits) and random values (the tree model's order); chg holds -1, 0, positives and a
    NaN, which is not counted; work is plain scratch preloaded with the sentinel"""
    L = api.lib()
    rng = np.random.default_rng(N % 9973)
    gN = M.node_grid(N)
    for kind in ("integers", "random"):
        q = rng.integers(-8, 9, N).astype(F64) if kind == "integers" else rng.normal(size=N) * 10.0 ** rng.integers(-3, 4, N)
        chg = np.abs(q)
        chg[rng.integers(0, N, max(N // 5, 1))] = -1.0
        chg[rng.integers(0, N, max(N // 7, 1))] = 0.0
        chg[N // 2] = np.nan
        qs, cs = pool.slot(q), pool.slot(chg)
        for fn, src, nv, (part, out) in ((L.dfl_volume_node_sum, qs, 1, M.node_sum(q)), (L.dfl_redistance_node_stats, cs, 2, M.node_stats(chg))):
            what = "%s N=%d %s" % ("node_sum" if nv == 1 else "node_stats", N, kind)
            work, res = pool.slot(sent(nv * M.MAX_PART)), pool.slot(sent(nv))
            fn(N, src.ptr, work.ptr, res.ptr, None)
            api.sync()
            got = exact(res, out, what)
            written = np.arange(nv * M.MAX_PART) < nv * gN
            assert_bits(work.check(what + " work", written)[:nv * gN], np.ravel(part), what + " partials")
            untouched(what, src)
            if kind == "integers":
                with np.errstate(invalid="ignore"):
                    ok = chg >= 0
                assert got[0] == (q.sum() if nv == 1 else ok.sum()) and (nv == 1 or got[1] == (chg[ok].max() if ok.any() else 0.0))
        pool.free()
    record("dfl_redistance_node_stats", "N=%d" % N, 0.0, exact=True, partials=gN)
    record("dfl_volume_node_sum", "N=%d" % N, 0.0, exact=True, partials=gN)


@pytest.mark.parametrize("npart", [1, 2, 255, 256, 257, 1000])
def test_reduce(npart, api, pool):
    L = api.lib()
    rng = np.random.default_rng(npart)
    for kind in ("integers", "random", "nan"):
        part = np.stack([rng.integers(-99, 100, npart), rng.integers(0, 1000, npart)], axis=1).astype(F64)
        if kind != "integers":
            part = np.stack([rng.normal(size=npart) * 10.0 ** rng.integers(-4, 5, npart), np.abs(rng.normal(size=npart))], axis=1)
        if kind == "nan":
            part[npart // 2, 1] = np.nan
            part[0, 1] = np.nan
        want = M.block_reduce(part, M.merge_pair)
        ps, out = pool.slot(part), pool.slot(sent(2))
        L.dfl_redistance_reduce(npart, ps.ptr, out.ptr, None)
        api.sync()
        got = exact(out, want, "reduce npart=%d %s" % (npart, kind))
        untouched("reduce", ps)
        if kind == "integers":
            assert got[0] == part[:, 0].sum() and got[1] == part[:, 1].max()
        if kind == "nan":
            assert got[1] == (np.nanmax(part[:, 1]) if npart > 2 else 0.0)
        pool.free()
    record("dfl_redistance_reduce", "npart=%d" % npart, 0.0, exact=True)


# ======================================================================================================================
# dfl_volume_classify, dfl_volume_emit
# ======================================================================================================================
def shift_of(name):
    return {"dyadic": M.DYADIC_SHIFT, "swapped-cube": 0.3}.get(name, M.ORBIT_SHIFT)


def run_classify(api, pool, b, d, ms, ref, what):
    L = api.lib()
    part, blk, out = pool.slot(sent(5 * b.nblk)), pool.slot(sent(b.nblk, I32), 0, I32), pool.slot(sent(5))
    L.dfl_volume_classify(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, d.level - ms, d.level + ms, blk.ptr, part.ptr, out.ptr, None)
    api.sync()
    got = exact(part, ref["part"], what + " part")
    exact(out, ref["out"], what + " out5")
    exact(blk, ref["blk_count"], what + " blk_count", I32)
    b.const(what)
    return got.reshape(-1, 5), blk


@pytest.mark.parametrize("name,nt", DECKS)
def test_classify_and_emit(name, nt, api, pool):
    """out5 and part [b][5] entry by entry (E), blk_count (A); then dfl_volume_emit on the counts classify just wrote: the
    ascending band list against the model, also with cap short by 1 and 5"""
    L, d = api.lib(), deck(name, nt)
    ms = shift_of(name)
    ref = cached(("classify", name, nt), lambda: M.classify(d.xg, d.ien, d.phi, d.level, ms))
    what = "classify %s/%s" % (name, nt)
    b = Bufs(pool, d)
    _, blk = run_classify(api, pool, b, d, ms, ref, what)
    band = np.flatnonzero(ref["band"])
    nb = len(band)
    if name == "dyadic":
        kind = np.array(d.info["kind"])
        for k in ("all == hi", "three == hi", "first == hi"):                                               # == hi is band
            assert ref["band"][kind == k].all() and not ref["inside"][kind == k].any()
        assert (ref["vals"][kind == "max == lo"][:, :4] == 0).all()                                         # == lo adds nothing
    if name == "on-level" and nt is None:
        nan = np.isnan(d.phi[d.ien]).any(axis=1)
        assert nan.sum() == 16 and (ref["vals"][nan][:, :4] == 0).all() and ref["band"][nan].any()
    # the scan of the device's counts, as the host does it
    base, chunk = pool.slot(sent(b.nblk + 1, I32), 0, I32), pool.slot(sent(L.dfl_scan_num_chunks(b.nblk), I32), 0, I32)
    L.dfl_scan_counts(b.nblk, blk.ptr, chunk.ptr, base.ptr, None)
    api.sync()
    exact(base, M.exclusive_scan(ref["blk_count"]), what + " blk_base", I32)
    settle(base)
    for short in (0, 1, 5):
        cap = nb - short
        if cap <= 0:
            continue
        lst = pool.slot(sent(cap, I32), 0, I32)
        L.dfl_volume_emit(d.NT, b.ien.ptr, b.w.ptr, d.N, d.level - ms, d.level + ms, base.ptr, lst.ptr, cap, None)
        api.sync()
        exact(lst, band[:cap], what + " list, cap short by %d" % short, I32)
        untouched(what, base)
        b.const(what + " emit")
    record("dfl_volume_classify", "%s/%s" % (name, nt or d.NT), 0.0, exact=True, band_tets=nb, inside=int(ref["inside"].sum()))
    record("dfl_volume_emit", "%s/%s" % (name, nt or d.NT), 0.0, exact=True, band_tets=nb)


@needs_ld
def test_classify_isolation(api, pool):
    """one live tet per workgroup: part[b][0 .. 3] are that tet's V_in and its band volumes at level, lo and hi, bit for bit (E)
    and each band volume within 4 c_vol u V K of the closed form (B); part[b][4] is the tree sum of the 256 tet volumes"""
    d = deck("isolation")
    live = d.info["live"]
    ms = M.ORBIT_SHIFT
    ref = cached(("classify", "isolation", None), lambda: M.classify(d.xg, d.ien, d.phi, d.level, ms))
    assert ref["band"].sum() + ref["inside"].sum() <= len(live) and ref["inside"].any() and ref["band"].sum() > 300
    b = Bufs(pool, d)
    got, _ = run_classify(api, pool, b, d, ms, ref, "classify isolation")
    assert_bits(got[:, :4], ref["vals"][live][:, :4], "the live tets' own values")
    cv = M.c_vol()[0]
    sel = ref["band"][live]
    worst = 0.0
    for j, c in enumerate((d.level, d.level - ms, d.level + ms)):
        want, V, K = M.closed_form_volume(d.xg, d.ien[live][sel], d.phi, c)
        err = np.abs(got[sel, 1 + j].astype(LD) - want)
        assert (err[K == 0] == 0).all()
        worst = max(worst, float((err[K > 0] / (4.0 * cv * LD(U) * V[K > 0] * K[K > 0])).max()))
    print(f"classify isolation: worst err / bound {worst:.3f} with c_vol = {cv:.2f}")
    record("dfl_volume_classify", "isolation, per tet against the closed form", worst, c_vol=cv, tets=int(sel.sum()))
    assert worst <= 1.0


# ======================================================================================================================
# dfl_volume_eval
# ======================================================================================================================
def run_eval(api, pool, b, d, lst, cand, what):
    L = api.lib()
    nband = len(lst)
    nblk = -(-nband // M.BLK)
    vals, part_w, out_w = M.evaluate(d.xg, d.ien, d.phi, lst, cand)
    ls, part, out = pool.ints(lst), pool.slot(sent(M.K * nblk)), pool.slot(sent(M.K))
    L.dfl_volume_eval(nband, ls.ptr, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, (f64 * M.K)(*cand), part.ptr, out.ptr, None)
    api.sync()
    got = exact(part, part_w, what + " part")
    exact(out, out_w, what + " outK")
    untouched(what, ls)
    b.const(what)
    return got.reshape(-1, M.K), vals


def candidates_for(d):
    """15 candidates: below every phi (the full volume), above every phi (zero), three equal to a node's phi exactly, two equal
    to each other, and the rest descending through the level"""
    ph = d.phi[~np.isnan(d.phi)]
    some = np.sort(ph[d.ien[~np.isnan(d.phi[d.ien]).any(axis=1)][::7].ravel()])
    c = [ph.min() - 1.0, ph.max() + 1.0, some[0], some[len(some) // 2], some[-1], d.level, d.level]
    c += list(d.level + np.linspace(0.4, -0.4, M.K - len(c)))
    assert len(c) == M.K
    return np.array(c, F64)


@pytest.mark.parametrize("name", ["orbit", "orbit-shared", "swapped-cube", "on-level", "dyadic"])
def test_eval(name, api, pool):
    """all 15 outputs and part [b][15] bit for bit (E) at nband 1, 255, 256, 257 and the whole band; a list that is not ascending
    and one that repeats a tet"""
    d = deck(name)
    ms = shift_of(name)
    ref = cached(("classify", name, None), lambda: M.classify(d.xg, d.ien, d.phi, d.level, ms))
    band = np.flatnonzero(ref["band"])
    cand = candidates_for(d)
    b = Bufs(pool, d)
    assert len(band) >= (257 if name != "dyadic" else 129)
    for nb in [n for n in (1, 255, 256, 257) if n <= len(band)] + [len(band)]:
        got, vals = run_eval(api, pool, b, d, band[:nb], cand, "eval %s nband=%d" % (name, nb))
    full = rm.tet_volumes(d.xg, d.ien[band], d.phi, d.level)[1]
    nan = np.isnan(d.phi[d.ien[band]]).any(axis=1)
    assert np.array_equal(vals[~nan, 0], full[~nan]) and (vals[:, 1] == 0).all() and np.array_equal(vals[:, 5], vals[:, 6])
    rng = np.random.default_rng(4)
    run_eval(api, pool, b, d, rng.permutation(band)[:300], cand, "eval %s, not ascending" % name)
    run_eval(api, pool, b, d, np.r_[band[:120], band[:120][::-1], band[5], band[5]], cand[::-1].copy(), "eval %s, repeats" % name)
    record("dfl_volume_eval", name, 0.0, exact=True, band_tets=len(band))


@needs_ld
def test_eval_isolation(api, pool):
    """a list with one live tet per workgroup of 256 entries (the others name a tet below every candidate): part[b][k] is that
    tet's volume at candidate k, bit for bit (E) and within 4 c_vol u V K of the closed form (B)"""
    d = deck("isolation")
    live = d.info["live"][:96]
    lst = np.full(M.BLK * len(live), 2, I64)           # tet 2 is a dead one: no workgroup has its live tet at thread 2
    assert 2 not in d.info["live"] and (d.ien[2] < 4).all()
    pos = np.arange(len(live)) * M.BLK + np.array(M.POSITIONS)[np.arange(len(live)) % 7][::-1]
    lst[pos] = live
    cand = d.level + np.array(M.ORBIT_OFFSETS)         # (the levels c_vol was measured at)
    assert len(cand) == M.K and cand.min() > d.phi[:4].max()
    b = Bufs(pool, d)
    got, vals = run_eval(api, pool, b, d, lst, cand, "eval isolation")
    assert_bits(got, vals[pos], "the live tets' own volumes")
    cv = M.c_vol()[0]
    worst = 0.0
    for k, c in enumerate(cand):
        want, V, K = M.closed_form_volume(d.xg, d.ien[live], d.phi, c)
        err = np.abs(got[:, k].astype(LD) - want)
        assert (err[K == 0] == 0).all()
        if (K > 0).any():
            worst = max(worst, float((err[K > 0] / (4.0 * cv * LD(U) * V[K > 0] * K[K > 0])).max()))
    print(f"eval isolation: worst err / bound {worst:.3f} with c_vol = {cv:.2f}")
    record("dfl_volume_eval", "isolation, per tet and candidate against the closed form", worst, c_vol=cv, tets=len(live))
    assert worst <= 1.0


# ======================================================================================================================
# dfl_volume_shift
# ======================================================================================================================
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_shift(N, api, pool):
    """only slot 4 of w changes, phi = fl(old + delta) bit for bit; a NaN keeps its bits (an addition would quiet the
    signalling one); +-inf, -0.0 and delta = 0"""
    L = api.lib()
    rng = np.random.default_rng(N)
    nan = np.array([0xFFF4000000000001, 0x7FF8000000000123], np.uint64).view(F64)      # a signalling and a quiet one
    written = np.zeros(6 * N, bool)
    written[4 * N:5 * N] = True
    for delta in (0.1, -2.0 ** -60, 0.0, -0.0, 1e308):
        phi = rng.normal(size=N) * 10.0 ** rng.integers(-6, 7, N)
        special = np.r_[nan, np.inf, -np.inf, -0.0, 0.0, 1.7e308]
        idx = rng.permutation(N)[:len(special)]
        phi[idx] = special[:len(idx)]
        w = rng.uniform(-2.0, 2.0, 6 * N)
        w[4 * N:5 * N] = phi
        ws = pool.slot(w)
        L.dfl_volume_shift(N, ws.ptr, delta, None)
        api.sync()
        got = ws.check("shift N=%d delta=%r" % (N, delta), written)[4 * N:5 * N]
        assert_bits(got, M.shift(phi, delta), "shift N=%d delta=%r" % (N, delta))
        pool.free()
    record("dfl_volume_shift", "N=%d" % N, 0.0, exact=True)


# ======================================================================================================================
# the chain
# ======================================================================================================================
@pytest.mark.parametrize("name", ["orbit-shared", "swapped-cube"])
def test_chain(name, api, pool):
    """cut -> dfl_scan_counts (twice) -> emit -> nodes -> node_stats on device outputs alone; the end state against the model"""
    L, d = api.lib(), deck(name)
    band = 0.3
    lo, hi = d.xg.min(axis=0), d.xg.max(axis=0)
    g = M.make_grid(lo, 1.0 / band, tuple(int(np.floor(q / band)) + 1 for q in hi - lo))
    gs = cgrid(g)
    ref = cached(("cut", name, None), lambda: M.cut(d.xg, d.ien, d.phi, d.level))
    F = ref["facets"]
    count, start, sets = M.cell_lists(F, g)
    nf, ne = len(F), int(start[-1])
    b = Bufs(pool, d)
    part, blk, cc = pool.slot(sent(2 * b.nblk)), pool.slot(sent(b.nblk, I32), 0, I32), pool.ints(np.zeros(g.ncell + 1))
    base, cs = pool.slot(sent(b.nblk + 1, I32), 0, I32), pool.slot(sent(g.ncell + 1, I32), 0, I32)
    chunk = pool.slot(sent(max(L.dfl_scan_num_chunks(b.nblk), L.dfl_scan_num_chunks(g.ncell)), I32), 0, I32)
    fac, ent = pool.slot(sent(9 * nf)), pool.slot(sent(ne, I32), 0, I32)
    ncand, lst, chg = pool.ints([0]), pool.slot(sent(d.N, I32), 0, I32), pool.slot(sent(d.N))
    work, out = pool.slot(sent(2 * M.MAX_PART)), pool.slot(sent(2))
    L.dfl_redistance_cut(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(gs), blk.ptr, cc.ptr, part.ptr, None)
    L.dfl_scan_counts(g.ncell, cc.ptr, chunk.ptr, cs.ptr, None)
    L.dfl_scan_counts(b.nblk, blk.ptr, chunk.ptr, base.ptr, None)
    L.dfl_redistance_emit(d.NT, b.ien.ptr, b.xg.ptr, b.w.ptr, d.N, d.level, C.byref(gs), base.ptr, cs.ptr, cc.ptr, fac.ptr, nf, ent.ptr, ne,
                          None)
    L.dfl_redistance_nodes(d.N, b.xg.ptr, b.w.ptr, d.level, band, C.byref(gs), cs.ptr, ent.ptr, fac.ptr, nf, None, ncand.ptr, lst.ptr,
                           chg.ptr, None)
    L.dfl_redistance_node_stats(d.N, chg.ptr, work.ptr, out.ptr, None)
    api.sync()
    what = "chain " + name
    assert base.get()[-1] == nf and cs.get()[-1] == ne
    same_numbers(fac.check(what + " facets", ALL), F, what + " facets")
    check_entries(ent.check(what, ALL).astype(I64), start, count, sets, what)
    exact(cc, np.r_[count, 0], what + " cell_fill", I32)
    new, cg, listed = M.nodes(d.xg, d.phi, d.level, band, g, start, M.entries_from(sets, start), F, nf)
    N = d.N
    slot4 = np.zeros(6 * N, bool)
    slot4[4 * N:5 * N] = True
    assert_bits(b.w.check(what + " w", slot4)[4 * N:5 * N], new, what + " phi")
    exact(chg, cg, what + " chg")
    exact(ncand, [len(listed)], what + " ncand", I32)
    exact(out, M.node_stats(cg)[1], what + " out2")
    untouched(what, b.ien, b.xg)
    # the brute-force model of the whole operation (every node against every facet) agrees with the cell-list one
    brute = rm.distance(d.xg, F)
    with np.errstate(invalid="ignore"):
        near = brute < band
    assert np.array_equal(near, cg >= 0) and near.any()
    m = np.where(near, brute, band)
    assert_bits(new, d.level + np.where(d.phi - d.level > 0.0, m, -m), what + ": phi against every node x every facet")
    record("chain", name, 0.0, exact=True, facets=nf, band_nodes=int(near.sum()))
