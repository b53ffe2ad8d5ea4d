"""Every launcher of the particle-field exchange (csrc/k_couple.hip, k_heat.hip, k_capture.hip, k_surface_contact.hip) alone,
through ctypes with the structs passed by value, against the model of tests/exchange_kernel_model.py.

Tier A (bitwise): the integer outputs -- the sorted V2E lists, the neighbour table (every Kuhn cube, the non-conforming fan,
the strip), the counting sort by tet with T around the scan's chunk sizes, the capture flags, the contact counters and their
fold, the heat fill and gather -- and point location by a check that does not depend on the walk's path: a tet >= 0 must
contain the point in np.longdouble, a point outside every tet beyond the bound must give -1 and lambda 0; every start (seed
grid, the right tet, a far tet) and every thread order must give the same tet and the same lambda bits; on the strip the
walk cap is met from both sides; a coordinate that is not finite gives -1, lambda 0 and no lost count.
Tier E (exact): the three node-sum instantiations on dyadic data, the correctly rounded parts of the capture deposits and
sources, the solid-surface contact without friction and grad_max against the float64 restatement in the source's operation
order, the drag sub-step under a thread order against the plain one.
Tier B (rounded): ENTRY BY ENTRY against np.longdouble under 8 c u A: A = the entry's own abs-sum (the model's A_*), c = what
the float64 restatement of the same law shows against u A (test_exchange_kernel_model_cpu.py; never measured on a kernel), 8
for FMA contraction and operand order as in the sibling kernel tests.

Every array sits between guard bands (guarded_buffers.py); overwrite outputs are preloaded with the sentinel, accumulate
outputs with known non-zero values; after each launch the bands, every const input and every entry the call must not write
are compared bit for bit.  Index arrays are the model's or a device output verified earlier in the same test.  No case aims
at a fault: all indices are in range; values that are not finite appear only as particle coordinates of dfl_couple_locate.
err / bound goes to the file named by DFL_PARITY_OUT (profiles/exchange_kernel_parity.jsonl is such a run)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import capture_model as cm
import dem_model as D
import exchange_kernel_model as X
import surface_contact_model as scm
from guarded_buffers import ALL, I32, SENT, Pool, Recorder, assert_bits, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
record = Recorder("a")
needs_ld = pytest.mark.skipif(not X.HAVE_EXTENDED, reason=X.EXTENDED_REASON)
vp, f64, i32, i64 = C.c_void_p, C.c_double, C.c_int32, C.c_int64
V3 = C.POINTER(f64 * 3)


class Sizes(C.Structure):
    _fields_ = [("radius", vp), ("mass", vp), ("sorted_r", vp), ("rmax", f64)]


class FrictionLaw(C.Structure):
    _fields_ = [("mu", f64), ("kt", f64), ("gamma_t", f64), ("dt", f64), ("inertia", f64)]


class ContactHistory(C.Structure):
    _fields_ = [("old_row", vp), ("old_count", vp), ("new_row", vp), ("new_count", vp), ("overflow", vp)]


class Grid3(C.Structure):
    _fields_ = [("lo", f64 * 3), ("inv", f64 * 3), ("n", i32 * 3)]


NODE_ARGS = [i32, vp, vp, vp, vp, vp, vp, vp, f64, vp, vp]
SIG = {
    "dfl_scan_temp_bytes": (i64, [i32]),
    "dfl_couple_sort_v2e": (None, [i32, vp, vp, vp]),
    "dfl_couple_neighbours": (None, [i32, vp, vp, vp, vp, vp]),
    "dfl_couple_locate": (None, [i32, vp, vp, vp, vp, vp, vp, V3, V3, i32, vp, vp, vp, vp]),
    "dfl_couple_fluid_step": (None, [i32, vp, vp, vp, vp, vp, f64, f64, vp, vp, f64, f64, V3, f64, vp, vp, vp, vp, vp]),
    "dfl_couple_sort_by_tet": (None, [i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dfl_couple_node_load": (None, NODE_ARGS),
    "dfl_couple_node_scalar": (None, NODE_ARGS),
    "dfl_couple_node_deposit": (None, NODE_ARGS),
    "dfl_heat_gather": (None, [i32, vp, vp, vp, vp]),
    "dfl_heat_conduction": (None, [i32, vp, f64, Sizes, f64, i32, vp, vp, vp, f64, vp, vp]),
    "dfl_heat_conduction_grid": (None, [i32, vp, f64, Sizes, Grid3, vp, vp, vp, f64, vp, vp]),
    "dfl_heat_update": (None, [i32, vp, vp, vp, vp, i32, f64, f64, vp, vp, vp, f64, f64, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp]),
    "dfl_heat_fill": (None, [i32, i32, f64, vp, vp, vp, vp]),
    "dfl_capture_flag": (None, [i32, vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, vp, vp, f64, f64, f64, f64, f64, f64, vp, vp, vp, vp]),
    "dfl_capture_source": (None, [i32, vp, f64, vp, vp, vp, vp]),
    "dfl_surface_grad_max": (None, [i32, vp, vp, vp, vp]),
    "dfl_surface_contact": (None, [i32, vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, Sizes, f64, f64, FrictionLaw, f64, f64, f64, vp,
                                   ContactHistory, vp, C.c_int, vp, vp, vp]),
}


def _declare(L):
    for name, (res, args) in SIG.items():
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


def test_struct_sizes_and_every_launcher_is_declared():
    import os
    import re
    assert C.sizeof(Grid3) == 64 and C.sizeof(Sizes) == 32 and C.sizeof(FrictionLaw) == 40 and C.sizeof(ContactHistory) == 40
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dedflow_amd", "csrc")
    for f in ("k_couple.hip", "k_heat.hip", "k_capture.hip", "k_surface_contact.hip"):
        text = open(os.path.join(src, f)).read()
        names = re.findall(r"^void (dfl_\w+)\(", text[text.index('extern "C"'):], re.M)
        assert names and not [n for n in names if n not in SIG], f


def exact(slot, want, what, dtype=F64):
    """the whole array == want bit for bit, the bands as uploaded"""
    got = slot.check(what, ALL)
    assert_bits(got, np.ravel(want), what, dtype)
    return got


def untouched(what, *slots):
    for s in slots:
        if s is not None:
            s.check(what + ": an array the call must not write changed")


def ptr(s):
    return None if s is None else s.ptr


def same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


def judge(got, model, A, c, what, kernel, case, live=None):
    """entry by entry under 8 c u A; an entry with A == 0 must be exact"""
    got, model, A = np.asarray(got, F64), np.asarray(model, LD).reshape(np.shape(got)), np.asarray(A, LD)
    A = np.broadcast_to(A.reshape(A.shape + (1,) * (got.ndim - A.ndim)), got.shape)
    live = np.ones(got.shape, bool) if live is None else np.broadcast_to(np.reshape(live, np.shape(live) + (1,) * (got.ndim - np.ndim(live))), got.shape)
    assert np.all(np.isfinite(got[live])), what + ": not finite"
    err, b = np.abs(got.astype(LD) - model).astype(F64), X.bound(A, c)
    assert np.all(err[live & (b == 0)] == 0), what + ": an entry without terms is not exact"
    pos = live & (b > 0)
    ratio = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
    record(kernel, case, ratio, c=float(c))
    print("%s %s: err / bound = %.3g (c = %.3g)" % (kernel, case, ratio, c))
    assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)


def mesh_slots(pool, m):
    vrow, vcol = m.v2e()
    return Out(x=pool.slot(m.x), ien=pool.ints(m.ien), vrow=pool.ints(vrow), vcol=pool.ints(vcol))


class Out(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


MESHES = [("kuhn%d-%g" % (M, j), (lambda M=M, j=j: X.kuhn(M, j))) for M, j in X.CUBES] + [("fan", X.fan), ("strip", X.strip)]


# ======================================================================================================================
# Tier A: V2E sort, neighbours, sort by tet
# ======================================================================================================================
@pytest.mark.parametrize("name,make", MESHES, ids=[n for n, _ in MESHES])
def test_sort_v2e_and_neighbours(name, make, api, pool):
    """every scrambled list comes back ascending with the same entries, vrow untouched; then, on the verified lists, nbr ==
    the face-dictionary model: -1 on boundary faces, symmetric on the conforming meshes, the lowest id on the fan"""
    L = api.lib()
    m = make()
    vrow, vcol = m.v2e()
    s_row, s_col, s_ien = pool.ints(vrow), pool.ints(X.scramble(vrow, vcol)), pool.ints(m.ien)
    L.dfl_couple_sort_v2e(m.N, s_row.ptr, s_col.ptr, None)
    api.sync()
    exact(s_col, vcol, name + " vcol", I32)
    untouched(name, s_row)
    L.dfl_couple_sort_v2e(m.N, s_row.ptr, s_col.ptr, None)      # sorted input: unchanged
    api.sync()
    exact(s_col, vcol, name + " vcol, second call", I32)
    record("dfl_couple_sort_v2e", name, 0.0, exact=True)
    nbr = pool.slot(sent(4 * m.T, I32), 0, I32)
    L.dfl_couple_neighbours(m.T, s_ien.ptr, s_row.ptr, s_col.ptr, nbr.ptr, None)
    api.sync()
    got = exact(nbr, m.nbr(), name + " nbr", I32).reshape(-1, 4)
    s_col.image[:] = s_col.dev.numpy()
    untouched(name, s_ien, s_row, s_col)
    if name != "fan":
        t, k = np.nonzero(got >= 0)
        assert np.all((got[got[t, k]] == t[:, None]).sum(axis=1) == 1), name + ": not symmetric"
    record("dfl_couple_neighbours", name, 0.0, exact=True)


def test_sort_v2e_and_neighbours_empty(api, pool):
    L = api.lib()
    s = [pool.slot(sent(4, I32), 0, I32) for _ in range(4)]
    L.dfl_couple_sort_v2e(0, s[0].ptr, s[1].ptr, None)
    L.dfl_couple_neighbours(0, s[0].ptr, s[1].ptr, s[2].ptr, s[3].ptr, None)
    api.sync()
    untouched("N = 0, T = 0", *s)


SORT_T = [1, 255, 257, 1023, 1024, 1025, 4095, 4096, 4097, 9000]


@pytest.mark.parametrize("T", SORT_T)
def test_sort_by_tet(T, api, pool):
    """tstart == the exclusive scan; members ascending by id inside every tet; tcount zero again; the unlocated (-1, -2)
    absent; entries beyond the located count, and tcount[T], untouched; a second call on the same scratch: the same bits"""
    L = api.lib()
    nbytes = L.dfl_scan_temp_bytes(T)
    for P, family in itertools.product((0, 1, 255, 256, 257, 513), ("random", "one_tet", "none")):
        rng = np.random.default_rng(1000 * T + P)
        tet = rng.integers(0, T, P)
        tet[rng.uniform(size=P) < 0.25] = -1
        tet[rng.uniform(size=P) < 0.1] = -2
        if family == "one_tet":
            tet = np.where(tet >= 0, T - 1, tet)
        elif family == "none":
            tet = np.where(np.arange(P) % 2, -1, -2)
        start, members = X.sort_by_tet(tet, T)
        n, nloc = max(P, 1), len(members)
        s_tet, tcount = pool.ints(tet if P else [0]), pool.ints(np.r_[np.zeros(T), 77])
        rank, slot, mem = (pool.slot(sent(n, I32), 0, I32) for _ in range(3))
        tstart = pool.slot(sent(T + 1, I32), 0, I32)
        temp = pool.slot(np.full(nbytes, 0xA5, np.uint8), 0, np.uint8)
        what = "sort_by_tet T=%d P=%d %s" % (T, P, family)
        got = []
        for call in range(2):
            L.dfl_couple_sort_by_tet(P, T, s_tet.ptr, tcount.ptr, rank.ptr, tstart.ptr, slot.ptr, mem.ptr, temp.ptr, nbytes, None)
            api.sync()
            exact(tstart, start, what + " tstart", I32)
            written = np.arange(n) < nloc
            g = mem.check(what + " members beyond the located", written)
            assert np.array_equal(g[:nloc], members), what + ": members"
            sl = slot.check(what + " slot beyond the located", written)[:nloc].astype(I64)
            assert np.array_equal(np.sort(sl), np.sort(members)) and np.array_equal(tet[sl], np.sort(tet[tet >= 0])), what + ": slot"
            untouched(what, s_tet, tcount)                    # tcount: zero again, tcount[T] never written
            rk = rank.check(what + " rank", np.arange(n) < P)[:P]
            assert np.all(rk[tet < 0] == -1)
            for t in np.unique(tet[tet >= 0])[:50]:
                assert sorted(rk[tet == t].tolist()) == list(range(int((tet == t).sum()))), what + ": rank"
            temp.check(what + " scan_temp", ALL)
            got.append((tstart.get().copy(), g[:nloc].copy()))
        same_bits(got[0][0], got[1][0], what)
        same_bits(got[0][1], got[1][1], what)
        pool.free()
    record("dfl_couple_sort_by_tet", "T%d" % T, 0.0, exact=True)


# ======================================================================================================================
# point location
# ======================================================================================================================
class Locate:
    """the guarded arrays of dfl_couple_locate on one mesh and one seed grid"""

    def __init__(self, pool, L, api, m, seed, lo, inv_h, gdim):
        self.pool, self.L, self.api, self.m = pool, L, api, m
        self.x, self.ien, self.nbr, self.seed = pool.slot(m.x), pool.ints(m.ien), pool.ints(m.nbr()), pool.ints(seed)
        self.lo, self.inv, self.gdim = (f64 * 3)(*lo), (f64 * 3)(*inv_h), gdim

    def run(self, pts, tet, order=None, lost0=7, what="locate"):
        P = len(pts)
        coord, s_tet, lam, lost = self.pool.slot(pts), self.pool.ints(tet), self.pool.slot(sent(4 * P)), self.pool.ints([lost0])
        s_ord = None if order is None else self.pool.ints(order)
        self.L.dfl_couple_locate(P, ptr(s_ord), coord.ptr, self.x.ptr, self.ien.ptr, self.nbr.ptr, self.seed.ptr, C.byref(self.lo),
                                 C.byref(self.inv), self.gdim, s_tet.ptr, lam.ptr, lost.ptr, None)
        self.api.sync()
        untouched(what, coord, self.x, self.ien, self.nbr, self.seed, s_ord)
        out = (s_tet.check(what + " tet", ALL).astype(I64), lam.check(what + " lambda", ALL).reshape(-1, 4).copy(),
               int(lost.check(what + " lost", ALL)[0]))
        for s in (coord, s_tet, lam, lost) + (() if s_ord is None else (s_ord,)):
            s.dev.free()
            self.pool.slots.remove(s)
        return out


def contained(m, pts, tet, lam, c, what, kernel, case, on_faces=False):
    """the check that does not follow the walk: a tet >= 0 contains the point in longdouble down to the bound, and its
    lambda is the longdouble one within the bound; -1 only where no tet contains the point beyond doubt; lambda 0 with it"""
    ok = tet >= 0
    ref, A = X.barycentric(m.x[m.ien[tet[ok]]], pts[ok], LD)
    b = X.bound(A, c)
    assert np.all(ref >= -X.LAMBDA_EPS - b), what + ": a tet does not contain its point"
    judge(lam[ok], ref, A, c, what, kernel, case)
    assert np.all(lam[~ok] == 0) and not np.signbit(lam[~ok]).any(), what + ": lambda of an unlocated particle"
    out = tet == -1
    if out.any():
        la, Aa = X.min_lambda_all(m, pts[out])
        sure = (la > -X.LAMBDA_EPS + X.bound(Aa, c)).all(axis=2).any(axis=1)
        assert not sure.any(), what + ": a point inside a tet was reported outside"


LOCATE_P = (1, 255, 256, 257, 513)


@needs_ld
@pytest.mark.parametrize("M,jitter", X.CUBES)
def test_locate_on_cubes(M, jitter, api, pool):
    """the families (interior, clear of every face by 1e-6, on shared faces / edges / vertices, outside each side, one tet)
    from the seed grid, from the right tet and from a far tet, plain and under a thread order: contained, and the same tet
    and lambda bits from every start wherever the containing tet is unique; no launch touches *lost; then P around the
    workgroup size and a launch that locates nobody"""
    L, m = api.lib(), X.kuhn(M, jitter)
    c = X.c_lambda()
    seed, lo, inv_h = X.seed_grid(m, 2)
    loc = Locate(pool, L, api, m, seed, lo, inv_h, 2)
    pts, unique, clear_t = X.locate_points(m)
    lam_clear = X.barycentric(m.x[m.ien[clear_t]], pts[150:300], LD)[0]
    assert lam_clear.min() >= 1e-6, "a point of the clear family is closer than 1e-6 of the tet to a face"
    P = len(pts)
    assert P == 513
    name = m.name
    tet0, lam0, lost = loc.run(pts, np.full(P, -1), what=name + " from the seed grid")
    assert lost == 7 and np.all(tet0 >= -1)
    contained(m, pts, tet0, lam0, c, name, "dfl_couple_locate", name + "-seed")
    assert np.array_equal(tet0[150:300], clear_t) and np.all(tet0[400:460] == -1) and np.all(tet0[460:] == m.T // 2)
    order = np.random.default_rng(9).permutation(P)
    starts = [("right", np.where(tet0 >= 0, tet0, -1)), ("far", np.full(P, m.T - 1)), ("tet0", np.zeros(P, I64))]
    for sname, start in starts:
        for od in (None, order):
            what = "%s from %s%s" % (name, sname, "" if od is None else " ordered")
            t, l, lost = loc.run(pts, start, od, what=what)
            assert lost == 7 and np.all(t >= -1)
            contained(m, pts, t, l, c, what, "dfl_couple_locate", "%s-%s%s" % (name, sname, "" if od is None else "-order"))
            assert np.array_equal(t[unique], tet0[unique]), what + ": another tet"
            same_bits(l[unique], lam0[unique], what + ": other lambda bits")
    t, l, lost = loc.run(pts, np.full(P, -1), order, what=name + " seed ordered")
    assert np.array_equal(t, tet0) and lost == 7
    same_bits(l, lam0, name + ": the thread order changed the result")
    for Pn in LOCATE_P[:-1]:
        sel = np.random.default_rng(Pn).permutation(P)[:Pn]
        t, l, lost = loc.run(pts[sel], np.full(Pn, -1), what="%s P=%d" % (name, Pn))
        assert lost == 7 and np.array_equal(t[unique[sel]], tet0[sel][unique[sel]])
        same_bits(l[unique[sel]], lam0[sel][unique[sel]], "%s P=%d" % (name, Pn))
    t, l, lost = loc.run(pts[400:460], np.full(60, -1), what=name + " nobody located")
    assert np.all(t == -1) and np.all(l == 0) and lost == 7


@needs_ld
def test_locate_walk_cap_on_the_strip(api, pool):
    """one seed cell holding tet 0: a particle whose tet lies >= 4096 face crossings away comes back -2 with lambda 0 and
    *lost rises by exactly their number from its preload; one that the model's walk reaches in <= 4096 - 64 steps is found;
    in between: a containing tet or -2, and *lost counts the -2"""
    L, m = api.lib(), X.strip()
    pts, tet, must_find, must_lose = X.strip_particles()
    assert must_find.sum() >= 50 and must_lose.sum() >= 50
    loc = Locate(pool, L, api, m, [0], (0.0, 0.0, 0.0), (1.0 / X.STRIP_CUBES, 1.0, 1.0), 1)
    for od in (None, np.random.default_rng(3).permutation(len(pts))):
        t, l, lost = loc.run(pts, np.full(len(pts), -1), od, lost0=1000, what="strip")
        assert np.all((t == tet) | (t == -2)), "neither the containing tet nor -2"
        assert np.array_equal(t[must_find], tet[must_find]), "a particle within the cap was not found"
        assert np.all(t[must_lose] == -2), "a particle beyond the cap was found"
        assert lost == 1000 + int((t == -2).sum())
        assert np.all(l[t == -2] == 0)
        contained(m, pts, t, l, X.c_lambda(), "strip", "dfl_couple_locate", "strip-cap" + ("" if od is None else "-order"))
    # from its own tet every particle is found at once, wherever it is
    t, l, lost = loc.run(pts, tet, what="strip from the right tet", lost0=1000)
    assert np.array_equal(t, tet) and lost == 1000


NONFINITE = [(np.inf, 0), (-np.inf, 1), (np.nan, 2), (np.inf, 2), (np.nan, 0), (-np.inf, 0)]


@needs_ld
@pytest.mark.parametrize("M,jitter", [(2, 0.0), (3, 0.0), (3, 0.2)])
def test_locate_refuses_a_coordinate_that_is_not_finite(M, jitter, api, pool):
    """+-inf and NaN in one coordinate and in two, from tet = -1 and from a tet >= 0: tet -1, lambda 0, *lost unchanged; the
    finite particles of the same launch get, bit for bit, what they get in a launch where those particles are finite"""
    L, m = api.lib(), X.kuhn(M, jitter)
    seed, lo, inv_h = X.seed_grid(m, 2)
    loc = Locate(pool, L, api, m, seed, lo, inv_h, 2)
    pts, _ = X.interior_points(m, 300, 31, clear=1e-3)
    bad = np.arange(300) % 7 == 3
    poisoned = pts.copy()
    for n, i in enumerate(np.flatnonzero(bad)):
        v, d = NONFINITE[n % len(NONFINITE)]
        poisoned[i, d] = v
        if n % 3 == 2:                                        # two coordinates
            poisoned[i, (d + 1) % 3] = NONFINITE[(n + 1) % len(NONFINITE)][0]
    assert np.isinf(poisoned).any() and np.isnan(poisoned).any() and (~np.isfinite(poisoned)).sum(axis=1).max() == 2
    ref_t, ref_l, _ = loc.run(pts, np.full(300, -1), what="finite")
    assert np.all(ref_t >= 0)
    for sname, start in (("seed", np.full(300, -1)), ("own", ref_t), ("tet0", np.zeros(300, I64))):
        t, l, lost = loc.run(poisoned, start, lost0=7, what="not finite from " + sname)
        assert np.all(t[bad] == -1), "a particle with a coordinate that is not finite was located or lost: %s" % t[bad]
        assert np.all(l[bad] == 0) and not np.signbit(l[bad]).any() and lost == 7
        assert np.array_equal(t[~bad], ref_t[~bad])
        same_bits(l[~bad], ref_l[~bad], "the finite particles changed")
    record("dfl_couple_locate", "%s-not-finite" % m.name, 0.0, exact=True)


def test_empty_launches_touch_nothing(api, pool):
    """P, N or T = 0: every launcher that may return at once does, whatever its pointers"""
    L = api.lib()
    guard = pool.slot(sent(8))
    z3 = (f64 * 3)(0.0, 0.0, 0.0)
    L.dfl_couple_locate(0, None, None, None, None, None, None, C.byref(z3), C.byref(z3), 1, None, None, None, None)
    for fn in NODE_FN.values():
        getattr(L, fn)(0, None, None, None, None, None, None, None, 1.0, None, None)
    L.dfl_heat_conduction(0, None, 0.1, Sizes(), 0.5, 2, None, None, None, 1.0, None, None)
    L.dfl_heat_conduction_grid(0, None, 0.1, Sizes(), Grid3(), None, None, None, 1.0, None, None)
    L.dfl_capture_source(0, None, 1.0, None, None, None, None)
    api.sync()
    untouched("empty launches", guard)


# ======================================================================================================================
# the node sums (Tier E)
# ======================================================================================================================
NODE_FN = {1: "dfl_couple_node_scalar", 3: "dfl_couple_node_load", 5: "dfl_couple_node_deposit"}


@pytest.mark.parametrize("P,family", [(1, "random"), (257, "random"), (513, "random"), (513, "one_tet"), (257, "none")])
def test_node_sums_exact_on_dyadic_data(P, family, api, pool):
    """lambda in eighths, small integer values, scale a power of two: every partial sum is exact, so the three
    instantiations == the model bit for bit and each other component by component; a node without a particle gets the
    zero that -scale * 0.0 gives"""
    L, m = api.lib(), X.kuhn(6, 0.2)
    assert m.N > 256
    tet, lam, val = X.dyadic_particles(m, P, 40 + P, one_tet=m.T // 3 if family == "one_tet" else None,
                                       located=0.0 if family == "none" else 0.8)
    start, members = X.sort_by_tet(tet, m.T)
    ms = mesh_slots(pool, m)
    s_start, s_mem, s_lam = pool.ints(start), pool.ints(np.r_[members, np.full(P - len(members), 0x5A5A5A5A)]), pool.slot(lam)
    got = {}
    for C_, scale in ((1, 0.5), (3, 4.0), (5, 1.0), (1, 1.0), (3, 1.0)):
        v = pool.slot(val[:, :C_])
        out = pool.slot(sent(C_ * m.N))
        getattr(L, NODE_FN[C_])(m.N, ms.vrow.ptr, ms.vcol.ptr, ms.ien.ptr, s_start.ptr, s_mem.ptr, s_lam.ptr, v.ptr, scale, out.ptr, None)
        api.sync()
        what = "%s P=%d %s scale=%g" % (NODE_FN[C_], P, family, scale)
        want = X.node_sum(m, start, members, lam, val[:, :C_], scale, C_)
        got[(C_, scale)] = exact(out, want, what).reshape(-1, C_).copy()
        untouched(what, ms.vrow, ms.vcol, ms.ien, s_start, s_mem, s_lam, v)
        touched = np.zeros(m.N, bool)
        touched[m.ien[tet[tet >= 0]].ravel()] = True
        z = got[(C_, scale)][~touched]
        assert np.all(z == 0) and np.all(np.signbit(z)), what + ": a node without a particle"
    same_bits(got[(1, 1.0)][:, 0], got[(3, 1.0)][:, 0], "scalar against load")
    same_bits(got[(3, 1.0)], got[(5, 1.0)][:, :3], "load against deposit")
    for C_ in (1, 3, 5):
        record(NODE_FN[C_], "P%d-%s" % (P, family), 0.0, exact=True)


# ======================================================================================================================
# the drag sub-step (Tier B, and Tier E under a thread order)
# ======================================================================================================================
@needs_ld
@pytest.mark.parametrize("name", X.FLUID_CASES)
def test_fluid_step(name, api, pool):
    """one size, per-particle sizes, and per-particle sizes all equal (within the one-size bound of the one-size model);
    lambda of a particle with tet < 0 is the sentinel: not read, and its imp is not written; a thread order changes no bit"""
    L = api.lib()
    k = X.fluid_case(name)
    c = X.c_fluid()
    m, P = k.mesh, k.P
    lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
    s_tet, s_lam, s_ien, s_w = pool.ints(k.tet), pool.slot(lam), pool.ints(m.ien), pool.slot(k.w)
    s_m, s_r, s_M, s_R = pool.slot(k.m), pool.slot(k.r), pool.slot(np.full(P, k.M)), pool.slot(np.full(P, k.R))
    order = pool.ints(np.random.default_rng(2).permutation(P))
    g = (f64 * 3)(*k.g)
    inside = k.tet >= 0
    for variant, mi, ri in (("one", None, None), ("sizes", s_m, s_r), ("equal", s_M, s_R)):
        model = X.fluid_run(k, LD, variant == "sizes")
        bits = []
        for od in (None, order):
            st = [pool.slot(q) for q in (k.coord, k.vel, k.acc, k.imp)]
            L.dfl_couple_fluid_step(P, ptr(od), s_tet.ptr, s_lam.ptr, s_ien.ptr, s_w.ptr, k.M if mi is None else np.nan,
                                    k.R if mi is None else np.nan, ptr(mi), ptr(ri), k.rho_f, k.mu_f, C.byref(g), k.dt,
                                    st[0].ptr, st[1].ptr, st[2].ptr, st[3].ptr, None)
            api.sync()
            what = "fluid_step %s %s%s" % (name, variant, "" if od is None else " ordered")
            untouched(what, s_tet, s_lam, s_ien, s_w, s_m, s_r, s_M, s_R, order)
            coord, vel, acc = (s.check(what, ALL).reshape(-1, 3).copy() for s in st[:3])
            imp = st[3].check(what + " imp of a particle outside", np.repeat(inside, 3)).reshape(-1, 3).copy()
            bits.append((coord, vel, acc, imp))
            if od is None:
                kern = "dfl_couple_fluid_step" + ("" if variant == "one" else "<%s>" % variant)
                judge(vel, model.vel, model.A_vel, c[0], what + " vel", kern + ":vel", name)
                judge(coord, model.coord, model.A_coord, c[1], what + " coord", kern + ":coord", name)
                judge(acc, model.acc, model.A_acc, c[2], what + " acc", kern + ":acc", name)
                judge(imp, model.imp, model.A_imp, c[3], what + " imp", kern + ":imp", name, live=inside)
            for s in st:
                s.dev.free()
                pool.slots.remove(s)
        for a, b in zip(*bits):
            same_bits(a, b, "fluid_step %s %s: the thread order changed the result" % (name, variant))


@needs_ld
@pytest.mark.parametrize("Pn", [0, 1, 255, 256, 257])
def test_fluid_step_particle_counts(Pn, api, pool):
    """P around the workgroup size on the arrays of the "low" family: the first P particles within the bound, everything
    behind them untouched; P = 0 launches nothing"""
    L = api.lib()
    k = X.fluid_case("low")
    c = X.c_fluid()
    lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
    s_tet, s_lam, s_ien, s_w, s_m, s_r = pool.ints(k.tet), pool.slot(lam), pool.ints(k.mesh.ien), pool.slot(k.w), pool.slot(k.m), pool.slot(k.r)
    g = (f64 * 3)(*k.g)
    first = np.arange(k.P) < Pn
    for poly in (False, True):
        model = X.fluid_run(k, LD, poly)
        st = [pool.slot(q) for q in (k.coord, k.vel, k.acc, k.imp)]
        L.dfl_couple_fluid_step(Pn, None, s_tet.ptr, s_lam.ptr, s_ien.ptr, s_w.ptr, np.nan if poly else k.M, np.nan if poly else k.R,
                                ptr(s_m if poly else None), ptr(s_r if poly else None), k.rho_f, k.mu_f, C.byref(g), k.dt,
                                st[0].ptr, st[1].ptr, st[2].ptr, st[3].ptr, None)
        api.sync()
        what = "fluid_step P=%d poly=%s" % (Pn, poly)
        untouched(what, s_tet, s_lam, s_ien, s_w, s_m, s_r)
        coord, vel, acc = (q.check(what + " beyond P", np.repeat(first, 3)).reshape(-1, 3)[:Pn] for q in st[:3])
        imp = st[3].check(what + " imp beyond P or outside", np.repeat(first & (k.tet >= 0), 3)).reshape(-1, 3)[:Pn]
        kern = "dfl_couple_fluid_step" + ("<sizes>" if poly else "")
        for j, (name, got) in enumerate((("vel", vel), ("coord", coord), ("acc", acc), ("imp", imp))):
            judge(got, model[name][:Pn], model["A_" + name][:Pn], c[j], what + " " + name, kern + ":" + name, "low-P%d" % Pn,
                  live=(k.tet[:Pn] >= 0) if name == "imp" else None)


# ======================================================================================================================
# heat
# ======================================================================================================================
@pytest.mark.parametrize("first,count", [(0, 1), (3, 255), (5, 256), (1, 257), (7, 513), (4, 0)])
def test_heat_fill(first, count, api, pool):
    L = api.lib()
    n = first + count + 9
    rng = np.random.default_rng(count)
    s = [pool.slot(rng.normal(size=n)) for _ in range(3)]
    L.dfl_heat_fill(first, count, 1234.5, s[0].ptr, s[1].ptr, s[2].ptr, None)
    api.sync()
    inside = (np.arange(n) >= first) & (np.arange(n) < first + count)
    for q, v in zip(s, (1234.5, 0.0, 0.0)):
        got = q.check("heat_fill outside [first, first + count)", inside)
        assert_bits(got[inside], np.full(count, v), "heat_fill")
    record("dfl_heat_fill", "first%d-count%d" % (first, count), 0.0, exact=True)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 513])
def test_heat_gather(P, api, pool):
    L = api.lib()
    rng = np.random.default_rng(P)
    temp, order = rng.uniform(300, 3000, P), rng.permutation(P)
    s_t, s_o, out = pool.slot(temp), pool.ints(order), pool.slot(sent(P))
    L.dfl_heat_gather(P, s_o.ptr, s_t.ptr, out.ptr, None)
    api.sync()
    exact(out, temp[order], "heat_gather")
    untouched("heat_gather", s_t, s_o)
    L.dfl_heat_gather(0, s_o.ptr, s_t.ptr, out.ptr, None)
    api.sync()
    exact(out, temp[order], "heat_gather P = 0")
    record("dfl_heat_gather", "P%d" % P, 0.0, exact=True)


@needs_ld
@pytest.mark.parametrize("poly,laser", [(False, False), (True, False), (False, True), (True, True)])
def test_heat_update(poly, laser, api, pool):
    """the four template variants; q NULL; w NULL and tet NULL (uncoupled: e untouched); tet[i] < 0 (a fifth of the
    particles, their lambda the sentinel); dt = 0: the rate exactly 0 and temp unchanged"""
    L = api.lib()
    k = X.heat_case()
    c = X.c_heat()
    m, P, H = k.mesh, k.P, X.HEAT
    lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
    s_tet, s_lam, s_ien, s_w, s_vel = pool.ints(k.tet), pool.slot(lam), pool.ints(m.ien), pool.slot(k.w), pool.slot(k.vel)
    s_m, s_r, s_q, s_p = pool.slot(k.m), pool.slot(k.r), pool.slot(k.q), pool.slot(k.laser)
    kern = "dfl_heat_update<%d,%d>" % (poly, laser)
    cases = [("full", True, "both", None), ("q-null", False, "both", None), ("w-null", True, "w", None), ("tet-null", True, "tet", None),
             ("dt0", True, "both", 0.0)]
    for case, use_q, coupled, dt in cases:
        model = X.heat_run(k, LD, poly, laser, q=use_q, coupled=coupled == "both", dt=dt)
        temp, rate, e = pool.slot(k.temp), pool.slot(sent(P)), pool.slot(k.e0)
        L.dfl_heat_update(P, None if coupled == "w" else s_tet.ptr, s_lam.ptr, s_ien.ptr, None if coupled == "tet" else s_w.ptr, m.N,
                          np.nan if poly else k.M, np.nan if poly else k.R, ptr(s_m if poly else None), ptr(s_r if poly else None),
                          s_vel.ptr, H["cp_p"], H["k_f"], H["rho_f"], H["mu_f"], H["pr13"], k.dt if dt is None else dt,
                          ptr(s_q if use_q else None), ptr(s_p if laser else None), temp.ptr, rate.ptr, e.ptr, None)
        api.sync()
        what = "%s %s" % (kern, case)
        untouched(what, s_tet, s_lam, s_ien, s_w, s_vel, s_m, s_r, s_q, s_p)
        inside = (k.tet >= 0) & (coupled == "both")
        got_e = e.check(what + " e of a particle without fluid", inside)
        got_t, got_r = temp.check(what, ALL), rate.check(what, ALL)
        if dt == 0.0:
            assert_bits(got_t, k.temp, what + " temp")
            assert_bits(got_r, np.zeros(P), what + " rate")
            assert_bits(got_e, k.e0, what + " e")
            record(kern, case, 0.0, exact=True)
            continue
        judge(got_t, model.temp, model.A_temp, c[0], what + " temp", kern + ":temp", case)
        judge(got_r, model.rate, model.A_rate, c[1], what + " rate", kern + ":rate", case)
        judge(got_e, model.e, model.A_e, c[2], what + " e", kern + ":e", case, live=inside)


@needs_ld
@pytest.mark.parametrize("Pn", [0, 1, 255, 256, 257])
def test_heat_update_particle_counts(Pn, api, pool):
    L = api.lib()
    k = X.heat_case()
    c = X.c_heat()
    m, H = k.mesh, X.HEAT
    lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
    s_tet, s_lam, s_ien, s_w, s_vel, s_q = pool.ints(k.tet), pool.slot(lam), pool.ints(m.ien), pool.slot(k.w), pool.slot(k.vel), pool.slot(k.q)
    model = X.heat_run(k, LD, False, False)
    temp, rate, e = pool.slot(k.temp), pool.slot(sent(k.P)), pool.slot(k.e0)
    L.dfl_heat_update(Pn, s_tet.ptr, s_lam.ptr, s_ien.ptr, s_w.ptr, m.N, k.M, k.R, None, None, s_vel.ptr, H["cp_p"], H["k_f"], H["rho_f"],
                      H["mu_f"], H["pr13"], k.dt, s_q.ptr, None, temp.ptr, rate.ptr, e.ptr, None)
    api.sync()
    what = "heat_update P=%d" % Pn
    untouched(what, s_tet, s_lam, s_ien, s_w, s_vel, s_q)
    first = np.arange(k.P) < Pn
    got_t, got_r = temp.check(what + " beyond P", first)[:Pn], rate.check(what + " beyond P", first)[:Pn]
    got_e = e.check(what + " e beyond P or without fluid", first & (k.tet >= 0))[:Pn]
    judge(got_t, model.temp[:Pn], model.A_temp[:Pn], c[0], what + " temp", "dfl_heat_update<0,0>:temp", "P%d" % Pn)
    judge(got_r, model.rate[:Pn], model.A_rate[:Pn], c[1], what + " rate", "dfl_heat_update<0,0>:rate", "P%d" % Pn)
    judge(got_e, model.e[:Pn], model.A_e[:Pn], c[2], what + " e", "dfl_heat_update<0,0>:e", "P%d" % Pn, live=k.tet[:Pn] >= 0)


def _grid(g):
    return Grid3((f64 * 3)(*g.lo), (f64 * 3)(*g.inv), (i32 * 3)(*[int(k) for k in g.n]))


@needs_ld
@pytest.mark.parametrize("P", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("poly", [False, True])
def test_heat_conduction(poly, P, api, pool):
    """the unit-box launcher and the mesh-grid launcher on dem_model's cell sort: q particle by particle within the bound, a
    particle without contact exactly 0; the two partners of a contact get exactly opposite heat where each has that one
    contact; on the grid the slots from cell_start[nbin] on (a tenth of the particles, outside it) get exactly 0"""
    L = api.lib()
    import heat_model as hm
    k = X.conduction_case(poly, P)
    c = X.c_conduction()
    temp = pool.slot(k.T)

    def run(launch, cell_of, nbin, active, case):
        _, start, order = D.cell_order(cell_of, nbin)
        s, _, sr = D.sorted_copies(order, k.x, k.v, None, k.r)
        i, j, _ = hm.contacts_all_pairs(k.x, k.r)
        live = active[i] & active[j]
        pairs = (i[live], j[live])
        model, A, delta = X.conduction(LD, k.x, k.r, k.T, k.k_p, pairs)
        assert delta.size == 0 or delta.min() >= 1e-9 * k.R
        cnt = np.bincount(pairs[0], minlength=P)
        s_sorted, s_sr, s_order, s_start = pool.slot(s), pool.slot(sr), pool.ints(order), pool.ints(start)
        s_st, q = pool.slot(k.T[order]), pool.slot(sent(P))
        sz = Sizes(None, None, s_sr.ptr, k.rmax) if poly else Sizes(None, None, None, 0.0)
        launch(P, s_sorted.ptr, np.nan if poly else k.R, sz, s_order.ptr, s_start.ptr, s_st.ptr, k.k_p, q.ptr)
        api.sync()
        untouched(case, s_sorted, s_sr, s_order, s_start, s_st)
        got = q.check(case, ALL)
        kern = "dfl_heat_conduction" + ("_grid" if "grid" in case else "") + ("<sizes>" if poly else "")
        assert np.all(got[cnt == 0] == 0) and not np.signbit(got[cnt == 0]).any(), case + ": a particle without contact"
        judge(got, model, A, c, case, kern, "%s-P%d" % (case, P), live=cnt > 0)
        single = (cnt[pairs[0]] == 1) & (cnt[pairs[1]] == 1)
        assert single.sum() >= 20 or P < 255
        if not single.any():
            return got
        assert np.all(got[pairs[0][single]] + got[pairs[1][single]] == 0), case + ": the partners' heat is not exactly opposite"
        assert np.abs(got[pairs[0][single]]).min() > 0
        return got

    cell = 1.0 / k.ncell
    everyone = np.ones(P, bool)
    box = run(lambda P_, so, R, sz, od, st, tt, kp, q: L.dfl_heat_conduction(P_, so, R, sz, cell, k.ncell, od, st, tt, kp, q, None),
              D.box_bins(k.x, cell, k.ncell), k.ncell ** 3, everyone, "box")
    g = D.Grid3((0.0, 0.0, 0.0), (k.ncell,) * 3, (k.ncell,) * 3)
    grid = run(lambda P_, so, R, sz, od, st, tt, kp, q: L.dfl_heat_conduction_grid(P_, so, R, sz, _grid(g), od, st, tt, kp, q, None),
               D.grid_bins(k.x, g), g.ncell + 1, everyone, "grid")
    same_bits(box, grid, "the box and the same cells as a mesh grid differ")
    # a grid over x < 0.9 only: the particles beyond it sit in the extra bin and exchange no heat
    g2 = D.Grid3((0.0, 0.0, 0.0), (k.ncell,) * 3, (k.ncell - 1, k.ncell, k.ncell))
    cell_of = D.grid_bins(k.x, g2)
    active = cell_of < g2.ncell
    assert 10 <= (~active).sum() <= P // 4 or P == 1
    part = run(lambda P_, so, R, sz, od, st, tt, kp, q: L.dfl_heat_conduction_grid(P_, so, R, sz, _grid(g2), od, st, tt, kp, q, None),
               cell_of, g2.ncell + 1, active, "grid-with-outsiders")
    assert np.all(part[~active] == 0)
    untouched("conduction", temp)


# ======================================================================================================================
# melt-pool capture
# ======================================================================================================================
@needs_ld
@pytest.mark.parametrize("poly", [False, True])
def test_capture_flag(poly, api, pool):
    """keep and rtet == the float64 restatement in tet_levelset.hpp's order (every case clear of both thresholds by the
    model's margins); dep[0] and dep[4] are single correctly rounded operations on exact operands: bitwise; dep[1..3] hold
    the u_f sum, which may be contracted: within the bound; temp NULL: dep[4] = 0; P around the workgroup size"""
    L = api.lib()
    k = X.capture_case(poly)
    m, P = k.mesh, k.P
    mass, radius = (k.m, k.r) if poly else (k.M, k.R)
    dec = cm.decide(m.x, m.ien, k.w, k.tet, k.lam, radius, cm.LEVEL, 1.0, 2.0, cm.T_MELT)
    assert cm.margins_ok(dec, cm.T_MELT)
    c = X.c_capture(X.capture_case)
    lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
    s_tet, s_lam, s_ien, s_x, s_w = pool.ints(k.tet), pool.slot(lam), pool.ints(m.ien), pool.slot(m.x), pool.slot(k.w)
    s_vel, s_temp, s_m, s_r = pool.slot(k.vel), pool.slot(k.temp), pool.slot(k.m), pool.slot(k.r)
    kern = "dfl_capture_flag" + ("<sizes>" if poly else "")
    for Pn, use_temp in ((P, True), (P, False), (1, True), (255, True), (256, True), (257, True)):
        args = (LD, m, k.w, k.tet[:Pn], k.lam[:Pn], k.vel[:Pn], k.temp[:Pn] if use_temp else None, mass[:Pn] if poly else mass,
                radius[:Pn] if poly else radius, k.rho_f, k.cp_p, cm.LEVEL, 1.0, 2.0, cm.T_MELT)
        model, rest = X.capture_flag(*args), X.capture_flag(F64, *args[1:])
        assert np.array_equal(model.keep, rest.keep)
        keep, rtet, dep = pool.slot(sent(P, I32), 0, I32), pool.slot(sent(P, I32), 0, I32), pool.slot(sent(5 * P))
        L.dfl_capture_flag(Pn, s_tet.ptr, s_lam.ptr, s_ien.ptr, s_x.ptr, s_w.ptr, m.N, s_vel.ptr, ptr(s_temp if use_temp else None),
                           np.nan if poly else k.M, np.nan if poly else k.R, ptr(s_m if poly else None), ptr(s_r if poly else None),
                           k.rho_f, k.cp_p, cm.LEVEL, 1.0, 2.0, cm.T_MELT, keep.ptr, rtet.ptr, dep.ptr, None)
        api.sync()
        what = "%s P=%d temp=%s" % (kern, Pn, use_temp)
        untouched(what, s_tet, s_lam, s_ien, s_x, s_w, s_vel, s_temp, s_m, s_r)
        wr = np.arange(P) < Pn
        assert np.array_equal(keep.check(what + " keep", wr)[:Pn], rest.keep), what + ": keep"
        assert np.array_equal(rtet.check(what + " rtet", wr)[:Pn], rest.rtet), what + ": rtet"
        got = dep.check(what + " dep", np.repeat(wr, 5))[:5 * Pn].reshape(-1, 5)
        assert_bits(got[:, 0], rest.dep[:, 0], what + " dep[0]")
        assert_bits(got[:, 4], rest.dep[:, 4], what + " dep[4]")
        assert not use_temp or Pn < 100 or np.abs(got[:, 4]).max() > 0
        judge(got[:, 1:4], model.dep[:, 1:4], model.A_dep[:, 1:4], c, what + " dep[1..3]", kern + ":dep", "P%d%s" % (Pn, "" if use_temp else "-no-temp"))
        for s in (keep, rtet, dep):
            s.dev.free()
            pool.slots.remove(s)
    L.dfl_capture_flag(0, *([None] * 5), m.N, None, None, 0.0, 0.0, None, None, *([1.0] * 6), None, None, None, None)
    api.sync()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_capture_source(N, api, pool):
    """q_vol, load and q_heat = A / time, one correctly rounded division each, under every combination of the three outputs
    being NULL: an output that is not passed, and the bands of the others, stay as they were"""
    L = api.lib()
    A = np.random.default_rng(N).normal(size=(N, 5))
    time = 0.0037
    s_A = pool.slot(A)
    for use in itertools.product((False, True), repeat=3):
        out = [pool.slot(sent(n * N)) for n in (1, 3, 1)]
        L.dfl_capture_source(N, s_A.ptr, time, *[ptr(o if u else None) for o, u in zip(out, use)], None)
        api.sync()
        for o, u, want in zip(out, use, (A[:, 0] / time, A[:, 1:4] / time, A[:, 4] / time)):
            exact(o, want, "capture_source %s" % (use,)) if u else untouched("capture_source %s" % (use,), o)
        untouched("capture_source", s_A)
        for o in out:
            o.dev.free()
            pool.slots.remove(o)
    record("dfl_capture_source", "N%d" % N, 0.0, exact=True)


# ======================================================================================================================
# solid-surface contact
# ======================================================================================================================
NCNT = 2 * X.SURFACE_SLOTS * X.SURFACE_SLOT_STRIDE + 1


def counters(step0=None, step1=None, total=0):
    """dfl_surface_counters as 2049 uint64 (viewed as float64 for the guarded buffer)"""
    a = np.zeros(NCNT, np.uint64)
    for k, s in enumerate((step0, step1)):
        if s is not None:
            a[k * 1024: (k + 1) * 1024: X.SURFACE_SLOT_STRIDE] = s
    a[-1] = np.uint64(total)
    return a.view(F64)


def read_counters(slot, what):
    a = slot.check(what, ALL).view(np.uint64)
    pad = np.ones(NCNT, bool)
    pad[:2048:X.SURFACE_SLOT_STRIDE] = False
    pad[-1] = False
    assert not a[pad].any(), what + ": the padding of the counters was written"
    return a[0:1024:X.SURFACE_SLOT_STRIDE].copy(), a[1024:2048:X.SURFACE_SLOT_STRIDE].copy(), int(a[-1])


@pytest.mark.parametrize("name,make", MESHES, ids=[n for n, _ in MESHES])
def test_surface_grad_max(name, make, api, pool):
    L, m = api.lib(), make()
    s_ien, s_x, out = pool.ints(m.ien), pool.slot(m.x), pool.slot([SENT])
    L.dfl_surface_grad_max(m.T, s_ien.ptr, s_x.ptr, out.ptr, None)
    api.sync()
    exact(out, [X.grad_max(m)], name + " grad_max")
    untouched(name, s_ien, s_x)
    L.dfl_surface_grad_max(0, s_ien.ptr, s_x.ptr, out.ptr, None)
    api.sync()
    exact(out, [0.0], name + " grad_max of no tet")
    record("dfl_surface_grad_max", name, 0.0, exact=True)


def test_surface_grad_max_degenerate(api, pool):
    """a deck of 300 tets with one flat tet among them: +inf"""
    L, m = api.lib(), X.kuhn(4)
    ien = m.ien[:300].copy()
    ien[271] = [0, 1, 5, 6]                                   # four nodes of the face z = 0: det == 0, the cross products not
    flat = X.Mesh("flat", m.x, ien)
    assert X.grad_max(flat) == np.inf
    s_ien, s_x, out = pool.ints(ien), pool.slot(m.x), pool.slot([SENT])
    L.dfl_surface_grad_max(300, s_ien.ptr, s_x.ptr, out.ptr, None)
    api.sync()
    exact(out, [np.inf], "grad_max with a flat tet")
    record("dfl_surface_grad_max", "one-flat-tet", 0.0, exact=True)


class Surface:
    """the guarded arrays of dfl_surface_contact on one case"""

    def __init__(self, pool, L, api, k, poly, friction):
        self.pool, self.L, self.api, self.k, self.poly, self.friction = pool, L, api, k, poly, friction
        m, P = k.mesh, k.P
        lam = np.where((k.tet >= 0)[:, None], k.lam, SENT)
        self.const = [pool.ints(k.tet), pool.slot(lam), pool.ints(m.ien), pool.slot(m.x), pool.slot(k.w), pool.slot(k.vel),
                      pool.slot(k.omega), pool.slot(k.m), pool.slot(k.r)]
        self.gm = [pool.slot([X.grad_max(m)]), pool.slot([0.0])]
        rng = np.random.default_rng(77)
        self.acc0, self.alpha0 = rng.normal(0, 10.0, (P, 3)), rng.normal(0, 100.0, (P, 3))

    def run(self, gm, cnt_image, cur, P=None, hist=None):
        k, c = self.k, self.const
        P = k.P if P is None else P
        acc, alpha, cnt = self.pool.slot(self.acc0), self.pool.slot(self.alpha0), self.pool.slot(cnt_image)
        sz = Sizes(c[8].ptr, c[7].ptr, None, 0.0) if self.poly else Sizes(None, None, None, 0.0)
        law = FrictionLaw(*X.LAW, np.nan if self.poly else 0.4 * k.M * k.R * k.R) if self.friction else FrictionLaw()
        self.L.dfl_surface_contact(P, c[0].ptr, c[1].ptr, c[2].ptr, c[3].ptr, c[4].ptr, k.mesh.N, c[5].ptr,
                                   c[6].ptr if self.friction else None, np.nan if self.poly else k.M, np.nan if self.poly else k.R, sz,
                                   X.KN, X.GN, law, scm.LEVEL, k.side, scm.T_SOLID, self.gm[gm].ptr,
                                   hist if hist is not None else ContactHistory(), cnt.ptr, cur, acc.ptr, alpha.ptr, None)
        self.api.sync()
        untouched("surface_contact", *self.const, *self.gm)
        return acc, alpha, cnt


@needs_ld
@pytest.mark.parametrize("kind,poly", [("plane", False), ("plane", True), ("sphere", False), ("sphere", True)])
def test_surface_contact_normal(kind, poly, api, pool):
    """without friction: acc == preload + the float64 restatement's addition bit for bit (contract(off)); a particle without
    contact is not written; alpha untouched; the counters: contacts in the low and buried in the high half of slot (block
    mod 64) of step[cur], the other parity folded into total and cleared; grad_max = 0 gives the same bits as the true one"""
    L = api.lib()
    k = X.surface_case(kind, poly)
    rest = X.surface_run(k, F64, poly, False)
    dec = scm.decide(k.mesh.x, k.mesh.ien, k.w, k.tet, k.lam, k.r if poly else k.R, scm.LEVEL, k.side, scm.T_SOLID)
    assert scm.margins_ok(dec, scm.T_SOLID) and np.array_equal(rest.contact, dec["contact"]) and np.array_equal(rest.buried, dec["buried"])
    assert rest.contact.sum() >= 10 and rest.buried.sum() >= 10
    far = (X.grad_max(k.mesh) > 0) & (rest.q > (rest.r * (rest.spread * X.grad_max(k.mesh))) * X.FAR_MARGIN) & rest.located
    assert far.sum() >= 1 and not (far & (rest.contact | rest.buried)).any()       # the early exit is taken, and rightly
    S = Surface(pool, L, api, k, poly, False)
    want = np.where(rest.contact[:, None], S.acc0 + rest.d_acc, S.acc0)
    old = np.arange(64, dtype=np.uint64) * 3 + 1 + (np.uint64(5) << np.uint64(32))    # the other parity: 64 slots to fold
    got = []
    for gm in (0, 1):
        acc, alpha, cnt = S.run(gm, counters(step0=None, step1=old, total=1000), 0)
        what = "surface_contact %s poly=%s grad_max %d" % (kind, poly, gm)
        a = acc.check(what + ": a particle without contact was written", np.repeat(rest.contact, 3))
        assert_bits(a, want.ravel(), what + " acc")
        untouched(what + " alpha", alpha)
        s0, s1, total = read_counters(cnt, what)
        assert np.array_equal(s0, X.surface_counts(rest.contact, rest.buried, k.P)), what + ": step[cur]"
        assert int(s0.sum()) == int(rest.contact.sum()) + (int(rest.buried.sum()) << 32)
        assert not s1.any() and total == 1000 + int((old & np.uint64(0xFFFFFFFF)).sum()), what + ": the fold"
        got.append((a.copy(), s0))
        # the next sub-step, with the other parity: this launch's counts go into the total
        cnt.image[:] = cnt.dev.numpy()
        acc2, alpha2, cnt2 = S.run(gm, cnt.image[cnt.lo: cnt.lo + NCNT], 1)
        t0, t1, total2 = read_counters(cnt2, what + " second launch")
        assert not t0.any() and np.array_equal(t1, s0) and total2 == total + int(rest.contact.sum())
    same_bits(got[0][0], got[1][0], "grad_max = 0 changed acc")
    assert np.array_equal(got[0][1], got[1][1])
    # P around the workgroup size on the same arrays: the particles behind P are not written and not counted
    for Pn in (1, 255, 256, 257):
        acc, alpha, cnt = S.run(0, counters(), 0, P=Pn)
        what = "surface_contact %s poly=%s P=%d" % (kind, poly, Pn)
        first = np.arange(k.P) < Pn
        a = acc.check(what + ": written behind P or without contact", np.repeat(rest.contact & first, 3))
        assert_bits(a, np.where(first[:, None], want, S.acc0).ravel(), what + " acc")
        untouched(what + " alpha", alpha)
        s0, s1, total = read_counters(cnt, what)
        assert np.array_equal(s0, X.surface_counts(rest.contact[:Pn], rest.buried[:Pn], Pn)) and not s1.any() and total == 0
    # P = 0: one workgroup still folds
    acc, alpha, cnt = S.run(0, counters(step0=old, step1=None, total=5), 1, P=0)
    untouched("surface_contact P = 0", acc, alpha)
    s0, s1, total = read_counters(cnt, "P = 0")
    assert not s0.any() and not s1.any() and total == 5 + int((old & np.uint64(0xFFFFFFFF)).sum())
    record("dfl_surface_contact" + ("<sizes>" if poly else ""), kind, 0.0, exact=True)


HIST_W = 4 * X.MAX_HISTORY
KEY_SURFACE = np.uint64(scm.KEY_SURFACE)


@needs_ld
@pytest.mark.parametrize("kind,poly", [("plane", False), ("plane", True), ("sphere", False), ("sphere", True)])
def test_surface_contact_friction(kind, poly, api, pool):
    """with friction: acc, alpha and the appended history entry against np.longdouble within the bound; new_count rises by one
    for a contact and is unchanged otherwise; the old rows, the entries below the sweep's count and above the new one, and
    *overflow are untouched; the spring of the previous sub-step is found behind stale keys; grad_max = 0: the same bits"""
    L = api.lib()
    k = X.surface_case(kind, poly)
    P = k.P
    model = X.surface_run(k, LD, poly, True, old=True)
    c = X.c_surface()
    mass = np.broadcast_to(np.asarray(k.m if poly else k.M, LD), (P,))
    iner = 0.4 * mass * np.broadcast_to(np.asarray(k.r if poly else k.R, LD), (P,)) ** 2
    con = model.contact
    # the previous rows: two stale partner keys, then (for the particles with a spring) the surface entry
    rng = np.random.default_rng(3)
    rows = sent(P * HIST_W).reshape(P, X.MAX_HISTORY, 4)
    ocount = np.zeros(P, I64)
    for i in range(P):
        n = i % 3
        rows[i, :n, 0] = (np.arange(n, dtype=np.uint64) + np.uint64(1000 + i)).view(F64)
        rows[i, :n, 1:] = rng.normal(size=(n, 3))
        if k.old[i] is not None:
            rows[i, n, 0] = np.array([KEY_SURFACE]).view(F64)[0]
            rows[i, n, 1:] = k.old[i]
            n += 1
        ocount[i] = n
    ncount = (np.arange(P) % 4).astype(I64)                  # what the sweep of this sub-step stored already
    nrows = sent(P * HIST_W).reshape(P, X.MAX_HISTORY, 4)
    for i in range(P):
        nrows[i, :ncount[i]] = rng.normal(size=(ncount[i], 4))
    S = Surface(pool, L, api, k, poly, True)
    s_orow, s_ocnt, s_over = pool.slot(rows), pool.ints(ocount), pool.ints([5])
    kern = "dfl_surface_contact<%sfriction>" % ("sizes," if poly else "")
    got = []
    for gm in (0, 1):
        s_nrow, s_ncnt = pool.slot(nrows), pool.ints(ncount)
        hist = ContactHistory(s_orow.ptr, s_ocnt.ptr, s_nrow.ptr, s_ncnt.ptr, s_over.ptr)
        acc, alpha, cnt = S.run(gm, counters(), 0, hist=hist)
        what = "%s %s grad_max %d" % (kern, kind, gm)
        untouched(what, s_orow, s_ocnt, s_over)
        a = acc.check(what + ": acc of a particle without contact", np.repeat(con, 3)).reshape(-1, 3)
        al = alpha.check(what + ": alpha of a particle without contact", np.repeat(con, 3)).reshape(-1, 3)
        exact(s_ncnt, ncount + con, what + " new_count", I32)
        mask = np.zeros((P, X.MAX_HISTORY, 4), bool)
        mask[np.flatnonzero(con), ncount[con]] = True
        r = s_nrow.check(what + ": history entries other than the appended one", mask.ravel()).reshape(P, X.MAX_HISTORY, 4)
        ent = r[np.flatnonzero(con), ncount[con]]
        assert np.all(np.ascontiguousarray(ent[:, 0]).view(np.uint64) == KEY_SURFACE), what + ": the key"
        s0, s1, total = read_counters(cnt, what)
        assert np.array_equal(s0, X.surface_counts(con, model.buried, P))
        if gm == 0:
            case = kind
            judge(a[con].astype(LD) - S.acc0[con], model.d_acc[con], (model.A_acc / mass + np.abs(a).max(axis=1))[con], c[0],
                  what + " acc", kern + ":acc", case)
            judge(al[con].astype(LD) - S.alpha0[con], model.d_alpha[con], (model.A_alpha / iner + np.abs(al).max(axis=1))[con], c[1],
                  what + " alpha", kern + ":alpha", case)
            judge(ent[:, 1:], model.xi[con], model.A_xi[con], c[2], what + " xi", kern + ":xi", case)
            assert np.abs(al[con] - S.alpha0[con]).max() > 0
        got.append((a.copy(), al.copy(), r.copy()))
    for x, y in zip(*got):
        same_bits(x, y, kern + ": grad_max = 0 changed the result")
