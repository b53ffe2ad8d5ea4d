"""Every launcher of the DEM contact sweep (csrc/k_dem.hip, csrc/k_walls.hip, csrc/dem_sweep.hpp) and dfl_scan_counts
(csrc/k_scan.hip) alone, through ctypes with the structs passed by value, against the model of tests/dem_model.py.

Tier A (bitwise): the scan and the cell sorts against the int64 model -- cell_of, cell_start, order and the sorted copies, at
P around the 256-thread workgroup, on random clouds, on the dyadic lattice whose points lie exactly on cell boundaries, on
points at and beyond the box, with every particle in one cell, and on the grid ncell = 49 whose fl(1 / fl(1 / n)) != n.
Tier E (exact): the force kernels on the dyadic lattice, where every intermediate of the normal law is exact: bit for bit
against the model and one variant against the other.
Tier B (rounded): acc (and alpha, and the history's springs) PARTICLE BY PARTICLE against the np.longdouble model under
8 c u A_i / m_i (/ I_i for alpha): A_i = the particle's own abs-sum, c = what the float64 restatement of the same law shows
against u A_i on the random families (dem_model.constant; test_dem_model_cpu.py), 8 for FMA contraction and operand order,
as in test_gpu_matrix_kernels.py and test_gpu_assembly_kernels.py.  A particle without contact must get exactly 0.0.  The
families keep every particle at least 1e-9 rmax from a contact's opening (asserted), so nothing is left out.

Every array sits between guard bands (guarded_buffers.py); overwrite outputs are preloaded with the sentinel; after each
launch the bands, every const input and every entry the operation must not write are compared bit for bit.  Arrays a kernel
indexes through (order, cell_start, the wall lists, the history counts) are the model's exact output or a device output
verified earlier in the same test.  No case aims at a fault.  err / bound and c go to the file named by DFL_PARITY_OUT
(profiles/dem_kernel_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import dem_model as D
import friction_model as fm
import walls_model as wm
from guarded_buffers import ALL, I32, Pool, Recorder, assert_bits, sent

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
U = D.U
record = Recorder("a")
needs_ld = pytest.mark.skipif(not D.HAVE_EXTENDED, reason=D.EXTENDED_REASON)
vp, f64, i32 = C.c_void_p, C.c_double, C.c_int32


class Sizes(C.Structure):
    _fields_ = [("radius", vp), ("mass", vp), ("sorted_r", vp), ("rmax", f64)]


class FrictionLaw(C.Structure):
    _fields_ = [("mu", f64), ("kt", f64), ("gamma_t", f64), ("dt", f64), ("inertia", f64)]


class ContactHistory(C.Structure):
    _fields_ = [("old_row", vp), ("old_count", vp), ("new_row", vp), ("new_count", vp), ("overflow", vp)]


class Grid3(C.Structure):
    _fields_ = [("lo", f64 * 3), ("inv", f64 * 3), ("n", i32 * 3)]


class WallTri(C.Structure):
    _fields_ = [("v", f64 * 9), ("n", f64 * 3), ("off", f64), ("pad", f64), ("node", i32 * 3), ("id", i32)]


def _declare(L):
    sort_tail = [vp] * 10 + [vp]   # cell_of rank count chunk_sum cell_start slot order sorted sorted_w sorted_r, stream
    sig = {
        "dfl_scan_counts": (None, [i32, vp, vp, vp, vp]),
        "dfl_scan_num_chunks": (i32, [i32]),
        "dfl_dem_sort_binned": (None, [i32, i32, vp, vp, vp, vp] + sort_tail),
        "dfl_dem_build_cells": (None, [i32, vp, vp, vp, vp, f64, i32] + sort_tail),
        "dfl_walls_build_cells": (None, [i32, vp, vp, vp, vp, Grid3] + sort_tail),
        "dfl_dem_forces": (None, [i32, vp, vp, f64, f64, Sizes, f64, f64, FrictionLaw, f64, i32, vp, vp, ContactHistory, vp, vp, vp]),
        "dfl_walls_forces": (None, [i32, vp, vp, f64, f64, Sizes, f64, f64, FrictionLaw, Grid3, vp, vp, vp, vp, Grid3, vp, vp, f64,
                                    vp, ContactHistory, vp, vp, vp]),
        "dfl_dem_integrate": (None, [i32, f64, vp, vp, vp, vp]),
        "dfl_dem_integrate_spin": (None, [i32, f64, C.POINTER(f64 * 3), vp, vp, vp, vp, vp, vp]),
        "dfl_dem_spin": (None, [i32, f64, vp, vp, vp]),
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


def test_struct_sizes():
    assert C.sizeof(WallTri) == 128 and C.sizeof(Grid3) == 64 and C.sizeof(Sizes) == 32 and C.sizeof(FrictionLaw) == 40


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


# ======================================================================================================================
# Tier A: the scan
# ======================================================================================================================
SCAN_SIZES = [0, 1, 3, 1023, 1024, 1025, 4096, 257 * 1024 - 1, 257 * 1024, 300 * 1024 + 5]


def _counts(kind, n):
    if kind == "zeros":
        return np.zeros(n, I64)
    if kind == "ones":
        return np.ones(n, I64)
    a = np.random.default_rng(40 + n).integers(0, 8, n)
    if n > 2048:
        a[1024:2048] = 0       # one chunk empty
    if n:
        a[(2 * n) // 3] = 100000
    return a


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_counts(n, api, pool):
    """start[0 .. n] = the exclusive scan, count[0 .. n) zeroed, count[n] and the bands untouched; chunk_sum is plain scratch:
    preloaded with zeros or with the sentinel it gives the same result; a second call on the zeroed counts returns zeros"""
    L = api.lib()
    nchunk = L.dfl_scan_num_chunks(n)
    assert nchunk == D.scan_num_chunks(n)
    for kind in ("zeros", "ones", "random"):
        data = _counts(kind, n)
        want = D.exclusive_scan(data)
        assert want[-1] < 2 ** 31
        for scratch in (np.zeros(nchunk, I32), sent(nchunk, I32)):
            count = pool.ints(np.r_[data, 77])
            start, chunk = pool.slot(sent(n + 1, I32), 0, I32), pool.slot(scratch, 0, I32)
            L.dfl_scan_counts(n, count.ptr, chunk.ptr, start.ptr, None)
            api.sync()
            what = "scan n=%d %s" % (n, kind)
            exact(start, want, what + " start", I32)
            exact(count, np.r_[np.zeros(n, I64), 77], what + " count", I32)
            chunk.check(what + " chunk_sum", ALL)
            start.reset(sent(n + 1, I32))
            L.dfl_scan_counts(n, count.ptr, chunk.ptr, start.ptr, None)
            api.sync()
            exact(start, np.zeros(n + 1, I64), what + " second call", I32)
            exact(count, np.r_[np.zeros(n, I64), 77], what + " count, second call", I32)
            pool.free()
    record("dfl_scan_counts", "n%d" % n, 0.0, exact=True)


def test_scan_counts_negative_n(api, pool):
    L = api.lib()
    s = [pool.slot(sent(4, I32), 0, I32) for _ in range(3)]
    L.dfl_scan_counts(-1, s[0].ptr, s[1].ptr, s[2].ptr, None)
    api.sync()
    untouched("scan n=-1", *s)


# ======================================================================================================================
# Tier A: the cell sorts
# ======================================================================================================================
def _coords(family, P, ncell, rng):
    if family == "random":
        return rng.uniform(0.0, 1.0, (P, 3))
    if family == "lattice":          # multiples of 2^-4: on the cell boundaries of ncell = 1, 2, 4, never on those of 49
        return rng.integers(0, 17, (P, 3)) / 16.0
    if family == "edges":            # at and beyond the box: clamped into the edge cells
        return rng.choice([0.0, 1.0, -0.3, 1.7, 0.5], (P, 3))
    return 0.301 + 0.001 * rng.uniform(0.0, 1.0, (P, 3))   # one cell of every grid


class SortBuffers:
    """the guarded arrays of one cell sort over nbin bins"""

    def __init__(self, pool, L, P, nbin, x, v, w, r):
        n = max(P, 1)
        self.x, self.v = pool.slot(x), pool.slot(v)
        self.w = None if w is None else pool.slot(w)
        self.r = None if r is None else pool.slot(r)
        self.cell_of, self.rank, self.slot = (pool.slot(sent(n, I32), 0, I32) for _ in range(3))
        self.count = pool.ints(np.zeros(nbin + 1))
        self.chunk = pool.slot(sent(L.dfl_scan_num_chunks(nbin), I32), 0, I32)
        self.cell_start = pool.slot(sent(nbin + 1, I32), 0, I32)
        self.order = pool.slot(sent(n, I32), 0, I32)
        self.sorted, self.sorted_w, self.sorted_r = pool.slot(sent(6 * n)), pool.slot(sent(3 * n)), pool.slot(sent(n))

    def tail(self):
        return [self.cell_of.ptr, self.rank.ptr, self.count.ptr, self.chunk.ptr, self.cell_start.ptr, self.slot.ptr, self.order.ptr,
                self.sorted.ptr, self.sorted_w.ptr, self.sorted_r.ptr, None]

    def verify(self, what, cell_of, nbin, x, v, w, r, binned=True):
        cnt, start, order = D.cell_order(cell_of, nbin)
        if binned:
            exact(self.cell_of, cell_of, what + " cell_of", I32)
            self.rank.check(what + " rank", ALL)
        exact(self.cell_start, start, what + " cell_start", I32)
        exact(self.order, order, what + " order", I32)
        s, sw, sr = D.sorted_copies(order, x, v, w, r)
        exact(self.sorted, s, what + " sorted")
        exact(self.sorted_w, sw, what + " sorted_w") if w is not None else untouched(what + " sorted_w", self.sorted_w)
        exact(self.sorted_r, sr, what + " sorted_r") if r is not None else untouched(what + " sorted_r", self.sorted_r)
        untouched(what, self.count, self.x, self.v, self.w, self.r)   # count: zeroed again, its last entry never written
        self.chunk.check(what + " chunk_sum", ALL)
        slot = self.slot.check(what + " slot", ALL).astype(I64)
        assert np.array_equal(np.sort(slot), np.arange(len(slot))), what + ": slot is no permutation"
        assert np.array_equal(np.asarray(cell_of)[slot], np.sort(cell_of)), what + ": slot does not follow cell_start"


@pytest.mark.parametrize("P", [1, 2, 255, 256, 257, 1000])
def test_dem_build_cells(P, api, pool):
    L = api.lib()
    for ncell in (1, 2, 4, 49):
        cell = 1.0 / ncell
        for k, family in enumerate(("random", "lattice", "edges", "one_cell")):
            rng = np.random.default_rng(1000 * P + 10 * ncell + k)
            x, v = _coords(family, P, ncell, rng), rng.normal(size=(P, 3))
            w, r = rng.normal(size=(P, 3)), rng.uniform(0.01, 0.02, P)
            cell_of = D.box_bins(x, cell, ncell)
            if family == "one_cell":
                assert len(set(cell_of.tolist())) == 1
            for use_w, use_r in ((False, False), (True, False), (False, True), (True, True)):
                b = SortBuffers(pool, L, P, ncell ** 3, x, v, w if use_w else None, r if use_r else None)
                L.dfl_dem_build_cells(P, b.x.ptr, b.v.ptr, ptr(b.w), ptr(b.r), cell, ncell, *b.tail())
                api.sync()
                b.verify("build_cells P=%d ncell=%d %s w=%s r=%s" % (P, ncell, family, use_w, use_r), cell_of, ncell ** 3, x, v,
                         w if use_w else None, r if use_r else None)
                pool.free()
    record("dfl_dem_build_cells", "P%d" % P, 0.0, exact=True)


def test_dem_build_cells_empty(api, pool):
    L = api.lib()
    b = SortBuffers(pool, L, 0, 8, np.zeros(3), np.zeros(3), None, None)
    L.dfl_dem_build_cells(0, b.x.ptr, b.v.ptr, None, None, 0.5, 2, *b.tail())
    api.sync()
    untouched("build_cells P=0", b.cell_of, b.rank, b.count, b.chunk, b.cell_start, b.slot, b.order, b.sorted, b.sorted_w, b.sorted_r)


def test_dem_sort_binned(api, pool):
    """the caller's bin pass: cell_of, rank and count from the model, nbin no multiple of 1024; the ranks in two arrival
    orders give the same order and sorted copies bit for bit"""
    L = api.lib()
    P, nbin = 1000, 1500
    rng = np.random.default_rng(77)
    x, v, w, r = rng.normal(size=(P, 3)), rng.normal(size=(P, 3)), rng.normal(size=(P, 3)), rng.uniform(0.01, 0.02, P)
    cell_of = rng.integers(0, nbin, P)
    cell_of[:40] = 1499
    cell_of[40:60] = 1023
    cnt, start, order = D.cell_order(cell_of, nbin)
    got = []
    for arrival in (np.arange(P), rng.permutation(P)):
        rank, seen = np.zeros(P, I64), np.zeros(nbin, I64)
        for i in arrival:
            rank[i] = seen[cell_of[i]]
            seen[cell_of[i]] += 1
        b = SortBuffers(pool, L, P, nbin, x, v, w, r)
        b.cell_of.reset(cell_of.astype(I32))
        b.rank.reset(rank.astype(I32))
        b.count.reset(np.r_[cnt, 0].astype(I32))
        L.dfl_dem_sort_binned(P, nbin, b.x.ptr, b.v.ptr, b.w.ptr, b.r.ptr, *b.tail())
        api.sync()
        untouched("sort_binned", b.cell_of, b.rank)
        b.count.image[b.count.lo: b.count.lo + nbin] = 0     # zeroed for the next pass
        b.verify("sort_binned", cell_of, nbin, x, v, w, r, binned=False)
        got.append([s.get() for s in (b.order, b.sorted, b.sorted_w, b.sorted_r)])
    for a, c in zip(*got):
        assert np.array_equal(a.view(np.uint8), c.view(np.uint8))
    record("dfl_dem_sort_binned", "P1000-nbin1500", 0.0, exact=True)


def _grid(g):
    return Grid3((f64 * 3)(*g.lo), (f64 * 3)(*g.inv), (i32 * 3)(*[int(k) for k in g.n]))


def test_walls_build_cells(api, pool):
    """an off-origin grid with n = (3, 5, 2) and inverses that are no powers of two; a third of the particles outside, on every
    side: they go to the extra bin, sorted behind all others by id, and cell_start[nx ny nz + 1] == P"""
    L = api.lib()
    ext = np.array([1.1, 1.7, 0.7])
    g = D.Grid3((-1.0, 2.0, 0.5), np.array([3, 5, 2]) / ext, (3, 5, 2))
    P = 600
    rng = np.random.default_rng(78)
    x = g.lo + ext * rng.uniform(0.0, 1.0, (P, 3))
    out = np.arange(P) % 3 == 0
    side = rng.integers(0, 6, P)
    for i in np.nonzero(out)[0]:
        d = side[i] // 2
        x[i, d] = g.lo[d] - 0.05 * (1 + i % 4) if side[i] % 2 == 0 else g.lo[d] + ext[d] + 0.05 * (1 + i % 4)
    assert set(side[out].tolist()) == set(range(6))
    v, w, r = rng.normal(size=(P, 3)), rng.normal(size=(P, 3)), rng.uniform(0.01, 0.02, P)
    cell_of = D.grid_bins(x, g)
    assert np.array_equal(cell_of == 30, out)
    for use_w, use_r in ((False, False), (True, True)):
        b = SortBuffers(pool, L, P, 31, x, v, w if use_w else None, r if use_r else None)
        L.dfl_walls_build_cells(P, b.x.ptr, b.v.ptr, ptr(b.w), ptr(b.r), _grid(g), *b.tail())
        api.sync()
        b.verify("walls_build_cells w=%s" % use_w, cell_of, 31, x, v, w if use_w else None, r if use_r else None)
        start, order = b.cell_start.get(), b.order.get()
        assert start[31] == P and start[30] == P - out.sum()
        assert np.array_equal(order[start[30]:], np.nonzero(out)[0])
        pool.free()
    record("dfl_walls_build_cells", "P600-3x5x2", 0.0, exact=True)


# ======================================================================================================================
# the force kernels
# ======================================================================================================================
HIST_W = 4 * D.MAX_HISTORY   # doubles per history row


class HistorySlots:
    """two guarded history slots (rows as [P][16] records of key + xi[3], live counts) and the overflow counter"""

    def __init__(self, pool, P, seed=None):
        rows = sent(P * HIST_W).reshape(P, D.MAX_HISTORY, 4)
        count = np.zeros(P, I64)
        if seed is not None:
            for i in range(P):
                c = int(seed.count[i])
                rows[i, :c, 0] = seed.key[i, :c].view(F64)
                rows[i, :c, 1:] = seed.xi[i, :c]
            count = seed.count
        self.P = P
        self.rows = [pool.slot(rows), pool.slot(sent(P * HIST_W))]
        self.count = [pool.ints(count), pool.slot(sent(P, I32), 0, I32)]
        self.overflow = pool.ints([5])
        self.cur, self.over = 0, 5

    def struct(self):
        a, b = self.cur, 1 - self.cur
        return ContactHistory(self.rows[a].ptr, self.count[a].ptr, self.rows[b].ptr, self.count[b].ptr, self.overflow.ptr)

    def verify(self, what, model, c_xi, kernel, case):
        """the new slot against the model's rows; the old slot untouched; the slots then swap roles"""
        a, b = self.cur, 1 - self.cur
        untouched(what + " old history", self.rows[a], self.count[a])
        cnt = exact(self.count[b], model.count, what + " new_count", I32).astype(I64)
        live = np.arange(D.MAX_HISTORY)[None, :] < cnt[:, None]
        got = self.rows[b].check(what + " history entries beyond the count", np.repeat(live.ravel(), 4)).reshape(self.P, D.MAX_HISTORY, 4)
        keys = np.ascontiguousarray(got[:, :, 0]).view(np.uint64)
        assert np.array_equal(keys[live], model.key[live]), what + ": the history keys are not the model's visit order"
        err = np.abs(got[:, :, 1:].astype(LD) - model.xi).max(axis=-1)[live].astype(F64)
        bnd = (8.0 * c_xi * U * model.X[live]).astype(F64)
        ratio = float((err / bnd).max()) if err.size else 0.0
        record(kernel + ":xi", case, ratio, c=float(c_xi))
        assert ratio <= 1.0, "%s: history spring err / bound = %.3g" % (what, ratio)
        self.over += model.over
        exact(self.overflow, [self.over], what + " overflow", I32)
        for s in (self.rows[b], self.count[b], self.overflow):
            s.image[:] = s.dev.numpy()      # verified: what the next sweep must leave alone
        self.cur = b
        return D.History(self.P, cnt, keys, got[:, :, 1:])


def judge(got, model_v, A, scale, c, what, kernel, case, in_contact):
    """component by component under 8 c u A_i / scale_i; a particle without contact: exactly 0.0"""
    got = np.asarray(got, F64).reshape(-1, 3)
    assert np.all(np.isfinite(got)), what + ": not finite"
    assert np.all(got[~in_contact] == 0.0), what + ": a particle without contact is not exactly 0.0"
    b = D.bound(A, scale, c)
    err = np.abs(got.astype(LD) - model_v).max(axis=1).astype(F64)
    live = in_contact & (b > 0)
    ratio = float((err[live] / b[live]).max()) if live.any() else 0.0
    assert np.all(err[in_contact & ~live] == 0.0), what
    record(kernel, case, ratio, c=float(c))
    print("%s %s: err / bound = %.3g (c = %.3g)" % (kernel, case, ratio, c))
    assert ratio <= 1.0, "%s: err / bound = %.3g at particle %d" % (what, ratio, int(np.argmax(np.where(live, err / np.where(live, b, 1), 0))))


class ForceRun:
    """the guarded arrays of one force launch on a state (x, v, w, r, m) sorted by the model's (cell, id) order"""

    def __init__(self, pool, x, v, w, r, m, cell_start, order):
        P = len(x)
        self.P = P
        s, sw, sr = D.sorted_copies(order, x, v, w, r)
        self.sorted, self.sorted_w, self.sorted_r = pool.slot(s), pool.slot(sw), pool.slot(sr)
        self.radius, self.mass = pool.slot(r), pool.slot(m)
        self.order, self.cell_start = pool.ints(order), pool.ints(cell_start)
        self.acc, self.alpha = pool.slot(sent(3 * P)), pool.slot(sent(3 * P))

    def sizes(self, poly, rmax):
        return Sizes(self.radius.ptr, self.mass.ptr, self.sorted_r.ptr, rmax) if poly else Sizes(None, None, None, 0.0)

    def inputs_untouched(self, what):
        untouched(what, self.sorted, self.sorted_w, self.sorted_r, self.radius, self.mass, self.order, self.cell_start)

    def reset_outputs(self):
        self.acc.reset(sent(3 * self.P))
        self.alpha.reset(sent(3 * self.P))


NAN = float("nan")


def _law(law, inertia):
    return FrictionLaw(law.mu, law.kt, law.gamma_t, law.dt, inertia)


def box_forces(L, run, poly, fric, R, M, rmax, kn, gn, law, cell, ncell, hist):
    sz = run.sizes(poly, rmax)
    fl = _law(law, 0.4 * M * R * R if not poly else NAN) if fric else FrictionLaw()
    L.dfl_dem_forces(run.P, run.sorted.ptr, run.sorted_w.ptr if fric else None, NAN if poly else R, NAN if poly else M, sz, kn, gn,
                     fl, cell, ncell, run.order.ptr, run.cell_start.ptr, hist.struct() if fric else ContactHistory(), run.acc.ptr,
                     run.alpha.ptr, None)


@needs_ld
def test_forces_exact_on_the_lattice(api, pool):
    """Tier E: one size (zeroed dfl_sizes) and per-particle sizes with every radius R and mass m (scalars NaN: not read) on
    the dyadic lattice == the model bit for bit and each other; touching second neighbours, the coincident pair and the wall
    overlap of exactly 0 contribute nothing; no contact: +0.0.  The same lattice shifted into a mesh grid, with an empty
    wall list, gives the same pair forces from dfl_walls_forces"""
    L = api.lib()
    x, v = D.dyadic_lattice()
    P, R, M, kn, gn, ncell = len(x), D.LATTICE_R, D.LATTICE_M, D.LATTICE_KN, D.LATTICE_GN, D.LATTICE_NCELL
    r, m = np.full(P, R), np.full(P, M)
    _, start, order = D.cell_order(D.box_bins(x, 1.0 / ncell, ncell), ncell ** 3)
    model = D.sweep(x, v, r, m, kn, gn, LD, slot_of=D.slots(order))
    assert (~model.in_contact).any()
    run = ForceRun(pool, x, v, np.zeros((P, 3)), r, m, start, order)
    got = []
    for poly in (False, True):
        run.reset_outputs()
        box_forces(L, run, poly, False, R, M, R, kn, gn, None, 1.0 / ncell, ncell, None)
        api.sync()
        what = "lattice poly=%s" % poly
        got.append(exact(run.acc, model.acc.astype(F64)[:, :].ravel(), what).copy())
        untouched(what, run.alpha)
        run.inputs_untouched(what)
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
    record("dfl_dem_forces", "lattice-exact", 0.0, exact=True)
    # the mesh grid: the lattice shifted by a dyadic vector, a 6 x 6 x 6 grid of the same cells around it, no walls
    shift = np.array([-1.0, 2.0, 0.5])
    g = D.Grid3(shift - 0.25, (4.0, 4.0, 4.0), (6, 6, 6))
    xs = x + shift
    cell_of = D.grid_bins(xs, g)
    assert cell_of.max() < 216
    _, start, order = D.cell_order(cell_of, 217)
    pairs = D.sweep(xs, v, r, m, kn, gn, LD, box=False, slot_of=D.slots(order))
    assert np.array_equal(D.sweep(x, v, r, m, kn, gn, LD, box=False).acc, pairs.acc)
    run = ForceRun(pool, xs, v, np.zeros((P, 3)), r, m, start, order)
    tri, plane, wstart, wlist, dropped = pool.slot(np.zeros(16)), pool.ints([0]), pool.ints([0, 0]), pool.ints([0]), pool.ints([3])
    wg = D.Grid3(g.lo, (1.0 / 1.5,) * 3, (1, 1, 1))
    for poly in (False, True):
        run.reset_outputs()
        L.dfl_walls_forces(P, run.sorted.ptr, None, NAN if poly else R, NAN if poly else M, run.sizes(poly, R), kn, gn, FrictionLaw(),
                           _grid(g), run.order.ptr, run.cell_start.ptr, tri.ptr, plane.ptr, _grid(wg), wstart.ptr, wlist.ptr, 1e-12,
                           dropped.ptr, ContactHistory(), run.acc.ptr, run.alpha.ptr, None)
        api.sync()
        what = "lattice in a mesh grid poly=%s" % poly
        exact(run.acc, pairs.acc.astype(F64).ravel(), what)
        untouched(what, run.alpha, tri, plane, wstart, wlist, dropped)
        run.inputs_untouched(what)
    record("dfl_walls_forces", "lattice-exact", 0.0, exact=True)


FAMILIES = [(n, False) for n in D.RANDOM_ONE + ("straddle4", "straddle49")] + [("poly", True), ("reach", True)]


@needs_ld
@pytest.mark.parametrize("name,poly", FAMILIES, ids=[n for n, _ in FAMILIES])
def test_dem_forces_normal(name, poly, api, pool):
    """Tier B, no friction: one size on the one-size families (and, there, the per-particle-size kernel with every radius R,
    which must give the same bits), per-particle sizes on the size families"""
    L = api.lib()
    fam = D.family(name)
    _, start, order = fam.order()
    model = D.variant_sweep(fam, poly, False, LD)
    assert model.margin.min() >= 1e-9 * fam.rmax
    c = D.constant(poly, False)[0]
    r, m = (fam.r, fam.m) if poly else (np.full(fam.P, fam.R), np.full(fam.P, fam.M))
    run = ForceRun(pool, fam.x, fam.v, np.zeros((fam.P, 3)), r, m, start, order)
    got = []
    for as_poly in ((True,) if poly else (False, True)):
        run.reset_outputs()
        box_forces(L, run, as_poly, False, fam.R, fam.M, fam.rmax, D.KN, D.GN, None, 1.0 / fam.ncell, fam.ncell, None)
        api.sync()
        what = "dem_forces %s sizes=%s" % (name, as_poly)
        got.append(run.acc.check(what, ALL).copy())
        untouched(what, run.alpha)
        run.inputs_untouched(what)
        judge(got[-1], model.acc, model.A_acc, model.mass, c, what, "dfl_dem_forces" + ("<sizes>" if as_poly else ""), name,
              model.in_contact)
    if len(got) == 2:
        assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)), name + ": the two variants differ on equal sizes"


@needs_ld
@pytest.mark.parametrize("name,poly", FAMILIES, ids=[n for n, _ in FAMILIES])
def test_dem_forces_friction(name, poly, api, pool):
    """Tier B with friction: three sweeps in a row with the history slots alternating; the first reads a seeded history (rows
    rotated, stale keys in front); between sweeps the state advances on the host from the device's verified acc and alpha,
    and the model reads the device's verified rows"""
    L = api.lib()
    fam = D.family(name)
    c = D.constant(poly, True)
    seed = D.seeded_history(fam, poly)
    hist = HistorySlots(pool, fam.P, seed)
    old = seed
    x, v, w = fam.x, fam.v, fam.w
    r, m = (fam.r, fam.m) if poly else (np.full(fam.P, fam.R), np.full(fam.P, fam.M))
    kernel = "dfl_dem_forces<%sfriction>" % ("sizes," if poly else "")
    for sweep in range(3):
        _, start, order = D.cell_order(D.box_bins(x, 1.0 / fam.ncell, fam.ncell), fam.ncell ** 3)
        model = D.variant_sweep(fam, poly, True, LD, old, (x, v, w))
        assert model.margin.min() >= 1e-9 * fam.rmax
        run = ForceRun(pool, x, v, w, r, m, start, order)
        box_forces(L, run, poly, True, fam.R, fam.M, fam.rmax, D.KN, D.GN, fam.law, 1.0 / fam.ncell, fam.ncell, hist)
        api.sync()
        what, case = "dem_forces friction %s sweep %d" % (name, sweep), "%s-sweep%d" % (name, sweep)
        acc, alpha = run.acc.check(what, ALL).reshape(-1, 3), run.alpha.check(what, ALL).reshape(-1, 3)
        run.inputs_untouched(what)
        judge(acc, model.acc, model.A_acc, model.mass, c[0], what + " acc", kernel, case, model.in_contact)
        judge(alpha, model.alpha, model.A_alpha, model.inertia, c[1], what + " alpha", kernel + ":alpha", case, model.in_contact)
        old = hist.verify(what, model, c[2], kernel, case)
        x, v = D.integrate(D.DT, x, v, acc, F64)
        w = D.spin(D.DT, w, alpha, F64)


@needs_ld
def test_history_overflow(api, pool):
    """one particle with 17 contacts: *overflow rises by exactly 1, its row holds the first 16 in visit order, the 17th still
    contributes its force with a zero spring"""
    L = api.lib()
    R, n = 0.05, 17
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), np.pi * (1 + 5 ** 0.5) * k
    x = np.vstack([[0.5, 0.5, 0.5], 0.5 + 1.9 * R * np.c_[np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)]])
    rng = np.random.default_rng(17)
    P = n + 1
    v, w = rng.normal(0, 0.1, (P, 3)), rng.normal(0, 3, (P, 3))
    r, m = np.full(P, R), np.full(P, 1.5)
    law = D.Law(D.MU, 2.0 / 7.0 * D.KN, D.GN, D.DT)
    ncell = 5
    _, start, order = D.cell_order(D.box_bins(x, 1.0 / ncell, ncell), ncell ** 3)
    seed = D.sweep(x, v, r, m, D.KN, D.GN, F64, slot_of=D.slots(order), w=w, law=law, old=D.History(P))
    old = D.History(P, seed.count, seed.key, seed.xi.astype(F64))
    model = D.sweep(x, v, r, m, D.KN, D.GN, LD, slot_of=D.slots(order), w=w, law=law, old=old)
    assert len(model.keys[0]) == 17 and model.over == 1 and model.count[0] == 16 and model.margin.min() >= 1e-9 * R
    assert max(len(k) for k in model.keys[1:]) <= 16
    c = D.constant(False, True)
    hist = HistorySlots(pool, P, old)
    run = ForceRun(pool, x, v, w, r, m, start, order)
    box_forces(L, run, False, True, R, 1.5, R, D.KN, D.GN, law, 1.0 / ncell, ncell, hist)
    api.sync()
    acc, alpha = run.acc.check("overflow", ALL), run.alpha.check("overflow", ALL)
    judge(acc, model.acc, model.A_acc, model.mass, c[0], "overflow acc", "dfl_dem_forces<friction>", "17-contacts", model.in_contact)
    judge(alpha, model.alpha, model.A_alpha, model.inertia, c[1], "overflow alpha", "dfl_dem_forces<friction>:alpha", "17-contacts",
          model.in_contact)
    hist.verify("overflow", model, c[2], "dfl_dem_forces<friction>", "17-contacts")
    assert hist.over == 6
    # without the contact that found no entry the force differs by far more than the bound: it did contribute
    last = int(model.keys[0][16])
    less = D.sweep(np.delete(x, last, 0), np.delete(v, last, 0), r[1:], m[1:], D.KN, D.GN, LD)
    assert np.abs(less.acc[0] - model.acc[0]).max() > 1e3 * D.bound(model.A_acc, model.mass, c[0])[0]


# ---- mesh walls ------------------------------------------------------------------------------------------------------
def _notched_cube():
    from dedflow_amd.meshgen import kuhn_box
    return kuhn_box(3, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (i == 2 and j == 2 and k == 2))


def _wall_case(which):
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube
    mesh, R = {"kuhn_cube3": (kuhn_cube, 0.04), "fan": (fan_mesh, 0.1), "notched_cube": (_notched_cube, 0.04)}[which]
    W = wm.Walls(mesh() if which != "kuhn_cube3" else mesh(3))
    rng = np.random.default_rng(3)
    x = rng.uniform(W.lo - 2 * R, W.hi + 2 * R, size=(50, 3))
    t = rng.integers(0, len(W.v), 70)
    lam = rng.dirichlet(np.ones(3), 70)
    x = np.vstack([x, np.einsum("na,nad->nd", lam, W.v[t]) + W.n[t] * rng.uniform(-0.5 * R, R, (70, 1))])
    if which == "notched_cube":   # the notch's inner vertex and its three inner edges stick into the domain
        c, a = 2.0 / 3.0, 0.4 * R
        x = np.vstack([x, [[c - a, c - a, c - a], [0.85, c - a, c - a], [c - a, 0.85, c - a], [c - a, c - 0.3 * R, 0.9],
                           [0.45, 0.55, 0.6 * R], [0.6 * R, 0.7 * R, 0.5]]])   # none on a triangle's diagonal: no ties
    return W, R, x, rng.normal(size=x.shape), rng.normal(0.0, 3.0, size=x.shape)


def _tri_records(W):
    rec = (WallTri * len(W.v))()
    for t in range(len(W.v)):
        rec[t].v[:] = W.v[t].ravel().tolist()
        rec[t].n[:] = W.n[t].tolist()
        rec[t].off, rec[t].pad, rec[t].id = W.off[t], 0.0, t
        rec[t].node[:] = [int(k) for k in W.node[t]]
    return np.frombuffer(rec, dtype=F64).copy()


def _wall_grid(W, R, n):
    """the header's rule: cell k lists, ascending, every triangle whose R-expanded bounding box overlaps it"""
    glo, ext = W.lo - R, (W.hi - W.lo) + 2 * R
    hw = ext.max() / n
    g = D.Grid3(glo, (1.0 / hw,) * 3, np.maximum(np.ceil(ext / hw - 1e-9), 1).astype(int))
    lists = [[] for _ in range(g.ncell)]
    pad = R * (1 + 1e-9) + 1e-12 * np.linalg.norm(W.hi - W.lo)
    for t in range(len(W.v)):
        lo = np.clip(np.floor((W.v[t].min(axis=0) - pad - g.lo) * g.inv), 0, g.n - 1).astype(int)
        hi = np.clip(np.floor((W.v[t].max(axis=0) + pad - g.lo) * g.inv), 0, g.n - 1).astype(int)
        for k in range(lo[2], hi[2] + 1):
            for j in range(lo[1], hi[1] + 1):
                for i in range(lo[0], hi[0] + 1):
                    lists[i + g.n[0] * (j + g.n[1] * k)].append(t)
    start = np.r_[0, np.cumsum([len(q) for q in lists])]
    return g, start, np.array([t for q in lists for t in q] or [0])


@needs_ld
@pytest.mark.parametrize("which", ["kuhn_cube3", "fan", "notched_cube"])
def test_walls_forces(which, api, pool):
    """Tier B on mesh walls, no friction and friction: the wall grid of one cell listing every triangle (the model's own
    candidate set) and the 2-per-axis grid of the header's rule agree bit for bit and stay inside the bound; a particle in
    the extra bin gets 0 / m and an empty row; face contacts, two coplanar triangles as one contact, and on the notched cube
    edge and vertex contacts, are all present"""
    L = api.lib()
    W, R, x, v, w = _wall_case(which)
    P, M = len(x), 1.5
    r, m = np.full(P, R), np.full(P, M)
    glo, ext = W.lo - R, (W.hi - W.lo) + 2 * R
    n = np.maximum(np.floor(ext / (4 * R)), 1)
    g = D.Grid3(glo, n / ext, n.astype(int))
    cell_of = D.grid_bins(x, g)
    active = cell_of < g.ncell
    assert (~active).sum() >= 5 and active.sum() >= 60
    _, start, order = D.cell_order(cell_of, g.ncell + 1)
    plane = np.array([fm.plane_id(W, W.n[t], W.off[t]) for t in range(len(W.v))])
    every = list(range(len(W.v)))
    mw = D.MeshWalls(W.v, W.n, W.off, W.node, plane, W.tol, [every if a else [] for a in active])
    law = D.Law(D.MU, 2.0 / 7.0 * D.KN, D.GN, D.DT)
    tri, planes, dropped = pool.slot(_tri_records(W)), pool.ints(plane), pool.ints([3])
    grids = []
    for cells in (1, 2):
        wg, ws, wl = _wall_grid(W, R, cells)
        grids.append((_grid(wg), pool.ints(ws), pool.ints(wl)))
    assert grids[0][1].host().tolist() == [0, len(every)] and grids[1][1].n == 9
    run = ForceRun(pool, x, v, w, r, m, start, order)
    for fric in (False, True):
        kw = dict(box=False, slot_of=D.slots(order), mesh=mw, active=active)
        if fric:
            kw.update(w=w, law=law, old=D.History(P))
        model, rest = D.sweep(x, v, r, m, D.KN, D.GN, LD, **kw), D.sweep(x, v, r, m, D.KN, D.GN, F64, **kw)
        assert model.margin.min() >= 1e-9 * R and model.dropped == 0
        kinds = {k >> 62 for row in model.keys for k in row}
        assert 1 in kinds and (which != "notched_cube" or {2, 3} <= kinds)
        c = np.maximum(D.sweep_c(model, rest), D.constant(False, fric))   # c of the restatement on this cloud, never below the box's
        assert np.all(c <= 16)
        got = []
        for gi, (wgrid, ws, wl) in enumerate(grids):
            run.reset_outputs()
            hist = HistorySlots(pool, P) if fric else None
            L.dfl_walls_forces(P, run.sorted.ptr, run.sorted_w.ptr if fric else None, R, M, run.sizes(False, R), D.KN, D.GN,
                               _law(law, 0.4 * M * R * R) if fric else FrictionLaw(), _grid(g), run.order.ptr, run.cell_start.ptr,
                               tri.ptr, planes.ptr, wgrid, ws.ptr, wl.ptr, float(W.tol), dropped.ptr,
                               hist.struct() if fric else ContactHistory(), run.acc.ptr, run.alpha.ptr, None)
            api.sync()
            what, case = "walls_forces %s friction=%s grid %d" % (which, fric, gi), "%s-grid%d" % (which, gi)
            kernel = "dfl_walls_forces" + ("<friction>" if fric else "")
            acc = run.acc.check(what, ALL).copy()
            judge(acc, model.acc, model.A_acc, model.mass, c[0], what, kernel, case, model.in_contact)
            got.append([acc])
            if fric:
                alpha = run.alpha.check(what, ALL).copy()
                judge(alpha, model.alpha, model.A_alpha, model.inertia, c[1], what + " alpha", kernel + ":alpha", case, model.in_contact)
                new = hist.verify(what, model, c[2], kernel, case)
                assert not new.count[~active].any()
                got[-1] += [alpha, new.count, new.key, new.xi]
            else:
                untouched(what, run.alpha)
            assert not acc.reshape(-1, 3)[~active].any()
            untouched(what, tri, planes, dropped, ws, wl)
            run.inputs_untouched(what)
        for a, b in zip(*got):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), \
                which + ": the two wall grids differ"


# ======================================================================================================================
# the integrators
# ======================================================================================================================
def _close(got, want_ld, scale, k, what, kernel, case):
    err = np.abs(np.asarray(got, F64).reshape(-1, 3).astype(LD) - want_ld).astype(F64)
    b = (k * U * scale).astype(F64)
    assert np.all(err[b == 0] == 0)
    ratio = float((err[b > 0] / b[b > 0]).max())
    record(kernel, case, ratio)
    assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)


@needs_ld
@pytest.mark.parametrize("P", [1, 85, 86, 257])
def test_integrators(P, api, pool):
    """v and omega against longdouble within 2 u (|v| + |dt a|) (two roundings: the product and the sum), x within
    2 u (|x| + |dt v|) of x + dt v for the v the kernel stored; with a body acceleration g the sum a + g is a third rounding:
    3 u (|v| + |dt a| + |dt g|).  acc and alpha are bit-unchanged; omega = NULL leaves alpha unread; on dyadic values the
    results are exact.  3 P crosses the 256-thread workgroup between P = 85 and 86"""
    L = api.lib()
    rng = np.random.default_rng(500 + P)
    for dyadic in (False, True):
        if dyadic:
            x, v, a, w, al = (rng.integers(-64, 65, (P, 3)) / 64.0 for _ in range(5))
            dt, g = 0.125, np.array([0.5, -0.25, 2.0])
        else:
            x, v, a, w, al = rng.uniform(0, 1, (P, 3)), rng.normal(0, 0.1, (P, 3)), rng.normal(0, 50, (P, 3)), rng.normal(0, 3, (P, 3)), rng.normal(0, 900, (P, 3))
            dt, g = 1.0e-4, np.array([0.3, -0.1, -9.81])
        case = "P%d%s" % (P, "-dyadic" if dyadic else "")

        def check(xs, vs, gg, kernel):
            xl, vl = D.integrate(dt, x, v, a, LD, gg)
            vd = vs.check(kernel + " vel", ALL).reshape(-1, 3)
            xd = xs.check(kernel + " coord", ALL).reshape(-1, 3)
            if dyadic:
                assert_bits(vd, vl.astype(F64), kernel + " vel")
                assert_bits(xd, xl.astype(F64), kernel + " coord")
                record(kernel, case, 0.0, exact=True)
                return
            k = 3.0 if np.any(gg) else 2.0
            _close(vd, vl, np.abs(v) + np.abs(dt * a) + np.abs(dt * gg), k, kernel + " vel", kernel + ":vel", case)
            _close(xd, x.astype(LD) + LD(dt) * vd.astype(LD), np.abs(x) + np.abs(dt * vd), 2.0, kernel + " coord", kernel + ":coord", case)

        def check_spin(ws, kernel):
            wd = ws.check(kernel + " omega", ALL).reshape(-1, 3)
            wl = D.spin(dt, w, al, LD)
            if dyadic:
                assert_bits(wd, wl.astype(F64), kernel + " omega")
                record(kernel, case + "-omega", 0.0, exact=True)
            else:
                _close(wd, wl, np.abs(w) + np.abs(dt * al), 2.0, kernel + " omega", kernel + ":omega", case)

        xs, vs, as_, ws, als = pool.slot(x), pool.slot(v), pool.slot(a), pool.slot(w), pool.slot(al)
        L.dfl_dem_integrate(P, dt, xs.ptr, vs.ptr, as_.ptr, None)
        api.sync()
        check(xs, vs, np.zeros(3), "dfl_dem_integrate")
        untouched("integrate", as_)
        for spin in (False, True):
            xs.reset(x.ravel()); vs.reset(v.ravel()); ws.reset(w.ravel())
            L.dfl_dem_integrate_spin(P, dt, C.byref((f64 * 3)(*g)), xs.ptr, vs.ptr, as_.ptr, ws.ptr if spin else None,
                                     als.ptr if spin else None, None)
            api.sync()
            check(xs, vs, g, "dfl_dem_integrate_spin")
            check_spin(ws, "dfl_dem_integrate_spin") if spin else untouched("integrate_spin omega=NULL", ws)
            untouched("integrate_spin", as_, als)
        xs.reset(x.ravel()); vs.reset(v.ravel()); ws.reset(w.ravel())
        L.dfl_dem_spin(P, dt, ws.ptr, als.ptr, None)
        api.sync()
        check_spin(ws, "dfl_dem_spin")
        untouched("spin", als, xs, vs, as_)
        pool.free()
