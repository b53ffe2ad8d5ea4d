"""Every launcher of the laser (csrc/k_laser.hip, csrc/k_laser_surface.hip) alone, through ctypes with the structs passed by
value, against the model of tests/laser_kernel_model.py.

Tier A (bitwise, integers): the bin of every particle, the hit keys as uint64 -- the 2^-40 depth grid, its clamp at both ends,
the face-index tie-break, edges and vertices included --, col_face and the scratch of the long runs, the snapshot
(count -> emit with the host's scan -> nodes) with its clip at cap, the radix-sorted node list with all 32 key bits.
Tier E (bitwise, float64 restatement in the source's order): the deposit, the tally tree, the list kernels, the surface
deposit's slot sums, and the exact claims of the column kernel (a particle behind the hit has rate +0.0, eta_p = 1 scatters
exactly nothing, no hit => missed == col_T, part[0] = ((P / 4) gx[i]) gy[j]).
Tier B (rounded): the column kernel entry by entry against np.longdouble under the a-priori bounds that
laser_kernel_model.laser_columns derives in its docstring (laser_model.step's rate_bound and T_rel, ULP_EXP = 3; a row of
part: its entries' bounds plus (ceil(len / 64) + 6) eps sum |term|), at every run length around the three paths of the
kernel; and bit-identical outputs when the entries of every run change places.

Every array sits between guard bands (guarded_buffers.py); overwrite outputs are preloaded with the sentinel, accumulate
outputs with known non-zero values; after each launch the bands, every const input and every entry the call must not write
are compared bit for bit.  No case aims at a fault: all indices are in range and no particle depth is non-finite.
err / bound goes to the file named by DFL_PARITY_OUT (profiles/laser_kernel_parity.jsonl is such a run)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import laser_kernel_model as K
from guarded_buffers import ALL, I32, U8, U32, U64, Pool, Recorder, assert_bits, sent
from krylov_model import EXTENDED_REASON, HAVE_EXTENDED

pytestmark = pytest.mark.gpu

F64, LD, I64 = np.float64, np.longdouble, np.int64
record = Recorder("a")
needs_ld = pytest.mark.skipif(not HAVE_EXTENDED, reason=EXTENDED_REASON)
vp, f64, i32, i64 = C.c_void_p, C.c_double, C.c_int32, C.c_int64
V3 = C.POINTER(f64 * 3)
Beam = K.CBeam

SIG = {
    "dfl_scan_num_chunks": (i32, [i32]),
    "dfl_tets_per_block": (i32, []),
    "dfl_laser_column_cap": (i32, []),
    "dfl_laser_bin": (None, [i32, vp, Beam, vp, vp, vp, vp, vp]),
    "dfl_laser_hit": (None, [i32, vp, Beam, f64, f64, vp, vp]),
    "dfl_laser_columns": (None, [i32, Beam, f64, f64, f64, vp, vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dfl_laser_deposit": (None, [i32, vp, vp, vp, Beam, f64, f64, vp, vp, vp, vp, vp]),
    "dfl_laser_tally": (None, [i32, f64, vp, vp, vp]),
    "dfl_laser_source_add": (None, [i32, vp, f64, vp, vp, vp]),
    "dfl_laser_surface_temp_bytes": (i64, [i32, i32]),
    "dfl_laser_surface_count": (None, [i32, vp, vp, vp, i32, f64, i32, V3, vp, vp]),
    "dfl_laser_surface_emit": (None, [i32, vp, vp, vp, i32, f64, i32, V3, vp, vp, vp, vp, vp, vp, i32, vp]),
    "dfl_laser_surface_nodes": (None, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dfl_laser_surface_deposit": (None, [Beam, vp, i32, i32, vp, vp, vp, vp, f64, f64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dfl_laser_surface_source_add": (None, [i32, vp, vp, f64, vp, vp, vp]),
    "dfl_laser_surface_power": (None, [i32, i32, vp, vp, vp, vp, vp]),
    "dfl_laser_surface_carry": (None, [i32, vp, vp, vp, vp, vp]),
    "dfl_laser_surface_carry_add": (None, [i32, f64, vp, vp, vp]),
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

    def out(self, n, dtype=F64):
        return self.slot(sent(max(int(n), 1), dtype), 0, dtype)


@pytest.fixture
def pool(api):
    p = FlatPool(api)
    yield p
    p.free()


@pytest.fixture(scope="module")
def cube():
    from dedflow_amd.meshgen import kuhn_cube
    return kuhn_cube(5, jitter=0.2)


def test_struct_sizes_and_every_launcher_is_declared():
    assert C.sizeof(K.CWallTri) == 128 and C.sizeof(Beam) == 120
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dedflow_amd", "csrc")
    seen = []
    for f in ("k_laser.hip", "k_laser_surface.hip"):
        text = open(os.path.join(src, f)).read()
        names = re.findall(r"^(?:void|I|int64_t) (dfl_\w+)\(", text[text.index('extern "C"'):], re.M)
        assert names and not [n for n in names if n not in SIG], f
        seen += names
    assert len(seen) == 7 + 9
    mine = open(os.path.abspath(__file__)).read()
    for n in seen:                                                   # ... and called by a test of this module
        assert re.search(r"\.%s\(" % n, mine), n


def exact(slot, want, what, dtype=F64):
    """the whole array == want bit for bit, the bands as uploaded"""
    got = slot.check(what, ALL)
    assert_bits(got[:np.size(want)], np.ravel(want), what, dtype)
    return got


def untouched(what, *slots):
    for s in slots:
        if s is not None:
            s.check(what + ": an array the call must not write changed")


def same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(U8), np.ascontiguousarray(b).view(U8)), what


def judge(got, model, bound, what, kernel, case):
    """entry by entry |got - model| <= bound; an entry whose bound is 0 must be exact"""
    got, model, bound = np.asarray(got, F64).ravel(), np.asarray(model, LD).ravel(), np.asarray(bound, F64).ravel()
    assert np.all(np.isfinite(got)), what + ": not finite"
    err = np.abs(got.astype(LD) - model).astype(F64)
    assert np.all(err[bound == 0] == 0), what + ": an entry with bound 0 is not exact"
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    record(kernel, case, ratio)
    print("%s %s: err / bound = %.3g" % (kernel, case, ratio))
    assert ratio <= 1.0, "%s: err / bound = %.3g" % (what, ratio)


# ======================================================================================================================
# Tier A: bin, hit
# ======================================================================================================================
BIN_CASES = [(n, P, "vertical") for n in K.BIN_N for P in K.BIN_P] + [(16, 1000, "oblique"), (4, 257, "oblique")]


@pytest.mark.parametrize("n,P,direction", BIN_CASES)
def test_bin(n, P, direction, api, pool):
    """cell_of bit for bit (n^2 + (i >> 3) outside, a NaN coordinate among them); count == the bincount over exactly
    n^2 + ((P - 1) >> 3) + 1 bins with the guard behind; rank a permutation of 0 .. count - 1 in every bin (atomics: no
    particular one); rate exactly +0.0 outside and untouched inside"""
    L = api.lib()
    b, coord, _ = K.bin_case(n, P, direction)
    cell, count, outside = K.laser_bin(coord, b)
    s_x, s_cell, s_rank, s_rate = pool.slot(coord), pool.out(P, I32), pool.out(P, I32), pool.out(P)
    s_count = pool.ints(np.full(len(count), 3))                      # accumulated: rank continues from what count held
    what = "bin n=%d P=%d %s" % (n, P, direction)
    L.dfl_laser_bin(P, s_x.ptr, K.c_beam(b), s_cell.ptr, s_rank.ptr, s_count.ptr, s_rate.ptr, None)
    api.sync()
    exact(s_cell, cell, what + " cell_of", I32)
    exact(s_count, count + 3, what + " count", I32)
    rate = s_rate.check(what + " rate inside the grid", outside)
    assert_bits(rate[outside], np.zeros(int(outside.sum())), what + " rate outside")
    rank = s_rank.check(what + " rank", ALL)
    o = np.lexsort((rank, cell))
    start = np.r_[0, np.cumsum(count)]
    assert np.array_equal(rank[o], 3 + np.arange(P) - start[cell[o]]), what + ": rank is not a permutation per bin"
    untouched(what, s_x)
    record("dfl_laser_bin", what, 0.0, exact=True)


def hit_launch(api, pool, tri_v, b, s_lo, scale, nf=None):
    L = api.lib()
    nf = len(tri_v) if nf is None else nf
    s_tri = pool.slot(K.wall_records(tri_v) if len(tri_v) else np.zeros(16))
    s_key = pool.out(b.ncol, U64)
    L.dfl_laser_hit(nf, s_tri.ptr, K.c_beam(b), s_lo, scale, s_key.ptr, None)
    api.sync()
    untouched("hit", s_tri)
    return s_key


@pytest.mark.parametrize("direction", ["vertical", "oblique"])
@pytest.mark.parametrize("nf", (0,) + K.HIT_NF)
def test_hit_keys(nf, direction, api, pool):
    """every key as uint64: the minimum over the faces of (depth field << 24 | face).  The faces (laser_kernel_model.hit_specials)
    decide a column by a shared edge, a shared vertex, the face index at identical depth, the face index inside one grid step
    (the deeper face first in the list wins), the depth two steps apart, the clamp at either end; a zero-area face, a face
    with a NaN vertex and a face outside the grid win nothing; both orientations; nf = 0 leaves all ones"""
    b, tri_v, _, _ = K.hit_case(max(nf, 1), direction)
    want = K.laser_hit(tri_v[:nf], b, K.HIT_S_LO, K.HIT_SCALE)
    s_key = hit_launch(api, pool, tri_v, b, K.HIT_S_LO, K.HIT_SCALE, nf)
    exact(s_key, want, "hit nf=%d %s" % (nf, direction), U64)
    if nf == 0:
        assert np.all(s_key.get() == np.uint64(K.NO_HIT))
    record("dfl_laser_hit", "nf=%d %s" % (nf, direction), 0.0, exact=True)


def test_hit_keys_on_a_coarse_and_an_offset_grid(api, pool):
    """the same faces on the host's kind of grid (s_lo and scale that are no powers of two) and on n = 4, 64"""
    for n, s_lo, scale in ((16, 0.9371, 2.0 ** 40 / 1.1173), (4, K.HIT_S_LO, K.HIT_SCALE), (64, 1.0, 2.0 ** 40 / 3.0)):
        _, tri_v, _, _ = K.hit_case(257, "oblique")
        b = K.frame(n, "oblique", h=K.H * 16 / n)
        s_key = hit_launch(api, pool, tri_v, b, s_lo, scale)
        exact(s_key, K.laser_hit(tri_v, b, s_lo, scale), "hit n=%d" % n, U64)
    record("dfl_laser_hit", "grids", 0.0, exact=True)


# ======================================================================================================================
# dfl_laser_columns: Tier A / E claims and Tier B entry by entry
# ======================================================================================================================
def columns_launch(api, pool, case, use_tri=True, **kw):
    """one launch on guarded buffers; the bands, the const inputs and everything the call must not write are checked here"""
    L = api.lib()
    a = dict(case)
    a.update(kw)
    b, P, ncol = a["b"], a["P"], a["b"].ncol
    ins = dict(gw=pool.slot(a["gw"]), cs=pool.ints(a["cell_start"]), order=pool.ints(a["order"]), sorted=pool.slot(a["sorted6"]),
               r=None if a["sorted_r"] is None else pool.slot(a["sorted_r"]),
               tri=pool.slot(K.wall_records(a["tri_v"], a["tri_id"])) if use_tri else None,
               key=pool.slot(a["colkey"] if use_tri else np.full(ncol, K.NO_HIT, U64), 0, U64))
    out = dict(k_tau=pool.out(P), k_id=pool.out(P, I32), rate=pool.out(P), col_T=pool.out(ncol), col_face=pool.out(ncol, I32),
               part=pool.out(6 * ncol))
    L.dfl_laser_columns(P, K.c_beam(b), a["power"], a["eta_p"], a["eta_s"], ins["gw"].ptr, ins["cs"].ptr, ins["order"].ptr,
                        ins["sorted"].ptr, None if ins["r"] is None else ins["r"].ptr, a["radius"],
                        None if ins["tri"] is None else ins["tri"].ptr, ins["key"].ptr, out["k_tau"].ptr, out["k_id"].ptr,
                        out["rate"].ptr, out["col_T"].ptr, out["col_face"].ptr, out["part"].ptr, None)
    api.sync()
    untouched("columns", *ins.values())
    m = K.run_columns(a, tri_v=a["tri_v"] if use_tri else None, colkey=a["colkey"] if use_tri else np.full(ncol, K.NO_HIT, U64))
    pad = np.zeros(max(P, 1) - P, bool)
    long_pos, written = np.r_[m["k_id"] >= 0, pad], np.r_[m["written"], pad]
    got = dict(rate=out["rate"].check("rate of ids outside every run", written), col_T=out["col_T"].check("col_T", ALL),
               col_face=out["col_face"].check("col_face", ALL), part=out["part"].check("part", ALL).reshape(6, ncol),
               k_tau=out["k_tau"].check("k_tau outside the long runs", long_pos),
               k_id=out["k_id"].check("k_id outside the long runs", long_pos))
    return got, m


COLUMN_CASES = [("n4-mono", 4, K.RUNS_N4, False), ("n4-poly", 4, K.RUNS_N4, True), ("n6-mono", 6, K.runs_n6(), False),
                ("n6-poly", 6, K.runs_n6(), True)]


@needs_ld
@pytest.mark.parametrize("name,n,lengths,poly", COLUMN_CASES, ids=[c[0] for c in COLUMN_CASES])
def test_columns_entry_by_entry(name, n, lengths, poly, api, pool):
    """run lengths 0 .. 1100 in one launch (the bitonic network, the counting fallback over three tiles, the chunked scan):
    col_face, part[0], the scratch of the long runs (tau and id in (s, id) order, nothing outside [lo, lo + len)) and the +0.0
    rate of every particle behind its column's hit bit for bit; rate, col_T and the rows of part under the model's bounds"""
    case = K.column_case(n, lengths, poly)
    got, m = columns_launch(api, pool, case)
    assert api.lib().dfl_laser_column_cap() == K.CAP
    assert_bits(got["col_face"], m["col_face"], name + " col_face", I32)
    assert_bits(got["part"][0], m["pc"], name + " part[0]")
    lp = m["k_id"] >= 0
    assert lp.any()
    assert_bits(got["k_id"][lp], m["k_id"][lp], name + " k_id", I32)
    assert_bits(got["k_tau"][lp], m["k_tau"][lp], name + " k_tau")
    w, z = m["written"], m["rate_exact0"]
    assert z.any() and (w & ~z).any()
    assert_bits(got["rate"][z], np.zeros(int(z.sum())), name + " rate behind the hit")
    judge(got["rate"][w], m["rate"][w], m["rate_bound"][w], name + " rate", "dfl_laser_columns", name + " rate")
    judge(got["col_T"], m["T"], m["T"].astype(F64) * m["T_rel"], name + " col_T", "dfl_laser_columns", name + " col_T")
    for row, label in ((1, "absorbed"), (2, "scattered"), (3, "substrate"), (4, "reflected"), (5, "missed")):
        judge(got["part"][row], m["part"][row], m["part_bound"][row], name + " " + label, "dfl_laser_columns", name + " " + label)
    has = m["has"]
    assert_bits(got["part"][3][~has], np.zeros(int((~has).sum())), name + " substrate without a hit")
    assert_bits(got["part"][4][~has], np.zeros(int((~has).sum())), name + " reflected without a hit")
    assert_bits(got["part"][5][has], np.zeros(int(has.sum())), name + " missed with a hit")
    same_bits(got["part"][5][~has], got["col_T"][~has], name + " missed == col_T")


@pytest.mark.parametrize("name,n,lengths,poly", COLUMN_CASES[1:3], ids=[c[0] for c in COLUMN_CASES[1:3]])
def test_columns_do_not_depend_on_the_position_inside_a_run(name, n, lengths, poly, api, pool):
    """the same (s, id) pairs at other positions of every run (short runs: the bitonic network; long ones: the counting
    fallback): every output bit for bit the same, the sorted scratch included"""
    case = K.column_case(n, lengths, poly)
    g0, m = columns_launch(api, pool, case)
    for seed in (1, 2):
        g1, _ = columns_launch(api, pool, K.permuted(case, seed))
        lp = m["k_id"] >= 0
        for k in ("col_T", "col_face", "part"):
            same_bits(g0[k], g1[k], name + " " + k)
        same_bits(g0["rate"][m["written"]], g1["rate"][m["written"]], name + " rate")
        same_bits(g0["k_tau"][lp], g1["k_tau"][lp], name + " k_tau")
        same_bits(g0["k_id"][lp], g1["k_id"][lp], name + " k_id")
    record("dfl_laser_columns", name + " permuted", 0.0, exact=True)


def test_columns_exact_claims(api, pool):
    """eta_p = 1: the scattered row is exactly +0.0.  No candidate list (tri = NULL, keys all ones): col_face = -1, substrate
    = reflected = +0.0, missed == col_T bit for bit and no particle is dark.  P = 0: cell_start is not read"""
    case = K.column_case(4, K.RUNS_N4, True)
    ncol = case["b"].ncol
    got, m = columns_launch(api, pool, case, eta_p=1.0)
    assert_bits(got["part"][2], np.zeros(ncol), "scattered at eta_p = 1")
    assert_bits(got["part"][0], m["pc"], "part[0]")
    got, m = columns_launch(api, pool, case, use_tri=False)
    assert not m["rate_exact0"].any() and np.all(got["rate"][m["written"]] > 0)
    assert_bits(got["col_face"], np.full(ncol, -1), "col_face without candidates", I32)
    assert_bits(got["part"][3], np.zeros(ncol), "substrate without candidates")
    assert_bits(got["part"][4], np.zeros(ncol), "reflected without candidates")
    same_bits(got["part"][5], got["col_T"], "missed == col_T")
    empty = dict(case, P=0, order=np.zeros(1, I64), sorted6=np.zeros(6), sorted_r=None, cell_start=np.full(ncol + 1, 12345))
    got, m = columns_launch(api, pool, empty)
    assert_bits(got["col_T"], m["pc"], "col_T without particles")
    assert_bits(got["part"][1:3], np.zeros((2, ncol)), "absorbed, scattered without particles")
    record("dfl_laser_columns", "exact claims", 0.0, exact=True)


# ======================================================================================================================
# Tier E: deposit, tally, list kernels
# ======================================================================================================================
@pytest.mark.parametrize("ns", K.LIST_SIZES)
def test_deposit(ns, api, pool):
    """power (overwritten) and energy (accumulated) == the face-then-column loop in float64; the keys are dfl_laser_hit's,
    verified first"""
    L = api.lib()
    d = K.deposit_case(ns)
    b = d["b"]
    s_tri = pool.slot(K.wall_records(d["tri_v"]))
    s_key = pool.out(b.ncol, U64)
    L.dfl_laser_hit(len(d["tri_v"]), s_tri.ptr, K.c_beam(b), K.HIT_S_LO, K.HIT_SCALE, s_key.ptr, None)
    api.sync()
    exact(s_key, d["colkey"], "deposit: keys", U64)
    s_key.image[:] = s_key.dev.numpy()
    s_off, s_face, s_T = pool.ints(d["soff"]), pool.ints(d["sface"]), pool.slot(d["col_T"])
    s_pow, s_en = pool.out(ns), pool.slot(d["energy"])
    power, energy = K.laser_deposit(ns, d["soff"], d["sface"], d["tri_v"], b, d["eta_s"], d["dt"], d["colkey"], d["col_T"], d["energy"])
    for call in range(2):                                            # energy accumulates, power is overwritten
        L.dfl_laser_deposit(ns, s_off.ptr, s_face.ptr, s_tri.ptr, K.c_beam(b), d["eta_s"], d["dt"], s_key.ptr, s_T.ptr, s_pow.ptr,
                            s_en.ptr, None)
        api.sync()
        exact(s_pow, power, "deposit ns=%d power" % ns)
        exact(s_en, energy, "deposit ns=%d energy, call %d" % (ns, call))
        energy = energy + d["dt"] * power
        untouched("deposit", s_off, s_face, s_tri, s_key, s_T)
    record("dfl_laser_deposit", "ns=%d" % ns, 0.0, exact=True)


@pytest.mark.parametrize("ncol", K.TALLY_NCOL)
def test_tally(ncol, api, pool):
    """all six outputs == the strided per-thread sums and the halving tree in float64"""
    L = api.lib()
    rng = np.random.default_rng(ncol)
    part = rng.uniform(0.0, 1.0, 6 * ncol) * 10.0 ** rng.integers(-3, 3, 6 * ncol)
    s_part, s_out = pool.slot(part), pool.out(6)
    L.dfl_laser_tally(ncol, 1234.5, s_part.ptr, s_out.ptr, None)
    api.sync()
    exact(s_out, K.laser_tally(ncol, 1234.5, part), "tally ncol=%d" % ncol)
    untouched("tally", s_part)
    record("dfl_laser_tally", "ncol=%d" % ncol, 0.0, exact=True)


def _list_data(n, N, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(N)[:n], rng.uniform(1.0, 2.0, n), rng.uniform(1.0, 2.0, N), rng.uniform(1.0, 2.0, N)


@pytest.mark.parametrize("ns", K.LIST_SIZES)
def test_source_add(ns, api, pool):
    L = api.lib()
    N = 2 * ns + 3
    node, energy, q, _ = _list_data(ns, N, ns)
    s_node, s_en, s_q = pool.ints(node), pool.slot(energy), pool.slot(q)
    L.dfl_laser_source_add(ns, s_node.ptr, 0.37, s_en.ptr, s_q.ptr, None)
    api.sync()
    e1, q1 = K.list_source_add(ns, node, 0.37, energy, q)
    exact(s_en, e1, "source_add energy")
    exact(s_q, q1, "source_add q")
    untouched("source_add", s_node)
    record("dfl_laser_source_add", "ns=%d" % ns, 0.0, exact=True)


@pytest.mark.parametrize("nmax", K.LIST_SIZES)
def test_surface_list_kernels(nmax, api, pool):
    """source_add, power, carry read *nu on the device: entries at or beyond min(nmax, *nu) keep their bits, with *nu below,
    equal to and above nmax; power zero-fills q[0 .. N); energy is zeroed exactly where it was consumed; carry_add over N"""
    L = api.lib()
    N = 2 * nmax + 5
    for nu in sorted({0, nmax // 2, max(nmax - 1, 0), nmax, nmax + 1, nmax + 300}):
        n = min(nmax, nu)
        unode, energy, q, carry = _list_data(nmax, N, 10 * nmax + nu)
        power = energy * 3.0
        s_nu, s_un = pool.ints([nu]), pool.ints(unode)
        what = "nmax=%d nu=%d" % (nmax, nu)
        s_en, s_q = pool.slot(energy), pool.slot(q)
        L.dfl_laser_surface_source_add(nmax, s_nu.ptr, s_un.ptr, 0.37, s_en.ptr, s_q.ptr, None)
        api.sync()
        e1, q1 = K.list_source_add(n, unode, 0.37, energy, q)
        exact(s_en, e1, what + " source_add energy")
        exact(s_q, q1, what + " source_add q")
        s_pw, s_q = pool.slot(power), pool.slot(q)
        L.dfl_laser_surface_power(N, nmax, s_nu.ptr, s_un.ptr, s_pw.ptr, s_q.ptr, None)
        api.sync()
        exact(s_q, K.surface_power(N, n, unode, power), what + " power q")
        untouched(what, s_pw)
        s_en, s_ca = pool.slot(energy), pool.slot(carry)
        L.dfl_laser_surface_carry(nmax, s_nu.ptr, s_un.ptr, s_en.ptr, s_ca.ptr, None)
        api.sync()
        e1, c1 = K.surface_carry(n, unode, energy, carry)
        exact(s_en, e1, what + " carry energy")
        exact(s_ca, c1, what + " carry")
        untouched(what, s_nu, s_un)
    carry, q = _list_data(1, N, nmax)[2:]
    s_ca, s_q = pool.slot(np.r_[carry, 5.0]), pool.slot(np.r_[q, 7.0])
    L.dfl_laser_surface_carry_add(N, 0.37, s_ca.ptr, s_q.ptr, None)
    api.sync()
    c1, q1 = K.surface_carry_add(N, 0.37, carry, q)
    exact(s_ca, np.r_[c1, 5.0], "carry_add carry (entry N untouched)")
    exact(s_q, np.r_[q1, 7.0], "carry_add q (entry N untouched)")
    record("dfl_laser_surface_lists", "nmax=%d" % nmax, 0.0, exact=True)


# ======================================================================================================================
# Tier A: the snapshot -- count, emit, nodes
# ======================================================================================================================
def snapshot_launch(api, pool, xg, ien, phi, level, side, direction, NT, cap=None, spare=8):
    """count on guarded buffers against the model; emit with the host's exclusive scan; every array bit for bit"""
    L = api.lib()
    N = len(phi)
    snap = K.Snapshot(xg, ien, phi, level, side, direction, NT)
    w = np.concatenate([np.full(4 * N, 0.123), phi])                 # phi = w + 4 N
    s_ien, s_x, s_w = pool.ints(np.asarray(ien).reshape(-1, 4)[:NT]), pool.slot(xg), pool.slot(w)
    nblk = -(-NT // L.dfl_tets_per_block())
    s_cnt = pool.out(nblk, I32)
    d3 = (f64 * 3)(*direction)
    L.dfl_laser_surface_count(NT, s_ien.ptr, s_x.ptr, s_w.ptr, N, level, side, d3, s_cnt.ptr, None)
    api.sync()
    exact(s_cnt, snap.blk_count, "blk_count", I32)
    assert snap.blk_count.sum() == snap.nf
    s_base = pool.ints(snap.blk_base)
    room = snap.nf + spare
    cap = room if cap is None else cap
    s_cand, s_F, s_tet, s_ij, s_t = pool.out(16 * room), pool.out(9 * room), pool.out(room, I32), pool.out(room, I32), pool.out(3 * room)
    L.dfl_laser_surface_emit(NT, s_ien.ptr, s_x.ptr, s_w.ptr, N, level, side, d3, s_base.ptr, s_cand.ptr, s_F.ptr, s_tet.ptr,
                             s_ij.ptr, s_t.ptr, cap, None)
    api.sync()
    untouched("snapshot", s_ien, s_x, s_w, s_base)
    n = min(cap, snap.nf)
    live = np.arange(room) < n
    got = dict(cand=s_cand.check("cand at or beyond cap", np.repeat(live, 16)), F=s_F.check("facets at or beyond cap", np.repeat(live, 9)),
               tet=s_tet.check("tet at or beyond cap", live), ij=s_ij.check("ij at or beyond cap", live),
               t=s_t.check("t at or beyond cap", np.repeat(live, 3)))
    assert_bits(got["F"][:9 * n], np.ravel(snap.F[:n]), "facets")
    assert_bits(got["t"][:3 * n], np.ravel(snap.t[:n]), "t")
    assert_bits(got["tet"][:n], snap.tet[:n], "tet", I32)
    assert_bits(got["ij"][:n], snap.ij[:n], "ij", I32)
    assert_bits(got["cand"][:16 * n], np.ravel(K.wall_records(snap.F[:n], -2 - snap.tet[:n])), "cand: v, n = 0, off = pad = 0, node = -1, id")
    return snap


@pytest.mark.parametrize("mask", range(16))
def test_snapshot_single_tet(mask, api, pool):
    """every sign mask (0, 1 or 2 facets), both sides, the beam from every side; and a node exactly at the level"""
    total = 0
    for at_level in (None, 0, 3):
        xg, ien, phi, level = K.single_tet(mask, at_level)
        for side in (1, -1):
            for direction in ((0.0, 0.0, -1.0), (0.6, 0.0, 0.8), (-0.28, 0.96, 0.0)):
                nf = snapshot_launch(api, pool, xg, ien, phi, level, side, direction, 1).nf
                total += nf if at_level is None else 0
    assert (total > 0) == (mask not in (0, 15))
    record("dfl_laser_surface_emit", "single tet mask=%d" % mask, 0.0, exact=True)


SNAP_FIELDS = ("plane_vertical", "plane_oblique", "sphere", "perpendicular", "in_plane", "constant_tets", "nan_and_inf")


@pytest.mark.parametrize("field", SNAP_FIELDS)
def test_snapshot_cube(field, cube, api, pool):
    """kuhn_cube(5, 0.2): every prefix NT of the tet list around the workgroup size, both sides"""
    xg, phi, level, direction = K.snapshot_fields(cube)[field]
    seen = 0
    for NT in K.SNAP_NT:
        for side in (1, -1):
            seen += snapshot_launch(api, pool, xg, cube.ien, phi, level, side, direction, NT).nf
    assert (seen == 0) == (field == "in_plane")
    record("dfl_laser_surface_emit", field, 0.0, exact=True)


def test_snapshot_clips_at_cap(cube, api, pool):
    """cap below the total, also between the two triangles of a quad: the records below cap are the same, nothing at or
    beyond cap is written in any of the five arrays"""
    xg, phi, level, direction = K.snapshot_fields(cube)["plane_vertical"]
    snap = K.Snapshot(xg, cube.ien, phi, level, -1, direction, 750)
    quad = np.flatnonzero(snap.per_tet == 2)
    first = np.searchsorted(snap.tet, quad[quad >= 256][0])          # a quad's first triangle: cap = first + 1 splits it
    assert snap.tet[first] == snap.tet[first + 1]
    for cap in (0, 1, first + 1, snap.nf - 1, snap.nf):
        snapshot_launch(api, pool, xg, cube.ien, phi, level, -1, direction, 750, cap=cap)
    record("dfl_laser_surface_emit", "cap", 0.0, exact=True)


@pytest.mark.parametrize("nfs", K.NODES_NFS)
def test_surface_nodes(nfs, api, pool):
    """unode[0 .. nu) == np.unique over all 32 key bits, start[4 nfs] == nu, fslot == searchsorted, unode beyond nu untouched"""
    L = api.lib()
    ien, tet = K.nodes_case(nfs)
    unode, fslot = K.surface_nodes(ien, tet)
    n, nu = 4 * nfs, len(unode)
    assert nu < n or nfs == 1
    nbytes = L.dfl_laser_surface_temp_bytes(n, 0)
    s_ien, s_tet = pool.ints(ien), pool.ints(tet)
    key, key_out = pool.out(n, U32), pool.out(n, U32)
    rec, rec_out, flag, fs, un = (pool.out(n, I32) for _ in range(5))
    start, chunk = pool.out(n + 1, I32), pool.out(L.dfl_scan_num_chunks(n), I32)
    temp = pool.slot(np.full(nbytes, 0xA5, U8), 0, U8)
    L.dfl_laser_surface_nodes(nfs, s_ien.ptr, s_tet.ptr, key.ptr, key_out.ptr, rec.ptr, rec_out.ptr, flag.ptr, chunk.ptr, start.ptr,
                              fs.ptr, un.ptr, temp.ptr, nbytes, None)
    api.sync()
    untouched("nodes", s_ien, s_tet)
    for s in (key, key_out, rec, rec_out, flag, start, chunk, temp):
        s.check("scratch bands", ALL)
    assert start.get()[n] == nu
    exact(fs, fslot, "fslot", I32)
    got = un.check("unode beyond nu", np.arange(n) < nu)
    assert_bits(got[:nu].view(U32), unode, "unode", U32)
    record("dfl_laser_surface_nodes", "nfs=%d" % nfs, 0.0, exact=True)


# ======================================================================================================================
# Tier E: the surface deposit
# ======================================================================================================================
SURF_CASES = [(2, "one", 0), (2, "many", 5), (16, "many", 0), (16, "many", 5), (16, "one", 5), (64, "one", 0), (64, "many", 5),
              (256, "many", 5)]


@pytest.mark.parametrize("n,kind,nfb", SURF_CASES)
def test_surface_deposit(n, kind, nfb, api, pool):
    """the keys are dfl_laser_hit's, verified first; power[0 .. 4 nfs) cleared, then the slot sums in ascending 4 c + a bit
    for bit (one facet over 64 x 64 columns: runs of 4096 terms summed by one thread); energy accumulates where a slot was
    summed and keeps its bits elsewhere; columns without a hit and columns that hit a boundary record write nothing"""
    L = api.lib()
    d = K.surface_deposit_case(n, kind, nfb)
    b, nfs = d["b"], d["nfs"]
    s_cand = pool.slot(K.wall_records(d["cand_v"], d["ids"]))
    s_ck = pool.out(b.ncol, U64)
    L.dfl_laser_hit(nfb + nfs, s_cand.ptr, K.c_beam(b), 0.0, 2.0 ** 40, s_ck.ptr, None)
    api.sync()
    exact(s_ck, d["colkey"], "surface deposit: keys", U64)
    s_ck.image[:] = s_ck.dev.numpy()
    nbytes = L.dfl_laser_surface_temp_bytes(0, 4 * b.ncol)
    s_ij, s_t, s_fs, s_T = pool.ints(d["ij"]), pool.slot(d["t"]), pool.ints(d["fslot"]), pool.slot(d["col_T"])
    key, key_out, val = pool.out(4 * b.ncol, U64), pool.out(4 * b.ncol, U64), pool.out(4 * b.ncol)
    s_pow, s_en = pool.slot(np.full(4 * nfs + 2, 9.5)), pool.slot(np.r_[d["energy"], 3.25, 3.25])
    temp = pool.slot(np.full(nbytes, 0xA5, U8), 0, U8)
    power, energy, val_m, summed = K.surface_deposit(b, d["colkey"], nfb, nfs, d["cand_v"], d["ij"], d["t"], d["fslot"], d["eta_s"],
                                                     d["dt"], d["col_T"], d["energy"])
    what = "surface deposit n=%d %s nfb=%d" % (n, kind, nfb)
    for call in range(2):
        L.dfl_laser_surface_deposit(K.c_beam(b), s_ck.ptr, nfb, nfs, s_cand.ptr, s_ij.ptr, s_t.ptr, s_fs.ptr, d["eta_s"], d["dt"],
                                    s_T.ptr, key.ptr, key_out.ptr, val.ptr, s_pow.ptr, s_en.ptr, temp.ptr, nbytes, None)
        api.sync()
        exact(val, val_m, what + " val")
        exact(s_pow, np.r_[power, 9.5, 9.5], what + " power (the entries behind 4 nfs untouched)")
        exact(s_en, np.r_[energy, 3.25, 3.25], what + " energy, call %d" % call)
        energy = np.where(summed, energy + d["dt"] * power, energy)
        untouched(what, s_ck, s_cand, s_ij, s_t, s_fs, s_T)
        for s in (key, key_out, temp):
            s.check(what + " scratch bands", ALL)
    record("dfl_laser_surface_deposit", what, 0.0, exact=True)
