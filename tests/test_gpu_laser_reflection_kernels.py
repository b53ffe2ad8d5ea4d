"""Every launcher of the laser's reflections (csrc/k_laser_reflect.hip) alone, through ctypes with the structs passed by value.

The trace kernel runs on synthetic triangle lists with dyadic coordinates under a vertical beam, so every quantity is exact;
the reference is a float64 restatement of the header's rules, written in this file (next_hit64: Moeller-Trumbore facet by
facet in scalar float64; the absorptivity, the power chain and the tally partials) and asserted to agree with
laser_reflection_model.next_hit; only the ray origin (primary_origin) is shared with the model.  Cases: 0
and 1 facets; a ray parallel to a facet (det == 0); a ray through a shared edge and through a shared vertex, and two
coplanar hits at equal tau, where the tie goes to the lower index -- in two lanes, and in one lane 64 entries apart --; a
facet of the origin tet in the way; a facet much larger than the others; back faces; a ray that runs to max_bounce.  The
records and their bounce-major sum, the tally tree and the reflection list (count -> scan -> emit, with its clip at cap) are
compared bit for bit with restatements too.

Every array sits between guard bands (guarded_buffers.py); after each launch the bands, every const input and every entry
the call must not write are compared bit for bit.  No case aims at a fault: all indices are in range.

The cell grid: every trace case runs again through dfl_laser_reflect_trace_grid on the cell lists that
dfl_laser_reflect_cells_count / dfl_scan_counts / dfl_laser_reflect_cells_emit build (each cell's entries compared, as a
set, with a restatement), with 16 and 64 lanes per ray, on the grids of GRIDS: one cell; 32^3 cells of edge 1/4 whose planes
hold the rays of the scenes (a ray along a cell boundary, through cell corners); an anisotropic grid; and a small box that
holds none of the rays' starting points (a ray that starts outside every facet's cell).  The scenes' walls span many cells,
the big wall all of them.  Every output must have the bits of the trace over all of R."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import laser_kernel_model as K
import laser_reflection_model as rf
from guarded_buffers import ALL, I32, U64, Pool, assert_bits, sent

pytestmark = pytest.mark.gpu

F64 = np.float64
vp, f64, i32, i64 = C.c_void_p, C.c_double, C.c_int32, C.c_int64
Beam = K.CBeam
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)
REC_BITS, NO_REC = 22, 1 << 48

class Grid3(C.Structure):
    _fields_ = [("lo", f64 * 3), ("inv", f64 * 3), ("n", i32 * 3)]


SIG = {
    "dfl_scan_num_chunks": (i32, [i32]),
    "dfl_tets_per_block": (i32, []),
    "dfl_scan_counts": (None, [i32, vp, vp, vp, vp]),
    "dfl_laser_reflect_temp_bytes": (i64, [i32]),
    "dfl_laser_reflect_count": (None, [i32, vp, vp, vp, i32, f64, vp, vp]),
    "dfl_laser_reflect_emit": (None, [i32, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp, i32, vp]),
    "dfl_laser_reflect_trace": (None, [Beam, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, vp]),
    "dfl_laser_reflect_cells_count": (None, [i32, vp, None, vp, vp]),
    "dfl_laser_reflect_cells_emit": (None, [i32, vp, None, vp, vp, vp, i32, vp]),
    "dfl_laser_reflect_trace_grid": (None, [Beam, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp,
                                            None, vp, vp, i32, vp, vp]),
    "dfl_laser_reflect_deposit": (None, [i32, vp, vp, vp, i32, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dfl_laser_reflect_tally": (None, [i32, i32, vp, vp, vp, vp, vp]),
}


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as Ap
    L = Ap.lib()                                                    # raises if the HIP library is missing: no fallback
    for name, (res, args) in SIG.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, [Grid3 if a is None else a for a in args]
    return Ap


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


def exact(slot, want, what, dtype=F64):
    got = slot.check(what, ALL)
    assert_bits(got[:np.size(want)], np.ravel(want), what, dtype)
    return got


def untouched(what, *slots):
    for s in slots:
        s.check(what + ": an array the call must not write changed")


def test_every_launcher_is_declared_and_called():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dedflow_amd", "csrc", "k_laser_reflect.hip")
    text = open(src).read()
    names = re.findall(r"^(?:void|I|int64_t) (dfl_\w+)\(", text[text.index('extern "C"'):], re.M)
    assert len(names) == 9 and not [n for n in names if n not in SIG]
    mine = open(os.path.abspath(__file__)).read()
    for n in names:
        assert re.search(r"\.%s\(" % n, mine), n


# ---- the trace kernel ---------------------------------------------------------------------------------------------------------
class Scene:
    """a reflection list by hand: triangles [nr, 9], a tet id (ascending) and a gradient each; `cands` are the indices of R
    that are the beam's candidates, in R's order"""

    def __init__(self, tris, tets, grads, cands):
        self.F = np.asarray(tris, F64).reshape(-1, 9)
        self.tet = np.asarray(tets, np.int64)
        self.g = np.asarray(grads, F64).reshape(-1, 3)
        self.cands = np.asarray(cands, np.int64)
        assert (np.diff(self.tet) >= 0).all() and len(self.tet) == len(self.F) == len(self.g)


def absorptivity64(model, eta_s, eps, d, g):
    if model == 0:
        return eta_s
    c = abs(rf.dot(d, g)) / np.sqrt(rf.dot(g, g) * rf.dot(d, d))
    return float(rf.absorptivity(1, eta_s, eps, np.asarray(c, F64)))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def next_hit64(sc, side, X, d, t0):
    """the header's next hit, facet by facet in scalar float64: written here from include/dedflow.h, not shared with
    laser_reflection_model.next_hit (which the GPU tests of the whole step use)"""
    best, bk, buv = np.inf, -1, (0.0, 0.0)
    with np.errstate(all="ignore"):
        for k in range(len(sc.F)):
            if sc.tet[k] == t0 or not (side * _dot(sc.g[k], d) > 0.0):
                continue
            A, B, Cc = sc.F[k, 0:3], sc.F[k, 3:6], sc.F[k, 6:9]
            e1, e2 = B - A, Cc - A
            p = _cross(d, e2)
            det = _dot(e1, p)
            if det == 0.0:
                continue
            s = X - A
            u = _dot(s, p) / det
            q = _cross(s, e1)
            v = _dot(d, q) / det
            tau = _dot(e2, q) / det
            if u >= 0.0 and v >= 0.0 and u + v <= 1.0 and tau > 0.0 and (bk < 0 or tau < best):   # ascending k: ties keep the lower
                best, bk, buv = tau, k, (u, v)
    return bk, buv[0], buv[1], best


def trace64(fr, sc, primary, col_T, side, model, mb, eta_s, eps, part):
    """float64 restatement of lr_trace_kernel; primary[c] = index into sc.cands or -1"""
    nb, nc = mb + 1, fr.ncol
    facet, ab = np.full((nb, nc), -1, np.int64), np.zeros((nb, nc))
    w = np.zeros((nb, nc, 3))
    end = np.zeros((2, nc))
    part = part.copy().reshape(6, nc)
    visited = {}
    for c in range(nc):
        if primary[c] < 0:
            continue
        k = int(sc.cands[primary[c]])
        wk, X = rf.primary_origin(fr.beam, fr.o, sc.F[k].reshape(3, 3), c)
        d = fr.dir.copy()
        p, sub, path = col_T[c], 0.0, []
        for b in range(nb):
            g = sc.g[k]
            a = absorptivity64(model, eta_s, eps, d, g) * p
            p = p - a
            sub = a if b == 0 else sub + a
            facet[b, c], ab[b, c], w[b, c] = k, a, wk
            path.append(k)
            if b == mb:
                end[1, c] = p
                break
            d = d - ((2.0 * rf.dot(d, g)) / rf.dot(g, g)) * g
            k2, u, v, _ = next_hit64(sc, side, X, d, sc.tet[k])
            assert k2 == rf.next_hit(sc, side, X, d, sc.tet[k])[0]
            if k2 < 0:
                end[0, c] = p
                break
            wk = np.array([(1.0 - u) - v, u, v])
            F = sc.F[k2]
            X = (wk[0] * F[0:3] + wk[1] * F[3:6]) + wk[2] * F[6:9]
            k = k2
        if not (model == 0 and len(path) == 1 and mb >= 1):         # (a model-0 ray without a second facet leaves them)
            part[3, c], part[4, c] = sub, end[0, c] + end[1, c]
        visited[c] = path
    return facet, ab, w, end, part.reshape(-1), visited


def run_trace(api, pool, fr, sc, primary, side=-1, model=0, mb=3, eta_s=0.75, eps=0.25):
    nc, nb, nr, nfs = fr.ncol, mb + 1, len(sc.F), len(sc.cands)
    cand = (K.CWallTri * max(nfs, 1))()
    for q, k in enumerate(sc.cands):
        cand[q].v[:] = list(sc.F[k])
        cand[q].node[:] = [-1, -1, -1]
        cand[q].id = int(-2 - sc.tet[k])
    cand_d = pool.slot(np.frombuffer(cand, np.uint8).copy(), 0, np.uint8)
    key = np.full(nc, NO_HIT, np.uint64)
    for c in range(nc):
        if primary[c] >= 0:
            key[c] = (np.uint64(1000 + c) << np.uint64(24)) | np.uint64(primary[c])
    col_T = 1.0 + np.arange(nc) / 64.0                              # dyadic
    part0 = np.arange(6 * nc, dtype=F64) + 0.5
    s = dict(key=pool.slot(key, 0, U64), ftet=pool.ints(sc.tet[sc.cands] if nfs else [0]), F=pool.slot(sc.F if nr else np.zeros(9)),
             tet=pool.ints(sc.tet if nr else [0]), g=pool.slot(sc.g if nr else np.zeros(3)), T=pool.slot(col_T))
    o = dict(facet=pool.out(nb * nc, I32), ab=pool.out(nb * nc), w=pool.out(3 * nb * nc), end=pool.out(2 * nc), part=pool.slot(part0))
    api.lib().dfl_laser_reflect_trace(K.c_beam(fr), s["key"].ptr, 0, nfs, cand_d.ptr, s["ftet"].ptr, nr, s["F"].ptr, s["tet"].ptr,
                                      s["g"].ptr, side, model, mb, eta_s, eps, s["T"].ptr, o["facet"].ptr, o["ab"].ptr, o["w"].ptr,
                                      o["end"].ptr, o["part"].ptr, None)
    api.sync()
    facet, ab, w, end, part, visited = trace64(fr, sc, primary, col_T, side, model, mb, eta_s, eps, part0)
    untouched("trace", cand_d, *s.values())
    exact(o["facet"], facet, "hit_facet", I32)
    exact(o["ab"], ab, "hit_abs")
    exact(o["w"], w, "hit_w")
    exact(o["end"], end, "ray_end")
    written = np.zeros((6, nc), bool)
    written[3:5, [c for c, q in visited.items() if not (model == 0 and len(q) == 1)]] = True
    got = o["part"].check("part", written.reshape(-1))
    assert_bits(got, part, "part")
    if nr:
        for gname, (glo, ghi, gn) in GRIDS.items():
            gr, start, entry = build_cells(api, pool, sc, glo, ghi, gn)
            for group in (16, 64):
                for q in o.values():
                    q.reset()
                vis = pool.out(nc)
                api.lib().dfl_laser_reflect_trace_grid(K.c_beam(fr), s["key"].ptr, 0, nfs, cand_d.ptr, s["ftet"].ptr, nr, s["F"].ptr,
                                                       s["tet"].ptr, s["g"].ptr, side, model, mb, eta_s, eps, s["T"].ptr, o["facet"].ptr,
                                                       o["ab"].ptr, o["w"].ptr, o["end"].ptr, o["part"].ptr, gr, start.ptr, entry.ptr, group,
                                                       vis.ptr, None)
                api.sync()
                what = f"grid {gname}, {group} lanes: "
                untouched(what + "trace", cand_d, start, entry, *s.values())
                exact(o["facet"], facet, what + "hit_facet", I32)
                exact(o["ab"], ab, what + "hit_abs")
                exact(o["w"], w, what + "hit_w")
                exact(o["end"], end, what + "ray_end")
                assert_bits(o["part"].check(what + "part", written.reshape(-1)), part, what + "part")
                v = vis.check(what + "visited", ALL)
                assert (v >= 0).all() and (v[primary < 0] == 0).all() and (v[[c for c, q in visited.items() if len(q) > 1]] > 0).all()
    return visited, facet, end


GRIDS = {"one cell": ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0), (1, 1, 1)),
         "planes on the rays": ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0), (32, 32, 32)),
         "anisotropic": ((-3.0, -5.0, -1.0), (5.0, 7.0, 9.0), (5, 17, 3)),
         "beside the starts": ((-3.0, -1.0, -1.0), (-0.5, 3.0, 3.0), (4, 8, 8))}


def build_cells(api, pool, sc, lo, hi, n):
    """count -> scan -> emit of the facets into the cells; each cell's entries against a restatement, as a set"""
    L = api.lib()
    lo, hi, n = np.array(lo), np.array(hi), np.array(n)
    inv = n / (hi - lo)                                             # dyadic for the grids used where it matters
    gr = Grid3((f64 * 3)(*lo), (f64 * 3)(*inv), (i32 * 3)(*[int(q) for q in n]))
    nr, ncell = len(sc.F), int(n.prod())
    V = sc.F.reshape(nr, 3, 3)
    with np.errstate(invalid="ignore"):
        c0 = np.clip(np.floor((V.min(axis=1) - lo) * inv), 0, n - 1).astype(np.int64)
        c1 = np.clip(np.floor((V.max(axis=1) - lo) * inv), 0, n - 1).astype(np.int64)
    cells = [[] for _ in range(ncell)]
    for f in range(nr):
        for z in range(c0[f, 2], c1[f, 2] + 1):
            for y in range(c0[f, 1], c1[f, 1] + 1):
                for x in range(c0[f, 0], c1[f, 0] + 1):
                    cells[(z * n[1] + y) * n[0] + x].append(f)
    counts = np.array([len(c) for c in cells])
    F = pool.slot(sc.F)
    cnt = pool.slot(np.zeros(ncell, I32), 0, I32)
    start, chunk = pool.out(ncell + 1, I32), pool.out(L.dfl_scan_num_chunks(ncell), I32)
    L.dfl_laser_reflect_cells_count(nr, F.ptr, gr, cnt.ptr, None)
    api.sync()
    exact(cnt, counts, "cell counts", I32)
    L.dfl_scan_counts(ncell, cnt.ptr, chunk.ptr, start.ptr, None)
    api.sync()
    st = np.concatenate([[0], np.cumsum(counts)])
    exact(start, st, "cell starts", I32)
    start.reset(st)                                                 # (its image: the trace must leave it alone)
    entry = pool.out(st[-1], I32)
    L.dfl_laser_reflect_cells_emit(nr, F.ptr, gr, start.ptr, cnt.ptr, entry.ptr, int(st[-1]), None)
    api.sync()
    untouched("cells", F, start)
    e = entry.check("cell entries", ALL)
    for c in range(ncell):
        assert sorted(e[st[c]:st[c + 1]].tolist()) == cells[c], c
    entry.reset(e[:max(int(st[-1]), 1)])
    return gr, start, entry


def frame(n=4):
    # vertical beam: e1 = (1, 0, 0), e2 = (0, -1, 0); column centres at odd multiples of 1/4 around the origin's (x, y)
    return K.Frame((0.0, 0.0, -1.0), (1.0, 1.0, 8.0), 0.5, n)


UP = (-1.0, 0.0, 1.0)                                               # g of the floor z = x: a vertical ray leaves along -x


def floor(y0=-4.0, y1=6.0):
    """the plane z = x over x in [0, 4]: two triangles of tet 0"""
    a, b, c, d = (0.0, y0, 0.0), (4.0, y0, 4.0), (4.0, y1, 4.0), (0.0, y1, 0.0)
    return [a + b + c, a + c + d]


def wall(x, ylo, yhi, zlo=-8.0, zhi=8.0):
    """one triangle in the plane x = const that covers y in (ylo, yhi) at z = 0"""
    return (x, ylo, zlo) + (x, yhi, zlo) + (x, (ylo + yhi) / 2, zhi + (zhi - zlo))


def primaries(fr, sc):
    """per column the first candidate (index into sc.cands) whose projection holds the centre, by the float64 tri_hit"""
    prim = np.full(fr.ncol, -1, np.int64)
    cu, cv = fr.beam.centres()
    for q in range(len(sc.cands) - 1, -1, -1):
        u, v, s = K.project(sc.F[sc.cands[q]].reshape(3, 3), fr)
        hit, _, _ = K.tri_hit(u, v, s, cu, cv)
        prim[hit] = q
    return prim


def test_no_facets_and_one_facet(api, pool):
    fr = frame()
    empty = Scene(np.zeros((0, 9)), [], np.zeros((0, 3)), [])
    visited, facet, end = run_trace(api, pool, fr, empty, np.full(fr.ncol, -1))
    assert not visited and (facet == -1).all() and not end.any()
    one = Scene(floor()[:1], [0], [UP], [0])
    prim = primaries(fr, one)
    assert 0 < (prim >= 0).sum() < fr.ncol
    visited, facet, end = run_trace(api, pool, fr, one, prim, model=1)
    assert all(p == [0] for p in visited.values()) and (end[0][prim >= 0] > 0).all() and not end[1].any()


def test_ties_go_to_the_lower_index(api, pool):
    """after the floor the ray of column centre (cx, cy) runs along -x at height z = cx.  Walls in x = -1: two triangles that
    share the edge y = 1.25 (a column centre), three that share a vertex on a ray, two coplanar overlapping ones; the lower
    index wins whether the two sit in different lanes or 64 entries apart in one lane"""
    fr = frame()
    G = (1.0, 0.0, 0.0)
    for pad in (0, 63):                                             # pad: misses between the two, so they meet in one lane
        filler = [wall(-1.0, 40.0 + q, 41.0 + q) for q in range(pad)]
        edge_lo = (-1.0, 1.25, -8.0) + (-1.0, 1.25, 24.0) + (-1.0, -3.0, 0.0)     # covers y < 1.25
        edge_hi = (-1.0, 1.25, -8.0) + (-1.0, 1.25, 24.0) + (-1.0, 5.0, 0.0)      # covers y > 1.25
        tris = floor() + [edge_hi] + filler + [edge_lo, wall(-1.0, -8.0, 8.0)]
        nr = len(tris)
        sc = Scene(tris, [0, 0] + list(range(1, nr - 1)), [UP, UP] + [G] * (nr - 2), [0, 1])
        prim = primaries(fr, sc)
        visited, facet, _ = run_trace(api, pool, fr, sc, prim, mb=1)
        cu, cv = fr.beam.centres()
        on_edge = [c for c in visited if fr.o[1] - cv[c] == 1.25]  # e2 = (0, -1, 0): y = o_y - cv
        assert on_edge and all(visited[c] == [visited[c][0], 2] for c in on_edge)       # edge_hi, the lower index of the three
        below = [c for c in visited if fr.o[1] - cv[c] < 1.25]
        assert below and all(visited[c][1] == nr - 2 for c in below)                    # edge_lo before the big wall behind it
    # a shared vertex on the ray of column (cx, cy) = (1.25, 0.75): the apex of three triangles, z = cx = 1.25 there
    apex = (-1.0, 0.75, 1.25)
    fan = [apex + (-1.0, -8.0, 9.0) + (-1.0, 9.0, 9.0), apex + (-1.0, 9.0, 9.0) + (-1.0, 9.0, -9.0), apex + (-1.0, 9.0, -9.0) + (-1.0, -8.0, 9.0)]
    sc = Scene(floor() + fan, [0, 0, 1, 2, 3], [UP, UP, G, G, G], [0, 1])
    visited, _, _ = run_trace(api, pool, fr, sc, primaries(fr, sc), mb=1)
    cu, cv = fr.beam.centres()
    at = [c for c in visited if cu[c] + fr.o[0] == 1.25 and fr.o[1] - cv[c] == 0.75]
    assert len(at) == 1 and visited[at[0]][1] == 2                  # all three hold the vertex; the lowest index


def test_parallel_facets_back_faces_and_the_origin_tet(api, pool):
    fr = frame()
    G = (1.0, 0.0, 0.0)
    lid = (-2.0, -8.0, 0.75) + (9.0, -8.0, 0.75) + (0.0, 30.0, 0.75)      # horizontal, at the height of a ray: det == 0 exactly
    back = wall(-0.5, -8.0, 8.0)                                    # g along -x: the ray does not enter the metal there
    own = wall(-0.25, -8.0, 8.0)                                    # a facet of the floor's tet in the way
    big = wall(-2.0, -512.0, 512.0, -512.0, 512.0)                  # much larger than the others
    tris = floor() + [own, lid, back, big]
    sc = Scene(tris, [0, 0, 0, 1, 2, 3], [UP, UP, G, (1.0, 0.0, 1.0), (-1.0, 0.0, 0.0), G], [0, 1])
    visited, facet, end = run_trace(api, pool, fr, sc, primaries(fr, sc), mb=1, model=1)
    assert visited and all(p[1] == 5 for p in visited.values())
    nan_g = Scene(tris, [0, 0, 0, 1, 2, 3], [UP, UP, G, (1.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (np.nan, 0.0, 0.0)], [0, 1])
    visited, _, end = run_trace(api, pool, fr, nan_g, primaries(fr, nan_g), mb=1)
    assert all(len(p) == 1 for p in visited.values())               # a NaN is not greater: nothing left to hit


@pytest.mark.parametrize("model,mb", [(0, 1), (0, 8), (1, 4), (1, 8)])
def test_a_ray_between_two_mirrors_runs_to_max_bounce(api, pool, model, mb):
    """floor -> wall x = -1 -> floor (from inside the groove) -> ... : whatever the path, it is the restatement's, bit for
    bit; under a cover z = 6 facing down the rays keep going until max_bounce"""
    fr = frame()
    cover = (-64.0, -64.0, 6.0) + (64.0, -64.0, 6.0) + (0.0, 128.0, 6.0)
    tris = floor() + [wall(-1.0, -8.0, 8.0), cover]
    sc = Scene(tris, [0, 0, 1, 2], [UP, UP, (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)], [0, 1])
    visited, facet, end = run_trace(api, pool, fr, sc, primaries(fr, sc), model=model, mb=mb, eps=0.25)
    assert visited and all(p[:4] == [p[0], 2, p[0], 3][:len(p)] for p in visited.values())
    if mb == 1:
        assert (end[1][[c for c in visited]] > 0).all() and not end[0].any()


# ---- records, sum, tally ------------------------------------------------------------------------------------------------------
def test_records_and_their_bounce_major_sum(api, pool):
    rng = np.random.default_rng(11)
    ncol, nb, nr = 300, 3, 40
    nrec = nb * ncol
    facet = rng.integers(-1, nr, nrec)
    facet[rng.random(nrec) < 0.5] = -1
    ab = np.where(facet >= 0, rng.integers(1, 64, nrec) / 8.0, 0.0)
    w = rng.integers(0, 9, (nrec, 3)) / 8.0
    rt = rng.integers(1, 8, (nr, 3)) / 8.0
    ij = np.zeros(nr, np.int64)
    for k in range(nr):
        for v in range(3):
            i = rng.integers(0, 4)
            j = (i + rng.integers(1, 4)) % 4
            ij[k] |= (i | j << 2) << (4 * v)
    nslot = 4 * nr
    fslot = rng.integers(0, 25, nslot)                              # few slots: long runs across bounces
    dt = 0.25
    power0, energy0 = np.full(nslot, 7.0), rng.integers(0, 16, nslot) / 4.0
    # restatement: lambda and the records, then per slot the sum from +0.0 in ascending record id
    val = np.zeros(4 * nrec)
    slot_of = np.full(4 * nrec, -1, np.int64)
    for o in np.nonzero(facet >= 0)[0]:
        k, e = facet[o], ij[facet[o]]
        for a in range(4):
            c = [(1.0 - rt[k, v]) if a == ((e >> (4 * v)) & 3) else (rt[k, v] if a == ((e >> (4 * v + 2)) & 3) else 0.0) for v in range(3)]
            lam = (w[o, 0] * c[0] + w[o, 1] * c[1]) + w[o, 2] * c[2]
            val[4 * o + a], slot_of[4 * o + a] = ab[o] * lam, fslot[4 * k + a]
    power, energy = np.zeros(nslot), energy0.copy()
    for s in np.unique(slot_of[slot_of >= 0]):
        acc = 0.0
        for r in np.nonzero(slot_of == s)[0]:
            acc += val[r]
        power[s] = acc
        energy[s] = energy0[s] + dt * acc
    L = api.lib()
    tb = L.dfl_laser_reflect_temp_bytes(4 * nrec)
    s = dict(facet=pool.ints(facet), ab=pool.slot(ab), w=pool.slot(w), ij=pool.ints(ij), rt=pool.slot(rt), fslot=pool.ints(fslot))
    key, key_out, vals = pool.out(4 * nrec, U64), pool.out(4 * nrec, U64), pool.out(4 * nrec)
    pw, en = pool.slot(power0), pool.slot(energy0)
    temp = pool.out(tb // 8 + 2)
    L.dfl_laser_reflect_deposit(nrec, s["facet"].ptr, s["ab"].ptr, s["w"].ptr, nr, s["ij"].ptr, s["rt"].ptr, s["fslot"].ptr, dt, key.ptr,
                                key_out.ptr, vals.ptr, pw.ptr, en.ptr, temp.ptr, tb, None)
    api.sync()
    untouched("deposit", *s.values())
    exact(vals, val, "record values")
    want_key = np.where(slot_of >= 0, (slot_of.astype(np.uint64) << np.uint64(REC_BITS)) | np.arange(4 * nrec, dtype=np.uint64),
                        np.uint64(NO_REC))
    exact(key_out, np.sort(want_key), "sorted keys", U64)
    exact(pw, power, "power")
    exact(en, energy, "energy")
    # no records at all: power is cleared, energy stays
    pw.reset(power0)
    en.reset(energy0)
    s["facet"].reset(np.full(nrec, -1))
    L.dfl_laser_reflect_deposit(nrec, s["facet"].ptr, s["ab"].ptr, s["w"].ptr, nr, s["ij"].ptr, s["rt"].ptr, s["fslot"].ptr, dt, key.ptr,
                                key_out.ptr, vals.ptr, pw.ptr, en.ptr, temp.ptr, tb, None)
    api.sync()
    exact(pw, np.zeros(nslot), "power without records")
    en.check("energy without records")


def _tree(cols):
    """thread t sums columns t, t + 256, ...; xor shuffles in the wave; waves 1, 2, 3 into wave 0 in that order"""
    acc = np.zeros(256)
    for c in range(len(cols)):
        acc[c % 256] += cols[c]
    lanes = acc.reshape(4, 64).copy()
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ off]
    return ((lanes[0, 0] + lanes[1, 0]) + lanes[2, 0]) + lanes[3, 0]


@pytest.mark.parametrize("ncol,mb", [(16, 1), (324, 8), (700, 5)])
def test_tally_tree(api, pool, ncol, mb):
    rng = np.random.default_rng(ncol)
    nb = mb + 1
    facet = rng.integers(-1, 5, (nb, ncol))
    ab = np.where(facet >= 0, rng.random((nb, ncol)), 0.0)
    end = rng.random((2, ncol))
    want = np.zeros(20)
    for b in range(nb):
        want[b] = _tree(ab[b])
        want[11 + b] = _tree((facet[b] >= 0).astype(F64))
    want[9], want[10] = _tree(end[0]), _tree(end[1])
    s = (pool.ints(facet), pool.slot(ab), pool.slot(end))
    out = pool.out(20)
    api.lib().dfl_laser_reflect_tally(ncol, mb, s[0].ptr, s[1].ptr, s[2].ptr, out.ptr, None)
    api.sync()
    untouched("tally", *s)
    exact(out, want, "tally")
    assert (want[11:11 + nb] == (facet >= 0).sum(axis=1)).all()


# ---- the reflection list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
def test_count_scan_emit(api, pool, clip):
    from dedflow_amd.meshgen import kuhn_cube
    m = kuhn_cube(5, jitter=0.2)
    phi = rf.groove_phi(m.xg)
    phi[7] = np.nan                                                 # its tets drop out: a NaN gradient is not > 0
    R = rf.Reflectors(m.xg, m.ien, phi, 0.0)
    N, T, nr = m.num_node, m.num_tet, len(R.tet)                    # (m.ien is flat: 4 T entries)
    assert nr > 100 and 4 * T == np.size(m.ien)
    L = api.lib()
    per = L.dfl_tets_per_block()
    nblk = (T + per - 1) // per
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = phi
    s = dict(ien=pool.ints(m.ien), xg=pool.slot(m.xg), w=pool.slot(w))
    cnt, base, chunk = pool.out(nblk, I32), pool.out(nblk + 1, I32), pool.out(L.dfl_scan_num_chunks(nblk), I32)
    L.dfl_laser_reflect_count(T, s["ien"].ptr, s["xg"].ptr, s["w"].ptr, N, 0.0, cnt.ptr, None)
    api.sync()
    per_blk = np.bincount(R.tet // per, minlength=nblk)
    exact(cnt, per_blk, "block counts", I32)
    L.dfl_scan_counts(nblk, cnt.ptr, chunk.ptr, base.ptr, None)
    api.sync()
    exact(base, np.concatenate([[0], np.cumsum(per_blk)]), "block bases", I32)
    cap = nr - 37 if clip else nr
    o = dict(F=pool.out(9 * cap), tet=pool.out(cap, I32), g=pool.out(3 * cap), ij=pool.out(cap, I32), t=pool.out(3 * cap))
    L.dfl_laser_reflect_emit(T, s["ien"].ptr, s["xg"].ptr, s["w"].ptr, N, 0.0, base.ptr, o["F"].ptr, o["tet"].ptr, o["g"].ptr, o["ij"].ptr,
                             o["t"].ptr, cap, None)
    api.sync()
    untouched("emit", *s.values())
    exact(base, np.concatenate([[0], np.cumsum(per_blk)]), "block bases after the emit", I32)
    ij = sum(((R.i[:, v] | R.j[:, v] << 2) << (4 * v)) for v in range(3))
    exact(o["F"], R.F[:cap], "facets")
    exact(o["tet"], R.tet[:cap], "tets", I32)
    exact(o["g"], R.g[:cap], "gradients")
    exact(o["ij"], ij[:cap], "edges", I32)
    exact(o["t"], R.t[:cap], "t")
