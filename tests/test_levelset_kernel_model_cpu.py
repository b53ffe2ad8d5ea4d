"""The model of the level-set geometry launchers (tests/levelset_kernel_model.py) against references that do not share its
decomposition, and the properties of its decks that tests/test_gpu_levelset_kernels.py rests on.  No GPU.

  volumes    the float64 restatement (redistance_model.tet_volumes: the header's corner / wedge decomposition) against the
             divided-difference closed form in np.longdouble on orbit, orbit-shared and isolation: c_vol = max |v - ref| /
             (u V K), every tet kept
  distances  the float64 dist2 (the header's seven candidates) against the Voronoi-region method in np.longdouble on triangles
             with every angle in [20, 160] degrees: c_dist = max |d^2 - ref| / (u max_v |p - v|^2), every pair kept; degenerate
             triangles only against the restatement's own longdouble form
  the tree   on exact integers any order gives the same bits (np.sum, np.max); on random values within (log2 n) u sum |v|
  the decks  192 negative determinants, the 16 x 24 (mask, order) pairs, 1 to 4 nodes on the level, dyadic exactness
  coverage   every dfl_redistance_* and dfl_volume_* launcher of include/dedflow_kernels.h is named by the GPU module

c_vol and c_dist go to the file named by DFL_PARITY_OUT (profiles/levelset_kernel_parity.jsonl is such a run)."""
import os
import re

import numpy as np
import pytest

import levelset_kernel_model as M
import redistance_model as rm
from guarded_buffers import Recorder

F64, LD, U = np.float64, np.longdouble, M.U
HERE = os.path.dirname(os.path.abspath(__file__))
record = Recorder("a")
needs_ld = pytest.mark.skipif(not M.HAVE_EXTENDED, reason=M.EXTENDED_REASON)


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    record.write()


# ---- the independent references ----------------------------------------------------------------------------------------------
@needs_ld
def test_closed_form_is_a_volume():
    """four positive nodes: exactly V (the third divided difference of t^3 is 1); {f > 0} and {-f > 0} fill the tet; one positive
    node: V t1 t2 t3"""
    d = M.orbit()
    v, V, K = M.closed_form_volume(d.xg, d.ien, d.phi, d.level)
    mask = M.tet_masks(d.ien, d.phi, d.level)
    assert np.abs(v[mask == 15] - V[mask == 15]).max() <= 64 * np.finfo(LD).eps * V.max()
    assert (v[mask == 0] == 0).all()
    w, _, _ = M.closed_form_volume(d.xg, d.ien, 2.0 * d.level - d.phi, d.level)
    assert np.abs(v + w - V).max() <= 64 * np.finfo(LD).eps * V.max()
    e = int(np.flatnonzero(mask == 1)[0])
    f = (d.phi[d.ien[e]] - d.level).astype(LD)
    t = [f[0] / (f[0] - f[j]) for j in (1, 2, 3)]
    assert abs(v[e] - V[e] * t[0] * t[1] * t[2]) <= 64 * np.finfo(LD).eps * V[e]


@needs_ld
def test_restatement_against_the_closed_form():
    c, n = M.c_vol()
    assert n == 384 + 384 + 384                      # every tet of the three decks
    d = M.orbit()
    ref, V, K = M.closed_form_volume(d.xg, d.ien, d.phi, d.level)
    v64 = rm.tet_volumes(d.xg, d.ien, d.phi, d.level)[0]
    vld = rm.tet_volumes(d.xg, d.ien, d.phi, d.level, dtype=LD)[0]
    plain = float((np.abs(v64.astype(LD) - ref) / V).max())
    worst_ld = float((np.abs(vld - ref) / V).max())
    print(f"c_vol = {c:.3f} over {n} tets; orbit: max |v - ref| / V float64 {plain:.2e}, longdouble {worst_ld:.2e}")
    record("restatement", "c_vol", 0.0, c=c, tets=n, orbit_abs_over_V=plain, orbit_longdouble_over_V=worst_ld)
    # every crossing point carries u |x| of the tet's own size, a corner of relative edge t >= 0.1 / 1.2 sees that 1 / t times
    # larger, three edges and three determinants of ~25 operations: a constant of some tens, at the most a few hundred; a
    # wrong sub-tet is an error of order 1 / u
    assert 0.0 < c < 512.0
    assert worst_ld < 64.0 * float(np.finfo(LD).eps)


@needs_ld
def test_dist2_against_the_region_method():
    c, n = M.c_dist()
    F, P = M.well_shaped(n)
    ang = M.triangle_angles(F)
    assert n == 4000 and len(F) == n and ang.min() >= 20.0 - 1e-9 and ang.max() <= 160.0 + 1e-9
    edge = np.sqrt(((F[:, 3:6] - F[:, 0:3]) ** 2).sum(axis=1))
    far = np.sqrt(((P - (F[:, 0:3] + F[:, 3:6] + F[:, 6:9]) / 3.0) ** 2).sum(axis=1))
    assert (far <= 2.0 * edge * (1 + 1e-12)).all()
    # every region is met: vertex, edge and face
    ref = np.array([M.region_dist2(P[i], F[i]) for i in range(400)], LD)
    vert = np.array([min(((P[i] - F[i, 3 * v:3 * v + 3]) ** 2).sum() for v in range(3)) for i in range(400)])
    assert (np.abs(ref - vert) < 1e-13).any() and (ref < 0.5 * vert).any()
    print(f"c_dist = {c:.3f} over {n} point-triangle pairs")
    record("restatement", "c_dist", 0.0, c=c, pairs=n)
    assert 0.0 < c < 32.0


@needs_ld
def test_degenerate_triangles_against_the_restatement():
    """zero area and coincident vertices: the float64 dist2 against its own longdouble form; the result is a distance to a
    segment or a point, so 16 u max_v |p - v|^2 holds"""
    rng = np.random.default_rng(2)
    A, B = rng.uniform(-1, 1, (200, 3)), rng.uniform(-1, 1, (200, 3))
    s = rng.uniform(0, 1, (200, 1))
    F = np.concatenate([np.c_[A, B, A + s * (B - A)], np.c_[A, A, B], np.c_[A, A, A]])
    P = rng.uniform(-1.5, 1.5, (len(F), 3))
    d64, dld = rm.dist2(P, F), rm.dist2(P.astype(LD), F.astype(LD))
    assert (np.abs(d64.astype(LD) - dld) <= 16 * U * M.dist_scale(P, F)).all()
    assert np.allclose(d64[400:], ((P[400:] - A) ** 2).sum(axis=1), rtol=1e-15, atol=0.0)      # three equal vertices: a point


# ---- the tree ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_block_reduce_on_integers(n):
    rng = np.random.default_rng(n)
    part = np.stack([rng.integers(-1000, 1000, n), rng.integers(0, 10 ** 6, n)], axis=1).astype(F64)
    out = M.block_reduce(part, M.merge_pair)
    assert out[0] == part[:, 0].sum() and out[1] == part[:, 1].max()
    assert M.block_reduce(part[:, :1], M.merge_sum)[0] == part[:, 0].sum()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 2047, 2048, 2049, 2 ** 21 - 1, 2 ** 21 + 2049])
def test_node_stage1_on_integers(N):
    q = np.random.default_rng(N % 1000).integers(-8, 9, N).astype(F64)
    part, out = M.node_sum(q)
    assert len(part) == min(-(-N // 2048), 1024) and out[0] == q.sum()
    chg = q.copy()
    chg[::7] = -1.0
    chg[N // 2] = np.nan
    part2, out2 = M.node_stats(chg)
    with np.errstate(invalid="ignore"):
        valid = chg >= 0
    assert out2[0] == valid.sum() and out2[1] == (chg[valid].max() if valid.any() else 0.0)


def test_tree_order_is_the_stated_one():
    """256 values whose sum depends on the order: the tree differs from the left-to-right sum and equals the hand-written
    butterfly; waves 1, 2, 3 are merged into wave 0 in that order"""
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 1, 256) * 10.0 ** rng.integers(-8, 8, 256)
    got = M.block_tree(v[:, None], M.merge_sum)[0]
    w = v.reshape(4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ off]
    assert got == ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
    assert got != ((w[0, 0] + w[3, 0]) + w[2, 0]) + w[1, 0] and got != np.cumsum(v)[-1]    # (these values tell the orders apart)
    assert abs(LD(got) - v.astype(LD).sum()) <= 8 * U * np.abs(v).sum()


@needs_ld
@pytest.mark.parametrize("n", [256, 1000, 5000])
def test_tree_sum_error_bound(n):
    v = np.random.default_rng(n).normal(size=(n, 1))
    got = M.block_reduce(v, M.merge_sum)[0]
    assert abs(LD(got) - v.astype(LD).sum()) <= np.ceil(np.log2(n)) * U * np.abs(v).sum()
    got = M.node_sum(v[:, 0])[1][0]
    assert abs(LD(got) - v.astype(LD).sum()) <= np.ceil(np.log2(n)) * U * np.abs(v).sum()


# ---- the cell grid -----------------------------------------------------------------------------------------------------------
def test_cell_grid_model():
    g = M.make_grid([0.0, 0.0, 0.0], 4.0, (4, 2, 3))
    assert M.cell(-1.0, 0.0, 4.0, 4) == 0 and M.cell(0.25, 0.0, 4.0, 4) == 1 and M.cell(0.2499999, 0.0, 4.0, 4) == 0 and M.cell(9.0, 0.0, 4.0, 4) == 3
    F = np.array([0.1, 0.1, 0.1, 0.6, 0.1, 0.1, 0.1, 0.3, 0.1])
    assert sorted(M.cells_of_facet(F, g)) == [0, 1, 2, 4, 5, 6]
    Fn = F.copy()
    Fn[3] = np.nan                                     # the second vertex drops out
    assert sorted(M.cells_of_facet(Fn, g)) == [0, 4]
    assert M.cells_of_facet(np.full(9, np.nan), g) == [] and M.cells_of_facet(np.r_[np.inf, F[1:3], F[3:5], -np.inf, np.nan, F[7:]], g) == []
    count, start, sets = M.cell_lists(np.stack([F, Fn, np.full(9, np.nan)]), g)
    assert count.sum() == 8 == start[-1] and sets[0] == {0, 1} and sets[1] == {0}
    e = M.entries_from(sets, start)
    runs = M.node_runs(np.array([0.3, 0.1, 0.1]), g, start)
    assert sum(hi - lo for lo, hi in runs) == 8 and set(np.concatenate([e[lo:hi] for lo, hi in runs])) == {0, 1}
    assert sum(hi - lo for lo, hi in M.node_runs(np.array([0.9, 0.4, 0.7]), g, start)) == 0
    # outside the box: clamped into the edge cells
    assert M.node_runs(np.array([-5.0, -5.0, -5.0]), g, start) == M.node_runs(np.array([0.0, 0.0, 0.0]), g, start)


# ---- the decks ---------------------------------------------------------------------------------------------------------------
def _local_orders(d):
    """per tet the permutation that maps its local nodes to the generic tet's vertices (by the coordinates modulo the offset)"""
    x = d.xg[d.ien]
    rel = x - x.min(axis=1, keepdims=True)
    ref = M.ORBIT_X - M.ORBIT_X.min(axis=0)
    return [tuple(int(np.argmin(np.abs(ref - r).sum(axis=1))) for r in t) for t in rel]


@pytest.mark.parametrize("build", [M.orbit, M.orbit_shared])
def test_orbit_properties(build):
    d = build()
    assert d.NT == 384 and (d.N == 4 * 384 if d.name == "orbit" else d.N == 8)
    assert (d.dets() < 0).sum() == 192 and (d.dets() > 0).sum() == 192
    pairs = set(zip(_local_orders(d), M.tet_masks(d.ien, d.phi, d.level).tolist()))
    assert len(pairs) == 16 * 24 and pairs == set(d.info["cases"])
    f = np.abs(d.phi[d.ien] - d.level)
    assert all(len(set(np.round(r, 12))) == 4 for r in f)              # no two |f| equal
    x = M.ORBIT_X
    for i in range(4):                                                 # no right angle between two edges at a vertex
        for j, k in [(a, b) for a in range(4) for b in range(a + 1, 4) if i not in (a, b)]:
            u, v = x[j] - x[i], x[k] - x[i]
            assert abs(u @ v) / np.sqrt((u @ u) * (v @ v)) > 0.02


def test_swapped_cube_properties():
    d = M.swapped_cube()
    assert d.NT == 384 and d.N == 125 and (d.dets() < 0).sum() == 192
    mask = M.tet_masks(d.ien, d.phi, d.level)
    assert len(set(mask.tolist()) - {0, 15}) >= 8 and (mask == 0).any() and (mask == 15).any()


def test_on_level_properties():
    d = M.on_level()
    cnt = d.info["count"]
    assert {1, 2, 3, 4, -1, -2} == set(cnt.tolist()) and d.NT == 24 * 65 + 3 + 16
    f = d.phi[d.ien] - d.level
    assert all(((f[cnt == k] == 0).sum(axis=1) == k).all() for k in (1, 2, 3, 4))
    assert (d.dets()[cnt > 0] < 0).sum() == (cnt > 0).sum() // 2
    assert (np.isnan(f).sum(axis=1)[cnt == -2] == 1).all() and np.isnan(d.phi).sum() == 16
    flat = f[cnt == -1]
    assert (flat == flat[:, :1]).all() and set(np.sign(flat[:, 0])) == {-1.0, 0.0, 1.0}
    # an on-level node is not positive: a tet whose other nodes are all negative has mask 0
    m = M.tet_masks(d.ien, d.phi, d.level)
    assert (m[cnt == 4] == 0).all()


@needs_ld
def test_dyadic_exactness():
    d = M.dyadic()
    assert np.array_equal(d.xg * 8.0, np.round(d.xg * 8.0)) and np.array_equal(d.phi * 16.0, np.round(d.phi * 16.0))
    kinds = set(d.info["kind"])
    assert kinds == {"cut", "all == hi", "max == lo", "inside", "three == hi", "first == hi"}
    assert (d.dets() < 0).any() and (d.dets() > 0).any() and (d.dets() != 0).all()
    masks = M.tet_masks(d.ien, d.phi, d.level)
    assert set(masks.tolist()) == set(range(16))
    F64_, _ = rm.facets(d.xg, d.ien, d.phi, d.level)
    FLD, _ = rm.facets(d.xg, d.ien, d.phi, d.level, dtype=LD)
    assert len(F64_) > 100 and np.array_equal(F64_.astype(LD), FLD)
    assert np.array_equal(F64_ * 32.0, np.round(F64_ * 32.0))          # t in {1/4, 1/2, 3/4, 1} on the 2^-3 lattice
    # the determinants are exact, so six times the volume is the same number in both precisions up to the one division
    for c in (d.level, d.level - M.DYADIC_SHIFT, d.level + M.DYADIC_SHIFT):
        v64 = rm.tet_volumes(d.xg, d.ien, d.phi, c)[0]
        vld = rm.tet_volumes(d.xg, d.ien, d.phi, c, dtype=LD)[0]
        full = rm.tet_volumes(d.xg, d.ien, d.phi, c)[1]
        assert (np.abs(v64.astype(LD) - vld) <= 3 * U * full).all()    # two divisions by 6 and one subtraction at the most
        assert np.array_equal(np.round(v64 * 6.0 * 2.0 ** 15), np.round(vld * 6 * LD(2.0) ** 15).astype(F64))
    # classification sits on the thresholds
    inside, band = M.vcm.classify(d, d.phi, d.level, M.DYADIC_SHIFT)
    kind = np.array(d.info["kind"])
    assert band[kind == "all == hi"].all() and band[kind == "three == hi"].all() and inside[kind == "inside"].all()
    assert band[kind == "first == hi"].all() and (d.phi[d.ien[kind == "first == hi", 0]] == d.level + M.DYADIC_SHIFT).all()
    assert not (band | inside)[kind == "max == lo"].any()


def test_isolation_properties():
    d = M.isolation()
    assert d.NT == 256 * 384
    live = d.info["live"]
    assert np.array_equal(live // 256, np.arange(384)) and set((live % 256).tolist()) == set(M.POSITIONS)
    mask = M.tet_masks(d.ien, d.phi, d.level)
    dead = np.ones(d.NT, bool)
    dead[live] = False
    assert (mask[dead] == 0).all() and (d.phi[d.ien[dead]] < d.level - 2.0).all()
    res = M.cut(d.xg, d.ien[:256 * 16], d.phi, d.level)
    assert np.array_equal(res["part"][:, 0], res["vol"][live[:16]]) and np.array_equal(res["part"][:, 1], res["dev"][live[:16]])


# ---- the launchers' models on a case with a known answer ---------------------------------------------------------------------
def test_nodes_model_on_one_facet():
    """the unit right triangle in z = 0: a node above its interior at height 1/2 has d = 1/2 exactly"""
    g = M.make_grid([-1.0, -1.0, -1.0], 1.0, (3, 3, 3))
    F = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    count, start, sets = M.cell_lists(F, g)
    x = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.25], [0.25, 0.25, 0.75], [0.25, 0.25, 0.5]])
    old = np.array([3.0, -3.0, 3.0, np.nan])
    new, chg, listed = M.nodes(x, old, 0.0, 0.5, g, start, M.entries_from(sets, start), F, 1)
    assert listed == {0, 1, 2, 3}
    assert new[0] == 0.5 and chg[0] == -1.0              # d == band is not inside the band
    assert new[1] == -0.25 and chg[1] == 2.75
    assert new[2] == 0.5 and chg[2] == -1.0 and np.isnan(new[3]) and chg[3] == -1.0


def test_shift_model():
    nan = np.array([0x7FF8000000000123], np.uint64).view(F64)[0]
    out = M.shift(np.array([1.0, nan, np.inf, -0.0]), 0.0)
    assert out.view(np.uint64)[1] == 0x7FF8000000000123 and out[2] == np.inf and out[0] == 1.0


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def test_every_launcher_is_named_by_the_gpu_module():
    with open(os.path.join(HERE, "..", "include", "dedflow_kernels.h")) as fh:
        names = set(re.findall(r"^\w[\w\s\*]*?\b(dfl_(?:redistance|volume)_\w+)\s*\(", fh.read(), re.M))
    assert len(names) >= 10, names
    with open(os.path.join(HERE, "test_gpu_levelset_kernels.py")) as fh:
        text = fh.read()
    tests = re.findall(r"^def (test_\w+)\(.*?(?=^def |\Z)", text, re.M | re.S)
    missing = [n for n in sorted(names) if not re.search(r"L\.%s\b" % n, text)]
    assert not missing and tests, "launchers no GPU test calls: %s" % missing
