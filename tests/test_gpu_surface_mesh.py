"""GPU tests of the surface mesh (include/dedflow.h "surface mesh"; host/surface_mesh.c, csrc/k_surface_mesh.hip) against
tests/surface_mesh_model.py through the C ABI: every count, the vertex coordinates, edges, t, field values, the index triples,
tri_tet and the area bit for bit.  Scenes: the single tet's 16 masks in both node orders, an inclined plane, a sphere, phi == level
on a node layer, a wavy surface on a mesh that crosses the scan chunk and the sort's block, renumbered meshes, bad values, a
collapsed tet, 0 / 1 / 3 / 8 fields, empty surfaces, list growth, the passive DflTimeStep hook and the off state.  The state
and the fields sit in guarded buffers and must come back untouched.  With DFL_PARITY_OUT set, one record per parity case goes
to that file (profiles/surface_mesh_parity.jsonl is such a run): every comparison is bitwise, so the recorded ratio is 0."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import porosity_model as pm
import surface_mesh_model as sm
from dedflow_amd.meshgen import kuhn_cube, single_tet, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits

pytestmark = pytest.mark.gpu
LD = sm.LD
record = Recorder("a")
LAUNCHES, LAUNCHES_EMPTY = 14, 5
_mesh_cache = {}


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    return A


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    record.write()


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def _cube(M):
    if M not in _mesh_cache:
        _mesh_cache[M] = kuhn_cube(M)
    return _mesh_cache[M]


def _launches(api, P):
    return int(api.lib().DflSurfaceMeshTestLaunches(P.mesh))


def _evaluate(api, pool, P, cfg, w, what, fields=(), off=0):
    """Set, one evaluation from guarded buffers, which must come back untouched; returns the device result"""
    P.set_surface_mesh(**cfg)
    assert P.surface_mesh_on
    ws = pool.slot(w, off=off)
    fs = [pool.slot(q, off=(off + k) & 1) for k, q in enumerate(fields)]
    got = P.surface_mesh(ws.ptr, [s.ptr for s in fs])
    ws.check(what + ": w")
    for k, s in enumerate(fs):
        s.check(f"{what}: field {k}")
    return got


def _compare(got, want, what, **extra):
    for k in sm.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["tris"].dtype == np.int32 and np.array_equal(got["tris"], want["tris"]), what
    assert np.array_equal(got["tri_tet"], want["tri_tet"]) and np.array_equal(got["edge"], want["edge"]), what
    assert_bits(got["verts"], want["verts"], what + ": verts")
    assert_bits(got["t"], want["t"], what + ": t")
    assert got["vals"].shape == want["vals"].shape, what
    assert_bits(got["vals"], want["vals"], what + ": vals")
    assert_bits(np.array([got["area"]]), np.array([want["area"]]), what + ": area")
    record("surface_mesh", what, 0.0, vertices=want["vertices"], triangles=want["triangles"], keys=want["keys_raw"],
           fields=int(want["vals"].shape[1]), **extra)


def _case(api, pool, P, mesh, cfg, w, what, fields=(), off=0):
    got = _evaluate(api, pool, P, cfg, w, what, fields, off)
    N = mesh.num_node
    want = sm.evaluate(mesh.xg, mesh.ien, w[4 * N:5 * N], cfg, fields)
    _compare(got, want, what)
    return got, want


def _check_manifold(got, mesh_lo=0.0, mesh_hi=1.0, closed=False):
    """every edge is used once per direction; an edge without its opposite has both vertices on the cube's boundary"""
    open_edges, ok = sm.manifold(got["tris"])
    assert ok
    wall = ((got["verts"] == mesh_lo) | (got["verts"] == mesh_hi)).any(axis=1)
    assert all(wall[a] and wall[b] for a, b in open_edges)
    assert not (closed and open_edges)
    return open_edges


# ---- the single tet ------------------------------------------------------------------------------------------------------------------
def _tet(negative):
    m = single_tet()
    if not negative:
        return m
    ien = np.array([0, 1, 3, 2], np.int32)                                  # the same tet with a negative determinant
    forn = np.array([int(np.flatnonzero(ien == o)[0]) for o in range(4)], np.int32)
    return dataclasses.replace(m, ien=ien, bound_forn=forn)


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("negative", [False, True])
def test_single_tet_all_masks(api, pool, negative, side):
    m = _tet(negative)
    assert (sm.det(m.xg.reshape(-1, 3)[m.ien.reshape(-1, 4)])[0] < 0) == negative
    P = api.Problem(m, bcs=[])
    try:
        for mask in range(16):
            f = np.array([0.4 + 0.2 * a if (mask >> a) & 1 else -0.3 - 0.1 * a for a in range(4)])
            cfg = sm.config(level=0.125, side=side)
            w = sm.state(m, side * f + 0.125)
            what = f"single/det{'-' if negative else '+'}/mask{mask}/side{side:+d}"
            got, want = _case(api, pool, P, m, cfg, w, what, fields=sm.nodal_fields(m, 2), off=mask & 1)
            np_ = bin(mask).count("1")
            assert got["triangles"] == (0 if np_ in (0, 4) else 2 if np_ == 2 else 1), what
            assert got["vertices"] == (0 if np_ in (0, 4) else 4 if np_ == 2 else 3), what
            if got["triangles"]:                                           # out of the metal, decided geometrically
                x = m.xg.reshape(-1, 3)[m.ien.reshape(-1, 4)].astype(LD)
                g = sm.gradient(x, f[m.ien.reshape(-1, 4)].astype(LD))[0]
                n = sm.normals(got["verts"].astype(LD)[got["tris"]])
                assert (n @ g < 0).all(), what
            assert _launches(api, P) == (LAUNCHES if got["triangles"] else LAUNCHES_EMPTY)
    finally:
        P.close()


# ---- planes and the sphere -------------------------------------------------------------------------------------------------------------
def test_inclined_plane(api, pool):
    m = _cube(4)
    assert m.num_tet == 384 > 256
    P = api.Problem(m)
    try:
        N = m.num_node
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * N, np.float64)
        for side in (1, -1):
            got, want = _case(api, pool, P, m, sm.config(side=side), sm.state(m, side * sm.inclined_plane(m)),
                              f"cube4/plane/side{side:+d}", fields=sm.nodal_fields(m, 1))
            assert got["triangles"] > 50 and _check_manifold(got)
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * N, np.float64), xg0, "xg")
    finally:
        P.close()


VOLUME_FACTOR = 64.0


def test_sphere_is_closed_and_encloses_the_metal_volume(api, pool):
    """kuhn_cube(8), centre (0.5, 0.5, 0.5), r = 0.3: a closed surface with V - E + F = 2 whose divergence-theorem volume
    (1 / 6) sum A . (B x C) is DflMeshLevelSetVolume of the same state within
        VOLUME_FACTOR x 2^-53 x (sum |A . (B x C)| / 6 + the level-set volume, a sum of non-negative terms).
    The factor: in the numpy model on the development machine the float64 divergence sum is 5.5 x 2^-53 x its sum of absolute
    terms from the longdouble one, the float64 tet-by-tet volume 0.24 x 2^-53 x its own sum from the longdouble one, and the two
    float64 numbers 3.2 x 2^-53 x (both sums) apart; the two longdouble numbers agree to 2e-20.  The device forms the same
    terms and adds them in another order, which moves a sum of n terms by at most about log2(n) / 2 more units; 64 leaves a
    factor of ten over what the model measures.  With side = -1 and the negated phi the triangles are the same, index for
    index."""
    m = _cube(8)
    N = m.num_node
    phi = sm.sphere(m)
    P = api.Problem(m)
    try:
        w = sm.state(m, phi)
        got, want = _case(api, pool, P, m, sm.config(), w, "cube8/sphere/side+1", fields=sm.nodal_fields(m, 1))
        _check_manifold(got, closed=True)
        E = len(sm.edge_uses(got["tris"])) // 2
        assert got["vertices"] - E + got["triangles"] == 2
        vol, scale = sm.enclosed_volume(got["verts"], got["tris"])
        wd = api.DeviceArray.from_numpy(w)
        metal = P.level_set_volume(wd, 0.0)
        err, bound = abs(float(vol) - metal), VOLUME_FACTOR * 2.0 ** -53 * (float(scale) + metal)
        print(f"surface mesh volume: divergence {float(vol)!r}, level-set {metal!r}, err {err:.3e}, err / bound {err / bound:.3e}")
        record("surface_mesh_volume", "cube8/sphere", err / bound, divergence=float(vol), level_set=metal)
        assert err <= bound and 0.08 < metal < 4.0 / 3.0 * np.pi * 0.3 ** 3
        neg, _ = _case(api, pool, P, m, sm.config(side=-1), sm.state(m, -phi), "cube8/sphere/side-1", fields=sm.nodal_fields(m, 1), off=1)
        for k in ("tris", "tri_tet", "edge"):
            assert np.array_equal(neg[k], got[k]), k
        for k in ("verts", "t", "vals"):
            assert_bits(neg[k], got[k], k)
        assert neg["area"] == got["area"]
    finally:
        P.close()


def test_phi_equal_to_level_at_nodes(api, pool):
    m = _cube(4)
    P = api.Problem(m)
    try:
        got, want = _case(api, pool, P, m, sm.config(level=0.25), sm.state(m, sm.node_plane(m) + 0.25), "cube4/node-layer")
        ien = m.ien.reshape(-1, 4)
        z = m.xg.reshape(-1, 3)[:, 2]
        cut = set()
        for tet in ien:                                                    # the cut edges, counted by hand: metal below z = 0.5
            for a in tet:
                for b in tet:
                    if z[a] < 0.5 <= z[b]:
                        cut.add((int(a), int(b)))
        assert got["vertices"] == len(cut) and set(map(tuple, got["edge"].tolist())) == cut
        assert (got["t"] == 1.0).all() and len(np.unique(got["verts"], axis=0)) == 25 < got["vertices"]
        areas = sm.areas(got["verts"][got["tris"]])
        assert (areas == 0).any() and (areas > 0).any()
        assert _check_manifold(got)
        assert np.isfinite(got["verts"]).all() and got["area"] == pytest.approx(1.0, abs=1e-14)
    finally:
        P.close()


# ---- beyond one scan chunk and one sort block -------------------------------------------------------------------------------------------
def test_wavy_surface_on_a_mesh_beyond_one_scan_chunk(api, pool):
    """z = 0.5 + 0.1 sin(2 pi x) cos(2 pi y) on the smallest Kuhn cube whose workgroup counts (two per workgroup of
    dfl_tets_per_block() tets: triangles and keys, one scan) exceed one chunk of the device scan, 4 x 256 entries: the tets'
    offsets come from two chunks.  The key count then exceeds the sort's single-workgroup limit and fills many workgroups of
    the run-head pass.  The run-head scan itself would need more than 1024 x 256 keys (a cube of about 103^3 cells) to leave
    its first chunk, which is no quick test; it calls the same dfl_scan_counts, which test_gpu_scan.py covers alone."""
    L = api.lib()
    per, chunk = int(L.dfl_tets_per_block()), 4 * int(L.dfl_tets_per_block())
    M = next(M for M in range(2, 200) if 2 * -(-6 * M ** 3 // per) > chunk)
    assert M == 28
    m = _cube(M)
    P = api.Problem(m)
    try:
        got, want = _case(api, pool, P, m, sm.config(), sm.state(m, sm.wavy(m)), f"cube{M}/wavy", fields=sm.nodal_fields(m, 2))
        assert int(L.dfl_scan_num_chunks(2 * -(-m.num_tet // per))) == 2
        assert want["keys_raw"] > 8 * int(L.dfl_surface_mesh_sort_block()) and want["keys_raw"] > 32 * per
        assert got["triangles"] > 2 * per
    finally:
        P.close()


# ---- renumbered meshes ---------------------------------------------------------------------------------------------------------------
def _geometric(got):
    """the triangles as coordinates, each rotated to start at its smallest corner: a set that no numbering changes"""
    out = set()
    for tri in got["verts"][got["tris"]].tolist():
        k = min(range(3), key=lambda q: tri[q])
        out.add(tuple(map(tuple, tri[k:] + tri[:k])))
    return out


@pytest.mark.parametrize("order", ["random", "reversed"])
def test_renumbered_mesh(api, pool, order):
    m = _cube(6)
    N, T = m.num_node, m.num_tet
    w = sm.state(m, sm.sphere(m, r=0.33, c=(0.45, 0.5, 0.55)))
    fields = sm.nodal_fields(m, 1)
    perm = np.random.default_rng(11).permutation(N) if order == "random" else np.arange(N)[::-1].copy()
    tperm = np.random.default_rng(12).permutation(T) if order == "random" else np.arange(T)[::-1].copy()   # new tet k = old tperm[k]
    P = api.Problem(m)
    try:
        base, _ = _case(api, pool, P, m, sm.config(), w, "cube6/sphere/unpermuted", fields=fields)
    finally:
        P.close()
    m2, w2 = pm.permuted(m, w, perm)
    inv_t = np.argsort(tperm)
    m2 = dataclasses.replace(m2, ien=np.ascontiguousarray(m2.ien.reshape(-1, 4)[tperm].reshape(-1)),
                             bound_f2e=inv_t[m2.bound_f2e].astype(np.int32))
    f2 = [q[np.argsort(perm)] for q in fields]
    P = api.Problem(m2)
    try:
        got, _ = _case(api, pool, P, m2, sm.config(), w2, f"cube6/sphere/{order}", fields=f2, off=1)
    finally:
        P.close()
    assert (got["vertices"], got["triangles"]) == (base["vertices"], base["triangles"])
    assert _geometric(got) == _geometric(base) and len(_geometric(base)) == base["triangles"]
    assert sorted(map(tuple, got["edge"].tolist())) == sorted(map(tuple, perm[base["edge"]].tolist()))
    assert sorted(got["vals"][:, 0].tolist()) == sorted(base["vals"][:, 0].tolist())


# ---- bad values, a collapsed tet -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_bad_phi_inside_on_the_surface_and_far_away(api, pool, value):
    m = _cube(6)
    N = m.num_node
    ien = m.ien.reshape(-1, 4)
    x = m.xg.reshape(-1, 3)
    w = sm.state(m, sm.sphere(m))
    clean = sm.evaluate(m.xg, m.ien, w[4 * N:5 * N], sm.config())
    centre = int(np.argmin(np.linalg.norm(x - 0.5, axis=1)))
    on_surface = int(clean["edge"][0, 0])
    P = api.Problem(m)
    try:
        for tag, node in (("inside", centre), ("surface", on_surface), ("far", 0)):
            bad = w.copy()
            bad[4 * N + node] = value
            got, want = _case(api, pool, P, m, sm.config(), bad, f"cube6/bad-{tag}/{value}", fields=sm.nodal_fields(m, 1))
            hit = np.isin(ien, node).any(axis=1)
            assert got["bad_nodes"] == 1 and got["bad_tets"] == hit.sum()
            assert not np.isin(got["tri_tet"], np.flatnonzero(hit)).any()
            assert np.isfinite(got["verts"]).all() and np.isfinite(got["t"]).all() and np.isfinite(got["vals"]).all()
            if tag != "surface":                                           # those tets were not cut: the rest is everything
                for k in ("tris", "tri_tet", "edge"):
                    assert np.array_equal(got[k], clean[k]), (tag, k)
                assert_bits(got["verts"], clean["verts"], tag)
            else:
                assert 0 < got["triangles"] < clean["triangles"]
                keep = ~np.isin(clean["tri_tet"], np.flatnonzero(hit))
                assert np.array_equal(got["tri_tet"], clean["tri_tet"][keep])
                assert_bits(got["verts"][got["tris"]], clean["verts"][clean["tris"][keep]], "the triangles that stay")
    finally:
        P.close()


def test_collapsed_tet_is_degenerate_and_emits_nothing(api, pool):
    """node b of a cut edge (a, b) is moved onto a after the set-up: the tets that hold both have a zero determinant"""
    m = _cube(4)
    N = m.num_node
    ien = m.ien.reshape(-1, 4)
    w = sm.state(m, sm.inclined_plane(m))
    clean = sm.evaluate(m.xg, m.ien, w[4 * N:5 * N], sm.config())
    a, b = (int(v) for v in clean["edge"][len(clean["edge"]) // 2])
    xg = m.xg.reshape(-1, 3).copy()
    xg[b] = xg[a]
    m2 = dataclasses.replace(m, xg=np.ascontiguousarray(xg.reshape(-1)))
    both = np.isin(ien, a).any(axis=1) & np.isin(ien, b).any(axis=1)
    P = api.Problem(m)
    try:
        api.DeviceArray(3 * N, np.float64, ptr=P.mesh.contents.device.contents.xg).upload(m2.xg)
        got, want = _case(api, pool, P, m2, sm.config(), w, "cube4/collapsed")
        assert (sm.det(xg[ien[both]]) == 0).all() and both.sum() >= 4
        assert got["degenerate_tets"] == both.sum() and got["bad_tets"] == 0
        assert not np.isin(got["tri_tet"], np.flatnonzero(both)).any() and got["triangles"] < clean["triangles"]
    finally:
        P.close()


# ---- fields -------------------------------------------------------------------------------------------------------------------------
def test_fields(api, pool, capfd):
    m = _cube(6)
    N = m.num_node
    w = sm.state(m, sm.sphere(m))
    P = api.Problem(m)
    try:
        results = {}
        for K in (0, 1, 3, 8):
            results[K], want = _case(api, pool, P, m, sm.config(), w, f"cube6/fields{K}", fields=sm.nodal_fields(m, K), off=K & 1)
            assert results[K]["vals"].shape == (want["vertices"], K)
        for K in (1, 3, 8):
            assert_bits(results[K]["vals"][:, 0], results[1]["vals"][:, 0], "field 0")
            assert np.array_equal(results[K]["tris"], results[0]["tris"])
        # a NaN at a node that is on no cut edge changes nothing
        fields = sm.nodal_fields(m, 3)
        off_surface = np.setdiff1d(np.arange(N), results[3]["edge"].ravel())[7]
        fields[1] = fields[1].copy()
        fields[1][off_surface] = np.nan
        got, _ = _case(api, pool, P, m, sm.config(), w, "cube6/fields3/nan-off-surface", fields=fields)
        assert_bits(got["vals"], results[3]["vals"], "vals with a NaN elsewhere")
        # nine fields: refused, the last evaluation stays
        capfd.readouterr()
        ptrs = [pool.slot(q).ptr for q in sm.nodal_fields(m, 9)]
        assert P.surface_mesh(pool.slot(w).ptr, ptrs) is None and "num_fields" in capfd.readouterr().err
        after = P.surface_mesh()
        for k in ("verts", "vals", "t"):
            assert_bits(after[k], got[k], k)
        assert np.array_equal(after["tris"], got["tris"]) and after["area"] == got["area"]
    finally:
        P.close()


# ---- empty surfaces --------------------------------------------------------------------------------------------------------------------
def test_empty_surface(api, pool):
    """all metal and all gas: no vertex, no triangle, area +0.0.  The evaluation stops after the count pass and the one wait: of the
    14 launches of a non-empty evaluation it runs 5 (the bad nodes, the classification, the scan's two, the counts) and skips
    the 9 that a triangle count of zero leaves without work (emit, sort, run heads, their scan's two, vertices, triangles, the
    area's second stage, the vertex count).  (A mesh without tets is not admitted by the mesh API.)"""
    m = _cube(4)
    P = api.Problem(m)
    try:
        full, _ = _case(api, pool, P, m, sm.config(), sm.state(m, sm.inclined_plane(m)), "cube4/before-empty")
        assert _launches(api, P) == LAUNCHES and full["triangles"] > 0
        for tag, phi in (("metal", np.ones(m.num_node)), ("gas", -np.ones(m.num_node))):
            got, _ = _case(api, pool, P, m, sm.config(), sm.state(m, phi), f"cube4/all-{tag}", fields=sm.nodal_fields(m, 1))
            assert got["vertices"] == got["triangles"] == 0 and got["area"] == 0.0 and not np.signbit(got["area"])
            assert got["verts"].shape == (0, 3) and got["tris"].shape == (0, 3) and _launches(api, P) == LAUNCHES_EMPTY
    finally:
        P.close()


# ---- growth, repeatability -------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (all(a[k] == b[k] for k in sm.COUNTS + ("area",)) and all(np.array_equal(a[k], b[k]) for k in ("tris", "tri_tet", "edge"))
            and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("verts", "t", "vals")))


def test_lists_grow_once_and_evaluations_repeat(api, pool):
    m = _cube(13)
    L = api.lib()
    small, large = sm.state(m, sm.sphere(m, r=0.12)), sm.state(m, sm.sphere(m, r=0.42))
    fields = sm.nodal_fields(m, 2)
    capk, capt = C.c_int32(), C.c_int32()
    P = api.Problem(m)
    try:
        a, want_a = _case(api, pool, P, m, sm.config(), small, "cube13/small", fields=fields)
        assert L.DflSurfaceMeshTestGrows(P.mesh, C.byref(capk), C.byref(capt)) == 1   # the first one sizes vals and no more
        assert want_a["keys_raw"] <= capk.value == 1024 and want_a["triangles"] <= capt.value == 1024
        b, want_b = _case(api, pool, P, m, sm.config(), large, "cube13/large", fields=fields)
        assert L.DflSurfaceMeshTestGrows(P.mesh, C.byref(capk), C.byref(capt)) == 2
        assert want_b["keys_raw"] > 1024 and capk.value == want_b["keys_raw"] + want_b["keys_raw"] // 2
        assert want_b["triangles"] > 1024 and capt.value == want_b["triangles"] + want_b["triangles"] // 2
        ws, wl = pool.slot(small, off=1), pool.slot(large)
        fs = [pool.slot(q).ptr for q in fields]
        api.sync()
        mem = int(L.DflDeviceMemoryInUse())
        c = P.surface_mesh(ws.ptr, fs)
        assert int(L.DflDeviceMemoryInUse()) == mem and L.DflSurfaceMeshTestGrows(P.mesh, None, None) == 2
        assert _same(a, c)
        d, e = P.surface_mesh(wl.ptr, fs), P.surface_mesh(wl.ptr, fs)
        assert _same(b, d) and _same(d, e) and L.DflSurfaceMeshTestGrows(P.mesh, None, None) == 2
    finally:
        P.close()
    P = api.Problem(m)                                                     # and in a fresh mesh
    try:
        assert _same(b, _evaluate(api, pool, P, sm.config(), large, "cube13/large/again", fields=fields))
    finally:
        P.close()


# ---- DflTimeStep ----------------------------------------------------------------------------------------------------------------------
def _two_steps(api, every):
    m = _cube(4)
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = np.minimum(0.75 - x[:, 2] - 0.8 * np.abs(x[:, 1] - 0.5), np.linalg.norm(x - 0.25, axis=1) - 0.2)
    wg[5 * N:] = 1700.0 + 1000.0 * (x[:, 2] - 0.4)
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if every is not None:
            P.set_surface_mesh(level=0.0, every=every)
            assert P.surface_mesh_on
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        o = dict(w=[], it=[], res=[], launches=[])
        for _ in range(2):
            it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)
            api.sync()
            o["it"].append(it)
            o["w"].append(st[0].numpy())
            if every is not None:
                o["launches"].append(_launches(api, P))
                o["res"].append(P.surface_mesh())
        o["dwgold"], o["dw"], o["F"] = st[1].numpy(), st[2].numpy(), F_d.numpy()
        return o
    finally:
        P.close()


def test_time_step_is_passive_and_fills_the_result(api):
    m = _cube(4)
    N = m.num_node
    base, on, second, never = _two_steps(api, None), _two_steps(api, 1), _two_steps(api, 2), _two_steps(api, 0)
    for run in (on, second, never):
        assert base["it"] == run["it"] and min(base["it"]) >= 0
        for k in range(2):
            assert np.isfinite(base["w"][k]).all()
            assert_bits(run["w"][k], base["w"][k], f"wgold after step {k}")
        for k in ("dwgold", "dw", "F"):
            assert_bits(run[k], base[k], k)
    for run in (on, second):                                               # the mesh of the last wgold with the field T
        w = run["w"][1]
        want = sm.evaluate(m.xg, m.ien, w[4 * N:5 * N], sm.config(), [w[5 * N:]])
        assert want["triangles"] > 0
        _compare(run["res"][1], want, "cube4/time-step")
    assert on["launches"] == [LAUNCHES, LAUNCHES] and on["res"][0]["triangles"] > 0
    assert second["launches"] == [0, LAUNCHES] and second["res"][0]["triangles"] == 0   # every = 2: nothing at the first step
    assert never["launches"] == [0, 0] and never["res"][1]["triangles"] == never["res"][1]["vertices"] == 0


# ---- refusals, off ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_off(api, capfd):
    m = _cube(6)
    N = m.num_node
    w = sm.state(m, sm.sphere(m))
    P = api.Problem(m)
    L = api.lib()
    try:
        wd = api.DeviceArray.from_numpy(w)
        capfd.readouterr()
        assert L.DflMeshSurfaceMesh(P.mesh, wd.ptr, None, 0) == -1           # without a configuration
        assert "no surface mesh" in capfd.readouterr().err
        p = [C.c_void_p(1) for _ in range(6)]
        nv = C.c_int32(7)
        assert L.DflMeshSurfaceMeshArrays(P.mesh, *[C.byref(q) for q in p], C.byref(nv)) == 0
        assert all(q.value is None for q in p) and nv.value == 0
        for reason, bad in (("level", dict(level=np.nan)), ("side", dict(side=0)), ("every", dict(every=-1))):
            P.set_surface_mesh(**dict(sm.config(), **bad))
            assert not P.surface_mesh_on and reason in capfd.readouterr().err
        P.set_surface_mesh(**sm.config())
        assert P.surface_mesh_on and capfd.readouterr().err == ""
        before = P.surface_mesh(wd)
        assert before["triangles"] > 0
        for reason, bad in (("level", dict(level=np.inf)), ("side", dict(side=3)), ("every", dict(every=-4))):
            P.set_surface_mesh(**dict(sm.config(), **bad))                 # refused: configuration and result stay
            assert P.surface_mesh_on and reason in capfd.readouterr().err
            assert _same(P.surface_mesh(), before)
        assert _same(P.surface_mesh(wd), before)                           # ... and it still evaluates as configured
        # a solver with a communicator: refused before anything is computed, but only with every > 0
        P.set_surface_mesh(**sm.config(every=1))
        comm = api.DflComm()
        L.KrylovSetComm(P.ksp, C.byref(comm))
        arr = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        capfd.readouterr()
        assert P.time_step(arr[0], arr[1], arr[2], F_d, dx_d)[0] == -1
        assert "surface mesh is single-GPU only" in capfd.readouterr().err
        assert _launches(api, P) == 0 and P.surface_mesh()["triangles"] == 0   # nothing was evaluated
        L.KrylovSetComm(P.ksp, None)
        P.set_surface_mesh()                                               # NULL frees
        assert not P.surface_mesh_on and L.DflSurfaceMeshTestGrows(P.mesh, None, None) == 0
        assert L.DflMeshSurfaceMesh(P.mesh, wd.ptr, None, 0) == -1 and "no surface mesh" in capfd.readouterr().err
        assert L.DflMeshSurfaceMeshArrays(P.mesh, *[C.byref(q) for q in p], C.byref(nv)) == 0 and p[0].value is None
        with pytest.raises(RuntimeError):
            P.surface_mesh(wd)
    finally:
        P.close()
