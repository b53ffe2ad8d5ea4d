"""CPU tests of the surface mesh (include/dedflow.h, "surface mesh"): the symbols, the library's host-only configuration check,
the numpy model (tests/surface_mesh_model.py) -- its orientation table against the sign of n . g in longdouble, its triangles
against the unwelded facets of redistance_model, what the scenes of test_gpu_surface_mesh.py promise -- and the PLY / STL writers
of dedflow_amd/surface_io.py."""
import ctypes as C
import os

import numpy as np
import pytest

import redistance_model as rm
import surface_mesh_model as sm
from dedflow_amd import surface_io as sio
from dedflow_amd.meshgen import kuhn_cube

LD = sm.LD
_cache = {}


def _cube(M):
    if M not in _cache:
        _cache[M] = kuhn_cube(M)
    return _cache[M]


def test_symbols_declared_and_exported():
    from dedflow_amd import api
    lib = api.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "dedflow.h")).read()
    ker = open(os.path.join(root, "include", "dedflow_kernels.h")).read()
    for n in ("DflSurfaceMeshCheck", "DflMeshSetSurfaceMesh", "DflMeshSurfaceMeshEnabled", "DflMeshSurfaceMesh",
              "DflMeshSurfaceMeshStats", "DflMeshSurfaceMeshArrays", "DflMeshSurfaceMeshCopy"):
        assert n in pub and hasattr(lib, n), n
    for n in ("dfl_surface_mesh_count", "dfl_surface_mesh_build", "dfl_surface_mesh_temp_bytes", "dfl_surface_mesh_sort_block"):
        assert n in ker and hasattr(lib, n), n
    assert hasattr(lib, "DflSurfaceMeshTestLaunches") and hasattr(lib, "DflSurfaceMeshTestGrows")
    for n in ("set_surface_mesh", "surface_mesh_on", "surface_mesh"):
        assert hasattr(api.Problem, n), n
    assert C.sizeof(api.DflSurfaceMesh) == 16 and C.sizeof(api.DflSurfaceMeshStats) == 7 * 8


def test_configuration_check():
    """every refusal of DflSurfaceMeshCheck, and the model's"""
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(200)

    def library(**kw):
        cfg = api.surface_mesh_config(**kw)
        return L.DflSurfaceMeshCheck(C.byref(cfg), why, 200), why.value.decode()

    for good in (dict(), dict(level=-3.5), dict(side=-1), dict(every=7), dict(every=0)):
        assert library(**good)[0] == 0 and sm.refusal(sm.config(**good)) is None, good
    for reason, bad in (("level", dict(level=np.nan)), ("level", dict(level=np.inf)), ("level", dict(level=-np.inf)),
                        ("side", dict(side=0)), ("side", dict(side=2)), ("side", dict(side=-3)), ("every", dict(every=-1)),
                        ("every", dict(every=-9))):
        rc, text = library(**bad)
        assert rc != 0 and reason in text and sm.refusal(sm.config(**bad)) == reason, (reason, bad, text)


# ---- the orientation table ------------------------------------------------------------------------------------------------------------
REGULAR = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])


def _draw(rng, n, mask, negative):
    """n well-shaped tets (a regular one of edge 2 sqrt 2 with every coordinate moved by up to 0.3, somewhere in a box of size
    10), node order for the wanted determinant sign, and f with the mask's signs and 0.05 <= |f| <= 1"""
    x = REGULAR[None] + rng.uniform(-0.3, 0.3, (n, 4, 3)) + rng.uniform(-5.0, 5.0, (n, 1, 3))
    if (sm.det(x)[0] < 0) != negative:
        x = x[:, [0, 1, 3, 2]]
    metal = ((mask >> np.arange(4)) & 1).astype(bool)
    f = rng.uniform(0.05, 1.0, (n, 4)) * np.where(metal, 1.0, -1.0)[None]
    return x, f


def test_swap_table_is_the_geometric_one():
    assert sm.derive_swap() == sm.SWAP


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("negative", [False, True])
def test_orientation_table_against_the_longdouble_normal(negative, side):
    """per mask 100 random well-shaped tets: the triangles the model lists (oriented by the table alone) have n . g < 0 in
    longdouble, on inputs whose triangle area is at least 1e-6 of the tet's largest face area (redrawn otherwise, at most 5 per
    mask; the distribution above gives t in [0.047, 0.953] and needs none)"""
    rng = np.random.default_rng(1000 + 2 * negative + (side < 0))
    for mask in range(1, 15):
        n, redrawn = 100, 0
        x, f = _draw(rng, n, mask, negative)
        level = rng.uniform(-2.0, 2.0)
        while True:
            assert ((sm.det(x) < 0) == negative).all()
            phi = side * f + level                                          # side (phi - level) has the signs of f
            ien = np.arange(4 * n).reshape(n, 4)
            res = sm.evaluate(x.reshape(-1), ien, phi.reshape(-1), sm.config(level=level, side=side), dtype=LD)
            assert res["triangles"] == n * (2 if bin(mask).count("1") == 2 else 1) and res["degenerate_tets"] == 0
            fl = side * (phi.astype(LD) - LD(level))
            g = sm.gradient(x.astype(LD), fl)[res["tri_tet"]]
            P = res["verts"][res["tris"]]
            s = rm.dot(sm.normals(P), g)
            face = np.max([sm.areas(x.astype(LD)[:, [a, b, c]]) for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))], axis=0)
            small = np.zeros(n, bool)
            small[res["tri_tet"][res["tri_area"] < 1e-6 * face[res["tri_tet"]]]] = True
            if not small.any():
                break
            redrawn += int(small.sum())
            x[small], f[small] = _draw(rng, int(small.sum()), mask, negative)
        assert redrawn <= 5, (mask, redrawn)
        assert (s < 0).all(), (mask, negative, side, int((s >= 0).sum()))


# ---- the model against the unwelded facets ---------------------------------------------------------------------------------------------
def _scenes():
    yield "plane4", _cube(4), sm.inclined_plane(_cube(4)), 0.0
    yield "sphere8", _cube(8), sm.sphere(_cube(8)), 0.0
    yield "nodes4", _cube(4), sm.node_plane(_cube(4)), 0.0
    yield "wavy12", _cube(12), sm.wavy(_cube(12)) + 0.25, 0.25


@pytest.mark.parametrize("side", [1, -1])
def test_soup_equality_with_the_redistancing_facets(side):
    """verts[tris] is redistance_model.facets bit for bit, in the same tet order, up to the swap of the second and third vertex"""
    for name, m, phi, level in _scenes():
        res = sm.evaluate(m.xg, m.ien, side * phi, sm.config(level=side * level, side=side))
        want, tet = rm.facets(m.xg, m.ien, phi, level)                      # (side phi) side - (side level) side = phi - level
        got = sm.soup(res)
        assert got.shape == want.shape and np.array_equal(res["tri_tet"], tet), name
        same = (got.view(np.uint64) == want.view(np.uint64)).all(axis=1)
        swapped = (got.view(np.uint64) == want[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]].view(np.uint64)).all(axis=1)
        assert (same | swapped).all() and swapped.any() and same.any(), name
        assert res["vertices"] == len(np.unique(res["keys"])) and (np.diff(res["keys"].astype(np.uint64)) > 0).all()
        assert (res["t"] > 0).all() and (res["t"] <= 1).all(), name


def test_scene_promises():
    # the inclined plane: manifold inside, open edges on the boundary only
    m = _cube(4)
    res = sm.evaluate(m.xg, m.ien, sm.inclined_plane(m), sm.config())
    open_edges, ok = sm.manifold(res["tris"])
    assert ok and open_edges
    on_wall = (np.abs(res["verts"] - 0.5) == 0.5).any(axis=1)
    assert all(on_wall[a] and on_wall[b] for a, b in open_edges)
    # the sphere: closed, a topological sphere, the volume of the metal
    m = _cube(8)
    phi = sm.sphere(m)
    res = sm.evaluate(m.xg, m.ien, phi, sm.config())
    open_edges, ok = sm.manifold(res["tris"])
    E = len(sm.edge_uses(res["tris"])) // 2
    assert ok and not open_edges and res["vertices"] - E + res["triangles"] == 2
    vol, scale = sm.enclosed_volume(res["verts"], res["tris"], LD)
    want = rm.volume(m.xg, m.ien, phi, 0.0, LD)
    assert abs(vol - want) <= 1e-15 * scale and 0.08 < float(vol) < 4.0 / 3.0 * np.pi * 0.3 ** 3
    neg = sm.evaluate(m.xg, m.ien, -phi, sm.config(side=-1))
    assert np.array_equal(neg["tris"], res["tris"]) and np.array_equal(neg["verts"].view(np.uint64), res["verts"].view(np.uint64))
    # phi == level on a node layer: one vertex per cut edge, coincident and distinct; zero-area triangles
    m = _cube(4)
    res = sm.evaluate(m.xg, m.ien, sm.node_plane(m), sm.config())
    assert (res["t"] == 1.0).all() and res["vertices"] > len(np.unique(res["verts"], axis=0)) == 25
    assert (res["tri_area"] == 0).any() and (res["tri_area"] > 0).any()
    open_edges, ok = sm.manifold(res["tris"])
    assert ok and open_edges
    assert float(res["area"]) == pytest.approx(1.0, abs=1e-14)


def test_tree_sum_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (0, 1, 255, 256, 257, 70000):
        v = rng.uniform(0.0, 1.0, n)
        assert abs(float(sm.tree_sum(v)) - float(np.sum(v.astype(LD)))) <= 1e-13 * max(n, 1)
    assert np.signbit(sm.tree_sum(np.zeros(0))) == False  # noqa: E712  (+0.0)


# ---- the writers -----------------------------------------------------------------------------------------------------------------------
def _mesh_and_fields():
    m = _cube(6)
    fields = sm.nodal_fields(m, 3)
    res = sm.evaluate(m.xg, m.ien, sm.sphere(m), sm.config(), fields)
    return res["verts"], res["tris"], res["vals"]


def test_ply_round_trip(tmp_path):
    verts, tris, vals = _mesh_and_fields()
    p = str(tmp_path / "a.ply")
    sio.write_ply(p, verts, tris, vals, ["T", "cool", "T_peak"])
    v, t, f, names = sio.read_ply(p)
    assert names == ["T", "cool", "T_peak"] and t.dtype == np.int32 and np.array_equal(t, tris)
    assert np.array_equal(v.view(np.uint64), verts.view(np.uint64)) and np.array_equal(f.view(np.uint64), vals.view(np.uint64))
    head = open(p, "rb").read(400).split(b"end_header")[0].decode()
    assert head.startswith("ply\nformat binary_little_endian 1.0\n") and "property double cool" in head
    assert os.path.getsize(p) == len(head) + len("end_header\n") + len(verts) * 6 * 8 + len(tris) * 13
    sio.write_ply(p, verts, tris)                                           # no fields
    v, t, f, names = sio.read_ply(p)
    assert names == [] and f.shape == (len(verts), 0) and np.array_equal(t, tris)
    with pytest.raises(ValueError):
        sio.write_ply(p, verts, tris, vals, ["x", "b", "c"])
    with pytest.raises(ValueError):
        sio.write_ply(p, verts, tris + len(verts))


def test_stl_round_trip(tmp_path):
    verts, tris, _ = _mesh_and_fields()
    tris = np.concatenate([tris, [[0, 0, 1]]]).astype(np.int32)             # and a zero-area triangle
    p = str(tmp_path / "a.stl")
    sio.write_stl(p, verts, tris)
    P, n = sio.read_stl(p)
    assert os.path.getsize(p) == 84 + 50 * len(tris)
    assert P.dtype == np.float32 and np.array_equal(P, verts[tris].astype(np.float32))
    assert np.array_equal(n[-1], np.zeros(3, np.float32))
    Q = verts[tris[:-1]]
    want = np.cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
    want /= np.linalg.norm(want, axis=1)[:, None]
    assert np.allclose(n[:-1], want, atol=1e-6) and np.allclose(np.linalg.norm(n[:-1], axis=1), 1.0, atol=1e-6)


def test_writers_take_an_empty_mesh(tmp_path):
    verts, tris = np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    p = str(tmp_path / "e.ply")
    sio.write_ply(p, verts, tris, np.zeros((0, 2)), ["a", "b"])
    v, t, f, names = sio.read_ply(p)
    assert v.shape == (0, 3) and t.shape == (0, 3) and f.shape == (0, 2) and names == ["a", "b"]
    p = str(tmp_path / "e.stl")
    sio.write_stl(p, verts, tris)
    P, n = sio.read_stl(p)
    assert P.shape == (0, 3, 3) and n.shape == (0, 3) and os.path.getsize(p) == 84
