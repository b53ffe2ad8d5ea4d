"""CPU checks of the DEM walls from mesh boundary faces: the numpy model (tests/walls_model.py) against the unit-box law and
closed forms, meshgen.kuhn_box, and the library's wall entry points being exported (no compute calls: no GPU here)."""
import os
import subprocess

import numpy as np

import walls_model as wm
from dedflow_amd.meshgen import fan_mesh, kuhn_box, kuhn_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KN, GN = 1.0e4, 1.0


def _near_box_points(R, seed):
    """points inside [0,1]^3, many within R of faces, box edges and box corners"""
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(0.0, 1.0, size=(100, 3))]
    for k in range(3):   # within R of 1, 2 and 3 faces
        p = rng.uniform(2 * R, 1 - 2 * R, size=(100, 3))
        ax = rng.permuted(np.tile(np.arange(3), (100, 1)), axis=1)[:, :k + 1]
        for col in range(k + 1):
            side = rng.integers(0, 2, 100)
            d = rng.uniform(0.05 * R, 0.95 * R, 100)
            p[np.arange(100), ax[:, col]] = np.where(side == 0, d, 1.0 - d)
        pts.append(p)
    return np.vstack(pts)


def test_model_on_the_unit_cube_is_the_box_law():
    m = kuhn_cube(8)
    W = wm.Walls(m)
    R = 0.05
    x = _near_box_points(R, 1)
    # centres exactly above mesh vertices and mesh edge midpoints of the wall planes, at height < R
    g = np.array([0.25, 0.375, 0.5625])
    above = [[0.6 * R, a, b] for a in g for b in g] + [[a, 1.0 - 0.3 * R, b] for a in g for b in g]
    x = np.vstack([x, np.array(above)])
    v = np.random.default_rng(2).normal(size=x.shape)
    box = wm.unit_box_wall_forces(x, v, R, KN, GN)
    got = np.array([wm.wall_contacts(W, p, u, R, KN, GN)[0] for p, u in zip(x, v)])
    assert np.count_nonzero(np.abs(box).sum(axis=1)) > 300
    assert np.abs(got - box).max() <= 1e-12 * np.abs(box).max()


def test_flat_wall_force_does_not_depend_on_where_the_mesh_edges_are():
    """a particle at height h above the plane z = 0: over a triangle's interior, over an in-plane mesh edge (axis-aligned
    and diagonal) and over a mesh vertex, on a wall triangulated coarser and finer than R"""
    for M, R in ((4, 0.05), (16, 0.2)):
        m = kuhn_box(M, (0, 0, 0), (1, 1, 1))
        W = wm.Walls(m, groups=[4])
        h = 0.4 * R
        e = 1.0 / M
        base = np.array([0.5, 0.5, 0.0])
        offsets = [(0.3 * e, 0.1 * e), (0.5 * e, 0.0), (0.0, 0.5 * e), (0.5 * e, 0.5 * e), (0.0, 0.0)]
        v = np.array([0.3, -0.2, -0.7])
        want = (KN * (R - h) - GN * v[2]) * np.array([0, 0, 1.0])
        for dx, dy in offsets:
            p = base + np.array([dx, dy, h])
            f, nd, contacts = wm.wall_contacts(W, p, v, R, KN, GN)
            assert nd == 0 and len(contacts) == 1, (M, dx, dy, contacts)
            assert np.abs(f - want).max() <= 1e-12 * np.abs(want).max(), (M, dx, dy, f, want)


def _l_shape(M=8):
    return kuhn_box(M, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (2 * i >= M and 2 * j >= M))


def test_convex_edge_gives_one_contact_along_the_bisector():
    """the re-entrant edge of the L-shape (x = y = 1/2): a centre at distance a < R from it on the bisector, opposite the
    middle of a mesh edge and opposite a mesh vertex, gets one contact kn (R - a) - gn v.n along the bisector"""
    M = 8
    W = wm.Walls(_l_shape(M))
    R, a = 0.08, 0.03
    nb = -np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)   # into the fluid quadrant facing the removed one
    v = np.array([-0.4, 0.1, 0.25])
    for z in (0.5 + 0.5 / M, 0.5):
        p = np.array([0.5, 0.5, z]) + a * nb
        f, nd, contacts = wm.wall_contacts(W, p, v, R, KN, GN)
        want = (KN * (R - a) - GN * (v @ nb)) * nb
        assert nd == 0 and len(contacts) == 1, contacts
        assert np.abs(f - want).max() <= 1e-12 * np.abs(want).max()


def test_kuhn_box_is_a_valid_mesh():
    meshes = [kuhn_box(5, (-1, -0.5, 0), (3, 0.5, 1)), kuhn_box((6, 3, 2), (0, 0, 0), (2, 1, 1)), _l_shape(6)]
    for m in meshes:
        xg, ien = m.xg.reshape(-1, 3), m.ien.reshape(-1, 4)
        x = xg[ien]
        vol = np.einsum("ij,ij->i", np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]), x[:, 3] - x[:, 0])
        assert (vol > 0).all()
        assert np.array_equal(np.unique(ien), np.arange(m.num_node))   # no orphan nodes
        # boundary faces == the faces that occur once
        faces = np.sort(np.concatenate([np.delete(ien, k, axis=1) for k in range(4)]), axis=1)
        u, cnt = np.unique(faces, axis=0, return_counts=True)
        exposed = {tuple(f) for f in u[cnt == 1]}
        bien = np.sort(m.bound_ien.reshape(-1, 3), axis=1)
        assert {tuple(f) for f in bien} == exposed and len(bien) == len(exposed)
        # f2e / forn: the face is the parent tet minus its forn vertex; groups by outward normal
        tets = ien[m.bound_f2e]
        keep = np.ones(tets.shape, bool)
        keep[np.arange(len(tets)), m.bound_forn] = False
        assert np.array_equal(np.sort(tets[keep].reshape(-1, 3), axis=1), bien)
        W = wm.Walls(m)
        for g in range(6):
            lo, hi = m.bound_elem_offset[g], m.bound_elem_offset[g + 1]
            want = np.zeros(3)
            want[g // 2] = 1.0 if g % 2 == 0 else -1.0     # inward normal of group x-, x+, ...
            assert hi > lo and np.abs(W.n[lo:hi] - want).max() < 1e-14
            assert np.array_equal(m.bound_node[m.bound_node_offset[g]:m.bound_node_offset[g + 1]],
                                  np.unique(m.bound_ien.reshape(-1, 3)[lo:hi]))


def test_model_walls_on_the_fan_mesh_point_inwards():
    m = fan_mesh()
    W = wm.Walls(m, groups=[0])
    # the centre of the ball is on the inner side of every wall triangle
    assert (-W.off > 0).all()


def test_library_exports_the_wall_entry_points():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "dedflow_amd", "libdedflow.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("ParticleContextSetWallMesh", "ParticleContextWallDroppedCount", "dfl_walls_build_cells", "dfl_walls_forces"):
        assert name in names, name
