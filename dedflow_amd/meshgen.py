"""Synthetic Kuhn-cube tet meshes and fields.

The reference ships no meshes (``box.h5`` / ``tet.h5`` are referenced by
``src/main.c:358-360`` but absent), so every input here is synthetic.  The
arrays follow the on-disk schema the reference reads (``src/MeshData.c:57-109``,
``src/Mesh.c:12-59``; written by ``tools/mesh_convert.py:116-126``):

  xg      f64[3N]   node coordinates, AoS
  ien     i32[4T]   tet connectivity, positive orientation
  bound   6 groups in the order x-,x+,y-,y+,z-,z+ with
          node_offset/node (sorted unique), elem_offset/ien(3 per face)/
          f2e (parent tet)/forn (local index of the tet vertex opposite the face,
          ``tools/mesh_convert.py:60-66``)
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

_PERMS = list(itertools.permutations(range(3)))


def _perm_is_odd(p) -> bool:
    inv = sum(1 for a in range(3) for b in range(a + 1, 3) if p[a] > p[b])
    return inv % 2 == 1


@dataclass
class TetMesh:
    M: int
    xg: np.ndarray  # f64 [3N]
    ien: np.ndarray  # i32 [4T]
    bound_node_offset: np.ndarray  # i32 [nb+1]
    bound_node: np.ndarray  # i32
    bound_elem_offset: np.ndarray  # i32 [nb+1]
    bound_ien: np.ndarray  # i32 [3*nf]
    bound_f2e: np.ndarray  # i32 [nf]
    bound_forn: np.ndarray  # i32 [nf]

    @property
    def num_node(self) -> int:
        return self.xg.size // 3

    @property
    def num_tet(self) -> int:
        return self.ien.size // 4

    @property
    def num_bound(self) -> int:
        return self.bound_node_offset.size - 1


def kuhn_cube(M: int, jitter: float = 0.0, seed: int = 20241016) -> TetMesh:
    """M^3 cells x 6 tets on [0,1]^3; node id = i + (M+1)(j + (M+1)k)."""
    n1 = M + 1
    N = n1 ** 3
    ids = np.arange(N, dtype=np.int64)
    ii = ids % n1
    jj = (ids // n1) % n1
    kk = ids // (n1 * n1)
    xg = np.stack([ii, jj, kk], axis=1).astype(np.float64) / M
    if jitter > 0.0:
        rng = np.random.default_rng(seed)
        d = rng.uniform(-jitter / M, jitter / M, size=(N, 3))
        interior = (ii > 0) & (ii < M) & (jj > 0) & (jj < M) & (kk > 0) & (kk < M)
        xg[interior] += d[interior]

    c = np.arange(M ** 3, dtype=np.int64)
    ci = c % M
    cj = (c // M) % M
    ck = c // (M * M)
    base = ci + n1 * (cj + n1 * ck)
    strides = (1, n1, n1 * n1)
    ien = np.empty((M ** 3, 6, 4), dtype=np.int32)
    for t, p in enumerate(_PERMS):
        v0 = base
        v1 = v0 + strides[p[0]]
        v2 = v1 + strides[p[1]]
        v3 = v2 + strides[p[2]]
        if _perm_is_odd(p):
            v1, v2 = v2, v1  # restore positive orientation
        ien[:, t, 0] = v0
        ien[:, t, 1] = v1
        ien[:, t, 2] = v2
        ien[:, t, 3] = v3
    ien = ien.reshape(-1, 4)

    node_off = [0]
    elem_off = [0]
    nodes, bien, f2e, forn = [], [], [], []
    ccoord = (ci, cj, ck)
    for ax in range(3):
        for side in (0, M):
            # only the cell layer touching the plane can hold boundary faces
            layer = np.nonzero(ccoord[ax] == (0 if side == 0 else M - 1))[0]
            cand = (layer[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
            sub = ien[cand].astype(np.int64)
            on = ((sub // strides[ax]) % n1) == side
            is_face = on.sum(axis=1) == 3
            tets = cand[is_face]
            on = on[is_face]
            opp = np.argmin(on, axis=1)  # the single False entry
            face_nodes = ien[tets][on].reshape(-1, 3)
            nodes.append(np.unique(face_nodes))
            bien.append(face_nodes.reshape(-1))
            f2e.append(tets.astype(np.int32))
            forn.append(opp.astype(np.int32))
            node_off.append(node_off[-1] + nodes[-1].size)
            elem_off.append(elem_off[-1] + tets.size)
    return TetMesh(
        M=M,
        xg=np.ascontiguousarray(xg.reshape(-1)),
        ien=np.ascontiguousarray(ien.reshape(-1)),
        bound_node_offset=np.asarray(node_off, dtype=np.int32),
        bound_node=np.concatenate(nodes).astype(np.int32),
        bound_elem_offset=np.asarray(elem_off, dtype=np.int32),
        bound_ien=np.concatenate(bien).astype(np.int32),
        bound_f2e=np.concatenate(f2e).astype(np.int32),
        bound_forn=np.concatenate(forn).astype(np.int32),
    )


def single_tet() -> TetMesh:
    """Reference-tet mesh with all four faces as boundary groups (cf. the
    DBG_TET configuration, ``src/main.c:357-361``)."""
    xg = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)
    ien = np.array([0, 1, 2, 3], dtype=np.int32)
    node_off, elem_off, nodes, bien, f2e, forn = [0], [0], [], [], [], []
    for opp in range(4):
        fn = np.array([v for v in range(4) if v != opp], dtype=np.int32)
        nodes.append(fn)
        bien.append(fn)
        f2e.append(np.array([0], dtype=np.int32))
        forn.append(np.array([opp], dtype=np.int32))
        node_off.append(node_off[-1] + 3)
        elem_off.append(elem_off[-1] + 1)
    return TetMesh(1, xg, ien, np.asarray(node_off, np.int32), np.concatenate(nodes),
                   np.asarray(elem_off, np.int32), np.concatenate(bien),
                   np.concatenate(f2e), np.concatenate(forn))


def synthetic_fields(mesh: TetMesh, seed_dw: int = 7):
    """wgalpha / dwgalpha of length 6N in the layout [u: Nx3 AoS | p | phi | T]
    (``src/main.c:108-118``).  u = e_x + 0.1 sin(2 pi x_perm), p-slot of wgalpha
    zero (``src/main.c:118``), phi = x, T = -x (cf. ``src/main.c:301-319``);
    dwgalpha = 0.1 * uniform[-1,1] including the pressure slot."""
    N = mesh.num_node
    x = mesh.xg.reshape(-1, 3)
    wg = np.zeros(6 * N)
    u = np.zeros((N, 3))
    u[:, 0] = 1.0 + 0.1 * np.sin(2 * np.pi * x[:, 1])
    u[:, 1] = 0.1 * np.sin(2 * np.pi * x[:, 2])
    u[:, 2] = 0.1 * np.sin(2 * np.pi * x[:, 0])
    wg[: 3 * N] = u.reshape(-1)
    wg[4 * N: 5 * N] = x[:, 0]
    wg[5 * N: 6 * N] = -x[:, 0]
    rng = np.random.default_rng(seed_dw)
    dwg = 0.1 * rng.uniform(-1.0, 1.0, size=6 * N)
    return wg, dwg


def dem_particles(P: int, radius: float, seed_x: int = 11, seed_v: int = 12):
    """DEM inputs of SURVEY.md section 8(d): centres uniform in the unit cube,
    velocities N(0, 0.1^2)."""
    x = np.random.default_rng(seed_x).uniform(0.0, 1.0, size=(P, 3))
    v = np.random.default_rng(seed_v).normal(0.0, 0.1, size=(P, 3))
    return np.ascontiguousarray(x.reshape(-1)), np.ascontiguousarray(v.reshape(-1)), radius


def dem_particles_poly(P: int, r_lo: float, r_hi: float, seed: int = 14):
    """P non-overlapping spheres in the unit box: radii uniform in [r_lo, r_hi], centres by random sequential addition
    (uniform in [r, 1 - r]^3, a candidate that overlaps an accepted sphere is drawn again).  Returns (x (P, 3), r (P,));
    raises ValueError when the box is too full to place them."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(r_lo, r_hi, size=P)
    h = 2.0 * r_hi  # grid cell: the neighbours of a candidate lie in the 27 cells around it
    n = max(1, int(1.0 / h))
    grid = {}
    x = np.empty((P, 3))
    for i in range(P):
        for _ in range(1000):
            c = rng.uniform(r[i], 1.0 - r[i], size=3)
            k = np.minimum((c * n).astype(int), n - 1)
            ok = True
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        for j in grid.get((k[0] + dx, k[1] + dy, k[2] + dz), ()):
                            d = c - x[j]
                            if d @ d < (r[i] + r[j]) ** 2:
                                ok = False
                                break
                        if not ok:
                            break
                    if not ok:
                        break
                if not ok:
                    break
            if ok:
                x[i] = c
                grid.setdefault((k[0], k[1], k[2]), []).append(i)
                break
        else:
            raise ValueError(f"dem_particles_poly: no room for particle {i} of {P}")
    return np.ascontiguousarray(x), r


def dem_lattice(lo, hi, radius: float, spacing: float | None = None, kind: str = "sc", jitter: float = 0.0, seed: int = 13,
                max_particles: int | None = None):
    """DEM centres on a simple-cubic ("sc") or face-centred cubic ("fcc") lattice filling the box [lo + R, hi - R], in
    x-fastest order.  spacing = the nearest-neighbour distance (default 1.9 R: every neighbour pair overlaps by 0.1 R, 6
    contacts per interior particle on "sc", 12 on "fcc"); jitter = uniform displacement of up to jitter * R per
    coordinate; max_particles keeps the first ones (the lowest layers).  Returns x as (P, 3)."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    s = 1.9 * radius if spacing is None else float(spacing)
    if kind == "sc":
        a, basis = s, np.zeros((1, 3))
    elif kind == "fcc":
        a = s * np.sqrt(2.0)
        basis = 0.5 * np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]], float)
    else:
        raise ValueError(kind)
    first, last = lo + radius, hi - radius
    n = np.floor((last - first) / a + 1e-9).astype(int) + 1
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(float)
    x = first + a * (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3)
    x = x[np.all(x <= last + 1e-12, axis=1)]
    x = x[np.lexsort((x[:, 0], x[:, 1], x[:, 2]))]
    if max_particles is not None:
        x = x[:max_particles]
    if jitter:
        x = x + np.random.default_rng(seed).uniform(-jitter * radius, jitter * radius, size=x.shape)
    return np.ascontiguousarray(x)


def fan_mesh(num_surface: int = 40, seed: int = 5) -> TetMesh:
    """A ball of tets around ONE central vertex: `num_surface` points on the unit sphere, their convex hull triangulated
    (2 V - 4 triangles), every triangle joined to the centre.  The central vertex is shared by 2 V - 4 tets -- V = 40 gives
    76, more than the 64 conflict-free classes of the compact assembly schedule, with a nodal row of V + 1 = 41 nonzeros
    (inside the reference's 64 per row, csr.c:10) and 76 JPL colors (inside its 256).  Boundary group 0 = the whole surface,
    groups 1-5 empty."""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(num_surface, 3))
    p /= np.linalg.norm(p, axis=1)[:, None]
    p *= rng.uniform(0.8, 1.0, size=(num_surface, 1))   # not all on one sphere: breaks symmetry, still star-shaped
    hull = ConvexHull(p / np.linalg.norm(p, axis=1)[:, None])
    tri = hull.simplices.astype(np.int64)
    xg = np.vstack([np.zeros((1, 3)), p])               # node 0 = the centre
    tets = np.column_stack([np.zeros(len(tri), np.int64), tri + 1])
    x = xg[tets]
    vol = np.einsum("ij,ij->i", np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]), x[:, 3] - x[:, 0])
    flip = vol < 0
    tets[flip, 2], tets[flip, 3] = tets[flip, 3].copy(), tets[flip, 2].copy()
    nf = len(tets)
    surf = np.arange(1, num_surface + 1, dtype=np.int32)
    return TetMesh(M=0, xg=np.ascontiguousarray(xg.reshape(-1)), ien=np.ascontiguousarray(tets.reshape(-1).astype(np.int32)),
                   bound_node_offset=np.array([0] + [num_surface] * 6, np.int32), bound_node=surf,
                   bound_elem_offset=np.array([0] + [nf] * 6, np.int32),
                   bound_ien=np.ascontiguousarray(tets[:, 1:].reshape(-1).astype(np.int32)),
                   bound_f2e=np.arange(nf, dtype=np.int32), bound_forn=np.zeros(nf, np.int32))


def kuhn_box(M, lo, hi, keep=None) -> TetMesh:
    """Kuhn tets (6 per cell, as kuhn_cube) on the axis-aligned box [lo, hi] with M cells per axis (an int, or one per
    axis).  keep(i, j, k) -> bool drops whole cells (e.g. a quadrant for an L-shape); nodes no kept cell uses are removed
    and the others renumbered in order.  Boundary groups are re-derived from the exposed tet faces by outward normal, in the
    order x-, x+, y-, y+, z-, z+ (faces of a group by parent tet, then local face); forn / f2e as in kuhn_cube."""
    Ms = np.broadcast_to(np.asarray(M, dtype=np.int64), (3,))
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n1 = Ms + 1
    strides = (1, int(n1[0]), int(n1[0] * n1[1]))
    ids = np.arange(int(np.prod(n1)), dtype=np.int64)
    ijk = np.stack([ids % n1[0], (ids // n1[0]) % n1[1], ids // (n1[0] * n1[1])], axis=1)
    xg = lo[None, :] + (hi - lo)[None, :] * (ijk / Ms[None, :])

    c = np.arange(int(np.prod(Ms)), dtype=np.int64)
    ci, cj, ck = c % Ms[0], (c // Ms[0]) % Ms[1], c // (Ms[0] * Ms[1])
    if keep is not None:
        mask = np.array([bool(keep(int(a), int(b), int(d))) for a, b, d in zip(ci, cj, ck)], dtype=bool)
        ci, cj, ck = ci[mask], cj[mask], ck[mask]
    base = ci + strides[1] * cj + strides[2] * ck
    ien = np.empty((base.size, 6, 4), dtype=np.int64)
    for t, p in enumerate(_PERMS):
        v0 = base
        v1 = v0 + strides[p[0]]
        v2 = v1 + strides[p[1]]
        v3 = v2 + strides[p[2]]
        if _perm_is_odd(p):
            v1, v2 = v2, v1
        ien[:, t, 0], ien[:, t, 1], ien[:, t, 2], ien[:, t, 3] = v0, v1, v2, v3
    ien = ien.reshape(-1, 4)
    used = np.unique(ien)
    renum = np.full(ids.size, -1, dtype=np.int64)
    renum[used] = np.arange(used.size)
    ien = renum[ien]
    xg = xg[used]

    # exposed faces: (tet, local face opposite vertex k) whose sorted node triple occurs once
    faces = np.stack([np.sort(np.delete(ien, k, axis=1), axis=1) for k in range(4)], axis=1).reshape(-1, 3)
    _, inv, cnt = np.unique(faces, axis=0, return_inverse=True, return_counts=True)
    exposed = np.nonzero(cnt[inv.reshape(-1)] == 1)[0]
    tet, opp = exposed // 4, exposed % 4
    fn = np.stack([np.delete(ien[t], k) for t, k in zip(tet, opp)]) if exposed.size else np.zeros((0, 3), np.int64)
    x = xg[fn]
    nrm = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])   # axis-aligned: every exposed face lies on a cell face
    axis = np.argmax(np.abs(nrm), axis=1)
    away = x[:, 0] - xg[ien[tet, opp]]                      # from the opposite vertex towards the face: outward
    side = (away[np.arange(axis.size), axis] > 0).astype(np.int64)
    group = 2 * axis + side
    node_off, elem_off, nodes, bien, f2e, forn = [0], [0], [], [], [], []
    for g in range(6):
        sel = np.nonzero(group == g)[0]
        sel = sel[np.lexsort((opp[sel], tet[sel]))]
        nodes.append(np.unique(fn[sel]))
        bien.append(fn[sel].reshape(-1))
        f2e.append(tet[sel])
        forn.append(opp[sel])
        node_off.append(node_off[-1] + nodes[-1].size)
        elem_off.append(elem_off[-1] + sel.size)
    return TetMesh(
        M=int(Ms.max()),
        xg=np.ascontiguousarray(xg.reshape(-1)),
        ien=np.ascontiguousarray(ien.reshape(-1).astype(np.int32)),
        bound_node_offset=np.asarray(node_off, dtype=np.int32),
        bound_node=np.concatenate(nodes).astype(np.int32),
        bound_elem_offset=np.asarray(elem_off, dtype=np.int32),
        bound_ien=np.concatenate(bien).astype(np.int32),
        bound_f2e=np.concatenate(f2e).astype(np.int32),
        bound_forn=np.concatenate(forn).astype(np.int32),
    )
