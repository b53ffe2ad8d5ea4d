"""numpy model of the surface mesh (include/dedflow.h, "surface mesh"), written from the header: the welded, oriented triangles
of phi = level with one vertex per cut mesh edge.  The crossing points are those of redistance_model._crossing and the triangle
order that of redistance_model.facets, so the shared arithmetic has one statement; the orientation is the table SWAP below.  In
float64 every operation has the association the header states, so a correct kernel agrees to the last bit; dtype=np.longdouble
runs the coordinates, areas and volumes in extended precision (every decision is taken from the float64 input either way).
Test infrastructure only; shared by test_surface_mesh_cpu.py and test_gpu_surface_mesh.py."""
import numpy as np

import redistance_model as rm

LD = np.longdouble
MAX_FIELDS = 8
COUNTS = ("vertices", "triangles", "bad_nodes", "bad_tets", "degenerate_tets")

# bit m of SWAP: in a tet with a positive determinant (tet_cross) and the mask m of metal nodes, the facets of lf_tet_facets have
# their normal (B - A) x (C - A) pointing into the metal, so the second and third index are swapped; a negative determinant
# inverts the answer.  derive_swap() recomputes it from geometry.
SWAP = 0x4D24


def derive_swap():
    """the table from one well-shaped tet per mask in longdouble: bit m set when n . g > 0 for a positive determinant"""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    ien = np.array([[0, 1, 2, 3]])
    table = 0
    for mask in range(1, 15):
        f = np.array([0.7 + 0.1 * a if (mask >> a) & 1 else -0.6 - 0.05 * a for a in range(4)])
        F, _ = rm.facets(x.reshape(-1), ien, f, 0.0, LD)
        g = gradient(x.astype(LD)[None], f.astype(LD)[None])[0]
        s = [float(rm.dot(normals(F.reshape(-1, 3, 3))[k], g)) for k in range(len(F))]
        assert all(v > 0 for v in s) or all(v < 0 for v in s), (mask, s)
        table |= (s[0] > 0) << mask
    return table


def refusal(cfg):
    """why DflSurfaceMeshCheck refuses the configuration, or None"""
    if not np.isfinite(cfg["level"]):
        return "level"
    if cfg["side"] not in (1, -1):
        return "side"
    if cfg["every"] < 0:
        return "every"
    return None


def config(level=0.0, side=1, every=0):
    return dict(level=level, side=side, every=every)


def det(x):
    """the tet's determinant in the association of tet_cross: x [n, 4, 3]"""
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    return rm.dot(e1, rm.cross(e2, e3))


def gradient(x, f):
    """g = sum_a f_a grad N_a of the tets x [n, 4, 3], f [n, 4]"""
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = rm.cross(e2, e3), rm.cross(e3, e1), rm.cross(e1, e2)
    d = rm.dot(e1, c23)
    return ((f[:, 1] - f[:, 0])[:, None] * c23 + (f[:, 2] - f[:, 0])[:, None] * c31 + (f[:, 3] - f[:, 0])[:, None] * c12) / d[:, None]


def normals(P):
    """(B - A) x (C - A) of the triangles P [n, 3, 3]"""
    return rm.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])


def areas(P):
    n = normals(P)
    return 0.5 * np.sqrt(rm.dot(n, n))


def tree_sum(v):
    """the fixed tree of the totals: workgroups of 256 consecutive entries (the xor tree inside every wave of 64, then waves 1,
    2, 3 into wave 0), the workgroups then by one workgroup (thread t takes t, t + 256, ... from +0.0; then the same tree)"""
    def block(a):                                                           # [nb, 256] -> [nb]
        a = a.reshape(-1, 4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            a = a + a[:, :, lane ^ off]
        w = a[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    v = np.asarray(v)
    if v.size == 0:
        return v.dtype.type(0.0)
    nb = -(-v.size // 256)
    part = block(np.concatenate([v, np.zeros(nb * 256 - v.size, v.dtype)]))
    rows = -(-nb // 256)
    p = np.concatenate([part, np.zeros(rows * 256 - nb, v.dtype)]).reshape(rows, 256)
    acc = np.zeros(256, v.dtype)
    for r in range(rows):
        take = np.arange(256) + 256 * r < nb
        acc = np.where(take, acc + p[r], acc)
    return block(acc[None])[0]


def facet_edges(pos):
    """per cut tet the local (i, j) of every facet vertex, i metal, in the order of lf_tet_facets: edges [n, 4, 2] (a tet's three
    or four crossing points), corner [n, 2, 3] (which of them every triangle takes), ntri [n]"""
    n = len(pos)
    npos = pos.sum(axis=1)
    order = np.argsort(~pos, axis=1, kind="stable")                        # metal first, each part in local order
    edges = np.zeros((n, 4, 2), np.int64)
    corner = np.zeros((n, 2, 3), np.int64)
    corner[:, 0] = (0, 1, 2)
    corner[:, 1] = (0, 2, 3)
    k = npos == 1
    for v in range(3):
        edges[k, v, 0], edges[k, v, 1] = order[k, 0], order[k, 1 + v]
    k = npos == 3
    for v in range(3):
        edges[k, v, 0], edges[k, v, 1] = order[k, v], order[k, 3]
    k = npos == 2
    a, b, c, d = (order[k, q] for q in range(4))
    for v, (i, j) in enumerate(((a, c), (a, d), (b, d), (b, c))):
        edges[k, v, 0], edges[k, v, 1] = i, j
    return edges, corner, np.where(npos == 2, 2, 1)


def evaluate(xg, ien, phi, cfg, fields=(), dtype=np.float64):
    """dict: verts [nv, 3], edge [nv, 2] (metal node first), t [nv], vals [nv, K], tris [nt, 3], tri_tet [nt], keys [nv]
    (uint64), the counts, area (the tree sum), tri_area [nt], emit = the ids of the emitting tets"""
    ien = np.asarray(ien).reshape(-1, 4).astype(np.int64)
    x64 = np.asarray(xg, np.float64).reshape(-1, 3)
    phi = np.asarray(phi, np.float64)
    level, side = float(cfg["level"]), int(cfg["side"])
    with np.errstate(invalid="ignore", over="ignore"):
        f = phi - level
        if side < 0:
            f = -f
        bad = ~np.isfinite(phi)
        metal = ~bad & (f > 0)
    bad_t = bad[ien].any(axis=1)
    npos = metal[ien].sum(axis=1)
    cut = ~bad_t & (npos > 0) & (npos < 4)
    with np.errstate(all="ignore"):
        d = det(x64[ien])
    degenerate = cut & ~(np.isfinite(d) & (d != 0))
    emit = np.flatnonzero(cut & ~degenerate)
    e_ien = ien[emit]
    pos = metal[e_ien]
    mask = (pos * (1 << np.arange(4))).sum(axis=1)
    edges, corner, ntri = facet_edges(pos)
    nedge = np.where(ntri == 2, 4, 3)
    r = np.arange(len(emit))[:, None]
    ni, nj = e_ien[r, edges[:, :, 0]], e_ien[r, edges[:, :, 1]]           # [n, 4] global nodes, metal first
    key4 = (np.minimum(ni, nj).astype(np.uint64) << np.uint64(32)) | np.maximum(ni, nj).astype(np.uint64)
    valid = np.arange(4)[None, :] < nedge[:, None]
    keys, first = np.unique(key4[valid], return_index=True)
    vi, vj = ni[valid][first], nj[valid][first]
    x = x64.astype(dtype)
    fd = f.astype(dtype)
    pair_x = np.stack([x[vi], x[vj]], axis=1) if len(keys) else np.zeros((0, 2, 3), dtype)
    pair_f = np.stack([fd[vi], fd[vj]], axis=1) if len(keys) else np.zeros((0, 2), dtype)
    verts = rm._crossing(pair_x, pair_f, 0, np.ones(len(keys), np.int64))
    with np.errstate(all="ignore"):
        t = pair_f[:, 0] / (pair_f[:, 0] - pair_f[:, 1])
        vals = np.zeros((len(keys), len(fields)), dtype)
        for k, q in enumerate(fields):
            q = np.asarray(q, np.float64).astype(dtype)
            vals[:, k] = q[vi] + t * (q[vj] - q[vi])
    vid = np.searchsorted(keys, key4)                                       # [n, 4] (garbage where not valid)
    swap = ((SWAP >> mask) & 1).astype(bool) ^ (d[emit] < 0)
    tri4 = vid[r[:, :, None], corner]                                       # [n, 2, 3]
    tri4 = np.where(swap[:, None, None], tri4[:, :, [0, 2, 1]], tri4)
    keep = np.arange(2)[None, :] < ntri[:, None]
    tris = tri4[keep].astype(np.int32).reshape(-1, 3)
    tri_tet = np.repeat(emit, ntri).astype(np.int32)
    tri_area = areas(verts[tris]) if len(tris) else np.zeros(0, dtype)
    return dict(verts=verts, edge=np.stack([vi, vj], axis=1).astype(np.int32).reshape(-1, 2), t=t, vals=vals, tris=tris,
                tri_tet=tri_tet, keys=keys, vertices=len(keys), triangles=len(tris), bad_nodes=int(bad.sum()),
                bad_tets=int(bad_t.sum()), degenerate_tets=int(degenerate.sum()), area=tree_sum(tri_area), tri_area=tri_area,
                emit=emit, keys_raw=int(valid.sum()))


def soup(res):
    """verts[tris]: [nt, 9]"""
    return res["verts"][res["tris"]].reshape(-1, 9)


def edge_uses(tris):
    """dict directed edge (a, b) -> uses"""
    uses = {}
    for a, b, c in np.asarray(tris).tolist():
        for e in ((a, b), (b, c), (c, a)):
            uses[e] = uses.get(e, 0) + 1
    return uses


def manifold(tris):
    """(open edges as a list of directed pairs, closed = every other edge is used exactly once in each direction)"""
    uses = edge_uses(tris)
    ok = all(n == 1 for n in uses.values())
    open_edges = [e for e in uses if (e[1], e[0]) not in uses]
    return open_edges, ok


def enclosed_volume(verts, tris, dtype=np.float64):
    """(1/6) sum A . (B x C) and the sum of the absolute terms"""
    P = np.asarray(verts).astype(dtype)[np.asarray(tris)]
    term = rm.dot(P[:, 0], rm.cross(P[:, 1], P[:, 2])) / dtype(6.0)
    return term.sum(dtype=dtype), np.abs(term).sum(dtype=dtype)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
def coords(mesh):
    return np.asarray(mesh.xg, np.float64).reshape(-1, 3)


def inclined_plane(mesh):
    x = coords(mesh)
    return 0.53 - (0.31 * x[:, 0] + 0.17 * x[:, 1] + 0.83 * x[:, 2])


def sphere(mesh, r=0.3, c=(0.5, 0.5, 0.5)):
    return r - np.linalg.norm(coords(mesh) - np.asarray(c), axis=1)


def node_plane(mesh, z0=0.5):
    return z0 - coords(mesh)[:, 2]


def wavy(mesh):
    x = coords(mesh)
    return 0.5 + 0.1 * np.sin(2 * np.pi * x[:, 0]) * np.cos(2 * np.pi * x[:, 1]) - x[:, 2]


def nodal_fields(mesh, K):
    """K nodal fields with no two equal values"""
    x = coords(mesh)
    n = np.arange(len(x))
    return [1500.0 / (k + 1) + (400.0 - 35.0 * k) * x[:, k % 3] - 250.0 * x[:, (k + 1) % 3] ** 2 + 0.001 * n for k in range(K)]


def state(mesh, phi, T=None):
    """w [6N] with phi and T; u and p are numbers nobody reads"""
    N = mesh.num_node
    w = np.zeros(6 * N)
    w[:4 * N] = 0.25 + 0.001 * np.arange(4 * N)
    w[4 * N:5 * N] = phi
    w[5 * N:] = nodal_fields(mesh, 1)[0] if T is None else T
    return w
