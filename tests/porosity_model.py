"""numpy model of the porosity record (include/dedflow.h, "porosity record"), written from the header: the labels from
scipy's connected components on the gas-node graph, relabelled to the smallest node id; the volumes, boxes and extremes in
float64 in the header's operation order (a correct kernel agrees to the last bit where the header fixes the order); np.longdouble
sums for the bound of the volumes.  And the scenes of the tests, each with what it promises.  Test infrastructure only; shared by
test_porosity_cpu.py (the model against a flood fill, the scenes' promises) and test_gpu_porosity.py (the kernels against the
model)."""
import dataclasses

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, shortest_path

import redistance_model as rm

LD = np.longdouble
INF = float("inf")
MAX_PORES = 65536
Z_PLUS = 1 << 5                 # the group z+ of a Kuhn cube: the atmosphere of the scenes
PORE_KEYS = ("label", "nodes", "tets", "volume", "volume_scale", "lo", "hi", "T_wall_min", "T_wall_max")
COUNTS = ("components", "pores", "listed", "bad_nodes", "bad_tets")
TOTALS = ("volume_metal", "volume_open", "volume_pores")


def config(level=0.0, side=1, open_groups=0, max_pores=1024, every=0):
    return dict(level=level, side=side, open_groups=open_groups, max_pores=max_pores, every=every)


def refusal(cfg):
    """why DflPorosityCheck refuses the configuration, or None"""
    if not np.isfinite(cfg["level"]):
        return "level"
    if cfg["side"] not in (1, -1):
        return "side"
    if cfg["open_groups"] < 0:
        return "open_groups"
    if not 1 <= cfg["max_pores"] <= MAX_PORES:
        return "max_pores"
    if cfg["every"] < 0:
        return "every"
    return None


def classify(phi, level, side):
    """(metal, gas, bad, f) per node"""
    phi = np.asarray(phi, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        f = phi - level
        if side < 0:
            f = -f
        bad = ~np.isfinite(phi)
        metal = ~bad & (f > 0)
    return metal, ~bad & ~metal, bad, f


def gas_graph(ien, gas, good, N):
    """the symmetric adjacency of the gas nodes: an edge where two of them share a tet without a bad node"""
    g = gas[ien] & good[:, None]
    r, c = [], []
    for a in range(4):
        for b in range(a + 1, 4):
            sel = g[:, a] & g[:, b]
            r.append(ien[sel, a])
            c.append(ien[sel, b])
    r, c = np.concatenate(r), np.concatenate(c)
    return coo_matrix((np.ones(2 * r.size, np.int8), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(N, N)).tocsr()


def labels(mesh, phi, level, side):
    """label [N]: the smallest node id of a gas node's component, -1 for metal, -2 for bad"""
    N = mesh.num_node
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    metal, gas, bad, _ = classify(phi, level, side)
    good = ~bad[ien].any(axis=1)
    _, comp = connected_components(gas_graph(ien, gas, good, N), directed=False)
    low = np.full(comp.max() + 1, N, np.int64)
    np.minimum.at(low, comp, np.arange(N))
    return np.where(gas, low[comp], np.where(bad, -2, -1)).astype(np.int32)


def flood_fill_labels(mesh, phi, level, side):
    """the same labels by a plain flood fill from every gas node in ascending id (small meshes)"""
    N = mesh.num_node
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    metal, gas, bad, _ = classify(phi, level, side)
    nbr = [set() for _ in range(N)]
    for tet in ien:
        if bad[tet].any():
            continue
        g = [int(a) for a in tet if gas[a]]
        for a in g:
            nbr[a].update(g)
    label = np.where(bad, -2, -1).astype(np.int32)
    for a in range(N):
        if not gas[a] or label[a] >= 0:
            continue
        label[a] = a
        stack = [a]
        while stack:
            for b in nbr[stack.pop()]:
                if label[b] < 0:
                    label[b] = a
                    stack.append(b)
    return label


def open_labels(mesh, label, open_groups):
    """the labels of the components that hold a node of a boundary face of a masked group (bound_f2e / bound_forn)"""
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    out = set()
    for g in range(min(mesh.num_bound, 31)):
        if not (open_groups >> g) & 1:
            continue
        for f in range(mesh.bound_elem_offset[g], mesh.bound_elem_offset[g + 1]):
            tet, opp = ien[mesh.bound_f2e[f]], mesh.bound_forn[f]
            out.update(int(label[tet[a]]) for a in range(4) if a != opp and label[tet[a]] >= 0)
    return out


def _seq_sum(v):
    """the sum from +0.0 in order"""
    return float(np.cumsum(np.concatenate([[0.0], v]))[-1])


def _lowest(v):
    """min where a NaN never wins, +inf of nothing; a zero is +0.0"""
    return float(np.fmin.reduce(np.asarray(v, np.float64).ravel(), initial=INF)) + 0.0


def _highest(v):
    return float(np.fmax.reduce(np.asarray(v, np.float64).ravel(), initial=-INF)) + 0.0


def evaluate(mesh, w, cfg):
    """dict: label, pore [N] int32; list = the listed pores (PORE_KEYS, and ld_volume = the longdouble sum); the counts and
    the three totals as longdouble sums, mesh_volume, porosity"""
    N = mesh.num_node
    w = np.asarray(w, np.float64)
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    x = np.asarray(mesh.xg, np.float64).reshape(-1, 3)
    phi, T = w[4 * N:5 * N], w[5 * N:6 * N]
    level, side = float(cfg["level"]), int(cfg["side"])
    metal, gas, bad, f = classify(phi, level, side)
    label = labels(mesh, phi, level, side)
    good = ~bad[ien].any(axis=1)
    has_gas = good & gas[ien].any(axis=1)
    comp_t = np.where(has_gas, label[ien[np.arange(len(ien)), np.argmax(gas[ien], axis=1)]], -1)
    opened = open_labels(mesh, label, int(cfg["open_groups"]))
    comps = np.unique(label[label >= 0])
    pores = np.array([c for c in comps if int(c) not in opened], np.int64)
    rank = {int(c): k for k, c in enumerate(pores)}
    pore = np.array([rank.get(int(l), -1) for l in label], np.int32)
    closed_t = np.array([int(c) in rank for c in comp_t])
    with np.errstate(all="ignore"):
        # (-phi) - (-level) = -(phi - level) to the last bit: the volume of {f > 0} for either side
        vp, full = rm.tet_volumes(mesh.xg, ien, side * phi, side * level, np.float64)
        vpL, fullL = rm.tet_volumes(mesh.xg, ien, side * phi, side * level, LD)
        gas_v, gas_L = full - vp, fullL - vpL
    gas_v, gas_L = np.where(np.isnan(gas_v), 0.0, gas_v), np.where(np.isnan(gas_L), LD(0), gas_L)
    listed = min(len(pores), int(cfg["max_pores"]))
    rows = []
    for c in pores[:listed]:
        idx = np.flatnonzero(comp_t == c)
        nodes = np.flatnonzero(label == c)
        pts = [x[nodes]]
        walls = []
        for j in range(4):
            mj = metal[ien[idx, j]]
            walls.append(T[ien[idx[mj], j]])
            for i in range(4):
                sel = idx[mj & gas[ien[idx, i]]]
                if sel.size:
                    fi, fj = f[ien[sel, i]], f[ien[sel, j]]
                    xi, xj = x[ien[sel, i]], x[ien[sel, j]]
                    with np.errstate(all="ignore"):
                        t = fi / (fi - fj)
                        pts.append(xi + t[:, None] * (xj - xi))
        pts = np.concatenate(pts)
        walls = np.concatenate(walls) if walls else np.zeros(0)
        rows.append(dict(label=int(c), nodes=int(nodes.size), tets=int(idx.size), volume=_seq_sum(gas_v[idx]),
                         volume_scale=_seq_sum(full[idx]), lo=tuple(_lowest(pts[:, d]) for d in range(3)),
                         hi=tuple(_highest(pts[:, d]) for d in range(3)), T_wall_min=_lowest(walls), T_wall_max=_highest(walls),
                         ld_volume=gas_L[idx].sum(dtype=LD), ld_scale=fullL[idx].sum(dtype=LD)))
    vm, vo, vc = vpL[good].sum(dtype=LD), gas_L[has_gas & ~closed_t].sum(dtype=LD), gas_L[has_gas & closed_t].sum(dtype=LD)
    both = float(vm) + float(vc)
    return dict(label=label, pore=pore, list=rows, components=int(comps.size), pores=int(len(pores)), listed=listed,
                bad_nodes=int(bad.sum()), bad_tets=int((~good).sum()), volume_metal=vm, volume_open=vo, volume_pores=vc,
                mesh_volume=fullL.sum(dtype=LD), closed_tets=int((has_gas & closed_t).sum()),
                porosity=float(vc) / both if both > 0 else 0.0)


# ---- the scenes -------------------------------------------------------------------------------------------------------------------
def lattice(mesh):
    """the integer coordinates (i, j, k) of a Kuhn cube's nodes"""
    n1 = mesh.M + 1
    ids = np.arange(mesh.num_node)
    return np.stack([ids % n1, (ids // n1) % n1, ids // (n1 * n1)], axis=1)


def temperature(mesh):
    """a T with no two equal values on a Kuhn cube or the fan"""
    x = np.asarray(mesh.xg).reshape(-1, 3)
    return 1500.0 + 400.0 * x[:, 0] - 250.0 * x[:, 1] + 90.0 * x[:, 2] * x[:, 0] + 0.001 * np.arange(len(x))


def state(mesh, phi, T=None, side=1):
    """w [6N] with phi (negated for side = -1: the same metal) and T; u and p are numbers nobody reads"""
    N = mesh.num_node
    w = np.zeros(6 * N)
    w[:4 * N] = 0.25 + 0.001 * np.arange(4 * N)
    w[4 * N:5 * N] = np.asarray(phi, np.float64) * (1.0 if side > 0 else -1.0)
    w[5 * N:] = temperature(mesh) if T is None else T
    return w


def plane(mesh, z0=0.55, side=1, open_groups=Z_PLUS, **kw):
    """metal below z = z0, gas above: no pore and one open component; with open_groups = 0 the atmosphere is the one pore"""
    x = np.asarray(mesh.xg).reshape(-1, 3)
    return config(level=0.0, side=side, open_groups=open_groups, **kw), state(mesh, z0 - x[:, 2], side=side)


def spheres(mesh, balls, z0=0.8, side=1, open_groups=Z_PLUS, **kw):
    """gas above z = z0 and inside the balls (centre, radius), metal elsewhere"""
    x = np.asarray(mesh.xg).reshape(-1, 3)
    phi = z0 - x[:, 2]
    for c, r in balls:
        phi = np.minimum(phi, np.linalg.norm(x - np.asarray(c), axis=1) - r)
    return config(level=0.0, side=side, open_groups=open_groups, **kw), state(mesh, phi, side=side)


ONE_BUBBLE = [((0.5, 0.5, 0.4), 0.2)]
TWO_BUBBLES = [((0.3, 0.3, 0.3), 0.17), ((0.7, 0.7, 0.45), 0.17)]
WALL_BUBBLE = [((0.0, 0.5, 0.35), 0.22)]       # touches the group x- (bit 0)


def boxes(mesh, blocks, side=1, open_groups=Z_PLUS, z_gas=None, **kw):
    """gas at the lattice nodes inside the blocks ((i0, i1), (j0, j1), (k0, k1)), inclusive, and in the layers k >= z_gas; metal
    elsewhere, phi = +-1"""
    ijk = lattice(mesh)
    gas = np.zeros(mesh.num_node, bool) if z_gas is None else ijk[:, 2] >= z_gas
    for b in blocks:
        gas |= np.all([(ijk[:, d] >= b[d][0]) & (ijk[:, d] <= b[d][1]) for d in range(3)], axis=0)
    return config(level=0.0, side=side, open_groups=open_groups, **kw), state(mesh, np.where(gas, -1.0, 1.0), side=side)


TOUCHING = [((3, 5), (3, 5), (3, 5)), ((5, 7), (5, 7), (5, 7))]      # cube13: the two blocks share the node (5, 5, 5) alone
SEPARATED = [((3, 5), (3, 5), (3, 5)), ((7, 9), (7, 9), (7, 9))]     # one layer of metal nodes (6) between them


def snake_nodes(mesh, k=6):
    """cube13: the lattice nodes of a one-node-wide serpentine in the layer k, in path order: the rows j = 1, 3, .. 11 over
    i = 1 .. 12, joined at alternating ends through the node of the row between"""
    n1 = mesh.M + 1
    path = []
    for r, j in enumerate(range(1, 12, 2)):
        run = list(range(1, 13)) if r % 2 == 0 else list(range(12, 0, -1))
        path += [(i, j) for i in run]
        if j + 2 < 12:
            path.append((run[-1], j + 1))
    return np.array([i + n1 * (j + n1 * k) for i, j in path])


def snake(mesh, side=1, open_groups=Z_PLUS, **kw):
    gas = np.zeros(mesh.num_node, bool)
    gas[snake_nodes(mesh)] = True
    return config(level=0.0, side=side, open_groups=open_groups, **kw), state(mesh, np.where(gas, -0.5, 1.0), side=side)


def graph_diameter(mesh, w, cfg, label_of):
    """the largest number of edges on a shortest path between two nodes of the component with this label"""
    N = mesh.num_node
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    metal, gas, bad, _ = classify(w[4 * N:5 * N], cfg["level"], cfg["side"])
    lab = labels(mesh, w[4 * N:5 * N], cfg["level"], cfg["side"])
    nodes = np.flatnonzero(lab == label_of)
    A = gas_graph(ien, gas, ~bad[ien].any(axis=1), N)[nodes][:, nodes]
    return int(shortest_path(A, unweighted=True, directed=False).max())


def many_pores(mesh, max_pores=16, side=1):
    """every node with three even lattice coordinates is an isolated gas node in metal; nothing is open"""
    gas = np.all(lattice(mesh) % 2 == 0, axis=1)
    return config(level=0.0, side=side, open_groups=0, max_pores=max_pores), state(mesh, np.where(gas, -1.0, 1.0), side=side)


def single_tet_masks(mesh, mask, side=1, open_groups=0):
    """the single tet with the gas nodes of the mask (bit a: node a is gas)"""
    phi = np.array([-0.3 - 0.1 * a if (mask >> a) & 1 else 0.4 + 0.2 * a for a in range(4)])
    return config(level=0.125, side=side, open_groups=open_groups), state(mesh, phi + 0.125, side=side)


def permuted(mesh, w, perm):
    """the mesh and the state with node a renumbered perm[a]; the tets and the faces keep their order"""
    N = mesh.num_node
    perm = np.asarray(perm)
    inv = np.argsort(perm)
    xg = np.asarray(mesh.xg).reshape(-1, 3)[inv].reshape(-1)
    off = mesh.bound_node_offset
    bnode = np.concatenate([np.sort(perm[mesh.bound_node[off[g]:off[g + 1]]]) for g in range(mesh.num_bound)])
    m = dataclasses.replace(mesh, xg=np.ascontiguousarray(xg), ien=perm[mesh.ien].astype(np.int32),
                            bound_node=bnode.astype(np.int32), bound_ien=perm[mesh.bound_ien].astype(np.int32))
    w2 = np.empty_like(w)
    w2[:3 * N] = w[:3 * N].reshape(-1, 3)[inv].reshape(-1)
    for k in (3, 4, 5):
        w2[k * N:(k + 1) * N] = w[k * N:(k + 1) * N][inv]
    return m, w2
