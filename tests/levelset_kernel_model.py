"""Model of the level-set geometry launchers (csrc/k_redistance.hip, csrc/k_volume.hip, csrc/level_facets.hpp,
csrc/block_ops.hpp) one launcher at a time.  Test infrastructure only; shared by test_levelset_kernel_model_cpu.py (the model
against independent references) and test_gpu_levelset_kernels.py (the launchers against the model).

The float64 restatement is redistance_model (facets, dist2, tet_volumes, grad_dev) and volume_correction_model.classify.  Added
here:
  the reduction tree   block_tree (xor butterfly 32 .. 1 in each 64-lane wave, then waves 1, 2, 3 into wave 0), block_reduce
                       (thread t takes i = t, t + 256, ... from the identity), node_stage1 (grid min(ceil(N / 2048), 1024),
                       every thread strides by grid * 256), tet_parts (one thread per tet, threads past the end hold zeros)
  the cell grid        cell (floor, clamp), facet_cells (bounding box of the finite vertices), node_runs (nine three-cell
                       runs), cell_lists (count, start and per cell the set of facet ids)
  the launchers        cut, nodes, node_stats, node_sum, classify, evaluate, shift on top of those
  independent references in np.longdouble, which do not restate the header: the volume of {f > 0} in a linear tet by the
                       divided-difference form, and the point-triangle distance by Voronoi regions
  the decks            orbit, orbit_shared, swapped_cube, on_level, dyadic, isolation (the builders stay here for the modules of
                       the other level-set kernels)."""
import itertools
from types import SimpleNamespace

import numpy as np

import redistance_model as rm
import volume_correction_model as vcm
from krylov_model import EXTENDED_REASON, HAVE_EXTENDED, U  # noqa: F401  (re-exported)

F64, LD, I64 = np.float64, np.longdouble, np.int64
BLK, WAVE = 256, 64
NODE_WORK, MAX_PART = 8, 1024
LANES, MAX_GROUP_BLOCKS = 16, 2048
K = vcm.K
PERMS = list(itertools.permutations(range(4)))
POSITIONS = (0, 1, 63, 64, 127, 128, 255)


# ---- the reduction tree ------------------------------------------------------------------------------------------------------
def merge_sum(a, b):
    return a + b


def merge_pair(a, b):
    """(sum, max): fmax passes over a NaN"""
    return np.stack([a[..., 0] + b[..., 0], np.fmax(a[..., 1], b[..., 1])], axis=-1)


def block_tree(v, merge):
    """v [..., 256, NV] -> [..., NV]: what thread 0 of the workgroup holds"""
    v = np.asarray(v, F64)
    w = v.reshape(v.shape[:-2] + (BLK // WAVE, WAVE, v.shape[-1]))
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off:
        w = merge(w, w[..., lane ^ off, :])
        off >>= 1
    r = w[..., 0, 0, :]
    for i in range(1, BLK // WAVE):
        r = merge(r, w[..., i, 0, :])
    return r


def block_reduce(part, merge):
    """part [npart, NV] -> [NV]: thread t merges i = t, t + 256, ... into the identity 0.0, then the tree"""
    part = np.asarray(part, F64)
    v = np.zeros((BLK, part.shape[1]))
    for s in range(0, len(part), BLK):
        c = part[s:s + BLK]
        v[:len(c)] = merge(v[:len(c)], c)
    return block_tree(v, merge)


def node_grid(N):
    return min(-(-N // (BLK * NODE_WORK)), MAX_PART)


def node_stage1(vals, merge, valid=None):
    """vals [N, NV] (valid [N]: the entries a thread merges at all) -> part [grid, NV]"""
    vals = np.asarray(vals, F64)
    N, g = len(vals), node_grid(len(vals))
    v = np.zeros((g * BLK, vals.shape[1]))
    for s in range(0, N, g * BLK):
        c = vals[s:s + g * BLK]
        m = merge(v[:len(c)], c)
        if valid is not None:
            m = np.where(valid[s:s + g * BLK, None], m, v[:len(c)])
        v[:len(c)] = m
    return block_tree(v.reshape(g, BLK, -1), merge)


def tet_parts(vals, merge):
    """vals [NT, NV], one thread per tet -> part [ceil(NT / 256), NV]"""
    vals = np.asarray(vals, F64)
    nblk = -(-len(vals) // BLK)
    v = np.zeros((nblk * BLK, vals.shape[1]))
    v[:len(vals)] = vals
    return block_tree(v.reshape(nblk, BLK, -1), merge)


def block_counts(c):
    """integer counts per tet -> per workgroup"""
    c = np.asarray(c, I64)
    nblk = -(-len(c) // BLK)
    p = np.zeros(nblk * BLK, I64)
    p[:len(c)] = c
    return p.reshape(nblk, BLK).sum(axis=1)


def exclusive_scan(c):
    return np.r_[0, np.cumsum(np.asarray(c, I64))]


# ---- the cell grid -----------------------------------------------------------------------------------------------------------
def make_grid(lo, inv_h, n):
    return SimpleNamespace(lo=np.asarray(lo, F64), inv_h=float(inv_h), n=tuple(int(q) for q in n), ncell=int(np.prod(n)))


def cell(x, lo, inv_h, n):
    u = np.floor((F64(x) - F64(lo)) * F64(inv_h))
    return int(0.0 if u < 0.0 else (float(n - 1) if u > float(n - 1) else u))


def facet_cells(F, g):
    """(lo[3], hi[3]) of the cells the bounding box of the finite vertices overlaps; None when no vertex is finite"""
    V = np.asarray(F, F64).reshape(3, 3)
    V = V[np.isfinite(V).all(axis=1)]
    if not len(V):
        return None
    mn, mx = V.min(axis=0), V.max(axis=0)
    return ([cell(mn[d], g.lo[d], g.inv_h, g.n[d]) for d in range(3)], [cell(mx[d], g.lo[d], g.inv_h, g.n[d]) for d in range(3)])


def cells_of_facet(F, g):
    r = facet_cells(F, g)
    if r is None:
        return []
    lo, hi = r
    return [cx + g.n[0] * (cy + g.n[1] * cz) for cz in range(lo[2], hi[2] + 1) for cy in range(lo[1], hi[1] + 1)
            for cx in range(lo[0], hi[0] + 1)]


def cell_lists(F, g, limit=None):
    """cell_count [ncell], cell_start [ncell + 1], and per cell the set of the facet ids < limit"""
    count = np.zeros(g.ncell, I64)
    sets = [set() for _ in range(g.ncell)]
    for i, f in enumerate(np.asarray(F, F64).reshape(-1, 9)):
        if limit is not None and i >= limit:
            continue
        for c in cells_of_facet(f, g):
            count[c] += 1
            sets[c].add(i)
    return count, exclusive_scan(count), sets


def entries_from(sets, start):
    """one valid entries array: every cell's ids ascending"""
    e = np.zeros(int(start[-1]), I64)
    for c, s in enumerate(sets):
        e[start[c]:start[c] + len(s)] = sorted(s)
    return e


def node_runs(p, g, cell_start):
    """the nine (lo, hi) entry ranges around the node"""
    cx = cell(p[0], g.lo[0], g.inv_h, g.n[0])
    x0, x1 = max(cx - 1, 0), min(cx + 1, g.n[0] - 1)
    cy, cz = cell(p[1], g.lo[1], g.inv_h, g.n[1]), cell(p[2], g.lo[2], g.inv_h, g.n[2])
    runs = []
    for r in range(9):
        y, z = cy + r % 3 - 1, cz + r // 3 - 1
        if y < 0 or y >= g.n[1] or z < 0 or z >= g.n[2]:
            runs.append((0, 0))
            continue
        row = g.n[0] * (y + g.n[1] * z)
        runs.append((int(cell_start[row + x0]), int(cell_start[row + x1 + 1])))
    return runs


# ---- the launchers -----------------------------------------------------------------------------------------------------------
def tet_masks(ien, phi, level):
    ph = np.asarray(phi, F64)[np.asarray(ien).reshape(-1, 4)]
    with np.errstate(invalid="ignore"):
        return ((ph - level > 0) * np.array([1, 2, 4, 8])).sum(axis=1)


def facet_counts(mask):
    npos = np.array([bin(int(m)).count("1") for m in mask], I64)
    return np.where((npos == 0) | (npos == 4), 0, np.where(npos == 2, 2, 1))


def tet_grad_dev(xg, ien, phi, level):
    """per tet ||g| - 1| of a cut tet (a NaN stays), 0 elsewhere"""
    ien = np.asarray(ien).reshape(-1, 4)
    out = np.zeros(len(ien))
    mask = tet_masks(ien, phi, level)
    k = np.flatnonzero((mask != 0) & (mask != 15))
    if k.size:
        x, ph = np.asarray(xg, F64).reshape(-1, 3)[ien[k]], np.asarray(phi, F64)[ien[k]]
        e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
        c23, c31, c12 = rm.cross(e2, e3), rm.cross(e3, e1), rm.cross(e1, e2)
        with np.errstate(invalid="ignore", divide="ignore"):
            gr = (((ph[:, 1] - ph[:, 0])[:, None] * c23 + (ph[:, 2] - ph[:, 0])[:, None] * c31) + (ph[:, 3] - ph[:, 0])[:, None] * c12) \
                / rm.dot(e1, c23)[:, None]
            out[k] = np.abs(np.sqrt(rm.dot(gr, gr)) - 1.0)
    return out


def cut(xg, ien, phi, level, grid=None):
    """dfl_redistance_cut: dict part [nblk, 2], blk_count [nblk], per-tet vol and dev, facets, and with a grid cell_count,
    cell_start and the sets"""
    ien = np.asarray(ien).reshape(-1, 4)
    vol = rm.tet_volumes(xg, ien, phi, level)[0]
    dev = tet_grad_dev(xg, ien, phi, level)
    F, tet = rm.facets(xg, ien, phi, level)
    vals = np.stack([vol, dev], axis=1)
    part = tet_parts(vals, merge_pair)
    # (a NaN deviation is passed over by fmax in the tree as soon as it meets a number, and the other threads hold 0)
    res = dict(part=part, vol=vol, dev=dev, facets=F, facet_tet=tet, blk_count=block_counts(facet_counts(tet_masks(ien, phi, level))))
    if grid is not None:
        res["cell_count"], res["cell_start"], res["sets"] = cell_lists(F, grid)
    return res


def nodes(xg, phi, level, band, g, cell_start, entries, facets, cap_facets, hold=None):
    """dfl_redistance_nodes on the lists as given: (new phi, chg, the set of listed nodes)"""
    x = np.asarray(xg, F64).reshape(-1, 3)
    old = np.asarray(phi, F64)
    new, chg, listed = old.copy(), np.zeros(len(x)), set()
    Fa = np.asarray(facets, F64).reshape(-1, 9)
    for a in range(len(x)):
        runs = node_runs(x[a], g, cell_start)
        kept = np.isnan(old[a]) or bool(hold is not None and hold[a])
        with np.errstate(invalid="ignore"):
            positive = old[a] - level > 0.0
        if sum(hi - lo for lo, hi in runs) == 0:
            chg[a] = -1.0
            if not kept:
                new[a] = level + (band if positive else -band)
            continue
        listed.add(a)
        ids = np.concatenate([np.asarray(entries[lo:hi], I64) for lo, hi in runs])
        ids = ids[(ids >= 0) & (ids < cap_facets)]
        best = np.inf
        if ids.size:
            best = np.fmin.reduce(rm.dist2(x[a][None, :], Fa[ids]), initial=np.inf)
        d = np.sqrt(best)
        in_band = bool(d < band)
        m = d if in_band else band
        now = level + (m if positive else -m)
        if not kept:
            new[a] = now
        chg[a] = (0.0 if kept else abs(now - old[a])) if in_band else -1.0
    return new, chg, listed


def node_stats(chg):
    chg = np.asarray(chg, F64)
    with np.errstate(invalid="ignore"):
        valid = chg >= 0.0
    part = node_stage1(np.stack([np.ones(len(chg)), chg], axis=1), merge_pair, valid)
    return part, block_reduce(part, merge_pair)


def node_sum(q):
    part = node_stage1(np.asarray(q, F64)[:, None], merge_sum)
    return part, block_reduce(part, merge_sum)


def classify(xg, ien, phi, level, max_shift):
    """dfl_volume_classify with lo = level - max_shift, hi = level + max_shift: dict vals [NT, 5], part, out5, band, blk_count"""
    ien = np.asarray(ien).reshape(-1, 4)
    inside, band = vcm.classify(SimpleNamespace(ien=ien), phi, level, max_shift)
    full = rm.tet_volumes(xg, ien, phi, level)[1]
    vals = np.zeros((len(ien), 5))
    vals[:, 4] = full
    vals[inside, 0] = full[inside]
    if band.any():
        for j, c in enumerate((level, level - max_shift, level + max_shift)):
            vals[band, 1 + j] = rm.tet_volumes(xg, ien[band], phi, c)[0]
    part = tet_parts(vals, merge_sum)
    return dict(vals=vals, part=part, out=block_reduce(part, merge_sum), band=band, inside=inside, blk_count=block_counts(band))


def evaluate(xg, ien, phi, lst, cand):
    """dfl_volume_eval: vals [nband, K], part, out"""
    rows = np.asarray(ien).reshape(-1, 4)[np.asarray(lst, I64)]
    vals = np.stack([rm.tet_volumes(xg, rows, phi, F64(c))[0] for c in cand], axis=1)
    part = tet_parts(vals, merge_sum)
    return vals, part, block_reduce(part, merge_sum)


def shift(phi, delta):
    phi = np.asarray(phi, F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(phi), phi, phi + F64(delta))


# ---- independent references in np.longdouble ---------------------------------------------------------------------------------
def closed_form_volume(xg, ien, phi, level):
    """per tet (v, V, K): v = V sum over f_i > 0 of f_i^3 / prod_{j != i} (f_i - f_j), V = |det| / 6, K the abs-sum of that form.
    The four f of every tet must be distinct."""
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, F64).reshape(-1, 3).astype(LD)[ien]
    f = np.asarray(phi, F64).astype(LD)[ien] - LD(level)
    e = x[:, 1:] - x[:, :1]
    det = (e[:, 0, 0] * (e[:, 1, 1] * e[:, 2, 2] - e[:, 1, 2] * e[:, 2, 1]) - e[:, 0, 1] * (e[:, 1, 0] * e[:, 2, 2] - e[:, 1, 2] * e[:, 2, 0])
           + e[:, 0, 2] * (e[:, 1, 0] * e[:, 2, 1] - e[:, 1, 1] * e[:, 2, 0]))
    V = np.abs(det) / LD(6)
    s, k = np.zeros(len(ien), LD), np.zeros(len(ien), LD)
    for i in range(4):
        prod = np.ones(len(ien), LD)
        for j in range(4):
            if j != i:
                prod = prod * (f[:, i] - f[:, j])
        assert (prod != 0).all(), "the closed form needs four distinct values"
        term = f[:, i] ** 3 / prod
        pos = f[:, i] > 0
        s += np.where(pos, term, LD(0))
        k += np.where(pos, np.abs(term), LD(0))
    return V * s, V, k


def region_dist2(p, tri):
    """squared distance of p to the triangle (A, B, C) by the Voronoi regions of its vertices, edges and face, in longdouble"""
    p, (a, b, c) = np.asarray(p, LD), np.asarray(tri, LD).reshape(3, 3)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        q = a
    else:
        bp = p - b
        d3, d4 = ab @ bp, ac @ bp
        cp = p - c
        d5, d6 = ab @ cp, ac @ cp
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        if d3 >= 0 and d4 <= d3:
            q = b
        elif d6 >= 0 and d5 <= d6:
            q = c
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            q = a + (d1 / (d1 - d3)) * ab
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            q = a + (d2 / (d2 - d6)) * ac
        elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
            q = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
        else:
            den = va + vb + vc
            q = a + (vb / den) * ab + (vc / den) * ac
    r = p - q
    return r @ r


def well_shaped(n, seed=7):
    """n triangles [n, 9] with every interior angle in [20, 160] degrees by construction, and n points within two edge lengths"""
    rng = np.random.default_rng(seed)
    F, P = np.zeros((n, 9)), np.zeros((n, 3))
    for i in range(n):
        al = rng.uniform(20.0, 140.0)
        be = rng.uniform(20.0, 160.0 - al)
        ga = 180.0 - al - be
        L = rng.uniform(0.05, 1.0)
        b_len = L * np.sin(np.radians(be)) / np.sin(np.radians(ga))              # |AC| by the law of sines
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        A = rng.uniform(-1.0, 1.0, 3) * L
        B = A + L * q[0]
        Cc = A + b_len * (np.cos(np.radians(al)) * q[0] + np.sin(np.radians(al)) * q[1])
        F[i] = np.r_[A, B, Cc]
        v = rng.normal(size=3)
        P[i] = (A + B + Cc) / 3.0 + v / np.linalg.norm(v) * rng.uniform(0.0, 2.0) * L
    return F, P


def triangle_angles(F):
    T = np.asarray(F, F64).reshape(-1, 3, 3)
    out = np.zeros((len(T), 3))
    for v in range(3):
        e1, e2 = T[:, (v + 1) % 3] - T[:, v], T[:, (v + 2) % 3] - T[:, v]
        out[:, v] = np.degrees(np.arccos((e1 * e2).sum(axis=1) / np.sqrt((e1 * e1).sum(axis=1) * (e2 * e2).sum(axis=1))))
    return out


def dist_scale(P, F):
    """max over the vertices of |p - v|^2"""
    T = np.asarray(F, F64).reshape(-1, 3, 3)
    return ((np.asarray(P, F64)[:, None, :] - T) ** 2).sum(axis=2).max(axis=1)


# ---- the decks ---------------------------------------------------------------------------------------------------------------
class Deck:
    """xg [N, 3], ien [NT, 4], phi [N], level; info: per tet what the builder put there"""

    def __init__(self, name, xg, ien, phi, level, **info):
        self.name, self.level, self.info = name, float(level), info
        self.xg = np.ascontiguousarray(xg, F64).reshape(-1, 3)
        self.ien = np.ascontiguousarray(ien, np.int32).reshape(-1, 4)
        self.phi = np.ascontiguousarray(phi, F64)
        self.N, self.NT = len(self.xg), len(self.ien)
        assert self.ien.min() >= 0 and self.ien.max() < self.N

    def first(self, nt):
        return Deck("%s[:%d]" % (self.name, nt), self.xg, self.ien[:nt], self.phi, self.level)

    def dets(self):
        x = self.xg[self.ien]
        return rm._det4(x[:, 0], x[:, 1], x[:, 2], x[:, 3])

    def w(self, seed=3):
        """the state [6 N] with phi in its slot and recognisable numbers everywhere else"""
        w = np.random.default_rng(seed).uniform(-2.0, 2.0, 6 * self.N)
        w[4 * self.N:5 * self.N] = self.phi
        return w


ORBIT_X = np.array([[0.03, 0.07, 0.02], [1.01, 0.13, 0.06], [0.21, 0.93, 0.17], [0.31, 0.27, 0.83]])   # no right angle
ORBIT_F = np.array([0.3, 0.5, 0.7, 1.1])                                                                # no two equal
ORBIT_LEVEL = 0.125
ORBIT_SHIFT = 0.2        # max_shift of the classification tests: below every |f|, so four positive nodes are inside
# the candidate levels (relative to ORBIT_LEVEL) the per-tet Tier B tests evaluate: level, lo, hi and twelve more, each at least
# 0.1 from every +-|f| so that no corner is smaller than the tet's own rounding
ORBIT_OFFSETS = (0.0, -0.2, 0.2, -0.95, -0.9, -0.8, -0.6, -0.4, -0.1, 0.1, 0.4, 0.6, 0.8, 0.9, 0.95)


def orbit_cases():
    """the 384 (local order, mask) pairs: local node b is the generic tet's vertex perm[b], bit b of mask: local node b positive"""
    return [(p, m) for p in PERMS for m in range(16)]


def _orbit_values(perm, mask):
    s = np.array([1.0 if mask >> b & 1 else -1.0 for b in range(4)])
    return ORBIT_X[list(perm)], ORBIT_LEVEL + s * ORBIT_F[list(perm)]


def orbit(spread=0.25):
    """every case on four nodes of its own, the tets side by side on an 8 x 8 x 6 lattice of pitch `spread`"""
    xs, ph = [], []
    for e, (perm, mask) in enumerate(orbit_cases()):
        x, f = _orbit_values(perm, mask)
        xs.append(x + spread * np.array([e % 8, e // 8 % 8, e // 64]))
        ph.append(f)
    n = len(xs)
    return Deck("orbit", np.concatenate(xs), np.arange(4 * n).reshape(n, 4), np.concatenate(ph), ORBIT_LEVEL, cases=orbit_cases())


def orbit_shared():
    """the same 384 cases on eight shared nodes: node 2 v + s is vertex v with sign s, so every gather goes through ien"""
    xg = np.repeat(ORBIT_X, 2, axis=0)
    phi = ORBIT_LEVEL + np.repeat(ORBIT_F, 2) * np.tile([-1.0, 1.0], 4)
    ien = [[2 * perm[b] + (mask >> b & 1) for b in range(4)] for perm, mask in orbit_cases()]
    return Deck("orbit-shared", xg, ien, phi, ORBIT_LEVEL, cases=orbit_cases())


def swapped_cube(M=4, jitter=0.2):
    """the jittered Kuhn cube with the first two nodes of every other tet swapped (a negative determinant) and a tilted plane"""
    from dedflow_amd.meshgen import kuhn_cube
    m = kuhn_cube(M, jitter=jitter)
    ien = np.array(m.ien, np.int32).reshape(-1, 4).copy()
    ien[1::2, :2] = ien[1::2, 1::-1]
    x = np.asarray(m.xg, F64).reshape(-1, 3)
    phi = (x - 0.5) @ (np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13))
    return Deck("swapped-cube%d" % M, x, ien, phi, 0.05)


def on_level():
    """orbit tets with 1 to 4 nodes exactly at level under every sign of the others, in every local order; three flat tets;
    a NaN at each node of four cut tets.  info count[e] = nodes at level (-1: flat, -2: NaN)"""
    xs, ph, count = [], [], []
    for perm in PERMS:
        for zero in range(1, 16):
            free = [b for b in range(4) if not zero >> b & 1]
            for signs in itertools.product((-1.0, 1.0), repeat=len(free)):
                x, f = _orbit_values(perm, 0)
                f = f.copy()
                f[[b for b in range(4) if zero >> b & 1]] = ORBIT_LEVEL
                for b, s in zip(free, signs):
                    f[b] = ORBIT_LEVEL + s * ORBIT_F[perm[b]]
                xs.append(x), ph.append(f), count.append(bin(zero).count("1"))
    for v in (ORBIT_LEVEL + 0.3, ORBIT_LEVEL, ORBIT_LEVEL - 0.3):
        xs.append(ORBIT_X), ph.append(np.full(4, v)), count.append(-1)
    for mask in (1, 6, 11, 14):
        for b in range(4):
            x, f = _orbit_values(PERMS[(mask + b) % 24], mask)
            f = f.copy()
            f[b] = np.nan
            xs.append(x), ph.append(f), count.append(-2)
    n = len(xs)
    xs = [x + 0.25 * np.array([e % 16, e // 16 % 16, e // 256]) for e, x in enumerate(xs)]
    return Deck("on-level", np.concatenate(xs), np.arange(4 * n).reshape(n, 4), np.concatenate(ph), ORBIT_LEVEL, count=np.array(count))


DYADIC_LEVEL, DYADIC_SHIFT = 0.25, 3.0 / 16.0


def dyadic():
    """Kuhn tets of cubes of edge 4/8 and 8/8 at lattice points, coordinates multiples of 2^-3, f = phi - level multiples of 2^-4
    with every positive / other difference a power of two, so every crossing parameter is 1/4, 1/2 or 3/4 and every crossing
    point, determinant and squared distance is exact.  Also tets with all four phi == level + 3/16 (hi of max_shift = 3/16),
    tets whose largest phi == level - 3/16 (lo), tets inside, tets with three phi == hi, and tets whose local node 0 alone is
    == hi with the others above, each in several local orders"""
    corner = np.array(list(itertools.product((0, 1), repeat=3)), F64)
    kuhn = []
    for p in itertools.permutations(range(3)):
        v = [0]
        for d in p:
            v.append(v[-1] | 1 << (2 - d))
        kuhn.append(v)
    # f * 16: (positive values, the others); with 0 among the others t = 1 where that node is on the level
    choices = [((1.0, 3.0), (-1.0,)), ((1.0,), (-1.0, -3.0)), ((2.0,), (-2.0, 0.0)), ((4.0,), (0.0, -4.0))]
    rng = np.random.default_rng(11)
    xs, ph, kind = [], [], []
    e = 0
    for edge in (0.5, 1.0):
        for kt in kuhn:
            for mask in range(16):
                perm = PERMS[(5 * e + 3) % 24]
                pos, neg = choices[e % 4]
                org = rng.integers(0, 17, 3) / 8.0
                x = (org + edge * corner[kt])[list(perm)]
                f = np.array([rng.choice(pos) if mask >> b & 1 else rng.choice(neg) for b in range(4)]) / 16.0
                xs.append(x), ph.append(DYADIC_LEVEL + f), kind.append("cut")
                e += 1
    for kt, perm in zip(kuhn, PERMS[1::4]):
        x = (np.array([1.0, 0.5, 0.25]) + 0.5 * corner[kt])[list(perm)]
        xs.append(x), ph.append(np.full(4, DYADIC_LEVEL + DYADIC_SHIFT)), kind.append("all == hi")
        xs.append(x), ph.append(DYADIC_LEVEL - DYADIC_SHIFT - np.array([0.0, 1.0, 2.0, 0.0])[list(perm)] / 16.0), kind.append("max == lo")
        xs.append(x), ph.append(DYADIC_LEVEL + DYADIC_SHIFT + np.array([1.0, 1.0, 2.0, 4.0])[list(perm)] / 16.0), kind.append("inside")
        xs.append(x), ph.append(DYADIC_LEVEL + np.array([3.0, 3.0, 3.0, 4.0])[list(perm)] / 16.0), kind.append("three == hi")
        xs.append(x), ph.append(DYADIC_LEVEL + DYADIC_SHIFT + np.array([0.0, 1.0, 2.0, 4.0]) / 16.0), kind.append("first == hi")
    n = len(xs)
    return Deck("dyadic", np.concatenate(xs), np.arange(4 * n).reshape(n, 4), np.concatenate(ph), DYADIC_LEVEL, kind=kind)


def isolation(cases=None, positions=POSITIONS, dead_phi=-3.0):
    """256 B tets, B = len(cases): workgroup b holds the orbit case cases[b] at thread positions[b % 7] and nothing else alive;
    every other tet is the generic tet on four nodes with phi = level + dead_phi (no positive node, below any lo used here).
    info live[b] = the tet id"""
    cases = orbit_cases() if cases is None else cases
    B = len(cases)
    xg, phi = [ORBIT_X], [np.full(4, ORBIT_LEVEL + dead_phi)]
    ien = np.tile(np.arange(4), (BLK * B, 1))
    live = []
    for b, (perm, mask) in enumerate(cases):
        x, f = _orbit_values(perm, mask)
        e = BLK * b + positions[b % len(positions)]
        ien[e] = 4 + 4 * b + np.arange(4)
        xg.append(x + 0.25 * np.array([b % 5, b % 3, b % 7])), phi.append(f), live.append(e)
    return Deck("isolation", np.concatenate(xg), ien, np.concatenate(phi), ORBIT_LEVEL, live=np.array(live), cases=cases)


# ---- the measured constants of the Tier B bounds -----------------------------------------------------------------------------
_const = {}


def c_vol():
    """max |v - closed form| / (u V K) of the float64 restatement over orbit, orbit-shared and isolation at level + every one of
    ORBIT_OFFSETS (level, the lo and hi of the classification tests, the candidates of the evaluation test), every tet kept;
    also the count of tets it was taken over"""
    if "vol" not in _const:
        worst, n = 0.0, 0
        for d in (orbit(), orbit_shared(), isolation()):
            sel = np.arange(d.NT) if d.name != "isolation" else d.info["live"]
            for c in d.level + np.array(ORBIT_OFFSETS):
                v = rm.tet_volumes(d.xg, d.ien[sel], d.phi, c)[0]
                ref, V, Kk = closed_form_volume(d.xg, d.ien[sel], d.phi, c)
                live = Kk > 0
                assert (v[~live] == 0).all() and (ref[~live] == 0).all()     # no positive node: both are exactly 0
                worst = max(worst, float((np.abs(v[live].astype(LD) - ref[live]) / (LD(U) * V[live] * Kk[live])).max()))
            n += len(sel)
        _const["vol"] = (worst, n)
    return _const["vol"]


def c_dist(n=4000):
    """max |d^2 - region method| / (u max_v |p - v|^2) of the float64 dist2 over the well-shaped family, every pair kept"""
    if "dist" not in _const:
        F, P = well_shaped(n)
        d2 = rm.dist2(P, F)
        ref = np.array([region_dist2(P[i], F[i]) for i in range(n)], LD)
        _const["dist"] = (float((np.abs(d2.astype(LD) - ref) / (LD(U) * dist_scale(P, F).astype(LD))).max()), n)
    return _const["dist"]
