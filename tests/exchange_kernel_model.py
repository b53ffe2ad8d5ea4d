"""numpy model of the particle-field exchange kernels, kernel by kernel (csrc/k_couple.hip, k_heat.hip, k_capture.hip,
k_surface_contact.hip; launchers in include/dedflow_kernels.h, laws in include/dedflow.h).  Behind
test_gpu_exchange_kernels.py; checked without a GPU by test_exchange_kernel_model_cpu.py.

Three restatements:
  int64       the integer outputs: V2E lists, the tet neighbour table (a face dictionary), the counting sort by tet
  float64     in the kernel's stated operation order where the source fixes one (tet_levelset.hpp and the contract(off)
              parts of k_capture.hip and k_surface_contact.hip: numpy never fuses a multiply-add), and the walk of
              couple_locate_kernel with its hash
  longdouble  everywhere: every float function takes a dtype; np.longdouble is the model and np.float64 the RESTATEMENT, the
              same code, which shows what float64 rounding alone does to the law (the constants c below: measured here,
              never on a kernel)
The laws themselves are pinned to coupling_model, heat_model, capture_model, surface_contact_model and friction_model by
the CPU test; the tangential law IS friction_model.tangential and the cell sort IS dem_model's.

Every rounded value comes with A, the entry's own abs-sum: the sum of the absolute values of the terms that are added up
to form it, plus |d value / d k| k kappa for a factor k that inherits the cancellation of u_f - v (kappa = sum_d |s_d|
(|u_f|_abs + |v|)_d / |s|^2) or of the tet gradient (surface_contact_model.gradient_condition).  A test grants 8 c u A."""
import numpy as np

import capture_model as cm
import coupling_model as cpm
import dem_model as D
import friction_model as fm
import heat_model as hm
import surface_contact_model as scm
from krylov_model import EXTENDED_REASON, HAVE_EXTENDED, U  # noqa: F401  (re-exported)

F64, LD, I64 = np.float64, np.longdouble, np.int64
LAMBDA_EPS = cpm.LAMBDA_EPS
MAX_WALK = 4096
SURFACE_SLOTS, SURFACE_SLOT_STRIDE = 64, 16
MAX_HISTORY = D.MAX_HISTORY
FAR_MARGIN = 1.0 + 1e-6
PI = {F64: F64(np.pi), LD: LD(np.pi)}     # M_PI is the double; the kernels use it in both roles


def bound(A, c):
    return (8.0 * c * U * np.asarray(A, LD)).astype(F64)


def ratio_c(rest, model, A):
    """the largest |restatement - model| / (u A) over the entries with A > 0; entries with A == 0 must agree exactly"""
    err, A = np.abs(np.asarray(rest, LD) - np.asarray(model, LD)), np.asarray(A, LD)
    assert np.all(err[A == 0] == 0)
    nz = A > 0
    return float((err[nz] / (U * A[nz])).max()) if nz.any() else 0.0


# ======================================================================================================================
# meshes
# ======================================================================================================================
class Mesh:
    def __init__(self, name, x, ien):
        self.name, self.x, self.ien = name, np.ascontiguousarray(x, F64).reshape(-1, 3), np.asarray(ien, I64).reshape(-1, 4)
        self.N, self.T = len(self.x), len(self.ien)
        self._cache = {}

    def v2e(self):
        if "v2e" not in self._cache:
            self._cache["v2e"] = v2e(self.ien, self.N)
        return self._cache["v2e"]

    def nbr(self):
        if "nbr" not in self._cache:
            self._cache["nbr"] = neighbours(self.ien)
        return self._cache["nbr"]


_MESH = {}


def kuhn(M, jitter=0.0):
    key = ("kuhn", M, jitter)
    if key not in _MESH:
        from dedflow_amd.meshgen import kuhn_cube
        m = kuhn_cube(M, jitter=jitter)
        _MESH[key] = Mesh("kuhn%d%s" % (M, "-jitter" if jitter else ""), m.xg, m.ien)
    return _MESH[key]


CUBES = [(M, j) for M in (2, 3, 4) for j in (0.0, 0.2)]


def fan():
    """three tets on ONE face (0, 1, 2): tet 0 below it, tets 1 and 2 (overlapping) above: non-conforming.  Across that face
    tet 0 sees tet 1 and tets 1 and 2 see tet 0: the lowest id wins"""
    x = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, -1.0], [0.25, 0.25, 1.0], [0.3, 0.2, 0.5]]
    return Mesh("fan", x, [[0, 2, 1, 3], [0, 1, 2, 4], [0, 1, 2, 5]])


STRIP_CUBES = 1500


def strip(n=STRIP_CUBES):
    """n unit cubes in a row along x, 6 Kuhn tets each: tets 6 c .. 6 c + 5 are cube c"""
    key = ("strip", n)
    if key not in _MESH:
        from dedflow_amd.meshgen import kuhn_box
        m = kuhn_box((n, 1, 1), (0.0, 0.0, 0.0), (float(n), 1.0, 1.0))
        _MESH[key] = Mesh("strip%d" % n, m.xg, m.ien)
    return _MESH[key]


def v2e(ien, N):
    """(vrow, vcol): the tets of every node, ascending"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    node, tet = ien.ravel(), np.repeat(np.arange(len(ien)), 4)
    o = np.lexsort((tet, node))
    return np.r_[0, np.cumsum(np.bincount(node, minlength=N))].astype(I64), tet[o]


def scramble(vrow, vcol, seed=3):
    """every list in a random order (the arrival order of an atomic fill is any order)"""
    rng, out = np.random.default_rng(seed), np.array(vcol, I64)
    for a in range(len(vrow) - 1):
        out[vrow[a]:vrow[a + 1]] = rng.permutation(out[vrow[a]:vrow[a + 1]])
    return out


def neighbours(ien):
    """nbr[t][k] = the lowest tet != t that has the three vertices of the face of t opposite local vertex k, -1 when none"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    faces = {}
    for t, v in enumerate(ien.tolist()):
        for k in range(4):
            faces.setdefault(tuple(sorted(v[:k] + v[k + 1:])), []).append(t)
    nbr = np.full((len(ien), 4), -1, I64)
    for t, v in enumerate(ien.tolist()):
        for k in range(4):
            other = [e for e in faces[tuple(sorted(v[:k] + v[k + 1:]))] if e != t]
            if other:
                nbr[t, k] = min(other)
    return nbr


def bfs(nbr, start=0):
    """the number of face crossings from tet `start` to every tet (-1: unreachable)"""
    dist = np.full(len(nbr), -1, I64)
    dist[start], front, d = 0, np.array([start]), 0
    while front.size:
        d += 1
        nxt = np.unique(nbr[front].ravel())
        nxt = nxt[(nxt >= 0)]
        nxt = nxt[dist[nxt] < 0]
        dist[nxt] = d
        front = nxt
    return dist


# ======================================================================================================================
# point location
# ======================================================================================================================
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _cross_abs(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)


def _dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def barycentric(x4, p, dtype):
    """(lambda [n][4], A [n][4]) of the points p [n][3] in the tets with vertices x4 [n][4][3], in barycentric()'s order.
    A_k (k = 1..3) = sum_d |r_d| |c_k|_abs,d / |det| + |lambda_k| |det|_abs / |det| (the abs-sum of the triple products over
    |det|; |c|_abs, |det|_abs: every product at its absolute value), A_0 = 1 + A_1 + A_2 + A_3"""
    x4, p = np.asarray(x4, dtype), np.asarray(p, dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1, e2, e3, r = x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0], x4[:, 3] - x4[:, 0], p - x4[:, 0]
        c = [_cross(e2, e3), _cross(e3, e1), _cross(e1, e2)]
        det = _dot3(e1, c[0])
        inv = dtype(1.0) / det
        lam = np.empty((len(p), 4), dtype)
        for k in range(3):
            lam[:, 1 + k] = _dot3(r, c[k]) * inv
        lam[:, 0] = dtype(1.0) - lam[:, 1] - lam[:, 2] - lam[:, 3]
        ca = [_cross_abs(e2, e3), _cross_abs(e3, e1), _cross_abs(e1, e2)]
        deta = _dot3(np.abs(e1), ca[0])
        A = np.empty((len(p), 4), LD)
        for k in range(3):
            A[:, 1 + k] = (_dot3(np.abs(r), ca[k]) + np.abs(lam[:, 1 + k] * det) * (deta / np.abs(det))) / np.abs(det)
        A[:, 0] = 1.0 + A[:, 1] + A[:, 2] + A[:, 3]
    return lam, A


def mix32(h):
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def grid_coord(x, lo, inv_h, g):
    """the seed-grid cell of a coordinate: a NaN goes to cell 0 by comparison"""
    with np.errstate(invalid="ignore"):
        c = np.floor((np.asarray(x, F64) - lo) * inv_h)
        return np.where(c >= g, g - 1, np.where(c >= 1.0, np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0), 0.0)).astype(I64)


class Walk:
    """tet, lam, steps, margin of walk()"""


def walk(mesh, pts, start, rule="each", cap=MAX_WALK, ids=None):
    """couple_locate_kernel in float64 from the tets `start` (< 0: no tet, the result is -1) for all particles at once.
    rule = "each": a tet accepts when each lambda compares >= -1e-12, and a point that is not finite is refused and ends
    outside; rule = "fmin": the earlier rule min-by-fmin >= -1e-12 without that check.
    Returns tet, lam (0 where tet < 0), steps (the number of tets evaluated) and margin: the smallest distance of a lambda
    from -1e-12 and, where the most negative face was taken among several, from the runner-up"""
    x, ien, nbr = mesh.x, mesh.ien, mesh.nbr()
    pts = np.asarray(pts, F64).reshape(-1, 3)
    P = len(pts)
    ids = np.arange(P) if ids is None else np.asarray(ids)
    t = np.array(start, I64)
    out = Walk()
    out.tet, out.lam = np.where(t < 0, -1, -2), np.zeros((P, 4))
    out.steps, out.margin = np.zeros(P, I64), np.full(P, np.inf)
    finite = np.isfinite(pts).all(axis=1)
    act = np.flatnonzero(t >= 0)
    for step in range(cap):
        if not act.size:
            break
        ta = t[act]
        lam, _ = barycentric(x[ien[ta]], pts[act], F64)
        out.steps[act], out.lam[act] = step + 1, lam
        with np.errstate(invalid="ignore"):
            if rule == "each":
                ok = (lam >= -LAMBDA_EPS).all(axis=1)
                refused = ~ok & ~finite[act]
            else:
                ok = np.fmin(np.fmin(lam[:, 0], lam[:, 1]), np.fmin(lam[:, 2], lam[:, 3])) >= -LAMBDA_EPS
                refused = np.zeros(len(act), bool)
            nb = nbr[ta]
            cand = (lam < -LAMBDA_EPS) & (nb >= 0)
            gap = np.abs(lam + LAMBDA_EPS)
            out.margin[act] = np.minimum(out.margin[act], np.where(np.isnan(gap), np.inf, gap).min(axis=1))
        ncand = cand.sum(axis=1)
        outside = ~ok & ~refused & (ncand == 0)
        lm = np.where(cand, lam, np.inf)
        best = lm.argmin(axis=1)                       # the first of equal ones, as `lam[k] < bestl`
        h = mix32(((ids[act].astype(np.uint64) * 0x9E3779B9) & 0xFFFFFFFF) ^ np.uint64(step))
        hashed = (ncand > 1) & ((h & 3) == 0)
        pick = ((h >> 2) % np.maximum(ncand, 1).astype(np.uint64)).astype(I64)
        kth = (cand & ((np.cumsum(cand, axis=1) - 1) == pick[:, None])).argmax(axis=1)
        second = np.sort(lm, axis=1)[:, 1]
        plain = ~ok & ~refused & (ncand > 1) & ~hashed
        with np.errstate(invalid="ignore"):
            out.margin[act[plain]] = np.minimum(out.margin[act[plain]], (second - lm.min(axis=1))[plain])
        best = np.where(hashed, kth, best)
        out.tet[act[ok]] = ta[ok]
        out.tet[act[outside | refused]] = -1
        go = ~ok & ~outside & ~refused
        t[act[go]] = nb[np.arange(len(act)), best][go]
        act = act[go]
    out.lam[out.tet < 0] = 0.0
    return out


def seed_start(pts, tet, seed, lo, inv_h, gdim):
    """the tet every walk starts from: tet[i], or the seed-grid tet of the particle's cell when tet[i] < 0"""
    pts = np.asarray(pts, F64).reshape(-1, 3)
    c = [grid_coord(pts[:, d], lo[d], inv_h[d], gdim) for d in range(3)]
    return np.where(np.asarray(tet) < 0, np.asarray(seed, I64)[c[0] + gdim * (c[1] + gdim * c[2])], tet)


def seed_grid(mesh, gdim):
    """a seed grid over the mesh's bounding box: per cell the lowest tet that contains the cell's centre"""
    lo, hi = mesh.x.min(axis=0), mesh.x.max(axis=0)
    inv_h = gdim / (hi - lo)
    k = np.arange(gdim ** 3)
    centre = lo + (np.stack([k % gdim, (k // gdim) % gdim, k // gdim ** 2], axis=1) + 0.5) / inv_h
    seed = brute(mesh, centre)[0]
    assert np.all(seed >= 0)
    return seed, lo, inv_h


def min_lambda_all(mesh, pts):
    """(lambda [P][T][4], A [P][T][4]) of every point in every tet, in longdouble: for the check that a point reported
    outside lies in no tet beyond doubt"""
    pts = np.asarray(pts, F64).reshape(-1, 3)
    P, T = len(pts), mesh.T
    lam, A = barycentric(np.repeat(mesh.x[mesh.ien][None], P, axis=0).reshape(P * T, 4, 3), np.repeat(pts, T, axis=0), LD)
    return lam.reshape(P, T, 4), A.reshape(P, T, 4)


def brute(mesh, pts):
    """(tet, lam) by testing every tet in float64, the lowest id winning; -1 and 0 outside (capture_model.brute_locate's rule
    with barycentric()'s arithmetic)"""
    pts = np.asarray(pts, F64).reshape(-1, 3)
    tet, lam = np.full(len(pts), -1, I64), np.zeros((len(pts), 4))
    for s in range(0, len(pts), 64):
        q = pts[s:s + 64]
        l, _ = barycentric(np.repeat(mesh.x[mesh.ien][None], len(q), axis=0).reshape(-1, 4, 3), np.repeat(q, mesh.T, axis=0), F64)
        l = l.reshape(len(q), mesh.T, 4)
        ok = (l >= -LAMBDA_EPS).all(axis=2)
        has, first = ok.any(axis=1), ok.argmax(axis=1)
        tet[s:s + 64] = np.where(has, first, -1)
        lam[s:s + 64] = np.where(has[:, None], l[np.arange(len(q)), first], 0.0)
    return tet, lam


def c_lambda():
    """c of lambda: the restatement against longdouble on random points in their tets and around them, on every cube"""
    c = 0.0
    for M, j in CUBES:
        m = kuhn(M, j)
        rng = np.random.default_rng(10 * M)
        t = rng.integers(0, m.T, 600)
        p = np.einsum("na,nad->nd", rng.dirichlet(np.ones(4), 600), m.x[m.ien[t]]) + rng.normal(0, 0.05, (600, 3)) * (np.arange(600) % 2)[:, None]
        a, A = barycentric(m.x[m.ien[t]], p, LD)
        b, _ = barycentric(m.x[m.ien[t]], p, F64)
        c = max(c, ratio_c(b, a, A))
    return c


def strip_particles(P=257):
    """points well inside tets of cubes all along the strip, dense around the cap; the containing tet, and the two masks of
    the cap test: the model's walk needs at most 4096 - 64 steps / the tet's BFS distance is >= 4096"""
    m = strip()
    rng = np.random.default_rng(12)
    cube = np.r_[rng.integers(0, 1300, P - 160), rng.integers(1300, 1400, 100), rng.integers(1400, 1500, 60)]
    tet = 6 * cube + rng.integers(0, 6, P)
    lam = rng.dirichlet(np.ones(4), P) * 0.6 + 0.1
    pts = np.einsum("na,nad->nd", lam, m.x[m.ien[tet]])
    d = bfs(m.nbr())[tet]
    return pts, tet, d + 1 <= MAX_WALK - 64, d >= MAX_WALK



# ---- particle positions ----------------------------------------------------------------------------------------------
def interior_points(mesh, P, seed, clear=0.0):
    """random points inside random tets, every lambda >= clear; returns (pts, tet)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, mesh.T, P)
    lam = rng.dirichlet(np.ones(4), P) * (1.0 - 4.0 * clear) + clear
    return np.einsum("na,nad->nd", lam, mesh.x[mesh.ien[t]]), t


def shared_points(mesh, P, seed):
    """points exactly on vertices, edge midpoints and face centroids of random tets (dyadic or one rounding away)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, mesh.T, P)
    w = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.25, 0.25, 0.5, 0], [0.5, 0.25, 0.25, 0]])[np.arange(P) % 4]
    w = np.stack([rng.permutation(r) for r in w])
    return np.einsum("na,nad->nd", w, mesh.x[mesh.ien[t]])


def outside_points(P, seed):
    """points outside each of the six sides of the unit cube in turn, 1e-3 to 0.3 away"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, (P, 3))
    k = np.arange(P) % 6
    off = 10.0 ** rng.uniform(-3, -0.5, P)
    p[np.arange(P), k // 2] = np.where(k % 2 == 0, -off, 1.0 + off)
    return p


def locate_points(mesh):
    """the 513 particles of the location tests on a cube: 150 random interior points, 150 clear of every face (lambda >= 1e-3),
    100 on shared faces / edges / vertices, 60 outside (ten per side), 53 in one tet.  Returns pts, the mask of the
    particles whose containing tet is unique (all but the shared ones), and the tets of the clear family"""
    clear, clear_t = interior_points(mesh, 150, 21, clear=1e-3)
    one = np.einsum("na,ad->nd", np.random.default_rng(5).dirichlet(np.ones(4), 53), mesh.x[mesh.ien[mesh.T // 2]])
    fam = [interior_points(mesh, 150, 20)[0], clear, shared_points(mesh, 100, 22), outside_points(60, 23), one]
    unique = np.repeat([True, True, False, True, True], [len(p) for p in fam])
    return np.vstack(fam), unique, clear_t


# ======================================================================================================================
# the sort by tet and the node sums
# ======================================================================================================================
def sort_by_tet(tet, T):
    tet = np.asarray(tet, I64)
    ok = np.flatnonzero(tet >= 0)
    return D.exclusive_scan(np.bincount(tet[ok], minlength=T)), ok[np.argsort(tet[ok], kind="stable")]


def node_sum(mesh, tstart, members, lam, val, scale, C):
    """out[C a + d] = -scale * sum over the tets e of node a (ascending) and the particles p of e (ascending) of
    lambda_{p, k(a, e)} val[p][d] in float64, in that order"""
    vrow, vcol = mesh.v2e()
    val, lam = np.asarray(val, F64).reshape(-1, C), np.asarray(lam, F64).reshape(-1, 4)
    s = np.zeros((mesh.N, C))
    for a in range(mesh.N):
        for e in vcol[vrow[a]:vrow[a + 1]]:
            k = 0
            for j in (1, 2, 3):
                if mesh.ien[e, j] == a:
                    k = j
            for p in members[tstart[e]:tstart[e + 1]]:
                s[a] += lam[p, k] * val[p]
    return (-F64(scale)) * s


def dyadic_particles(mesh, P, seed, one_tet=None, located=0.8):
    """tet, lambda in multiples of 1/8 with sum 1, integer values [P][5] in -8 .. 8"""
    rng = np.random.default_rng(seed)
    tet = rng.integers(0, mesh.T, P) if one_tet is None else np.full(P, one_tet)
    tet = np.where(rng.uniform(size=P) < located, tet, np.where(np.arange(P) % 2, -1, -2))
    cut = np.sort(rng.integers(0, 9, (P, 3)), axis=1)
    lam = np.diff(np.c_[np.zeros(P, I64), cut, np.full(P, 8)], axis=1) / 8.0
    return tet, lam, rng.integers(-8, 9, (P, 5)).astype(F64)


# ======================================================================================================================
# the drag sub-step
# ======================================================================================================================
def _interp_sum(lam, f, dtype):
    """sum_b lambda_b f_b in the order b = 0..3 from 0.0, and its abs-sum"""
    s, a = np.zeros(f.shape[:1] + f.shape[2:], dtype), np.zeros(f.shape[:1] + f.shape[2:], LD)
    for b in range(4):
        l = lam[:, b].reshape((-1,) + (1,) * (f.ndim - 2))
        s = s + l * f[:, b]
        a = a + np.abs(l * f[:, b]).astype(LD)
    return s, a


def _kappa(s, auf, v):
    """the amplification of |s| = |u_f - v|: sum_d |s_d| (|u_f|_abs + |v|)_d / |s|^2, 0 where s == 0"""
    s2 = (s * s).sum(axis=1).astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = (np.abs(s) * (auf + np.abs(v))).sum(axis=1).astype(LD) / s2
    return np.where(s2 > 0, k, 0.0)


class Out(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def fluid_step(dtype, mesh, w, tet, lam, coord, vel, acc, imp, mass, radius, rho_f, mu_f, g, dt):
    """couple_fluid_kernel: returns vel, coord, acc, imp [P][3] with their abs-sums A_*, and re; mass and radius scalars or [P]"""
    P = len(tet)
    tet = np.asarray(tet, I64)
    x, v, a, i0 = (np.asarray(q, dtype).reshape(-1, 3) for q in (coord, vel, acc, imp))
    m, r = (np.broadcast_to(np.asarray(q, dtype), (P,)) for q in (mass, radius))
    rho_f, mu_f, dt, g = dtype(rho_f), dtype(mu_f), dtype(dt), np.asarray(g, dtype)
    inside = tet >= 0
    u = np.asarray(w, dtype)[:3 * mesh.N].reshape(-1, 3)
    lam = np.where(inside[:, None], np.asarray(lam, dtype).reshape(-1, 4), 0)
    uf, auf = _interp_sum(lam, u[mesh.ien[np.where(inside, tet, 0)]], dtype)
    diam = dtype(2.0) * r
    rho_p = m / (dtype(4.0) / dtype(3.0) * PI[dtype] * r * r * r)
    s = uf - v
    re = rho_f * np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]) * diam / mu_f
    low = re <= 1000.0
    f = np.where(low, dtype(1.0) + dtype(0.15) * np.power(re, dtype(0.687)), dtype(0.44) * re / dtype(24.0))
    tau = rho_p * diam * diam / (dtype(18.0) * mu_f)
    k = (f / tau)[:, None]
    buoy = (dtype(1.0) - rho_f / rho_p)[:, None]
    den = dtype(1.0) / (dtype(1.0) + dt * k)
    vin = (v + dt * (a + buoy * g + k * uf)) * den
    vout = v + dt * (a + g)
    vn = np.where(inside[:, None], vin, vout)
    dimp = m[:, None] * k * (uf - vn) * dt
    out = Out(vel=vn, coord=x + dt * vn, acc=(vn - v) * (dtype(1.0) / dt), imp=np.where(inside[:, None], i0 + dimp, i0), re=re)
    # abs-sums
    kap = (1.0 + np.where(low, 0.687 * (f - 1.0) / f, 1.0).astype(LD) * _kappa(s, auf, v))[:, None]
    A_in = (np.abs(v) + np.abs(dt) * (np.abs(a) + np.abs(buoy * g) + k * auf)).astype(LD) * den + np.abs(dt * den * (uf - vin) * k) * kap
    A_out = (np.abs(v) + np.abs(dt) * (np.abs(a) + np.abs(g))).astype(LD)
    A_v = np.where(inside[:, None], A_in, A_out)
    out.A_vel, out.A_coord = A_v, np.abs(x).astype(LD) + np.abs(dt) * A_v
    out.A_acc = A_v / np.abs(dt) + np.abs(out.acc)
    out.A_imp = np.abs(i0).astype(LD) + np.where(inside[:, None], np.abs(m[:, None] * k * dt) * (auf + A_v) + np.abs(dimp) * kap, 0.0)
    return out


FLUID = dict(rho_f=1.2, mu_f=1.8e-2, g=(0.3, -0.2, -9.81), R=0.01, rho_p=7800.0)


def fluid_case(name, P=513, seed=0):
    """the input families of the drag sub-step on kuhn(3, 0.2); name: "low" (Re 0.01 .. 900), "high" (Re 1100 .. 5000),
    "re0" (u_f == v exactly: a constant dyadic field), "stiff" (dt / tau = 1e6), "slack" (dt / tau = 1e-6), "outside" (every
    tet < 0).  A fifth of the particles of every family has tet < 0"""
    mesh = kuhn(3, 0.2)
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    R, rho_p, rho_f, mu_f = FLUID["R"], FLUID["rho_p"], FLUID["rho_f"], FLUID["mu_f"]
    r = rng.uniform(0.5 * R, R, P)
    r[0] = R
    m = rho_p * 4.0 / 3.0 * np.pi * r ** 3
    M0 = rho_p * 4.0 / 3.0 * np.pi * R ** 3
    tau = rho_p * (2 * R) ** 2 / (18.0 * mu_f)
    dt = {"stiff": 1e6 * tau, "slack": 1e-6 * tau}.get(name, 0.37 * tau)
    tet = rng.integers(0, mesh.T, P)
    tet[np.arange(P) % 5 == 4] = -1
    tet[7 % P] = -2
    if name == "outside":
        tet[:] = -1
    lam = rng.dirichlet(np.ones(4), P)
    w = np.zeros(6 * mesh.N)
    w[:3 * mesh.N] = rng.normal(0, 1.0, 3 * mesh.N)
    vel = rng.normal(0, 1.0, (P, 3))
    if name == "re0":
        w[:3 * mesh.N] = np.tile([0.5, -1.25, 2.0], mesh.N)
        lam = dyadic_particles(mesh, P, seed)[1]
        vel[:] = [0.5, -1.25, 2.0]
    elif name in ("low", "high"):
        uf = cpm.interpolate(w, mesh.ien, np.maximum(tet, 0), lam)
        d = rng.normal(size=(P, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        target = 10.0 ** rng.uniform(-2, np.log10(900.0), P) if name == "low" else rng.uniform(1100.0, 5000.0, P)
        vel = uf + d * (target * mu_f / (rho_f * 2 * R))[:, None]
    return Out(mesh=mesh, P=P, tet=tet, lam=lam, w=w, coord=rng.uniform(0, 1, (P, 3)), vel=vel, acc=rng.normal(0, 5.0, (P, 3)),
               imp=rng.normal(0, 1e-6, (P, 3)), R=R, M=M0, r=r, m=m, dt=dt, rho_f=rho_f, mu_f=mu_f, g=FLUID["g"])


FLUID_CASES = ("low", "high", "re0", "stiff", "slack", "outside")


def fluid_run(case, dtype, poly, same_size=False):
    c = case
    m, r = (c.m, c.r) if poly and not same_size else (c.M, c.R)
    return fluid_step(dtype, c.mesh, c.w, c.tet, c.lam, c.coord, c.vel, c.acc, c.imp, m, r, c.rho_f, c.mu_f, c.g, c.dt)


_CONST = {}


def _cached(key, fn):
    if key not in _CONST:
        _CONST[key] = fn()
    return _CONST[key]


def c_fluid():
    """c of (vel, coord, acc, imp): the largest over the families, mono and poly"""
    def measure():
        c = np.zeros(4)
        for name in FLUID_CASES:
            case = fluid_case(name)
            for poly in (False, True):
                a, b = fluid_run(case, LD, poly), fluid_run(case, F64, poly)
                c = np.maximum(c, [ratio_c(b[k], a[k], a["A_" + k]) for k in ("vel", "coord", "acc", "imp")])
        return c
    return _cached("fluid", measure)


def c_pow():
    """c of pow alone: |float64 pow - longdouble pow| / (u pow) for Re in 1e-6 .. 1000"""
    re = 10.0 ** np.linspace(-6, 3, 4001)
    ref = np.power(re.astype(LD), LD(0.687))
    return float((np.abs(np.power(re, 0.687).astype(LD) - ref) / (U * ref)).max())


# ======================================================================================================================
# heat
# ======================================================================================================================
def heat_update(dtype, mesh, w, tet, lam, vel, temp, e0, mass, radius, cp_p, k_f, rho_f, mu_f, pr13, dt, q=None, laser=None,
                coupled=True):
    """heat_update_kernel: temp, rate, e [P] with A_*; coupled False: w or tet NULL"""
    P = len(temp)
    ti, e0 = np.asarray(temp, dtype), np.asarray(e0, dtype)
    m, r = (np.broadcast_to(np.asarray(x, dtype), (P,)) for x in (mass, radius))
    cp_p, k_f, rho_f, mu_f, pr13, dt = (dtype(x) for x in (cp_p, k_f, rho_f, mu_f, pr13, dt))
    cap = m * cp_p
    qq = np.zeros(P, dtype) if q is None else np.asarray(q, dtype)
    if laser is not None:
        qs = qq + np.asarray(laser, dtype)
        qa = (np.abs(qq) + np.abs(np.asarray(laser, dtype))).astype(LD) / cap
    else:
        qs, qa = qq, np.abs(qq).astype(LD) / cap
    qc = qs / cap
    inside = (np.asarray(tet, I64) >= 0) if coupled else np.zeros(P, bool)
    tsafe = np.where(inside, np.asarray(tet, I64), 0) if coupled else np.zeros(P, I64)
    lam = np.where(inside[:, None], np.asarray(lam, dtype).reshape(-1, 4), 0)
    nodes = mesh.ien[tsafe]
    wv = np.asarray(w, dtype)
    tf, atf = _interp_sum(lam, wv[5 * mesh.N:][nodes], dtype)
    uf, auf = _interp_sum(lam, wv[:3 * mesh.N].reshape(-1, 3)[nodes], dtype)
    v = np.asarray(vel, dtype).reshape(-1, 3)
    diam = dtype(2.0) * r
    s = uf - v
    re = rho_f * np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]) * diam / mu_f
    nu = dtype(2.0) + dtype(0.6) * np.sqrt(re) * pr13
    itau = (nu * k_f * PI[dtype] * diam) / cap
    den = dtype(1.0) + dt * itau
    tin = (ti + dt * (qc + tf * itau)) / den
    tn = np.where(inside, tin, ti + dt * qc)
    de = dt * cap * (tf - tn) * itau
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = cap * (tn - ti) / dt if dt != 0 else np.zeros(P, dtype)
    kap = 1.0 + 0.5 * ((nu - 2.0) / nu).astype(LD) * _kappa(s, auf, v)
    A_in = (np.abs(ti) + np.abs(dt) * (qa + atf * itau)).astype(LD) / den + np.abs(dt * (tf - tin) * itau / den) * kap
    A_t = np.where(inside, A_in, np.abs(ti) + np.abs(dt) * qa)
    out = Out(temp=tn, rate=rate, e=np.where(inside, e0 + de, e0), A_temp=A_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.A_rate = cap * A_t / np.abs(dt) + np.abs(rate) if dt != 0 else np.zeros(P, LD)
    out.A_e = np.abs(e0).astype(LD) + np.where(inside, np.abs(dt * cap * itau) * (atf + A_t) + np.abs(de) * kap, 0.0)
    return out


HEAT = dict(cp_p=500.0, k_f=0.66, rho_f=1.2, mu_f=1.8e-2, pr13=float(np.cbrt(1.0 * 1.8e-2 / 0.66)))


def heat_case(P=513, seed=4):
    c = fluid_case("low", P, seed)
    rng = np.random.default_rng(seed)
    c.w[5 * c.mesh.N:] = rng.uniform(300.0, 2000.0, c.mesh.N)
    c.temp, c.e0 = rng.uniform(300.0, 3000.0, P), rng.normal(0, 1e-3, P)
    c.q, c.laser = rng.normal(0, 1e-2, P), rng.uniform(0, 5e-2, P)
    tau_T = c.M * HEAT["cp_p"] / (2.0 * HEAT["k_f"] * np.pi * 2 * c.R)
    c.dt = 0.4 * tau_T
    return c


def heat_run(case, dtype, poly, laser, q=True, coupled=True, dt=None):
    c = case
    m, r = (c.m, c.r) if poly else (c.M, c.R)
    return heat_update(dtype, c.mesh, c.w, c.tet, c.lam, c.vel, c.temp, c.e0, m, r, HEAT["cp_p"], HEAT["k_f"], HEAT["rho_f"],
                       HEAT["mu_f"], HEAT["pr13"], c.dt if dt is None else dt, q=c.q if q else None,
                       laser=c.laser if laser else None, coupled=coupled)


def c_heat():
    def measure():
        c, case = np.zeros(3), heat_case()
        for poly in (False, True):
            for laser in (False, True):
                for q, coupled in ((True, True), (False, True), (True, False)):
                    a, b = heat_run(case, LD, poly, laser, q, coupled), heat_run(case, F64, poly, laser, q, coupled)
                    c = np.maximum(c, [ratio_c(b[k], a[k], a["A_" + k]) for k in ("temp", "rate", "e")])
        return c
    return _cached("heat", measure)


def conduction(dtype, x, r, T, k_p, pairs):
    """q_i = sum_j H_ij (T_j - T_i) over the given contacts (i, j, .) with heat_model.conductance in `dtype`, and A_i = sum_j
    |term| (r_i + r_j + dist) / delta: delta = (r_i + r_j) - dist cancels (heat_model.conduction's condition sum)"""
    x, T = np.asarray(x, dtype).reshape(-1, 3), np.asarray(T, dtype)
    r = np.broadcast_to(np.asarray(r, dtype), (len(x),))
    i, j = pairs[0], pairs[1]
    d = x[i] - x[j]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    term = hm.conductance(r[i], r[j], dist, dtype(k_p)) * (T[j] - T[i])
    rs = r[i] + r[j]
    q, A = np.zeros(len(x), dtype), np.zeros(len(x), LD)
    np.add.at(q, i, term)
    np.add.at(A, i, np.abs(term).astype(LD) * ((rs + dist) / (rs - dist)).astype(LD))
    return q, A, (rs - dist).astype(F64)


def conduction_case(poly, P=513, seed=9, ncell=10):
    """a cloud in the unit box dense enough for a few contacts per particle, and isolated touching pairs for the exact
    opposite-heat check (particles 0..19: ten pairs far from everything else is not guaranteed, so the test selects the
    particles with exactly one contact from the model)"""
    rng = np.random.default_rng(seed + poly)
    R = 0.25 / ncell * 0.9           # cell edge >= 4 R / 0.9
    x = rng.uniform(0.02, 0.98, (P, 3))
    half = P // 3
    d = rng.normal(size=(half, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x[half:2 * half] = np.clip(x[:half] + d * rng.uniform(1.2, 1.95, (half, 1)) * R * (0.5 if poly else 1.0), 0.001, 0.999)   # inside every grid over the box
    r = rng.uniform(0.5 * R, R, P) if poly else np.full(P, R)
    return Out(x=x, r=r, R=R, rmax=R, T=rng.uniform(300.0, 2000.0, P), k_p=20.0, ncell=ncell, P=P, v=np.zeros((P, 3)))


def c_conduction():
    def measure():
        c = 0.0
        for poly in (False, True):
            k = conduction_case(poly)
            pairs = hm.contacts_all_pairs(k.x, k.r)
            a, A, _ = conduction(LD, k.x, k.r, k.T, k.k_p, pairs)
            b, _, _ = conduction(F64, k.x, k.r, k.T, k.k_p, pairs)
            c = max(c, ratio_c(b, a, A))
        return c
    return _cached("conduction", measure)


# ======================================================================================================================
# the tet level-set geometry in tet_levelset.hpp's order
# ======================================================================================================================
def tet_interp(l, f):
    return ((l[:, 0] * f[:, 0] + l[:, 1] * f[:, 1]) + l[:, 2] * f[:, 2]) + l[:, 3] * f[:, 3]


def tet_cross(x4):
    """(c23, c31, c12, det) of tet_cross()"""
    e1, e2, e3 = x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0], x4[:, 3] - x4[:, 0]
    c23, c31, c12 = _cross(e2, e3), _cross(e3, e1), _cross(e1, e2)
    return c23, c31, c12, (e1[:, 0] * c23[:, 0] + e1[:, 1] * c23[:, 1]) + e1[:, 2] * c23[:, 2]


def tet_gradient(x4, phi):
    """(g, |g|) of tet_levelset()"""
    c23, c31, c12, det = tet_cross(x4)
    d1, d2, d3 = ((phi[:, k] - phi[:, 0])[:, None] for k in (1, 2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        g = ((d1 * c23 + d2 * c31) + d3 * c12) / det[:, None]
        return g, np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])


def grad_max(mesh):
    """surface_grad_max_kernel in float64: the largest sqrt((c0 c0 + c1 c1) + c2 c2) / det in absolute value, a NaN above inf"""
    c23, c31, c12, det = tet_cross(mesh.x[mesh.ien])
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.abs(np.stack([np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) / det for c in (c23, c31, c12)]))
    return np.ascontiguousarray(g).view(np.uint64).max().view(F64) if g.size else F64(0.0)


def _gather(mesh, w, tet, dtype):
    inside = np.asarray(tet, I64) >= 0
    nodes = mesh.ien[np.where(inside, np.asarray(tet, I64), 0)]
    wv = np.asarray(w, dtype)
    N = mesh.N
    return inside, nodes, wv[:3 * N].reshape(-1, 3)[nodes], wv[4 * N:5 * N][nodes], wv[5 * N:][nodes], np.asarray(mesh.x, dtype)[nodes]


# ---- capture ---------------------------------------------------------------------------------------------------------
def capture_flag(dtype, mesh, w, tet, lam, vel, temp, mass, radius, rho_f, cp_p, level, side, reach, T_melt):
    """capture_flag_kernel: keep, rtet, dep [P][5], A_dep; the decision in tet_levelset.hpp's order"""
    P = len(tet)
    tet = np.asarray(tet, I64)
    inside, nodes, u4, phi4, T4, x4 = _gather(mesh, w, tet, dtype)
    l = np.where(inside[:, None], np.asarray(lam, dtype).reshape(-1, 4), 0)
    m, r = (np.broadcast_to(np.asarray(q, dtype), (P,)) for q in (mass, radius))
    phi_p, T_f = tet_interp(l, phi4), tet_interp(l, T4)
    gn = tet_gradient(x4, phi4)[1]
    with np.errstate(invalid="ignore"):
        reach_c = dtype(side) * (phi_p - dtype(level)) + (dtype(reach) * r) * gn
        cap = inside & (reach_c >= 0) & (T_f >= dtype(T_melt))
    uf, auf = _interp_sum(l, u4, dtype)
    v = np.asarray(vel, dtype).reshape(-1, 3)
    dep, A = np.zeros((P, 5), dtype), np.zeros((P, 5), LD)
    dep[:, 0] = m / dtype(rho_f)
    dep[:, 1:4] = m[:, None] * (v - uf)
    A[:, 1:4] = np.abs(m)[:, None] * (np.abs(v) + auf)
    if temp is not None:
        dep[:, 4] = (m * dtype(cp_p)) * (np.asarray(temp, dtype) - T_f)
    dep[~cap], A[~cap] = 0, 0
    return Out(keep=np.where(cap, 0, 1), rtet=np.where(cap, tet, -1), dep=dep, A_dep=A, captured=cap)


def c_capture(case_fn):
    def measure():
        c = 0.0
        for poly in (False, True):
            k = case_fn(poly)
            a, b = (capture_flag(dt, k.mesh, k.w, k.tet, k.lam, k.vel, k.temp, k.m if poly else k.M, k.r if poly else k.R, k.rho_f,
                                 k.cp_p, cm.LEVEL, 1.0, 2.0, cm.T_MELT) for dt in (LD, F64))
            assert np.array_equal(a.keep, b.keep)
            c = max(c, ratio_c(b.dep[:, 1:4], a.dep[:, 1:4], a.A_dep[:, 1:4]))
        return c
    return _cached("capture", measure)


def capture_case(poly, P=513, seed=5):
    """capture_model.decision_case on kuhn(4, 0.2) with capture_model.linear_fields, tets and lambdas by brute()"""
    from dedflow_amd.meshgen import kuhn_cube
    mesh = kuhn(4, 0.2)
    k = cm.decision_case(kuhn_cube(4, jitter=0.2), P=P, seed=seed)
    tet, lam = brute(mesh, k["pts"])
    return Out(mesh=mesh, P=P, w=cm.linear_fields(mesh.x), tet=tet, lam=lam, vel=k["vel"], temp=k["temp"], M=k["mass"], R=k["R"],
               m=k["m"], r=k["r"], rho_f=k["rho_f"], cp_p=k["cp_p"])


# ---- solid-surface contact --------------------------------------------------------------------------------------------
def surface_contact(dtype, mesh, w, tet, lam, vel, mass, radius, kn, gamma_n, level, side, T_solid, law=None, omega=None,
                    old=None):
    """surface_contact_kernel: per particle the masks contact and buried, the additions d_acc and d_alpha [P][3], the new
    spring xi [P][3] (friction), with A_acc, A_alpha, A_xi (before the division by m and I: scale them).  law = (mu, kt,
    gamma_t, dt); old[i] = the previous spring of the surface contact or None"""
    P = len(tet)
    tet = np.asarray(tet, I64)
    inside, nodes, u4, phi4, T4, x4 = _gather(mesh, w, tet, dtype)
    l = np.where(inside[:, None], np.asarray(lam, dtype).reshape(-1, 4), 0)
    m, r = (np.broadcast_to(np.asarray(q, dtype), (P,)) for q in (mass, radius))
    v = np.asarray(vel, dtype).reshape(-1, 3)
    side, level, kn, gamma_n = dtype(side), dtype(level), dtype(kn), dtype(gamma_n)
    q = -(side * (tet_interp(l, phi4) - level))
    T_f = tet_interp(l, T4)
    g, gn = tet_gradient(x4, phi4)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = inside & (gn > 0) & (T_f < dtype(T_solid))
        s = q / gn
        contact, buried = ok & (s > -r) & (s < r), ok & (s <= -r)
        nrm = (-(side * g)) / gn[:, None]
    delta = r - s
    vn = (v[:, 0] * nrm[:, 0] + v[:, 1] * nrm[:, 1]) + v[:, 2] * nrm[:, 2]
    fn = kn * delta - gamma_n * vn
    im = dtype(1.0) / m
    out = Out(contact=contact, buried=buried, s=s, fn=fn, spread=(np.abs(phi4[:, 1] - phi4[:, 0]) + np.abs(phi4[:, 2] - phi4[:, 0]))
              + np.abs(phi4[:, 3] - phi4[:, 0]), q=q, r=r, located=inside, gn=gn, T_f=T_f)
    with np.errstate(invalid="ignore", divide="ignore"):
        kg = np.where(contact, np.linalg.norm(scm.gradient_condition(mesh.x[nodes], np.asarray(w, F64)[4 * mesh.N:5 * mesh.N][nodes]),
                                              axis=1) / gn.astype(LD), 0.0)
    S = (np.abs(kn) * (r + np.abs(s)) + np.abs(gamma_n) * (np.abs(v) * np.abs(nrm)).sum(axis=1)).astype(LD)
    vabs = np.abs(v).sum(axis=1).astype(LD)
    AF = S + (np.abs(kn * s) + 2.0 * (np.abs(gamma_n) * vabs + np.abs(fn))).astype(LD) * kg
    d_acc, d_alpha, xi = np.zeros((P, 3), dtype), np.zeros((P, 3), dtype), np.zeros((P, 3), dtype)
    A_alpha, A_xi = np.zeros(P, LD), np.zeros(P, LD)
    if law is None:
        d_acc = np.where(contact[:, None], (fn[:, None] * nrm) * im[:, None], 0)
    else:
        mu, kt, gt, dts = (dtype(z) for z in law)
        om = np.asarray(omega, dtype).reshape(-1, 3)
        for i in np.flatnonzero(contact):
            ell = max(r[i] - delta[i], dtype(0.0))
            x0 = None if old is None or old[i] is None else np.asarray(old[i], dtype)
            Ft, tq, x1 = fm.tangential(x0, nrm[i], fn[i], ell, v[i], om[i], mu, kt, gt, dts)
            d_acc[i] = (fn[i] * nrm[i] + Ft) * im[i]
            d_alpha[i] = tq * (dtype(1.0) / (dtype(0.4) * m[i] * r[i] * r[i]))
            xi[i] = x1
            Vc = vabs[i] + LD(ell) * np.abs(om[i]).sum()
            xo = 0.0 if x0 is None else np.abs(x0).sum()
            Tt = (1.0 + kg[i]) * ((np.abs(kt) * (xo + np.abs(dts) * Vc) + np.abs(gt) * Vc) + np.abs(mu) * AF[i])
            AF[i] += Tt
            A_alpha[i], A_xi[i] = LD(ell) * Tt, Tt / np.abs(kt)
    out.update(d_acc=d_acc, d_alpha=d_alpha, xi=xi, A_acc=np.where(contact, AF, 0.0), A_alpha=A_alpha, A_xi=A_xi, nrm=nrm)
    return out


KN, GN, MU, DT_S = 1.0e4, 3.0, 0.4, 1e-5
LAW = (MU, 2.0 / 7.0 * KN, GN, DT_S)


def surface_case(kind, poly, P=513, side=1.0):
    """surface_contact_model's plane or sphere case on kuhn(4, 0.2), tets and lambdas by brute()"""
    mesh = kuhn(4, 0.2)
    k = (scm.plane_case if kind == "plane" else scm.sphere_case)(P, poly)
    w = (scm.plane_fields if kind == "plane" else scm.sphere_fields)(mesh.x, side)
    tet, lam = brute(mesh, k["pts"])
    rng = np.random.default_rng(P)
    old = [rng.normal(0, 1e-6, 3) if i % 3 else None for i in range(P)]
    return Out(mesh=mesh, P=P, w=w, tet=tet, lam=lam, vel=k["vel"], omega=k["omega"], M=k["mass"], R=k["R"], m=k["m"], r=k["r"],
               side=side, old=old)


def surface_run(k, dtype, poly, friction, old=False):
    return surface_contact(dtype, k.mesh, k.w, k.tet, k.lam, k.vel, k.m if poly else k.M, k.r if poly else k.R, KN, GN, scm.LEVEL,
                           k.side, scm.T_SOLID, law=LAW if friction else None, omega=k.omega, old=k.old if old else None)


def c_surface():
    """c of (acc, alpha, xi) with friction, the largest over plane and sphere, one size and sizes, with and without history"""
    def measure():
        c = np.zeros(3)
        for kind in ("plane", "sphere"):
            for poly in (False, True):
                k = surface_case(kind, poly)
                for old in (False, True):
                    a, b = surface_run(k, LD, poly, True, old), surface_run(k, F64, poly, True, old)
                    assert np.array_equal(a.contact, b.contact) and np.array_equal(a.buried, b.buried)
                    mass = np.broadcast_to(np.asarray(k.m if poly else k.M, LD), (k.P,))
                    iner = 0.4 * mass * np.broadcast_to(np.asarray(k.r if poly else k.R, LD), (k.P,)) ** 2
                    c = np.maximum(c, [ratio_c(b.d_acc, a.d_acc, (a.A_acc / mass)[:, None] * np.ones(3)),
                                       ratio_c(b.d_alpha, a.d_alpha, (a.A_alpha / iner)[:, None] * np.ones(3)),
                                       ratio_c(b.xi, a.xi, a.A_xi[:, None] * np.ones(3))])
        return c
    return _cached("surface", measure)


def surface_counts(contact, buried, P):
    """step[cur] after one launch: slot (block mod 64) holds contacts | buried << 32 of its blocks (uint64 [64])"""
    out = np.zeros(SURFACE_SLOTS, np.uint64)
    for b in range(max((P + 255) // 256, 1)):
        sl = slice(256 * b, min(256 * (b + 1), P))
        out[b % SURFACE_SLOTS] += np.uint64(int(contact[sl].sum()) | (int(buried[sl].sum()) << 32))
    return out
