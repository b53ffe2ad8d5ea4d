"""numpy restatement of the track cross-sections (include/dedflow.h, "track cross-sections"; host/track.c, csrc/k_track.hip),
in two forms: float64 in the stated operation order for every decision and every vertex coordinate (the pair list, the
extents and the vertices are the library's bit for bit), and np.longdouble for the three area sums (the library sums in a
fixed tree; the test holds it to 1e-12 x area_scale of these).  Scalars are Python floats: IEEE doubles, one rounding per
operation, no fused multiply-add.  Test infrastructure only."""
import numpy as np

LD = np.longdouble
INF = float("inf")
Y, H, F, G = 0, 1, 2, 3
MAX_STATION = 64
EXTENTS = ("height", "depth", "y_lo_clad", "y_hi_clad", "y_lo_fused", "y_hi_fused")
AREAS = ("area_clad", "area_fused", "area_scale")


def config(stations, origin=(0.0, 0.0, 0.0), normal=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), level=0.0, side=1, T_fuse=0.0, every=0):
    return dict(stations=[float(c) for c in stations], origin=tuple(map(float, origin)), normal=tuple(map(float, normal)),
                up=tuple(map(float, up)), level=float(level), side=int(side), T_fuse=float(T_fuse), every=int(every))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frame(cfg):
    """n, u, t as float64 [3] each"""
    normal, up = np.array(cfg["normal"], np.float64), np.array(cfg["up"], np.float64)
    n = normal / np.sqrt(_dot(normal, normal))
    u = up - _dot(up, n) * n
    u = u / np.sqrt(_dot(u, u))
    t = np.array([u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0]])
    return n, u, t


def nodal(xg, w, T_peak, cfg):
    """s, y, h, f, g of every node; T_peak None: every g is -inf"""
    x = np.asarray(xg, np.float64).reshape(-1, 3)
    N = x.shape[0]
    n, u, t = frame(cfg)
    d = x - np.array(cfg["origin"], np.float64)
    dc = (d[:, 0], d[:, 1], d[:, 2])
    with np.errstate(invalid="ignore", over="ignore"):
        s, y, h = _dot(dc, n), _dot(dc, t), _dot(dc, u)
        f = np.asarray(w, np.float64)[4 * N:5 * N] - cfg["level"]
        if cfg["side"] < 0:
            f = -f
        g = np.full(N, -INF) if T_peak is None else np.asarray(T_peak, np.float64) - cfg["T_fuse"]
    return s, y, h, f, g


def pair_list(ien, s, f, stations):
    """the pair list (tet ids, by station then ascending) and the 65 segment offsets"""
    tets = np.asarray(ien).reshape(-1, 4)
    metal = (f[tets] > 0.0).any(axis=1)
    segs, off = [], np.zeros(MAX_STATION + 1, np.int32)
    with np.errstate(invalid="ignore"):
        for k, c in enumerate(stations):
            npos = ((s[tets] - c) > 0.0).sum(axis=1)
            segs.append(np.flatnonzero((npos > 0) & (npos < 4) & metal).astype(np.int32))
            off[k + 1] = off[k] + segs[-1].size
    off[len(stations) + 1:] = off[len(stations)]
    return (np.concatenate(segs) if segs else np.zeros(0, np.int32)), off


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def facet_edges(sigma):
    """the facets of the surface sigma = 0 in one tet as lf_tet_facets_ijt orders them: triangles of edges (i, j)"""
    pos = [a for a in range(4) if sigma[a] > 0.0]
    neg = [a for a in range(4) if not sigma[a] > 0.0]
    if len(pos) == 1:
        return [[(pos[0], o) for o in neg]]
    if len(pos) == 3:
        return [[(o, neg[0]) for o in pos]]
    if len(pos) == 2:
        (a, b), (c, d) = pos, neg
        q = [(a, c), (a, d), (b, d), (b, c)]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def _carry(qa, qb, t):
    return [a + t * (b - a) for a, b in zip(qa, qb)]


def clip(poly, comp, inside, cap):
    """Sutherland-Hodgman over vertices [y, h, f, g]: U when inside, then the crossing from the inside vertex towards the
    outside one when exactly one of U, V is inside; a vertex beyond cap is dropped"""
    out = []
    n = len(poly)
    for e in range(n):
        U, V = poly[e], poly[(e + 1) % n]
        iu, iv = inside(U[comp]), inside(V[comp])
        if iu and len(out) < cap:
            out.append(U)
        if iu != iv:
            A, B = (U, V) if iu else (V, U)
            tau = _div(A[comp], A[comp] - B[comp])
            if len(out) < cap:
                out.append(_carry(A, B, tau))
    return out


def fan_area(poly, dtype=float):
    """(the area in dtype, whether the float64 area is a NaN and so counts 0)"""
    a64, a = 0.0, dtype(0.0)
    y0, h0 = poly[0][Y], poly[0][H]
    for k in range(1, len(poly) - 1):
        ay, ah, by, bh = poly[k][Y] - y0, poly[k][H] - h0, poly[k + 1][Y] - y0, poly[k + 1][H] - h0
        a64 = a64 + 0.5 * abs(ay * bh - by * ah)
        if dtype is not float:
            a = a + dtype(0.5) * abs(dtype(ay) * dtype(bh) - dtype(by) * dtype(ah))
    if a64 != a64:
        return dtype(0.0), 0.0
    return (a if dtype is not float else a64), a64


def positive(q):
    return q > 0.0


def not_positive(q):
    return not q > 0.0


def not_negative(q):
    return q >= 0.0


def cut_pair(nodes, sigma):
    """the polygons of one pair: per facet (triangle, clad, fused) as vertex lists; nodes: four [y, h, f, g]"""
    out = []
    for tri_edges in facet_edges(sigma):
        tri = []
        for i, j in tri_edges:
            t = _div(sigma[i], sigma[i] - sigma[j])
            tri.append(_carry(nodes[i], nodes[j], t))
        metal = clip(tri, F, positive, 4)
        clad = clip(metal, H, positive, 5)
        fused = clip(clip(metal, H, not_positive, 5), G, not_negative, 6)
        out.append((tri, clad, fused))
    return out


def _empty():
    r = dict(area_clad=0.0, area_fused=0.0, area_scale=0.0, height=-INF, depth=-INF, y_lo_clad=INF, y_hi_clad=-INF,
             y_lo_fused=INF, y_hi_fused=-INF, pairs=0, dilution=0.0)
    r["ld"] = {k: LD(0.0) for k in AREAS}
    return r


def empty_result(num_station):
    return [_empty() for _ in range(num_station)]


def evaluate(mesh, w, T_peak, cfg):
    """(results per station, pair list, offsets).  A result holds the float64 areas summed pair by pair in list order, the
    extents bit for bit as the library reports them, pairs, dilution of the float64 areas, and under "ld" the three areas in
    np.longdouble"""
    s, y, h, f, g = nodal(mesh.xg, w, T_peak, cfg)
    tets = np.asarray(mesh.ien).reshape(-1, 4)
    lst, off = pair_list(mesh.ien, s, f, cfg["stations"])
    res = []
    for k, c in enumerate(cfg["stations"]):
        r = _empty()
        r["pairs"] = int(off[k + 1] - off[k])
        for e in lst[off[k]:off[k + 1]]:
            nd = tets[e]
            nodes = [[float(y[a]), float(h[a]), float(f[a]), float(g[a])] for a in nd]
            sigma = [float(s[a]) - c for a in nd]
            pc = pf = ps = 0.0
            for tri, clad, fused in cut_pair(nodes, sigma):
                a_ld, a = fan_area(tri, LD)
                ps, r["ld"]["area_scale"] = ps + a, r["ld"]["area_scale"] + a_ld
                if len(clad) >= 3:
                    a_ld, a = fan_area(clad, LD)
                    pc, r["ld"]["area_clad"] = pc + a, r["ld"]["area_clad"] + a_ld
                    for v in clad:
                        if v[H] > r["height"]: r["height"] = v[H]
                        if v[Y] < r["y_lo_clad"]: r["y_lo_clad"] = v[Y]
                        if v[Y] > r["y_hi_clad"]: r["y_hi_clad"] = v[Y]
                if len(fused) >= 3:
                    a_ld, a = fan_area(fused, LD)
                    pf, r["ld"]["area_fused"] = pf + a, r["ld"]["area_fused"] + a_ld
                    for v in fused:
                        if -v[H] > r["depth"]: r["depth"] = -v[H]
                        if v[Y] < r["y_lo_fused"]: r["y_lo_fused"] = v[Y]
                        if v[Y] > r["y_hi_fused"]: r["y_hi_fused"] = v[Y]
            r["area_clad"], r["area_fused"], r["area_scale"] = r["area_clad"] + pc, r["area_fused"] + pf, r["area_scale"] + ps
        for key in EXTENTS:
            r[key] = r[key] + 0.0                                   # a zero extent is +0.0
        both = r["area_clad"] + r["area_fused"]
        r["dilution"] = r["area_fused"] / both if both > 0.0 else 0.0
        res.append(r)
    return res, lst, off


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------
BEAD = dict(area_clad=0.05, area_fused=0.0625, height=0.2, depth=0.1, y_lo_clad=-0.25, y_hi_clad=0.25, y_lo_fused=-0.375,
            y_hi_fused=0.375, dilution=5.0 / 9.0)
BEAD_STATIONS = (0.25, 0.3, 0.41, 0.5)


def state(N, phi, T=0.0):
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = phi
    w[5 * N:] = T
    return w


def bead(mesh, stations=BEAD_STATIONS):
    """the bead of the issue on the unit cube: (cfg, w, T_peak).  phi = 0.7 - z - 0.8 |y - 0.5| is piecewise linear on a
    mesh with a node plane at y = 0.5; the clad is the triangle |y'| < 0.25 (1 - h / 0.2), the fused zone the trapezoid
    -0.1 <= h <= 0 under the same flanks"""
    x = mesh.xg.reshape(-1, 3)
    phi = 0.7 - x[:, 2] - 0.8 * np.abs(x[:, 1] - 0.5)
    T_peak = 1700.0 + 1000.0 * (x[:, 2] - 0.4)
    cfg = config(stations, origin=(0.0, 0.5, 0.5), normal=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), level=0.0, side=1, T_fuse=1700.0)
    return cfg, state(mesh.num_node, phi), T_peak


ALL_FUSED = -1e300      # a finite T_fuse below every T_peak: every g is positive (the configuration refuses -inf)


def all_metal(mesh, stations, normal=(1.0, 0.0, 0.0), origin=(0.0, 0.0, 0.5), up=(0.0, 0.0, 1.0)):
    """the area rule: everything metal and fused, so area_clad + area_fused is the area of the plane inside the mesh"""
    cfg = config(stations, origin=origin, normal=normal, up=up, level=-1.0, side=1, T_fuse=ALL_FUSED)
    return cfg, state(mesh.num_node, 1.0), np.zeros(mesh.num_node)


def wavy(mesh, num_station=5, side=1, seed=3):
    """a generic case on any mesh, in the coordinates xi of its bounding box: (cfg, w, T_peak).  An oblique frame, a tilted,
    rippled surface around mid height, a peak temperature that crosses T_fuse inside the metal, and num_station stations
    across the mesh, the middle one exactly at the s of a node"""
    x = mesh.xg.reshape(-1, 3)
    lo, hi = x.min(axis=0), x.max(axis=0)
    xi = (x - lo) / (hi - lo)
    rng = np.random.default_rng(seed)
    phi = 0.62 - xi[:, 2] + 0.11 * np.sin(5.0 * xi[:, 0] + 1.0) * np.cos(4.0 * xi[:, 1]) + 0.01 * rng.uniform(-1, 1, x.shape[0])
    if side < 0:
        phi = -phi
    T_peak = 1500.0 + 900.0 * xi[:, 2] + 150.0 * np.cos(3.0 * xi[:, 1] + xi[:, 0]) + 5.0 * rng.uniform(-1, 1, x.shape[0])
    base = dict(origin=tuple(lo + np.array([0.1, 0.45, 0.47]) * (hi - lo)), normal=(1.0, 0.2, -0.1), up=(0.05, -0.1, 1.0),
                level=0.02 * side, side=side, T_fuse=1900.0)
    w = state(mesh.num_node, phi)
    s = nodal(mesh.xg, w, T_peak, config([0.0], **base))[0]
    stations = np.linspace(s.min(), s.max(), num_station + 2)[1:-1]
    mid = num_station // 2
    on_node = s[np.argmin(np.abs(s - stations[mid]))]
    if (mid == 0 or on_node > stations[mid - 1]) and (mid == num_station - 1 or on_node < stations[mid + 1]):
        stations[mid] = on_node
    return config(stations, **base), w, T_peak
