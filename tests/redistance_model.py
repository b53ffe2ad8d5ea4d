"""numpy model of the level-set redistancing (include/dedflow.h, "level-set redistancing"): the text of that section, facet
by facet and node by node against every facet (brute force, no grid).  Written from the header, not from the kernel.  In
float64 every operation has the association the header states, so a correct kernel agrees to the last bit; dtype=np.longdouble
runs the same model in extended precision (the decisions -- which nodes are positive -- are taken from the float64 input either
way).  Test infrastructure only; shared by test_redistance_cpu.py (the model against analysis) and test_gpu_redistance.py (the
kernels against the model)."""
import itertools

import numpy as np

LD = np.longdouble


def refusal(level, band, every=0):
    """why DflMeshSetRedistance refuses the configuration, or None"""
    if not np.isfinite(level):
        return "level"
    if not np.isfinite(band) or not band > 0.0:
        return "band"
    if every < 0:
        return "every"
    return None


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _tets(xg, ien, phi, level, dtype):
    ien = np.asarray(ien).reshape(-1, 4)
    x = np.asarray(xg, np.float64).reshape(-1, 3).astype(dtype)[ien]          # [T, 4, 3]
    ph = np.asarray(phi, np.float64).astype(dtype)[ien]
    with np.errstate(invalid="ignore"):
        f = ph - dtype(level)
        pos = f > 0
    return ien, x, ph, f, pos


def _crossing(x, f, i, j):
    """P_ij of the tets whose arrays are given: x [n, 4, 3], f [n, 4], local indices i (positive), j [n]"""
    r = np.arange(len(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = f[r, i] / (f[r, i] - f[r, j])
        return x[r, i] + t[:, None] * (x[r, j] - x[r, i])


def _cases(pos):
    """per tet: number of positive nodes, and for the cut tets the local indices the header names"""
    npos = pos.sum(axis=1)
    order = np.argsort(~pos, axis=1, kind="stable")                           # positives first, each part in local order
    return npos, order


def facets(xg, ien, phi, level, dtype=np.float64):
    """the facet list [nf, 9] in ascending tet id, a quad's first triangle first; and the tet of every facet"""
    ien, x, ph, f, pos = _tets(xg, ien, phi, level, dtype)
    npos, order = _cases(pos)
    T = len(ien)
    out = np.zeros((T, 2, 9), dtype)
    nf = np.where((npos == 0) | (npos == 4), 0, np.where(npos == 2, 2, 1))
    k = np.flatnonzero(npos == 1)
    if k.size:
        i = order[k, 0]
        for v in range(3):
            out[k, 0, 3 * v:3 * v + 3] = _crossing(x[k], f[k], i, order[k, 1 + v])
    k = np.flatnonzero(npos == 3)
    if k.size:
        j = order[k, 3]
        for v in range(3):
            out[k, 0, 3 * v:3 * v + 3] = _crossing(x[k], f[k], order[k, v], j)
    k = np.flatnonzero(npos == 2)
    if k.size:
        a, b, c, d = (order[k, q] for q in range(4))
        Q = [_crossing(x[k], f[k], a, c), _crossing(x[k], f[k], a, d), _crossing(x[k], f[k], b, d), _crossing(x[k], f[k], b, c)]
        out[k, 0] = np.concatenate([Q[0], Q[1], Q[2]], axis=1)
        out[k, 1] = np.concatenate([Q[0], Q[2], Q[3]], axis=1)
    keep = np.arange(2)[None, :] < nf[:, None]
    return out[keep], np.repeat(np.arange(T), nf)


def _lower(best, cand, ok=None):
    """best where the candidate does not win; a NaN never wins"""
    with np.errstate(invalid="ignore"):
        win = cand < best
    if ok is not None:
        win &= ok
    return np.where(win, cand, best)


def dist2(p, F):
    """squared point-facet distance, p [..., 3] against F [..., 9] (broadcast): the seven candidates of the header"""
    A, B, C = F[..., 0:3], F[..., 3:6], F[..., 6:9]
    zero, one = p.dtype.type(0), p.dtype.type(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        best = np.full(np.broadcast(p[..., 0], A[..., 0]).shape, np.inf, p.dtype)
        for V in (A, B, C):
            r = p - V
            best = _lower(best, dot(r, r))
        for U, V in ((A, B), (B, C), (C, A)):
            e = V - U
            ee = dot(e, e)
            ok = ee > 0
            t = dot(p - U, e) / np.where(ok, ee, one)
            t = np.where(t < 0, zero, np.where(t > 1, one, t))
            r = p - (U + t[..., None] * e)
            best = _lower(best, dot(r, r), ok)
        ab, ac = B - A, C - A
        n = cross(ab, ac)
        nn = dot(n, n)
        w = p - A
        n_b = np.broadcast_to(n, w.shape)
        b1, b2 = dot(cross(w, np.broadcast_to(ac, w.shape)), n_b), dot(cross(np.broadcast_to(ab, w.shape), w), n_b)
        ok = (nn > 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= nn)
        s = dot(w, n_b)
        best = _lower(best, (s * s) / np.where(nn > 0, nn, one), ok)
    return best


def distance(xg, F, dtype=np.float64, nodes=None, chunk=256):
    """d_a = sqrt(min over all facets of dist2), +inf without a facet; nodes: only these (the others +inf)"""
    x = np.asarray(xg, np.float64).reshape(-1, 3).astype(dtype)
    N = len(x)
    d2 = np.full(N, np.inf, dtype)
    idx = np.arange(N) if nodes is None else np.flatnonzero(nodes)
    F = np.asarray(F, dtype)
    if len(F):
        for s in range(0, idx.size, chunk):
            sel = idx[s:s + chunk]
            with np.errstate(invalid="ignore"):
                d2[sel] = np.fmin.reduce(dist2(x[sel][:, None, :], F[None, :, :]), axis=1, initial=np.inf)
    return np.sqrt(d2)


def hold_mask(mesh, hold_groups):
    held = np.zeros(mesh.num_node, bool)
    for g in range(min(mesh.num_bound, 31)):
        if (hold_groups >> g) & 1:
            held[mesh.bound_node[mesh.bound_node_offset[g]:mesh.bound_node_offset[g + 1]]] = True
    return held


def redistance(mesh, phi, level, band, hold_groups=0, dtype=np.float64, nodes=None):
    """dict: phi (the new field, float64 input bits where a node keeps its value), d, facets, band (the nodes with d < band),
    kept (held or NaN)"""
    phi = np.asarray(phi, np.float64)
    F, _ = facets(mesh.xg, mesh.ien, phi, level, dtype)
    d = distance(mesh.xg, F, dtype, nodes)
    with np.errstate(invalid="ignore"):
        positive = phi - level > 0
        m = np.where(d < dtype(band), d, dtype(band))
    new = dtype(level) + np.where(positive, m, -m)
    kept = np.isnan(phi) | hold_mask(mesh, hold_groups)
    new = np.where(kept, phi.astype(dtype), new)
    with np.errstate(invalid="ignore"):
        in_band = d < dtype(band)
    return dict(phi=new, d=d, facets=F, band=in_band, kept=kept)


# ---- the statistics ------------------------------------------------------------------------------------------------------------
def _det4(q0, q1, q2, q3):
    return dot(q1 - q0, cross(q2 - q0, q3 - q0))


def tet_volumes(xg, ien, phi, level, dtype=np.float64):
    """per tet the volume of {phi > level} in the header's decomposition (a NaN value counts 0), and the tet volumes"""
    ien, x, ph, f, pos = _tets(xg, ien, phi, level, dtype)
    npos, order = _cases(pos)
    six = dtype(6)
    full = np.abs(_det4(x[:, 0], x[:, 1], x[:, 2], x[:, 3])) / six
    vol = np.where(npos == 4, full, dtype(0))
    r = np.arange(len(ien))
    for count in (1, 3):
        k = np.flatnonzero(npos == count)
        if not k.size:
            continue
        lone = order[k, 0] if count == 1 else order[k, 3]
        others = [order[k, 1 + v] if count == 1 else order[k, v] for v in range(3)]
        P = [_crossing(x[k], f[k], lone, o) if count == 1 else _crossing(x[k], f[k], o, lone) for o in others]
        corner = np.abs(_det4(x[k, lone], P[0], P[1], P[2])) / six
        vol[k] = corner if count == 1 else full[k] - corner
    k = np.flatnonzero(npos == 2)
    if k.size:
        a, b, c, d = (order[k, q] for q in range(4))
        u = [x[k, a], _crossing(x[k], f[k], a, c), _crossing(x[k], f[k], a, d)]
        v = [x[k, b], _crossing(x[k], f[k], b, c), _crossing(x[k], f[k], b, d)]
        vol[k] = ((np.abs(_det4(u[0], u[1], u[2], v[0])) + np.abs(_det4(u[1], u[2], v[0], v[1])))
                  + np.abs(_det4(u[2], v[0], v[1], v[2]))) / six
    return np.where(np.isnan(vol), dtype(0), vol), full


def volume(xg, ien, phi, level, dtype=np.float64):
    return tet_volumes(xg, ien, phi, level, dtype)[0].astype(LD).sum()


def grad_dev(xg, ien, phi, level, dtype=np.float64):
    """max of ||g| - 1| over the cut tets, a NaN passed over, 0 without one"""
    ien, x, ph, f, pos = _tets(xg, ien, phi, level, dtype)
    npos = pos.sum(axis=1)
    cut = (npos > 0) & (npos < 4)
    if not cut.any():
        return 0.0
    x, ph = x[cut], ph[cut]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = cross(e2, e3), cross(e3, e1), cross(e1, e2)
    det = dot(e1, c23)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (((ph[:, 1] - ph[:, 0])[:, None] * c23 + (ph[:, 2] - ph[:, 0])[:, None] * c31) + (ph[:, 3] - ph[:, 0])[:, None] * c12) \
            / det[:, None]
        dev = np.abs(np.sqrt(dot(g, g)) - 1)
    dev = dev[~np.isnan(dev)]
    return float(dev.max()) if dev.size else 0.0


def stats(mesh, phi, res, level, dtype=np.float64):
    """DflRedistanceStats of the call that turned phi into res (a dict of redistance)"""
    old, new = np.asarray(phi, np.float64), np.asarray(res["phi"], np.float64)
    with np.errstate(invalid="ignore"):
        change = np.where(res["kept"], 0.0, np.abs(new - old))[res["band"]]
    return dict(facets=len(res["facets"]), band_nodes=int(res["band"].sum()), max_change=float(change.max()) if change.size else 0.0,
                grad_dev_before=grad_dev(mesh.xg, mesh.ien, old, level, dtype), grad_dev_after=grad_dev(mesh.xg, mesh.ien, new, level, dtype),
                volume_before=float(volume(mesh.xg, mesh.ien, old, level, dtype)),
                volume_after=float(volume(mesh.xg, mesh.ien, new, level, dtype)))


def clipped_cube_volume(n, s):
    """volume of {x in [0, 1]^3 : n . x > s}, every n_d != 0: the cube minus the corner simplex sum
    (1 / (6 n0 n1 n2)) sum over the cube's vertices v of (-1)^|v| max(0, s - n . v)^3 (after x_d -> 1 - x_d where n_d < 0)"""
    n, s = np.asarray(n, LD), LD(s)
    s = s - n[n < 0].sum()
    n = np.abs(n)
    below = LD(0)
    for v in itertools.product((0, 1), repeat=3):
        below += (-1) ** sum(v) * max(LD(0), s - (n * np.array(v, LD)).sum()) ** 3
    return float(1 - below / (6 * n.prod()))
