"""numpy restatement of the solidification record (include/dedflow.h, "solidification record"): the elementwise rules in
float64 without fused multiply-add -- numpy rounds every operation on its own, so the device must match bit for bit -- and the
recovered gradient in np.longdouble with the abs-sum of every product that enters S_d, which scales the parity bound.  The
skip rules of the gradient (|det| > 0, the mean phi of a tet) are decided in float64 in the device's operation order, so that
model and device take the same tets.  Also the state sequences of the GPU parity test and what they promise.  Test
infrastructure only."""
import numpy as np

LD = np.longdouble
F64 = np.float64


def config(T_front, use_phi=False, level=0.0, side=1, in_time_step=False):
    return dict(T_front=float(T_front), use_phi=bool(use_phi), level=float(level), side=int(side), in_time_step=bool(in_time_step))


def state(N, phi, T):
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = phi
    w[5 * N:] = T
    return w


def node_metal(w, cfg):
    N = w.size // 6
    if not cfg["use_phi"]:
        return np.ones(N, bool)
    return F64(cfg["side"]) * (w[4 * N:5 * N] - cfg["level"]) > 0.0


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _tet_cross(x, dtype):
    """c23, c31, c12, det of tet_cross in its operation order, in `dtype`; x [T, 4, 3]"""
    x = x.astype(dtype)
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = _cross(e2, e3), _cross(e3, e1), _cross(e1, e2)
    det = (e1[:, 0] * c23[:, 0] + e1[:, 1] * c23[:, 1]) + e1[:, 2] * c23[:, 2]
    return c23, c31, c12, det


def tet_counts(xg, ien, w, cfg):
    """boolean [T]: the tets that add to the gradient sums, decided in float64 as the device decides"""
    N = w.size // 6
    tets = ien.reshape(-1, 4)
    det = _tet_cross(xg.reshape(-1, 3)[tets], F64)[3]
    counts = np.abs(det) > 0.0
    if cfg["use_phi"]:
        phi = w[4 * N:5 * N][tets]
        mean = ((phi[:, 0] + phi[:, 1]) + (phi[:, 2] + phi[:, 3])) * 0.25
        counts &= F64(cfg["side"]) * (mean - cfg["level"]) > 0.0
    return counts


def recovered_gradient(xg, ien, w, cfg):
    """grad [N, 3] (longdouble), the abs-sum scale A_d / V [N, 3] of the parity bound, and V [N]"""
    N = w.size // 6
    tets = ien.reshape(-1, 4)
    counts = tet_counts(xg, ien, w, cfg)
    c23, c31, c12, det = _tet_cross(xg.reshape(-1, 3)[tets], LD)
    Tn = w[5 * N:][tets].astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        g1, g2, g3 = c23 / det[:, None], c31 / det[:, None], c12 / det[:, None]
    g0 = -((g1 + g2) + g3)
    prod = [Tn[:, b, None] * g for b, g in enumerate((g0, g1, g2, g3))]
    ge = ((prod[0] + prod[1]) + prod[2]) + prod[3]
    ae = sum(np.abs(p) for p in prod)
    ad = np.abs(det)
    S, A, V = np.zeros((N, 3), LD), np.zeros((N, 3), LD), np.zeros(N, LD)
    for b in range(4):
        n = tets[counts, b]
        np.add.at(S, n, ad[counts, None] * ge[counts])
        np.add.at(A, n, ad[counts, None] * ae[counts])
        np.add.at(V, n, ad[counts])
    pos = V > 0
    grad, scale = np.zeros((N, 3), LD), np.zeros((N, 3), LD)
    grad[pos] = S[pos] / V[pos, None]
    scale[pos] = A[pos] / V[pos, None]
    return grad, scale, V


def front_speed(grad3, cool):
    """R and |G| of the header, float64"""
    g = np.asarray(grad3, F64).reshape(-1, 3)
    G = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(G > 0.0, np.asarray(cool, F64) / G, 0.0), G


class Record:
    """the record of one mesh; update() returns (freeze nodes ascending, melt nodes ascending) and leaves grad3 of the freeze
    nodes as the longdouble gradient rounded to float64 with .grad_ref / .grad_scale holding the unrounded values"""

    def __init__(self, N, cfg):
        self.N, self.cfg = N, cfg
        self.reset()

    def reset(self):
        N = self.N
        self.T_prev = np.full(N, np.nan)
        self.T_peak = np.full(N, -np.inf)
        self.t_liquid = np.zeros(N)
        self.melts = np.zeros(N, np.int32)
        self.t_solid = np.full(N, np.nan)
        self.cool = np.zeros(N)
        self.grad3 = np.zeros((N, 3))
        self.metal = np.zeros(N, bool)
        self.t, self.updates, self.primed = 0.0, 0, False
        self.freeze_last = np.zeros(0, np.int32)
        self.melt_last = np.zeros(0, np.int32)

    def update(self, w, dt, xg=None, ien=None):
        N, Tf = self.N, F64(self.cfg["T_front"])
        dt = F64(dt)
        Tn = w[5 * N:].copy()
        metal = node_metal(w, self.cfg)
        self.updates += 1
        none = np.zeros(0, np.int32)
        if not self.primed:
            self.T_prev = Tn
            self.T_peak = np.fmax(self.T_peak, Tn)
            self.metal = metal
            self.primed = True
            self.freeze_last = self.melt_last = none
            return none, none
        Tp = self.T_prev
        valid = ~np.isnan(Tn)
        with np.errstate(invalid="ignore", divide="ignore"):
            above_p, above_n = Tp >= Tf, Tn >= Tf
            theta = (Tp - Tf) / (Tp - Tn)
            melt_part = (1.0 - (Tf - Tp) / (Tn - Tp)) * dt
            cool = (Tp - Tn) / dt
        m = valid & metal
        both, freeze, melt = m & above_p & above_n, m & above_p & ~above_n, m & ~above_p & above_n
        self.T_peak = np.where(valid, np.fmax(self.T_peak, Tn), self.T_peak)
        self.metal = np.where(valid, metal, self.metal)
        self.t_liquid = self.t_liquid.copy()
        self.t_liquid[both] += dt
        self.t_liquid[freeze] += (theta * dt)[freeze]
        self.t_liquid[melt] += melt_part[melt]
        self.t_solid, self.cool, self.grad3, self.melts = self.t_solid.copy(), self.cool.copy(), self.grad3.copy(), self.melts.copy()
        self.t_solid[freeze] = (F64(self.t) + theta * dt)[freeze]
        self.cool[freeze] = cool[freeze]
        self.melts[melt] += 1
        self.t_solid[melt] = np.nan
        self.cool[melt] = 0.0
        self.grad3[melt] = 0.0
        if xg is not None and freeze.any():
            grad, scale, V = recovered_gradient(xg, ien, w, self.cfg)
            self.grad_ref, self.grad_scale, self.grad_V = grad, scale, V
            self.grad3[freeze] = grad[freeze].astype(F64)
        self.T_prev = np.where(valid, Tn, Tp)
        self.t = float(F64(self.t) + dt)
        self.freeze_last = np.flatnonzero(freeze).astype(np.int32)
        self.melt_last = np.flatnonzero(melt).astype(np.int32)
        return self.freeze_last, self.melt_last


def stats(T_front, T_prev, T_peak, t_solid, cool, grad3, metal, freeze_last=0, melt_last=0):
    """the statistics of the header from the given arrays (the device's own, for a bit-for-bit comparison)"""
    rec = ~np.isnan(t_solid)
    R, G = front_speed(grad3, cool)
    metal = np.asarray(metal, bool)

    def lo(a):
        return float(np.fmin.reduce(a[rec], initial=np.inf))

    def hi(a, sel=rec):
        return float(np.fmax.reduce(a[sel], initial=-np.inf))

    with np.errstate(invalid="ignore"):
        liquid = int((metal & (T_prev >= T_front)).sum())
    return dict(frozen=int(rec.sum()), liquid=liquid, freeze_events_last=int(freeze_last), melt_events_last=int(melt_last),
                G_min=lo(G), G_max=hi(G), cool_min=lo(cool), cool_max=hi(cool), R_min=lo(R), R_max=hi(R),
                T_peak_max=hi(T_peak, metal))


# ---- the state sequences of the parity test -----------------------------------------------------------------------------------
T_FRONT = 1650.0
LEVEL = 0.25          # dyadic, as every planted phi offset: the planted means are exact
DTS = (0.05, 0.0125, 0.1, 0.03)


def _tet_count(ien, N):
    return np.bincount(ien, minlength=N)


def planted_nodes(mesh):
    """(hub, p0, p1, p2, p3): the node with the most tets, and four others (the four nodes of a single tet) for the T patterns"""
    N = mesh.num_node
    hub = int(np.argmax(_tet_count(mesh.ien, N)))
    cand = [n for n in range(N) if n != hub] if N > 4 else list(range(N))
    return hub, cand[0], cand[len(cand) // 3], cand[len(cand) // 2], cand[-1]


def sequence(mesh, use_phi, seed=3):
    """(cfg, [w_0 .. w_4], DTS): w_0 primes, w_k ends update k.  Random T around T_front and, planted,
         p0  above, below, above, below, below: freezes, melts again, freezes a second time;
         p1  T_front exactly, below, T_front exactly, T_front exactly, below: Tp == T_front (theta = 0) and Tn == T_front;
         p2  Tp == Tn above, then Tp == Tn below;
         p3  a NaN at w_2.
       With use_phi: p1 lies exactly on `level` (not metal), one tet has the mean phi exactly `level`, and every tet of the
       metal node p0 has its other non-hub nodes deep in the gas: none of p0's tets counts."""
    N = mesh.num_node
    rng = np.random.default_rng(seed + (100 if use_phi else 0) + N)
    hub, p0, p1, p2, p3 = planted_nodes(mesh)
    tets = mesh.ien.reshape(-1, 4)
    phi = LEVEL + rng.uniform(-0.3, 1.0, N)
    if use_phi:
        if N == 4:
            phi = LEVEL + np.array([1.0, 0.0, -0.5, -0.5])        # p0 metal, p1 on the level, the mean exactly the level
        else:
            mine = (tets == p0).any(axis=1)
            nbrs = np.setdiff1d(np.unique(tets[mine]), [p0, hub])
            phi[nbrs] = LEVEL - 8.0
            phi[p0] = LEVEL + 0.125
            taken = np.union1d(nbrs, [p0, p1])
            free = np.flatnonzero(~np.isin(tets, taken).any(axis=1))
            e1 = list(tets[free[-1]])
            if hub in e1:
                e1.remove(hub)
                e1.insert(0, hub)
            else:
                phi[hub] = LEVEL + 1.0
            phi[e1] = LEVEL + np.array([0.5, 0.25, -0.5, -0.25])
            phi[p1] = LEVEL
    Ts = [T_FRONT + rng.uniform(-40.0, 40.0, N) for _ in range(5)]
    for k, v in enumerate((0.5, -0.5, 0.75, -0.25, -0.375)):
        Ts[k][p0] = T_FRONT + v
    for k, v in enumerate((0.0, -0.5, 0.0, 0.0, -1.0)):
        Ts[k][p1] = T_FRONT + v
    for k, v in enumerate((0.25, 0.25, -0.25, -0.25, -0.25)):
        Ts[k][p2] = T_FRONT + v
    Ts[2][p3] = np.nan
    cfg = config(T_FRONT, use_phi=use_phi, level=LEVEL, side=1)
    return cfg, [state(N, phi, T) for T in Ts], DTS


def run_model(mesh, cfg, states, dts):
    """the Record after the prime and every update, with the per-update events: [(freeze, melt, snapshot dict)]"""
    rec = Record(mesh.num_node, cfg)
    rec.update(states[0], dts[0])
    out = []
    for w, dt in zip(states[1:], dts):
        f, m = rec.update(w, dt, mesh.xg, mesh.ien)
        out.append((f.copy(), m.copy()))
    return rec, out
