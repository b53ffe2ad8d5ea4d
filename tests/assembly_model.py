"""Plain numpy model of the assembly kernels (dedflow_amd/csrc/k_assemble.hip, k_assemble2.hip, asm_device.hpp), written from
the weak form as the kernels and DESIGN.md document it: the literal 4-point (volume) and 3-point (face) quadrature loops,
never the kernels' reassociated "eleven scalar sums".  Test infrastructure only.

Every value is an `AV`: the value `v` (np.longdouble for the model, np.float64 for the float64 restatement of the same
formulas), its ABS-SUM `a` -- the same expression with every term replaced by its absolute value -- and `t`, the abs-sum of
only those terms that carry a stabilisation parameter (tauM, tauC, tau_phi, tau_T).  The leaves are the edge vectors of a tet
(coordinate differences: one rounding each), the nodal fields and the float64 constants of asm_device.hpp; a quotient takes its
denominator as exact (what the cancellation in a determinant costs is part of the measured constant c, and for the stretched
family of the factor kappa_inf(J)).  Bounds of the GPU tests are err <= 8 c u K a (+ 2.2e-14 t for the Newton-seeded kernels),
per entry, never per array.

int64 mode: the pure data-movement operations (records, ordered sums, gathers, the nonzero search) take any dtype.
"""
import types

import numpy as np

from krylov_model import EXTENDED_REASON, HAVE_EXTENDED, U  # noqa: F401  (re-exported)

F64, LD, I64, I32 = np.float64, np.longdouble, np.int64, np.int32

# ---- constants of asm_device.hpp, the float64 values the compiler sees ------------------------------------------------------
RHOC, DT = 0.5, 5e-2
ALPHAM = (3.0 - RHOC) / (1.0 + RHOC)
ALPHAF = 1.0 / (1.0 + RHOC)
GAMMA = 0.5 + ALPHAM - ALPHAF
RHO, CP, KAPPA, MU = 1.0e3, 1.0, 0.66, 10.0 / 3.0
GW, GWB = 0.0416666666666667, 0.1666666666666667
SHA, SHB = 0.5854101966249685, 0.1381966011250105
F3 = 0.6666666666666667
FACT1, FACT2 = ALPHAM, DT * ALPHAF * GAMMA
SHL = np.full((4, 4), SHB)
SHL[np.arange(4), np.arange(4)] = SHA                       # SHL[a, q]
SHLUB = np.array([0.0, GWB, GWB, F3, 0.0, GWB, F3, GWB, 0.0, F3, GWB, GWB,
                  GWB, 0.0, GWB, F3, GWB, 0.0, F3, GWB, F3, 0.0, GWB, GWB,
                  F3, GWB, 0.0, GWB, GWB, F3, 0.0, GWB, GWB, GWB, 0.0, F3,
                  GWB, F3, GWB, 0.0, GWB, GWB, F3, 0.0, F3, GWB, GWB, 0.0]).reshape(4, 3, 4)   # [iorn, q, a]
NV2 = np.array([1.0, 1.0, 1.0, -1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -1.0]).reshape(4, 3)
NREC, XUREC, FREC = 16, 8, 8
NEWTON = 2.2e-14   # (3/2) 2^-46: one Newton step from a 2^-23 seed (asm_device.hpp, rsqrt_nr1)


# ======================================================================================================================
# value / abs-sum / tau-abs-sum arithmetic
# ======================================================================================================================
class AV:
    __slots__ = ("v", "a", "t")

    def __init__(self, v, a=None, t=None):
        self.v = v
        self.a = np.abs(v) if a is None else a
        self.t = np.zeros_like(self.a) if t is None else t

    @staticmethod
    def of(x, like):
        if isinstance(x, AV):
            return x
        return AV(np.asarray(x).astype(like.v.dtype))

    def __add__(self, o):
        o = AV.of(o, self)
        return AV(self.v + o.v, self.a + o.a, self.t + o.t)

    __radd__ = __add__

    def __sub__(self, o):
        o = AV.of(o, self)
        return AV(self.v - o.v, self.a + o.a, self.t + o.t)

    def __rsub__(self, o):
        return AV.of(o, self) - self

    def __neg__(self):
        return AV(-self.v, self.a, self.t)

    def __mul__(self, o):
        o = AV.of(o, self)
        a = self.a * o.a
        return AV(self.v * o.v, a, a - (self.a - self.t) * (o.a - o.t))

    __rmul__ = __mul__

    def over(self, den):
        """self / den with an exact denominator (an array of the model's dtype)"""
        d = np.abs(den)
        return AV(self.v / den, self.a / d, self.t / d)

    def _unary(self, v):
        """a function of a positive argument: the relative width a / v of the argument carries over"""
        a = np.abs(v) * (self.a / np.abs(self.v))
        return AV(v, a)

    def sqrt(self):
        return self._unary(np.sqrt(self.v))

    def rsqrt(self):
        return self._unary(1.0 / np.sqrt(self.v))

    def recip(self):
        return self._unary(1.0 / self.v)

    def fabs(self):
        return AV(np.abs(self.v), self.a, self.t)

    def tau(self):
        """mark as a stabilisation parameter: every term it enters counts into t"""
        return AV(self.v, self.a, self.a.copy())

    def __getitem__(self, k):
        return AV(self.v[k], self.a[k], self.t[k])

    def sum(self, axis):
        return AV(self.v.sum(axis), self.a.sum(axis), self.t.sum(axis))

    def reshape(self, *s):
        return AV(self.v.reshape(*s), self.a.reshape(*s), self.t.reshape(*s))

    @staticmethod
    def stack(items, axis=-1):
        return AV(np.stack([i.v for i in items], axis), np.stack([i.a for i in items], axis),
                  np.stack([i.t for i in items], axis))

    @staticmethod
    def zeros(shape, dt):
        return AV(np.zeros(shape, dt))

    def scatter_add(self, n, idx):
        """sum of the entries into n slots, entry k into slot idx[k] (flat)"""
        out = AV.zeros(n, self.v.dtype)
        for dst, src in ((out.v, self.v), (out.a, self.a), (out.t, self.t)):
            np.add.at(dst, np.asarray(idx).ravel(), src.ravel())
        return out


def _in(x, dt):
    """float64 inputs in the model's dtype; longdouble inputs (the rotated copies of the identity tests) stay as they are"""
    x = np.asarray(x)
    return x if (x.dtype == LD and dt == LD) else np.asarray(x, F64).astype(dt)


def dot3(p, q):
    """sum over the last axis (3 terms, in order)"""
    return p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]


# ======================================================================================================================
# geometry
# ======================================================================================================================
class Geo:
    """shg (B,4,3), inv (B,3,3) = d xi_i / d x_j, det (signed), detJ = |det|, gg = sum G_ij^2, tr = trace G, itr = 1 / tr"""


def geometry(X, dt=LD):
    """X (B,4,3) float64 vertex coordinates.  Closed form: cofactors over the determinant (tet_geometry)."""
    X = _in(X, dt)
    j = [[AV(X[:, c + 1, r] - X[:, 0, r]) for c in range(3)] for r in range(3)]   # j[r][c]: column c = x_{c+1} - x_0
    c00 = j[1][1] * j[2][2] - j[1][2] * j[2][1]
    c01 = j[1][2] * j[2][0] - j[1][0] * j[2][2]
    c02 = j[1][0] * j[2][1] - j[1][1] * j[2][0]
    det = j[0][0] * c00 + j[0][1] * c01 + j[0][2] * c02
    adj = [[c00, j[0][2] * j[2][1] - j[0][1] * j[2][2], j[0][1] * j[1][2] - j[0][2] * j[1][1]],
           [c01, j[0][0] * j[2][2] - j[0][2] * j[2][0], j[0][2] * j[1][0] - j[0][0] * j[1][2]],
           [c02, j[0][1] * j[2][0] - j[0][0] * j[2][1], j[0][0] * j[1][1] - j[0][1] * j[1][0]]]
    g = Geo()
    g.inv = AV.stack([AV.stack([adj[i][k].over(det.v) for k in range(3)]) for i in range(3)], axis=1)   # (B,3,3)
    g.det, g.detJ = det, det.fabs()
    s0 = AV.stack([-g.inv[:, 0, d] - g.inv[:, 1, d] - g.inv[:, 2, d] for d in range(3)])
    g.shg = AV.stack([s0, g.inv[:, 0], g.inv[:, 1], g.inv[:, 2]], axis=1)                            # (B,4,3)
    G = [[dot3(g.inv[:, i], g.inv[:, k]) for k in range(3)] for i in range(3)]
    gg = G[0][0] * G[0][0]
    for i in range(3):
        for k in range(3):
            if i or k:
                gg = gg + G[i][k] * G[i][k]
    g.gg, g.tr = gg, G[0][0] + G[1][1] + G[2][2]
    g.itr = g.tr.recip()
    return g


def kappa_inf(X):
    """kappa_inf(J) of every tet, in longdouble"""
    X = np.asarray(X, F64).astype(LD)
    J = np.stack([X[:, c + 1] - X[:, 0] for c in range(3)], axis=2)            # (B,3,3) columns = edges
    Ji = geometry(X, LD).inv.v
    return (np.abs(J).sum(2).max(1) * np.abs(Ji).sum(2).max(1)).astype(F64)


def geometry_from_record(rec, dt=LD):
    """the Geo a kernel sees that READS the cached record (tet_lhs_kernel): shg, |det J|, gg, 1 / tr G are its leaves"""
    rec = _in(np.asarray(rec).reshape(-1, 16), dt)
    g = Geo()
    g.shg = AV(rec[:, :12].reshape(-1, 4, 3))
    g.detJ, g.gg, g.itr = AV(rec[:, 12]), AV(rec[:, 13]), AV(rec[:, 14])
    return g


def geometry_record(g):
    """the elem_geometry_kernel record: shg[12], |det J|, gg, 1 / tr G, pad"""
    B = g.detJ.v.shape[0]
    z = AV.zeros(B, g.detJ.v.dtype)
    return AV.stack([g.shg[:, a, d] for a in range(4) for d in range(3)] + [g.detJ, g.gg, g.itr, z])


# ======================================================================================================================
# element residual: six rows per node (u0 u1 u2 p phi T)
# ======================================================================================================================
def element_fields(ien, N, wg, dwg):
    """nodal values of the tets: W (B,4,6) = u0 u1 u2 p phi T with p from the RATE vector, D (B,4,6) = the rates"""
    ien = np.asarray(ien, I64).reshape(-1, 4)

    def gather(vec):
        return np.stack([vec[3 * ien], vec[3 * ien + 1], vec[3 * ien + 2], dwg[3 * N + ien], vec[4 * N + ien],
                         vec[5 * N + ien]], axis=2)
    return gather(np.asarray(wg, F64)), gather(np.asarray(dwg, F64))


def tet_residual(X, W, D, dt=LD):
    """eF (B,4,6): rows of node a, summed over the four quadrature points"""
    g = geometry(X, dt)
    W, D = AV(_in(W, dt)), AV(_in(D, dt))
    shg, wq = g.shg, g.detJ * GW
    grad = [[None] * 3 for _ in range(6)]
    for comp in range(6):
        for d in range(3):
            s = shg[:, 0, d] * W[:, 0, comp]
            for b in range(1, 4):
                s = s + shg[:, b, d] * W[:, b, comp]
            grad[comp][d] = s
    divu = grad[0][0] + grad[1][1] + grad[2][2]
    mu, kap = MU / RHO, KAPPA / (RHO * CP)
    t0 = 4.0 / (DT * DT)
    out = [[None] * 6 for _ in range(4)]
    for q in range(4):
        def at(V, comp):
            s = V[:, 0, comp] * SHL[0, q]
            for b in range(1, 4):
                s = s + V[:, b, comp] * SHL[b, q]
            return s
        qw, qd = [at(W, c) for c in range(6)], [at(D, c) for c in range(6)]
        u = qw[:3]
        rL = [qd[i] * RHO + u[0] * RHO * grad[i][0] + u[1] * RHO * grad[i][1] + u[2] * RHO * grad[i][2] + grad[3][i]
              for i in range(3)]
        t1 = None
        for r in range(3):   # u . G . u = |J^-T u|^2: column r of J^-1 against u
            v = g.inv[:, 0, r] * u[0] + g.inv[:, 1, r] * u[1] + g.inv[:, 2, r] * u[2]
            t1 = v * v if t1 is None else t1 + v * v
        y = t1 + g.gg * (3.0 * mu * mu)
        tauM = ((y + t0).rsqrt() * (1.0 / RHO)).tau()
        tauC = (y.sqrt() * g.itr).tau()
        tauP = (t1 + t0).rsqrt().tau()
        tauT = ((t1 + t0 + g.gg * (3.0 * kap * kap)).rsqrt() * (1.0 / (RHO * CP))).tau()
        conv = [u[0] * shg[:, b, 0] + u[1] * shg[:, b, 1] + u[2] * shg[:, b, 2] for b in range(4)]
        tmp0 = [qd[i] * RHO + (u[0] - tauM * rL[0]) * RHO * grad[i][0] + (u[1] - tauM * rL[1]) * RHO * grad[i][1]
                + (u[2] - tauM * rL[2]) * RHO * grad[i][2] for i in range(3)]
        tmp1 = [[(grad[i][k] + grad[k][i]) * MU + tauM * RHO * rL[i] * u[k] - tauM * tauM * RHO * rL[i] * rL[k]
                 for k in range(3)] for i in range(3)]
        for i in range(3):
            tmp1[i][i] = tmp1[i][i] - qw[3] + tauC * RHO * divu
        bp = qd[4] + u[0] * grad[4][0] + u[1] * grad[4][1] + u[2] * grad[4][2]
        btc = (qd[5] + u[0] * grad[5][0] + u[1] * grad[5][1] + u[2] * grad[5][2]) * (RHO * CP)
        for a in range(4):
            sh = SHL[a, q]
            rows = [(tmp0[i] * sh + shg[:, a, 0] * tmp1[i][0] + shg[:, a, 1] * tmp1[i][1] + shg[:, a, 2] * tmp1[i][2]) * wq
                    for i in range(3)]
            rows.append((divu * sh + tauM * rL[0] * shg[:, a, 0] + tauM * rL[1] * shg[:, a, 1]
                         + tauM * rL[2] * shg[:, a, 2]) * wq)
            rows.append(bp * (tauP * conv[a] + sh) * wq)
            rows.append((btc * (tauT * (RHO * CP) * conv[a] + sh)
                         + (grad[5][0] * shg[:, a, 0] + grad[5][1] * shg[:, a, 1] + grad[5][2] * shg[:, a, 2]) * KAPPA) * wq)
            for k in range(6):
                out[a][k] = rows[k] if out[a][k] is None else out[a][k] + rows[k]
    return AV.stack([AV.stack(out[a]) for a in range(4)], axis=1)


# ======================================================================================================================
# element Jacobian: the sixteen 4x4 (u,p) blocks of one tet, eJ (B,4,4,16), block entry i * 4 + j
# ======================================================================================================================
def tet_jacobian(X, Uv, dt=LD):
    """Uv (B,4,3): nodal velocities; X (B,4,3) vertex coordinates, or the Geo of a cached geometry record"""
    g = X if isinstance(X, Geo) else geometry(X, dt)
    Uv = AV(_in(Uv, dt))
    shg = g.shg
    knu = MU / RHO
    A = lambda x: x[:, :, None]   # noqa: E731  (node a along axis 1)
    Bx = lambda x: x[:, None, :]  # noqa: E731  (node b along axis 2)
    ga, gb = [A(shg[:, :, d]) for d in range(3)], [Bx(shg[:, :, d]) for d in range(3)]
    eK = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]
    blk = [None] * 16

    def add(k, term):
        blk[k] = term if blk[k] is None else blk[k] + term
    for q in range(4):
        uq = [Uv[:, 0, d] * SHL[0, q] + Uv[:, 1, d] * SHL[1, q] + Uv[:, 2, d] * SHL[2, q] + Uv[:, 3, d] * SHL[3, q]
              for d in range(3)]
        conv = shg[:, :, 0] * uq[0][:, None] + shg[:, :, 1] * uq[1][:, None] + shg[:, :, 2] * uq[2][:, None]   # (B,4)
        tmp = conv[:, 1] * conv[:, 1] + conv[:, 2] * conv[:, 2] + conv[:, 3] * conv[:, 3]
        y = tmp + g.gg * (3.0 * knu * knu)
        tau0 = ((y + 4.0 / (DT * DT)).rsqrt() * (1.0 / RHO)).tau()[:, None, None]
        tau1 = (y.sqrt() * g.itr).tau()[:, None, None]
        w = (g.detJ * GW)[:, None, None]
        sa, sb = SHL[:, q][None, :, None], SHL[:, q][None, None, :]
        ca, cb = A(conv), Bx(conv)
        one = AV(np.ones((1, 1, 1), dt))
        t = (one * (FACT1 * RHO) * sa * sb + tau0 * (FACT1 * RHO * RHO) * ca * sb + cb * (FACT2 * RHO) * sa
             + tau0 * (FACT2 * RHO * RHO) * ca * cb + eK * (FACT2 * MU)) * w
        for i in range(3):
            add(i * 4 + i, t)
            for k in range(3):
                add(i * 4 + k, ga[k] * gb[i] * (FACT2 * MU) * w + tau1 * (FACT2 * RHO) * ga[i] * gb[k] * w)
            add(i * 4 + 3, -(ga[i] * sb * w) + tau0 * RHO * ca * gb[i] * w)                              # dRM/dP
            add(12 + i, tau0 * (FACT1 * RHO) * ga[i] * sb * w + gb[i] * FACT2 * sa * w
                + tau0 * (FACT2 * RHO) * ga[i] * cb * w)                                                 # dRC/dU
        add(15, tau0 * eK * w)                                                                           # dRC/dP
    return AV.stack(blk)


# ======================================================================================================================
# weak-BC face terms: eF (B,4,4) (u0 u1 u2 p rows of node a), eJ (B,4,4,16)
# ======================================================================================================================
def face_terms(X, W4, iorn, dt=LD):
    """X (B,4,3) the parent tets, W4 (B,4,4) = u0 u1 u2 p (p from the rate vector), iorn (B,) the face orientations"""
    g = geometry(X, dt)
    W4 = AV(_in(W4, dt))
    iorn = np.asarray(iorn, I64)
    shg = g.shg
    sbq = SHLUB[iorn].astype(dt)                                   # (B,3,4)  [q, a]
    n2 = NV2[iorn].astype(dt)                                      # (B,3)
    nv = [(g.inv[:, 0, n] * n2[:, 0] + g.inv[:, 1, n] * n2[:, 1] + g.inv[:, 2, n] * n2[:, 2]) * g.detJ for n in range(3)]
    grad = [[shg[:, 0, d] * W4[:, 0, c] + shg[:, 1, d] * W4[:, 1, c] + shg[:, 2, d] * W4[:, 2, c] + shg[:, 3, d] * W4[:, 3, c]
             for d in range(3)] for c in range(4)]
    hin = None
    for k in range(3):
        w = g.inv[:, k, 0] * nv[0] + g.inv[:, k, 1] * nv[1] + g.inv[:, k, 2] * nv[2]
        hin = w * w if hin is None else hin + w * w
    tau_b = hin.sqrt() * (4.0 * MU)
    shnorm = [shg[:, a, 0] * nv[0] + shg[:, a, 1] * nv[1] + shg[:, a, 2] * nv[2] for a in range(4)]
    eF = [[None] * 4 for _ in range(4)]
    eJ = [[[None] * 16 for _ in range(4)] for _ in range(4)]

    def acc(lst, k, term):
        lst[k] = term if lst[k] is None else lst[k] + term
    for q in range(3):
        s = [AV(sbq[:, q, a]) for a in range(4)]
        qb = [W4[:, 0, c] * s[0] + W4[:, 1, c] * s[1] + W4[:, 2, c] * s[2] + W4[:, 3, c] * s[3] for c in range(4)]
        u = qb[:3]
        unor = u[0] * nv[0] + u[1] * nv[1] + u[2] * nv[2]
        uneg = (unor - unor.fabs()) * 0.5
        tmp0 = [nv[k] * qb[3] - (nv[0] * grad[k][0] + nv[1] * grad[k][1] + nv[2] * grad[k][2]) * MU
                - (nv[0] * grad[0][k] + nv[1] * grad[1][k] + nv[2] * grad[2][k]) * MU - uneg * RHO * u[k] + tau_b * u[k]
                for k in range(3)]
        tmp1 = [[-((nv[k] * u[m] + nv[m] * u[k]) * MU) for m in range(3)] for k in range(3)]
        for a in range(4):
            for i in range(3):
                acc(eF[a], i, (s[a] * tmp0[i] + shg[:, a, 0] * tmp1[i][0] + shg[:, a, 1] * tmp1[i][1]
                               + shg[:, a, 2] * tmp1[i][2]) * GWB)
            acc(eF[a], 3, -(s[a] * unor * GWB))
            for b in range(4):
                d = (-((shnorm[b] * s[a] + shnorm[a] * s[b]) * MU) - s[a] * s[b] * RHO * uneg + tau_b * s[a] * s[b]) \
                    * (FACT2 * GWB)
                ss = s[a] * s[b]
                for i in range(3):
                    acc(eJ[a][b], i * 4 + i, d)
                    for m in range(3):
                        acc(eJ[a][b], i * 4 + m, (-(s[a] * MU * shg[:, b, i] * nv[m]) - s[b] * MU * shg[:, a, m] * nv[i])
                            * (FACT2 * GWB))
                    acc(eJ[a][b], 12 + i, -(ss * FACT2 * nv[i] * GWB))
                    acc(eJ[a][b], i * 4 + 3, ss * nv[i] * GWB)
    B = X.shape[0]
    z = AV.zeros(B, dt)
    F = AV.stack([AV.stack(eF[a]) for a in range(4)], axis=1)
    J = AV.stack([AV.stack([AV.stack([e if e is not None else z for e in eJ[a][b]]) for b in range(4)], axis=1)
                  for a in range(4)], axis=1)
    return F, J


# ======================================================================================================================
# records and the data-movement kernels (any dtype: int64 for the bitwise tier)
# ======================================================================================================================
def pack_nodes(N, xg, wg, dwg, dtype=F64):
    """(nodep (N,16), nodexu (N,8)): x[3] u[3] phi T du[3] p dphi dT pad pad, and x[3] u[3] pad pad.  dwg None: rate slots 0."""
    xg, wg = np.asarray(xg).astype(dtype), np.asarray(wg).astype(dtype)
    nodep, nodexu = np.zeros((N, NREC), dtype), np.zeros((N, XUREC), dtype)
    nodep[:, 0:3] = nodexu[:, 0:3] = xg.reshape(N, 3)
    nodep[:, 3:6] = nodexu[:, 3:6] = wg[:3 * N].reshape(N, 3)
    nodep[:, 6], nodep[:, 7] = wg[4 * N:5 * N], wg[5 * N:6 * N]
    if dwg is not None:
        dwg = np.asarray(dwg).astype(dtype)
        nodep[:, 8:11] = dwg[:3 * N].reshape(N, 3)
        nodep[:, 11], nodep[:, 12], nodep[:, 13] = dwg[3 * N:4 * N], dwg[4 * N:5 * N], dwg[5 * N:6 * N]
    return nodep, nodexu


def frec_index(N):
    """F index of the six live slots of every packed residual record: (N,6)"""
    n = np.arange(N, dtype=I64)
    return np.stack([3 * n, 3 * n + 1, 3 * n + 2, 3 * N + n, 4 * N + n, 5 * N + n], axis=1)


def unpack_rhs(N, Fp, F):
    """F + the packed records (reference layout)"""
    out = np.array(F, copy=True)
    out[frec_index(N).ravel()] += np.asarray(Fp).reshape(N, FREC)[:, :6].ravel()
    return out


def rhs_node_sum(N, goff, gidx, partial, F):
    out = np.array(F, copy=True)
    part = np.asarray(partial).reshape(-1, 6)
    idx = frec_index(N)
    for n in range(N):
        for g in gidx[goff[n]:goff[n + 1]]:
            out[idx[n]] += part[g]
    return out


def face_sum(keys, off, ent, parked, width, target, index_of):
    """target[index_of(key, lane)] += sum of parked[ent * width + lane] in list order"""
    out = np.array(target, copy=True)
    parked = np.asarray(parked).reshape(-1, width)
    for k, key in enumerate(keys):
        s = np.zeros(width, out.dtype)
        for e in ent[off[k]:off[k + 1]]:
            s = s + parked[e]
        for lane in range(width):
            out[index_of(int(key), lane)] += s[lane]
    return out


def gather_ien(ien, batch_ind):
    return np.asarray(ien).reshape(-1, 4)[np.asarray(batch_ind, I64)].reshape(-1)


def find_nz(rp, ci, row, col):
    """position of `col` in the sorted row `row` (plain linear search)"""
    for k in range(rp[row], rp[row + 1]):
        if ci[k] == col:
            return k
    raise KeyError((row, col))


def elem_nzmap(ien_b, rp, ci):
    ien_b = np.asarray(ien_b).reshape(-1, 4)
    return np.array([find_nz(rp, ci, e[a], e[b]) for e in ien_b for a in range(4) for b in range(4)], I32)


def nodal_pattern(ien, N):
    """sorted nodal CSR pattern of a tet mesh"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    pairs = np.unique((ien[:, :, None] * N + ien[:, None, :]).ravel())
    rows, cols = pairs // N, pairs % N
    rp = np.zeros(N + 1, I32)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(I32), cols.astype(I32)


def nzmap_fast(ien, rp, ci):
    """(T,4,4) nonzero of every (tet, a, b); the pattern must hold every pair"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    N = rp.size - 1
    key = np.repeat(np.arange(N, dtype=I64), np.diff(rp)) * N + ci
    pos = np.searchsorted(key, ien[:, :, None] * N + ien[:, None, :])
    assert np.array_equal(key[pos], ien[:, :, None] * N + ien[:, None, :])
    return pos


# ======================================================================================================================
# mesh-level sums
# ======================================================================================================================
def mesh_vertices(xg, ien):
    return np.asarray(xg, F64).reshape(-1, 3)[np.asarray(ien, I64).reshape(-1, 4)]


def assemble_tet(xg, ien, N, wg, dwg, rp=None, ci=None, dt=LD, want_F=True):
    """(F (6N) in the reference layout, blocks (nnz,16)) of AssembleSystemTet; blocks None without a pattern"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    X = mesh_vertices(xg, ien)
    W, D = element_fields(ien, N, wg, dwg)
    F = blocks = None
    if want_F:
        F = tet_residual(X, W, D, dt).scatter_add(6 * N, frec_index(N)[ien])
    if rp is not None:
        eJ = tet_jacobian(X, W[:, :, :3], dt)
        nz = nzmap_fast(ien, rp, ci)
        blocks = eJ.scatter_add(ci.size * 16, nz[:, :, :, None] * 16 + np.arange(16)).reshape(ci.size, 16)
    return F, blocks


def face_fields(ien_f, N, wg, dwg):
    ien_f = np.asarray(ien_f, I64).reshape(-1, 4)
    wg, dwg = np.asarray(wg, F64), np.asarray(dwg, F64)
    return np.stack([wg[3 * ien_f], wg[3 * ien_f + 1], wg[3 * ien_f + 2], dwg[3 * N + ien_f]], axis=2)


def assemble_face(xg, ien, N, f2e, forn, wg, dwg, rp=None, ci=None, dt=LD):
    """(F (6N), blocks (nnz,16)) of the weak-BC faces f2e / forn"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    ien_f = ien[np.asarray(f2e, I64)]
    eF, eJ = face_terms(mesh_vertices(xg, ien_f), face_fields(ien_f, N, wg, dwg), forn, dt)
    F = eF.scatter_add(6 * N, frec_index(N)[ien_f][:, :, :4])
    blocks = None
    if rp is not None:
        nz = nzmap_fast(ien_f, rp, ci)
        blocks = eJ.scatter_add(ci.size * 16, nz[:, :, :, None] * 16 + np.arange(16)).reshape(ci.size, 16)
    return F, blocks


def blocks_from_reference(rp, vals):
    """(nnz,16) 4x4 blocks (entry i * 4 + j) from the four reference-layout value arrays A00 A01 A10 A11"""
    rp = np.asarray(rp, I64)
    nnz = int(rp[-1])
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    start, ln = rp[row], np.diff(rp)[row]
    k = np.arange(nnz) - start
    out = np.zeros((nnz, 16), np.asarray(vals[0]).dtype)
    for (m, br, bc, i0, j0) in ((vals[0], 3, 3, 0, 0), (vals[1], 3, 1, 0, 3), (vals[2], 1, 3, 3, 0), (vals[3], 1, 1, 3, 3)):
        for ii in range(br):
            for jj in range(bc):
                out[:, (i0 + ii) * 4 + j0 + jj] = np.asarray(m)[start * br * bc + k * bc + ii * ln * bc + jj]
    return out


def continuity_identity(xg, ien, wg):
    """sum over tets of |det J| / 6 * div u_h from the mesh and u alone, with its abs-sum: AV scalars"""
    ien = np.asarray(ien, I64).reshape(-1, 4)
    g = geometry(mesh_vertices(xg, ien), LD)
    u = AV(np.asarray(wg, F64)[:3 * (np.asarray(xg).size // 3)].reshape(-1, 3)[ien].astype(LD))   # (T,4,3)
    div = None
    for b in range(4):
        for d in range(3):
            term = g.shg[:, b, d] * u[:, b, d]
            div = term if div is None else div + term
    return (div * g.detJ * (LD(1) / LD(6))).sum(0)


# ======================================================================================================================
# inputs: tet soup, geometry families, field regimes
# ======================================================================================================================
FAMILIES = ("unit", "scale1e-5", "scale1e3", "stretched", "translated", "negative")
KAPPA_FAMILIES = ("stretched",)      # the bound carries kappa_inf(J); c is the unit family's
REGIMES = ("synthetic", "u0", "convective", "dwg0")


def apply_family(x, family):
    """x (n,3) unit-scale coordinates -> the family's"""
    x = np.array(x, F64)
    if family == "scale1e-5":
        return x * 1e-5
    if family == "scale1e3":
        return x * 1e3
    if family == "stretched":
        return x * np.array([1.0, 1.0, 1e-3])
    if family == "translated":
        return x * 1e-2 + 1e3
    return x


def tet_soup(B, family="unit", seed=3):
    """B disjoint tets on 4B distinct nodes in shuffled node order: (xg (12B,), ien (4B,) int32).  The first B tets of a
    larger soup with the same seed have the same shapes.  `negative`: vertices 1 and 2 swapped, det J < 0."""
    rng = np.random.default_rng(seed)
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F64)
    k = np.arange(B)
    X = corners[None] + rng.uniform(-0.2, 0.2, (B, 4, 3)) + 1.5 * np.stack([k % 5, (k // 5) % 5, k // 25], 1)[:, None, :]
    if family == "negative":
        X[:, [1, 2]] = X[:, [2, 1]]
    perm = np.random.default_rng(seed + 1000 + B).permutation(4 * B)
    xg = np.empty((4 * B, 3))
    xg[perm] = apply_family(X.reshape(-1, 3), family)
    return np.ascontiguousarray(xg.reshape(-1)), np.ascontiguousarray(perm.astype(I32))


def fields(xg, regime, seed=7):
    """(wg, dwg) of length 6N in the layout [u: N x 3 | p | phi | T]"""
    from dedflow_amd.meshgen import synthetic_fields
    N = np.asarray(xg).size // 3
    wg, dwg = synthetic_fields(types.SimpleNamespace(xg=np.asarray(xg, F64), num_node=N), seed)
    rng = np.random.default_rng(seed + 1)
    if regime == "u0":
        wg[:3 * N] = 0.0
        dwg = rng.normal(size=6 * N)
    elif regime == "convective":
        d = rng.normal(size=(N, 3))
        wg[:3 * N] = (1e3 * d / np.linalg.norm(d, axis=1)[:, None]).reshape(-1)
    elif regime == "dwg0":
        dwg = np.zeros(6 * N)
    return wg, dwg


def scaled_mesh(mesh, family):
    import copy
    m = copy.copy(mesh)
    m.xg = np.ascontiguousarray(apply_family(mesh.xg.reshape(-1, 3), family).reshape(-1))
    return m


# ======================================================================================================================
# bounds
# ======================================================================================================================
def ratio_c(err, ab, K=1.0):
    """the constant c that `err` shows against u K a: max err / (u K a) over the entries with a > 0"""
    err, ab = np.asarray(err, LD), np.asarray(ab, LD) * np.asarray(K, LD)
    nz = ab > 0
    return float((err[nz] / (U * ab[nz])).max()) if np.any(nz) else 0.0


def bound(model, c, K=1.0, newton=False):
    """8 c u K a (+ 2.2e-14 t): float64 array shaped as the model"""
    b = 8.0 * c * U * np.asarray(K, LD) * model.a
    if newton:
        b = b + NEWTON * model.t
    return np.asarray(b, F64)


def restatement_error(model, rest):
    return np.abs(rest.v.astype(LD) - model.v)
