"""numpy model of every launcher of csrc/k_laser.hip and csrc/k_laser_surface.hip, one function per launcher, written from
include/dedflow_kernels.h and the kernel sources.  It imports laser_model, laser_surface_model and redistance_model and
changes none of them.  Test infrastructure only; shared by test_laser_kernel_model_cpu.py and test_gpu_laser_kernels.py.

  * Integer outputs (the bin of a particle, the hit key, the face of a column, the snapshot's lists) are int64 / uint64 from a
    float64 restatement in the source's operation order.  numpy has no fused multiply-add and both .hip files and
    laser_geom.hpp switch contraction off, so a correct kernel agrees to the last bit.
  * Sums whose order the source fixes completely (the deposit's face-then-column loop, the tally's strided sums and halving
    tree, the surface deposit's per-slot sum in ascending 4 c + a, the one-multiply-one-add list kernels) are float64
    restatements in that order: bit for bit again.
  * Everything that goes through exp / expm1 (rate, col_T and the rows of part that derive from them) is np.longdouble,
    sequential in (s, id) order, with laser_model.step's arithmetic and its a-priori bounds.

The cases of the GPU tests are built here too, so that the CPU tests can assert what each case is named for."""
import ctypes as C
import math

import numpy as np

import laser_model as lm
import laser_surface_model as lsm
import redistance_model as rm  # noqa: F401  (the facets of laser_surface_model.Candidates are redistance_model's)

F64, LD, I64, U64 = np.float64, np.longdouble, np.int64, np.uint64
EPS = lm.EPS
ULP_EXP = lm.ULP_EXP
CAP, WAVE, BLK = 512, 64, 256
FACE_BITS, DEPTH_BITS = 24, 40
FACE_MASK = (1 << FACE_BITS) - 1
NO_HIT = (1 << 64) - 1
Q_TOP = float(2 ** DEPTH_BITS - 1)
REC_BITS = 20
OUTSIDE_SHIFT = 3
PI = math.pi


class CBeam(C.Structure):
    _fields_ = [("o", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3), ("dir", C.c_double * 3), ("h", C.c_double),
                ("area", C.c_double), ("n", C.c_int32)]


class CWallTri(C.Structure):
    _fields_ = [("v", C.c_double * 9), ("n", C.c_double * 3), ("off", C.c_double), ("pad", C.c_double), ("node", C.c_int32 * 3),
                ("id", C.c_int32)]


def c_beam(b):
    return CBeam((C.c_double * 3)(*b.o), (C.c_double * 3)(*b.e1), (C.c_double * 3)(*b.e2), (C.c_double * 3)(*b.dir), b.h, b.area, b.n)


# ---- the beam frame -----------------------------------------------------------------------------------------------------------
class Frame:
    """dfl_laser_beam: o, (e1, e2, dir) as laser_model.Beam builds them, h, area = h h, n (even)"""

    def __init__(self, direction, origin, h, n, power=400.0, w=0.2):
        assert n % 2 == 0
        self.beam = lm.Beam(origin, direction, power, w, h, (n / 2 - 0.5) * h)
        assert self.beam.n == n
        b = self.beam
        self.o, self.e1, self.e2, self.dir = b.origin.copy(), b.e1, b.e2, b.dir
        self.h, self.area, self.n, self.ncol = float(h), float(h) * float(h), n, n * n

    def world(self, uvs):
        """o + u e1 + v e2 + s dir in float64 (exact in the vertical frame on dyadic data)"""
        uvs = np.asarray(uvs, F64)
        return self.o + uvs[..., 0:1] * self.e1 + uvs[..., 1:2] * self.e2 + uvs[..., 2:3] * self.dir


def project(v, b):
    """u, v, s of points [..., 3]"""
    d = np.asarray(v, F64) - b.o
    with np.errstate(invalid="ignore", over="ignore"):
        return lm.dot3(b.e1, d), lm.dot3(b.e2, d), lm.dot3(b.dir, d)


def column_centre(i, b):
    return ((np.asarray(i) - b.n // 2).astype(F64) + 0.5) * b.h


def column_range(u, v, b):
    """(i0, i1, j0, j1) of one projected face: fmin / fmax skip a NaN, as C's do"""
    half, top = float(b.n // 2), float(b.n - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        ulo, uhi = np.fmin(u[0], np.fmin(u[1], u[2])), np.fmax(u[0], np.fmax(u[1], u[2]))
        vlo, vhi = np.fmin(v[0], np.fmin(v[1], v[2])), np.fmax(v[0], np.fmax(v[1], v[2]))
        i0 = int(np.fmin(np.fmax(np.floor(ulo / b.h - 0.5) + half, 0.0), top + 1.0))
        i1 = int(np.fmax(np.fmin(np.ceil(uhi / b.h - 0.5) + half, top), -1.0))
        j0 = int(np.fmin(np.fmax(np.floor(vlo / b.h - 0.5) + half, 0.0), top + 1.0))
        j1 = int(np.fmax(np.fmin(np.ceil(vhi / b.h - 0.5) + half, top), -1.0))
    return i0, i1, j0, j1


def edge_functions(u, v, cu, cv):
    a0, a1, a2 = u[0] - cu, u[1] - cu, u[2] - cu
    b0, b1, b2 = v[0] - cv, v[1] - cv, v[2] - cv
    return a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0


def tri_hit(u, v, s, cu, cv):
    """the centre rays (cu, cv) (arrays) against one projected face: hit [m], w [m, 3], depth [m]"""
    cu, cv = np.asarray(cu, F64), np.asarray(cv, F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w0, w1, w2 = edge_functions(u, v, cu, cv)
        tot = (w0 + w1) + w2
        hit = (tot != 0.0) & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))   # a NaN fails the signs
        w = np.stack([w0 / tot, w1 / tot, w2 / tot], axis=-1)
        d = (w[..., 0] * s[0] + w[..., 1] * s[1]) + w[..., 2] * s[2]
    return hit, w, d


def face_columns(tv, b):
    """the columns (ascending id: j outer, i inner) under one face's bounding box, and tri_hit there"""
    u, v, s = project(tv.reshape(3, 3), b)
    i0, i1, j0, j1 = column_range(u, v, b)
    if i1 < i0 or j1 < j0:
        z = np.zeros(0, I64)
        return z, np.zeros(0, bool), np.zeros((0, 3)), np.zeros(0)
    jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    hit, w, d = tri_hit(u, v, s, column_centre(ii, b), column_centre(jj, b))
    return ii + b.n * jj, hit, w, d


def depth_field(d, s_lo, scale):
    """floor of (depth - s_lo) scale clamped to [0, 2^40 - 1]; a NaN gives 0 (fmax)"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.fmin(np.fmax((np.asarray(d, F64) - s_lo) * scale, 0.0), Q_TOP)
    return q.astype(U64)


# ---- k_laser.hip --------------------------------------------------------------------------------------------------------------
def laser_bin(coord, b):
    """cell_of [P], count [n n + ((P - 1) >> 3) + 1], outside [P] (rate is written 0 there and nowhere else)"""
    x = np.asarray(coord, F64).reshape(-1, 3)
    P = len(x)
    u, v, _ = project(x, b)
    with np.errstate(invalid="ignore", over="ignore"):
        qu, qv = np.floor(u / b.h), np.floor(v / b.h)
        half = float(b.n // 2)
        inside = (qu >= -half) & (qu < half) & (qv >= -half) & (qv < half)
    c = b.ncol + (np.arange(P) >> OUTSIDE_SHIFT)
    qi, qj = np.where(inside, qu, 0.0).astype(I64), np.where(inside, qv, 0.0).astype(I64)
    cell = np.where(inside, (qi + b.n // 2) + b.n * (qj + b.n // 2), c)
    nbins = b.ncol + ((P - 1) >> OUTSIDE_SHIFT) + 1
    return cell, np.bincount(cell, minlength=nbins), ~inside


def laser_hit(tri_v, b, s_lo, scale):
    """colkey [n n] uint64: all ones, then the minimum over the faces of depth field << 24 | face"""
    tri_v = np.asarray(tri_v, F64).reshape(-1, 9)
    key = np.full(b.ncol, NO_HIT, U64)
    for f in range(len(tri_v)):
        col, hit, _, d = face_columns(tri_v[f], b)
        if hit.any():
            k = (depth_field(d[hit], s_lo, scale) << U64(FACE_BITS)) | U64(f)
            key[col[hit]] = np.minimum(key[col[hit]], k)
    return key


def key_face(key):
    """face index of every key (-1: no hit) and its depth field"""
    key = np.asarray(key, U64)
    return np.where(key == U64(NO_HIT), -1, (key & U64(FACE_MASK)).astype(I64)), key >> U64(FACE_BITS)


def tau64(r, b):
    """the optical depth A / a of one particle as the kernel writes it: (pi (r r)) (1 / area)"""
    r = np.asarray(r, F64)
    return (PI * (r * r)) * (1.0 / b.area)


def laser_columns(P, b, power, eta_p, eta_s, gw, cell_start, order, sorted6, sorted_r, radius, tri_v, tri_id, colkey):
    """dfl_laser_columns.  Exact (float64): pc = part[0], col_face, s_hit, k_tau / k_id of the runs longer than the cap (by
    position; k_id = -1 elsewhere), lit, written (the ids of the runs: rate of every other id is not touched).  np.longdouble with a-priori bounds: rate / rate_bound by id (rate_exact0: the
    entries that must be +0.0), T / T_rel, and part[1..6) with part_bound.

    The bounds.  rate_bound and T_rel are laser_model.step's, with its argument: (k + 12) eps S on the optical depth in front
    of entry k of its run (4 roundings per term, the scan's tree and the carries), the ulp allowance of exp and expm1, and
    the roundings of the products.  Of a row of part:
      absorbed   the sum of rate[id]: every entry's own bound, plus the summation -- lane l adds its entries of the chunks
                 0, 1, ... sequentially (ceil(len / 64) additions at most), wave_sum adds 6 levels: (ceil(len / 64) + 6) eps
                 sum |term|
      scattered  got - eta_p got per entry: relative bound r_k of got on both operands and one rounding of the difference,
                 (got + mine) r_k + eps |got - mine|; the same summation term.  eta_p = 1: mine == got, the row is exactly 0
      substrate  eta_s T_c: T_rel + 1 rounding;  reflected (1 - eta_s) T_c: T_rel + 2;  missed T_c: T_rel"""
    n, ncol = b.n, b.ncol
    gw = np.asarray(gw, F64)
    ci, cj = np.arange(ncol) % n, np.arange(ncol) // n
    pc = ((power / 4.0) * gw[ci]) * gw[n + cj]
    face_idx, _ = key_face(colkey)
    has = (face_idx >= 0) & (tri_v is not None)
    s_hit, col_face = np.zeros(ncol), np.full(ncol, -1, I64)
    for c in np.nonzero(has)[0]:
        u, v, s = project(np.asarray(tri_v, F64).reshape(-1, 3, 3)[face_idx[c]], b)
        _, _, d = tri_hit(u, v, s, column_centre(ci[c:c + 1], b), column_centre(cj[c:c + 1], b))
        s_hit[c], col_face[c] = d[0], tri_id[face_idx[c]]
    rate, bound, exact0 = np.zeros(max(P, 1), LD), np.zeros(max(P, 1)), np.zeros(max(P, 1), bool)
    T, T_rel = pc.astype(LD).copy(), np.full(ncol, 4 * EPS)
    part, pb = np.zeros((6, ncol), LD), np.zeros((6, ncol))
    part[0] = pc
    k_tau, k_id, lit = np.full(max(P, 1), np.nan), np.full(max(P, 1), -1, I64), np.ones(max(P, 1), bool)
    written = np.zeros(max(P, 1), bool)
    S_max = 0.0
    if P > 0:
        x = np.asarray(sorted6, F64).reshape(-1, 6)[:, :3]
        s_all = project(x, b)[2]
        r_all = np.asarray(sorted_r, F64) if sorted_r is not None else np.full(len(x), float(radius))
        t_all = tau64(r_all, b)
        order = np.asarray(order, I64)
    for c in range(ncol if P > 0 else 0):
        lo, hi = int(cell_start[c]), int(cell_start[c + 1])
        ln = hi - lo
        if ln == 0:
            continue
        s, ids = s_all[lo:hi], order[lo:hi]
        run = np.lexsort((ids, s))                                   # ascending (s, id)
        dark = has[c] & (s > s_hit[c])
        lit[lo:hi] = ~dark
        if ln > CAP:
            k_tau[lo:hi], k_id[lo:hi] = np.where(dark, 0.0, t_all[lo:hi])[run], ids[run]
        S, sa, ss = LD(0), LD(0), LD(0)
        ab, sb, aa, sabs = 0.0, 0.0, 0.0, 0.0
        for k, q in enumerate(run):
            i = ids[q]
            tau = LD(0) if dark[q] else (LD(np.pi) * (LD(r_all[lo + q]) * LD(r_all[lo + q]))) / LD(b.area)
            got = LD(pc[c]) * np.exp(-S) * (-np.expm1(-tau))
            mine = LD(eta_p) * got
            rel = (k + 12) * EPS * float(S) + (2 * ULP_EXP + 12) * EPS
            rate[i], bound[i], exact0[i], written[i] = mine, float(mine) * rel, dark[q], True
            sa += mine
            ss += got - mine
            ab += float(mine) * rel
            sb += float(got + mine) * rel + EPS * float(abs(got - mine))
            aa += float(abs(mine))
            sabs += float(abs(got - mine))
            S += tau
        T[c] = LD(pc[c]) * np.exp(-S)
        T_rel[c] = (ln + 12) * EPS * float(S) + (ULP_EXP + 4) * EPS
        S_max = max(S_max, float(S))
        tree = (math.ceil(ln / WAVE) + 6) * EPS
        part[1, c], pb[1, c] = sa, ab + tree * aa
        part[2, c], pb[2, c] = ss, (0.0 if eta_p == 1.0 else sb + tree * sabs)
    part[3] = np.where(has, LD(eta_s) * T, LD(0))
    part[4] = np.where(has, (LD(1) - LD(eta_s)) * T, LD(0))
    part[5] = np.where(has, LD(0), T)
    Tf = T.astype(F64)
    pb[3], pb[4], pb[5] = np.abs(part[3].astype(F64)) * (T_rel + EPS), np.abs(part[4].astype(F64)) * (T_rel + 2 * EPS), np.where(has, 0.0, Tf * T_rel)
    return dict(pc=pc, col_face=col_face, s_hit=s_hit, has=has, rate=rate[:P], rate_bound=bound[:P], rate_exact0=exact0[:P],
                T=T, T_rel=T_rel, part=part, part_bound=pb, k_tau=k_tau[:P], k_id=k_id[:P], lit=lit[:P], written=written[:P], S_max=S_max)


def seq_sum(terms, start=0.0):
    """start + t0 + t1 + ... strictly left to right in float64 (np.cumsum is sequential)"""
    terms = np.asarray(terms, F64)
    return float(np.cumsum(np.concatenate([[start], terms]))[-1]) if terms.size else float(start)


def laser_deposit(ns, soff, sface, tri_v, b, eta_s, dt, colkey, col_T, energy):
    """power [ns] and energy [ns] after the call: the face-then-column loop, acc += (eta_s col_T) w[kv]"""
    tri_v = np.asarray(tri_v, F64).reshape(-1, 9)
    face_idx, _ = key_face(colkey)
    col_T = np.asarray(col_T, F64)
    cache = {}
    power = np.zeros(ns)
    for a in range(ns):
        acc = 0.0
        for e in range(int(soff[a]), int(soff[a + 1])):
            f, kv = int(sface[e]) >> 2, int(sface[e]) & 3
            if f not in cache:
                col, hit, w, _ = face_columns(tri_v[f], b)
                won = hit & (face_idx[col] == f)
                cache[f] = (col[won], w[won])
            col, w = cache[f]
            acc = seq_sum((eta_s * col_T[col]) * w[:, kv], acc)
        power[a] = acc
    return power, np.asarray(energy, F64) + dt * power


def laser_tally(ncol, power, part):
    """thread t sums columns t, t + 256, ... from +0.0; then the halving tree over 256 threads"""
    part = np.asarray(part, F64).reshape(6, ncol)
    acc = np.zeros((6, BLK))
    for lo in range(0, ncol, BLK):
        m = min(BLK, ncol - lo)
        acc[:, :m] = acc[:, :m] + part[:, lo:lo + m]
    off = BLK // 2
    while off > 0:
        acc[:, :off] = acc[:, :off] + acc[:, off:2 * off]
        off >>= 1
    out = acc[:, 0].copy()
    out[0] = power - out[0]
    return out


def list_source_add(n, index, inv_time, energy, q):
    """q[index[a]] += energy[a] inv_time; energy[a] = 0 for a < n (the indices are distinct)"""
    energy, q = np.array(energy, F64), np.array(q, F64)
    idx = np.asarray(index, I64)[:n]
    q[idx] = q[idx] + energy[:n] * inv_time
    energy[:n] = 0.0
    return energy, q


def surface_power(N, n, unode, power):
    q = np.zeros(N)
    q[np.asarray(unode, I64)[:n]] = np.asarray(power, F64)[:n]
    return q


def surface_carry(n, unode, energy, carry):
    energy, carry = np.array(energy, F64), np.array(carry, F64)
    idx = np.asarray(unode, I64)[:n]
    carry[idx] = carry[idx] + energy[:n]
    energy[:n] = 0.0
    return energy, carry


def surface_carry_add(N, inv_time, carry, q):
    return np.zeros(N), np.asarray(q, F64) + np.asarray(carry, F64) * inv_time


# ---- k_laser_surface.hip ------------------------------------------------------------------------------------------------------
class Snapshot:
    """count and emit: the candidates of laser_surface_model.Candidates for the first NT tets, the per-workgroup counts and
    the packed edges ij = sum_v (i | j << 2) << 4 v"""

    def __init__(self, xg, ien, phi, level, side, direction, NT):
        ien = np.asarray(ien).reshape(-1, 4)[:NT]
        with np.errstate(invalid="ignore", over="ignore"):             # (a coordinate that is not finite)
            self.cand = c = lsm.Candidates(xg, ien, phi, level, side, direction)
        self.nf, self.F, self.tet, self.t = len(c.tet), c.F, c.tet, c.t
        self.ij = ((c.i | (c.j << 2)) << (4 * np.arange(3))[None, :]).sum(axis=1) if self.nf else np.zeros(0, I64)
        self.per_tet = np.bincount(c.tet, minlength=NT)
        nblk = -(-NT // BLK)
        self.blk_count = np.add.reduceat(np.r_[self.per_tet, np.zeros(nblk * BLK - NT, I64)], np.arange(0, nblk * BLK, BLK))
        self.blk_base = np.r_[0, np.cumsum(self.blk_count)][:nblk]


def surface_nodes(ien, tet):
    """unode (ascending, distinct), fslot [4 nfs]; ids compare as unsigned 32-bit"""
    keys = np.asarray(ien, I64).reshape(-1, 4)[np.asarray(tet, I64)].reshape(-1) & 0xFFFFFFFF
    unode = np.unique(keys)
    return unode, np.searchsorted(unode, keys)


def surface_deposit(b, colkey, nfb, nfs, cand_v, ij, t, fslot, eta_s, dt, col_T, energy):
    """power [4 nfs], energy [4 nfs] after the call and val [4 n n]: ls_record_kernel's lambda in float64, then per slot the
    sum from +0.0 in ascending 4 c + a"""
    cand_v = np.asarray(cand_v, F64).reshape(-1, 3, 3)
    face_idx, _ = key_face(colkey)
    k_all = face_idx - nfb
    col_T, t, ij, fslot = np.asarray(col_T, F64), np.asarray(t, F64).reshape(-1, 3), np.asarray(ij, I64), np.asarray(fslot, I64)
    val, slot_of = np.zeros(4 * b.ncol), np.full(4 * b.ncol, -1, I64)
    cols = np.nonzero((face_idx >= 0) & (k_all >= 0) & (k_all < nfs))[0]
    for k in np.unique(k_all[cols]):
        cc = cols[k_all[cols] == k]
        u, v, s = project(cand_v[nfb + k], b)
        hit, w, _ = tri_hit(u, v, s, column_centre(cc % b.n, b), column_centre(cc // b.n, b))
        cc, w = cc[hit], w[hit]
        e, pw = int(ij[k]), eta_s * col_T[cc]
        for a in range(4):
            cs = []
            for vx in range(3):
                i, j, tv = (e >> (4 * vx)) & 3, (e >> (4 * vx + 2)) & 3, t[k, vx]
                cs.append(1.0 - tv if a == i else (tv if a == j else 0.0))
            lam = (w[:, 0] * cs[0] + w[:, 1] * cs[1]) + w[:, 2] * cs[2]
            val[4 * cc + a], slot_of[4 * cc + a] = pw * lam, fslot[4 * k + a]
    power = np.zeros(4 * nfs)
    live = np.nonzero(slot_of >= 0)[0]                                # ascending record id
    np.add.at(power, slot_of[live], val[live])                        # unbuffered: one addition after the other
    summed = np.zeros(4 * nfs, bool)
    summed[slot_of[live]] = True
    energy = np.where(summed, np.asarray(energy, F64) + dt * power, np.asarray(energy, F64))
    return power, energy, val, summed


# ==== the cases of the GPU tests ===============================================================================================
H = 2.0 ** -4
VERTICAL = (0.0, 0.0, -1.0)
OBLIQUE = lsm.DIRECTIONS["oblique"]
ORIGIN = (0.5, 0.25, 0.0)             # dyadic: the vertical frame projects dyadic points exactly, s = -z


def frame(n, direction="vertical", h=H):
    return Frame(lsm.DIRECTIONS[direction], ORIGIN, h, n)


BIN_N, BIN_P = (2, 4, 16), (1, 255, 256, 257, 1000)


def bin_case(n, P, direction="vertical"):
    """coord [P, 3] and the names of the special points (index -> name) that fit into P"""
    b = frame(n, direction)
    rng = np.random.default_rng(100 * n + P)
    half = n // 2 * H
    uvs = np.stack([rng.uniform(-1.5 * half, 1.5 * half, P), rng.uniform(-1.5 * half, 1.5 * half, P), rng.uniform(0.1, 0.9, P)], 1)
    special = {}
    names = [("edge_u", (H * (n // 2 - 1), 0.5 * H, 0.5)), ("edge_v", (-0.5 * H, -H * (n // 2 - 1), 0.5)), ("minus_half", (-half, -half, 0.5)),
             ("plus_half_u", (half, 0.0, 0.5)), ("plus_half_v", (0.0, half, 0.5)), ("far", (1e9, -1e9, 0.5)), ("nan", (np.nan, 0.0, 0.5)),
             ("corner", (0.0, 0.0, 0.5))]
    for k, (name, p) in enumerate(names):
        i = (37 * k + 3) % max(P, 1) if P > 1 else 0
        if P == 1 and name != "minus_half":
            continue
        if i in special:
            continue
        uvs[i] = p
        special[i] = name
    return b, b.world(uvs), special


HIT_S_LO, HIT_SCALE = 1.0, 2.0 ** 40   # the depth grid covers [1, 2) in steps of 2^-40
STEP = 2.0 ** -40
HIT_NF = (1, 255, 256, 257)
HIT_N = 16


def _flat(p0, p1, p2, d):
    return [(p0[0], p0[1], d), (p1[0], p1[1], d), (p2[0], p2[1], d)]


def hit_specials():
    """the named faces of the hit cases in frame coordinates (u, v, s), n = 16, h = 2^-4: all in the half u >= 0"""
    h = H
    a_u, b_u, a_v, b_v = 0.5 * h, 3.5 * h, -7.5 * h, -4.5 * h
    tie_lo, tie_hi = 1.25 + 0.25 * STEP, 1.25 + 0.75 * STEP
    S = [
        ("diag_deep", _flat((a_u, a_v), (b_u, a_v), (b_u, b_v), 1.5)),          # shares the diagonal and its end vertices ...
        ("diag_shallow", _flat((a_u, a_v), (b_u, b_v), (a_u, b_v), 1.4)),       # ... with this one: centres on both
        ("coplanar_first", _flat((4 * h, -8 * h), (8 * h, -8 * h), (8 * h, -4 * h), 1.3)),
        ("coplanar_second", _flat((4 * h, -8 * h), (8 * h, -4 * h), (8 * h, -8 * h), 1.3)),   # the same triangle, back-facing
        ("tie_deeper_first", _flat((0.0, -4 * h), (4 * h, -4 * h), (0.0, 0.0), tie_hi)),
        ("tie_shallower_second", _flat((0.0, -4 * h), (4 * h, -4 * h), (0.0, 0.0), tie_lo)),
        ("separated_deeper_first", _flat((4 * h, -4 * h), (8 * h, -4 * h), (4 * h, 0.0), 1.25 + 2.5 * STEP)),
        ("separated_shallower_second", _flat((4 * h, -4 * h), (8 * h, -4 * h), (4 * h, 0.0), 1.25)),
        ("below_first", _flat((0.0, 0.0), (4 * h, 0.0), (0.0, 4 * h), 0.5)),
        ("below_second", _flat((0.0, 0.0), (4 * h, 0.0), (0.0, 4 * h), 0.25)),
        ("top_exact", _flat((4 * h, 0.0), (8 * h, 0.0), (4 * h, 4 * h), 2.0)),
        ("top_beyond", _flat((4 * h, 0.0), (8 * h, 0.0), (4 * h, 4 * h), 3.0)),
        ("zero_area", _flat((0.5 * h, 4.5 * h), (2.5 * h, 4.5 * h), (1.5 * h, 4.5 * h), 1.01)),
        ("nan_vertex", [(0.0, 4 * h, 1.01), (np.nan, 4 * h, 1.01), (0.0, 8 * h, 1.01)]),
        ("under_both", _flat((0.0, 4 * h), (6 * h, 4 * h), (0.0, 8 * h), 1.45)),
        ("straddle", [(6 * h, 5 * h, 1.2), (12 * h, 5 * h, 1.3), (6 * h, 11 * h, 1.1)]),
        ("outside", _flat((10 * h, 0.0), (12 * h, 0.0), (10 * h, 2 * h), 1.05)),
    ]
    return [n for n, _ in S], np.array([f for _, f in S], F64)


def hit_case(nf, direction="vertical"):
    """tri_v [nf, 3, 3] in world coordinates, the frame, and the names of the special faces present (name -> face)"""
    b = frame(HIT_N, direction)
    names, spec = hit_specials()
    rng = np.random.default_rng(7 + nf)
    faces = [spec[k] for k in range(min(nf, len(spec)))]
    while len(faces) < nf:                                          # sloped filler triangles over the half u < 0, both orientations
        c = np.array([rng.uniform(-8 * H, -H), rng.uniform(-8 * H, 8 * H)])
        p = c + rng.uniform(-1.5 * H, 1.5 * H, (3, 2))
        p[:, 0] = np.minimum(p[:, 0], -2.0 ** -10)
        faces.append(np.concatenate([p, rng.uniform(1.6, 1.9, (3, 1))], 1))
    if nf > len(spec):                                              # the last face of the list wins its columns
        faces[-1] = np.array(_flat((-8 * H, -8 * H), (-5 * H, -8 * H), (-8 * H, -5 * H), 1.1))
    uvs = np.array(faces, F64)
    return b, b.world(uvs), {n: k for k, n in enumerate(names) if k < nf}, uvs


def wall_records(tri_v, ids=None):
    """dfl_wall_tri records [nf, 16] float64 words (128 bytes each): v, n = 0, off = pad = 0, node = -1, id"""
    tri_v = np.asarray(tri_v, F64).reshape(-1, 9)
    rec = np.zeros((len(tri_v), 16), F64)
    rec[:, :9] = tri_v
    tail = np.full((len(tri_v), 4), -1, np.int32)
    tail[:, 3] = np.arange(len(tri_v)) if ids is None else ids
    rec[:, 14:16] = tail.view(F64)
    return rec


RUNS_N4 = (0, 65, 3, 1, 63, 64, 2, 127, 128, 129, 511, 512, 513, 1100, 0, 700)   # columns 1, 2, 8, 9, 12 have a hit
EXTRA = 24                        # entries behind the last column (the bins of the particles outside the grid): never touched
RADIUS_MONO, RADIUS_POLY = 0.005, (0.002, 0.008)


def runs_n6():
    rng = np.random.default_rng(66)
    ln = rng.integers(0, 40, 36)
    ln[[0, 7, 20, 35]] = (513, 64, 1, 130)
    return tuple(int(v) for v in ln)


def column_faces(n):
    """two flat candidate faces in the vertical frame: a boundary record (id 7) over the columns with v < 0 at depth 0.6 and a
    facet record (id -2 - 41) over those with v > 0 and u < 0 at depth 0.5; the quadrant u > 0, v > 0 has no hit"""
    L = n * H
    f0 = _flat((-L, -L), (L, -L), (0.0, -2.0 ** -7), 0.6)
    f1 = _flat((-L, 2.0 ** -7), (-2.0 ** -7, 2.0 ** -7), (-L, L), 0.5)
    return np.array([f0, f1], F64), np.array([7, -2 - 41], I64)


def column_case(n, lengths, poly, seed=0):
    """a synthetic sorted cloud in the vertical frame: runs of the given lengths, ids scrambled against position, blocks of
    equal depths in every run of three or more, particles behind, at and in front of the column's hit"""
    b = frame(n)
    assert len(lengths) == b.ncol
    rng = np.random.default_rng(1000 * n + seed)
    P, Pt = int(sum(lengths)), int(sum(lengths)) + EXTRA
    cell_start = np.r_[0, np.cumsum(lengths)].astype(I64)
    order = rng.permutation(Pt)
    tri_uvs, tri_id = column_faces(n)
    tri_v = b.world(tri_uvs)
    colkey = laser_hit(tri_v, b, 0.0, 2.0 ** 40)
    face_idx, _ = key_face(colkey)
    depth = np.round(rng.uniform(0.05, 0.95, P) * 2 ** 20) / 2 ** 20     # dyadic: s = -z exactly
    for c in range(b.ncol):
        lo, ln = cell_start[c], lengths[c]
        if ln >= 3:                                                   # blocks of equal depth
            for _ in range(max(1, ln // 16)):
                k = rng.integers(0, ln - 1)
                m = int(min(ln - k, rng.integers(2, 6)))
                depth[lo + k: lo + k + m] = depth[lo + k]
            if ln > 100:
                k = rng.permutation(ln)[:70]                           # a block longer than one chunk of the scan
                depth[lo + k] = depth[lo + k[0]]
        if face_idx[c] >= 0 and ln >= 3:
            u, v, s = project(tri_v[face_idx[c]], b)
            d = tri_hit(u, v, s, column_centre(np.array([c % n]), b), column_centre(np.array([c // n]), b))[2][0]
            depth[lo], depth[lo + 1] = d, np.nextafter(d, 1.0)        # exactly at the hit: lit; one ulp behind it: dark
    cu, cv = column_centre(np.arange(n), b), column_centre(np.arange(n), b)
    col = np.repeat(np.arange(b.ncol), lengths)
    uvs = np.stack([cu[col % n] + rng.uniform(-0.4, 0.4, P) * H, cv[col // n] + rng.uniform(-0.4, 0.4, P) * H, depth], 1)
    uvs = np.concatenate([uvs, rng.uniform(0.1, 0.9, (EXTRA, 3))])
    sorted6 = np.concatenate([b.world(uvs), rng.uniform(-1, 1, (Pt, 3))], 1)
    r = rng.uniform(RADIUS_POLY[0], RADIUS_POLY[1], Pt) if poly else None
    gw = rng.uniform(0.05, 0.3, 2 * n)
    return dict(b=b, P=Pt, cell_start=cell_start, order=order, sorted6=sorted6, sorted_r=r, radius=RADIUS_MONO, gw=gw,
                tri_v=tri_v, tri_id=tri_id, colkey=colkey, lengths=tuple(lengths), power=400.0, eta_p=0.35, eta_s=0.7)


def permuted(case, seed=1):
    """the same (s, id) pairs at other positions of every run"""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([case["cell_start"][c] + rng.permutation(ln) for c, ln in enumerate(case["lengths"])] +
                          [np.arange(case["cell_start"][-1], case["P"])]).astype(I64)
    out = dict(case)
    out["order"], out["sorted6"] = case["order"][perm], case["sorted6"][perm]
    out["sorted_r"] = None if case["sorted_r"] is None else case["sorted_r"][perm]
    return out


def run_columns(case, **kw):
    a = dict(case)
    a.update(kw)
    return laser_columns(a["P"], a["b"], a["power"], a["eta_p"], a["eta_s"], a["gw"], a["cell_start"], a["order"], a["sorted6"],
                         a["sorted_r"], a["radius"], a["tri_v"], a["tri_id"], a["colkey"])


def deposit_case(ns):
    """the hit case nf = 257 in the vertical frame with its model keys; every (face, vertex) given to one of ns nodes, the
    last node (ns > 1) without faces"""
    b, tri_v, names, _ = hit_case(257)
    colkey = laser_hit(tri_v, b, HIT_S_LO, HIT_SCALE)
    rng = np.random.default_rng(ns)
    nf = len(tri_v)
    if ns == 1:
        pairs = [(0, 4 * f + int(rng.integers(0, 3))) for f in range(nf)]
    else:
        lost = names["outside"]                                        # node 0 has this face alone: it wins no column
        pairs = [(0 if f == lost else int(rng.integers(1, ns - 1)), 4 * f + kv) for f in range(nf) for kv in range(3)]
    pairs.sort()
    node = np.array([p[0] for p in pairs])
    sface = np.array([p[1] for p in pairs], I64)
    soff = np.searchsorted(node, np.arange(ns + 1))
    col_T = rng.uniform(0.5, 2.0, b.ncol)
    energy = rng.uniform(1.0, 2.0, ns)
    return dict(b=b, tri_v=tri_v, names=names, colkey=colkey, soff=soff, sface=sface, col_T=col_T, energy=energy, ns=ns,
                eta_s=0.7, dt=2.0 ** -10 * 1.3)


TALLY_NCOL = (4, 255, 256, 257, 65536)
LIST_SIZES = (1, 256, 257)


def single_tet(mask, at_level=None):
    """one tet with the nodes of `mask` above the level 0.25; at_level: that node exactly at the level"""
    xg = np.array([[0.0, 0.0, 0.0], [1.0, 0.125, 0.0], [0.25, 1.0, 0.125], [0.125, 0.25, 1.0]])
    phi = np.array([0.25 + (0.1 + 0.07 * a if (mask >> a) & 1 else -0.2 + 0.03 * a) for a in range(4)])
    if at_level is not None:
        phi[at_level] = 0.25
    return xg.reshape(-1), np.array([[0, 1, 2, 3]], np.int32), phi, 0.25


def snapshot_fields(m):
    """the fields of the kuhn_cube(5, 0.2) snapshot cases: name -> (xg, phi, level, direction)"""
    xg = np.asarray(m.xg, F64).reshape(-1, 3)
    ien = np.asarray(m.ien).reshape(-1, 4)
    d = {k: np.asarray(v) / np.linalg.norm(v) for k, v in lsm.DIRECTIONS.items()}
    out = {}
    out["plane_vertical"] = (xg, lsm.plane_phi(xg), lsm.PLANE_LEVEL, d["vertical"])
    out["plane_oblique"] = (xg, lsm.plane_phi(xg), lsm.PLANE_LEVEL, d["oblique"])
    out["sphere"] = (xg, np.sqrt(((xg - 0.5) ** 2).sum(axis=1)), 0.3, d["oblique"])
    out["perpendicular"] = (xg, xg[:, 0] - 0.5, 0.0137, d["vertical"])        # g . dir = rounding noise of both signs
    xd = np.round(xg * 1024.0) / 1024.0                                        # 10-bit coordinates: every product is exact
    out["in_plane"] = (xd, xd[:, 0].copy(), 0.49, d["vertical"])               # g . dir == 0 exactly
    phi = lsm.plane_phi(xg).copy()
    for e in range(0, 50, 5):
        phi[ien[e]] = 0.31
    out["constant_tets"] = (xg, phi, lsm.PLANE_LEVEL, d["vertical"])
    full = lsm.Candidates(xg, ien, lsm.plane_phi(xg), lsm.PLANE_LEVEL, lsm.SIDE, d["vertical"])
    phi, xb = lsm.plane_phi(xg).copy(), xg.copy()
    phi[int(full.nodes[3, 1])] = np.nan
    xb[int(full.nodes[len(full.tet) // 2, 2]), 1] = np.inf
    out["nan_and_inf"] = (xb, phi, lsm.PLANE_LEVEL, d["vertical"])
    return out


SNAP_NT = (1, 255, 256, 257, 750)
NODES_NFS = (1, 63, 64, 65, 300)


def nodes_case(nfs):
    """a synthetic tet list whose node ids use all 32 key bits (0 and 2^31 - 1 among them); facet 1 is of facet 0's tet"""
    rng = np.random.default_rng(nfs)
    ntet = max(2, nfs)
    pool = np.unique(np.r_[0, 2 ** 31 - 1, rng.integers(0, 2 ** 31 - 1, max(4, nfs)), rng.integers(0, 300, max(4, nfs))])
    ien = np.stack([rng.permutation(pool)[:4] for _ in range(ntet)]).astype(np.int32)
    ien[0] = (2 ** 31 - 1, 0, pool[1], pool[2])
    tet = np.sort(rng.integers(0, ntet, nfs))
    tet[0] = 0
    if nfs > 1:
        tet[1] = 0
    return ien, tet


SURF_N = (2, 16, 64, 256)


def surface_deposit_case(n, kind, nfb):
    """`one`: a single facet over the whole grid; `many`: a tiling of small facets over part of the grid.  nfb boundary records
    in front, shallower than the facets over a few columns.  ij, t and fslot are synthetic but well-formed: i != j, 0 < t < 1,
    four distinct slots per facet"""
    h = 2.0 ** -4 if n <= 64 else 2.0 ** -6
    b = frame(n, h=h)
    rng = np.random.default_rng(10 * n + nfb + (kind == "one"))
    L = n // 2 * h
    faces = []
    for q in range(nfb):                                            # small boundary faces near the corner (-L, -L)
        c = np.array([-L + (q + 1) * h * 0.5 * n / 8, -L + h * n / 8])
        faces.append(np.concatenate([c + np.array([[-1, -1], [1.3, -1], [-1, 1.2]]) * h * max(1, n // 8), np.full((3, 1), 0.2)], 1))
    if kind == "one":
        faces.append(np.array([(-3 * L, -2 * L, 0.5), (3 * L, -2 * L, 0.7), (0.0, 4 * L, 0.6)]))
    else:
        m = min(n // 2, 24)                                          # m x m cells of two facets over [-L, 0.7 L)^2
        e = 1.7 * L / m
        for q in range(m * m):
            x0, y0 = -L + (q % m) * e, -L + (q // m) * e
            z = rng.uniform(0.4, 0.9, 4)
            faces.append(np.array([(x0, y0, z[0]), (x0 + e, y0, z[1]), (x0 + e, y0 + e, z[2])]))
            faces.append(np.array([(x0, y0, z[0]), (x0 + e, y0 + e, z[2]), (x0, y0 + e, z[3])]))
    cand_v = b.world(np.array(faces, F64))
    nfs = len(faces) - nfb
    colkey = laser_hit(cand_v, b, 0.0, 2.0 ** 40)
    i = rng.integers(0, 4, (nfs, 3))
    j = (i + rng.integers(1, 4, (nfs, 3))) % 4
    ij = ((i | (j << 2)) << (4 * np.arange(3))[None, :]).sum(axis=1)
    t = rng.uniform(0.05, 0.95, (nfs, 3))
    nslot = 4 if nfs == 1 else nfs + 3
    fslot = np.stack([rng.permutation(nslot)[:4] for _ in range(nfs)]).reshape(-1)
    ids = np.r_[np.arange(nfb), -2 - np.arange(nfs)]
    return dict(b=b, cand_v=cand_v, ids=ids, nfb=nfb, nfs=nfs, colkey=colkey, ij=ij, t=t, fslot=fslot,
                col_T=rng.uniform(0.5, 2.0, b.ncol), energy=rng.uniform(1.0, 2.0, 4 * nfs), eta_s=0.7, dt=1.3 * 2.0 ** -9)
