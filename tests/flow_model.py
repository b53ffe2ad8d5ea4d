"""numpy model of particle inflow and outflow (ParticleContextAdd / ParticleContextRemove; model in include/dedflow.h).

Every floating-point expression follows the operation order the header states (no fused multiply-add), so the GPU
kernels (csrc/k_flow.hip) must reproduce these numbers bit for bit."""
import math

import numpy as np

M64 = (1 << 64) - 1
BLOCKED_KEY = 1 << 63
MAX_HISTORY = 16


def splitmix64(a):
    z = (a + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def slot_hash(seed, call, k, axis):
    return splitmix64(splitmix64(splitmix64(seed) ^ call) ^ ((4 * k + axis) & M64))


def unit_pm1(h):
    return 2.0 * (float(h >> 11) * 2.0 ** -53) - 1.0


def _norm3(a):
    return math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


class Inlet:
    """the slot lattice of include/dedflow.h (host constants in IEEE double, left to right)"""

    def __init__(self, origin, edge_u, edge_v, R, jitter=0.0, seed=0):
        o, u, v = ([float(q) for q in a] for a in (origin, edge_u, edge_v))
        self.R, self.seed = float(R), int(seed)
        lu, lv = _norm3(u), _norm3(v)
        self.nu = int(math.floor(lu / (2.0 * R))) if R > 0 else 0
        self.nv = int(math.floor(lv / (2.0 * R))) if R > 0 else 0
        self.nslot = self.nu * self.nv
        jitter = min(max(float(jitter), 0.0), 1.0)
        if self.nslot == 0:
            return
        ju = jitter * (0.5 * (lu / self.nu - 2.0 * R))
        jv = jitter * (0.5 * (lv / self.nv - 2.0 * R))
        self.pu = [u[d] / self.nu for d in range(3)]
        self.pv = [v[d] / self.nv for d in range(3)]
        self.base = [(o[d] + 0.5 * self.pu[d]) + 0.5 * self.pv[d] for d in range(3)]
        self.ou = [(u[d] / lu) * ju for d in range(3)]
        self.ov = [(v[d] / lv) * jv for d in range(3)]

    def centres(self, call):
        """[nslot][3] candidate centres of Add call `call`"""
        out = np.empty((self.nslot, 3))
        if self.nslot == 0:
            return out
        k = np.arange(self.nslot)
        i, j = (k % self.nu).astype(np.float64), (k // self.nu).astype(np.float64)
        r0 = np.array([unit_pm1(slot_hash(self.seed, call, int(s), 0)) for s in k])
        r1 = np.array([unit_pm1(slot_hash(self.seed, call, int(s), 1)) for s in k])
        for d in range(3):
            out[:, d] = (((self.base[d] + i * self.pu[d]) + j * self.pv[d]) + r0 * self.ou[d]) + r1 * self.ov[d]
        return out

    def blocked(self, call, coord):
        """slot flags: an existing centre closer than 2R to the candidate"""
        c = self.centres(call)
        y = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
        if len(y) == 0 or self.nslot == 0:
            return np.zeros(self.nslot, bool)
        dd = y[:, None, :] - c[None, :, :]
        d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        return (d2 < (2.0 * self.R) * (2.0 * self.R)).any(axis=0)

    def ranked_free(self, call, blocked):
        """the free slots in ascending (H(c, k, 2) >> 1, k)"""
        keys = [BLOCKED_KEY if blocked[k] else slot_hash(self.seed, call, k, 2) >> 1 for k in range(self.nslot)]
        order = sorted(range(self.nslot), key=lambda k: (keys[k], k))
        return [k for k in order if not blocked[k]]


class InflowModel:
    """ParticleContextAdd: credit, cap, selection and the appended state"""

    def __init__(self, inlet, per_call, max_particles, vel=(0.0, 0.0, 0.0)):
        self.inlet, self.per_call, self.max_particles = inlet, float(per_call), int(max_particles)
        self.vel = np.asarray(vel, dtype=np.float64)
        self.call, self.credit = 0, 0.0
        self.blocked_total = 0

    def add(self, coord, vel, tags, next_tag):
        """one Add call on (coord [P][3], vel [P][3], tags [P]); returns the new arrays and the number inserted"""
        call = self.call
        self.call += 1
        self.credit += self.per_call
        want = math.floor(self.credit)
        self.credit -= want
        P = len(coord)
        want = int(min(want, max(self.max_particles - P, 0)))
        if want <= 0:
            return coord, vel, tags, 0
        free = self.inlet.ranked_free(call, self.inlet.blocked(call, coord)) if self.inlet.nslot else []
        take = free[:want]
        n = len(take)
        self.blocked_total += want - n
        c = self.inlet.centres(call)[take] if n else np.empty((0, 3))
        coord = np.concatenate([coord, c])
        vel = np.concatenate([vel, np.tile(self.vel, (n, 1))])
        tags = np.concatenate([tags, next_tag + np.arange(n, dtype=np.int64)])
        return coord, vel, tags, n


def outflow_keep(coord, planes, tet=None, outside_mesh=False):
    """keep flags: not beyond any plane ((n0 x0 + n1 x1) + n2 x2 > d) and, outside_mesh, not at tet == -1"""
    x = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(x), bool)
    for n0, n1, n2, d in np.asarray(planes, dtype=np.float64).reshape(-1, 4):
        out |= ((n0 * x[:, 0] + n1 * x[:, 1]) + n2 * x[:, 2]) > d
    if outside_mesh and tet is not None:
        out |= np.asarray(tet) == -1
    return ~out


def remap_history(keys, xi, counts, keep):
    """the history rows after a stable compaction: keys [P][16] uint64, xi [P][16][3], counts [P] -> the survivors' rows with
    partner keys (kind 0) remapped to new ids, entries of removed partners dropped, order kept"""
    keep = np.asarray(keep, bool)
    newid = np.cumsum(keep) - keep
    Pn = int(keep.sum())
    nk = np.zeros((Pn, MAX_HISTORY), np.uint64)
    nx = np.zeros((Pn, MAX_HISTORY, 3))
    nc = np.zeros(Pn, np.int32)
    for i in np.flatnonzero(keep):
        j, m = newid[i], 0
        for e in range(int(counts[i])):
            key = int(keys[i, e])
            if key >> 62 == 0:
                if not keep[key]:
                    continue
                key = int(newid[key])
            nk[j, m] = key
            nx[j, m] = xi[i, e]
            m += 1
        nc[j] = m
    return nk, nx, nc
