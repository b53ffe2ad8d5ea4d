"""numpy model of the level-set volume correction (include/dedflow.h, "level-set volume correction"): the classification of
the tets, the K-section search with its trial candidate, the status rules and the refusal texts, on top of
redistance_model.tet_volumes (the per-tet volume of the redistancing statistics).  Written from the header.  The sums are
taken in np.longdouble and rounded once, where the kernels add float64 partials in a fixed tree, so volumes agree to a few
units in the last place and the search takes the same path except where a decision hangs on those.  Test infrastructure only;
shared by test_volume_correction_cpu.py and test_gpu_volume_correction.py."""
import numpy as np

import redistance_model as rm

LD = np.longdouble
K = 15
PASSES = 12
STATUS = {0: "corrected", 1: "already within tolerance", 2: "not bracketed", 3: "pass limit reached"}


def refusal(level, side=1, max_shift=0.1, tol=1e-10, target=np.nan, every=0):
    """the text DflVolumeCorrectionCheck gives for the configuration (its beginning), or None"""
    if not np.isfinite(level):
        return "level is not finite"
    if not np.isfinite(max_shift):
        return "max_shift is not finite"
    if not max_shift > 0.0:
        return "max_shift must be positive"
    if not np.isfinite(tol):
        return "tol is not finite"
    if tol < 0.0:
        return "tol must not be negative"
    if side not in (1, -1):
        return "side must be +1 or -1"
    if every < 0:
        return "every must not be negative"
    if np.isinf(target):
        return "target is infinite"
    return None


def classify(mesh, phi, level, max_shift):
    """per tet: inside (four phi > level + max_shift) and band (not inside, a phi > level - max_shift); a NaN is not >"""
    ph = np.asarray(phi, np.float64)[np.asarray(mesh.ien).reshape(-1, 4)]
    with np.errstate(invalid="ignore"):
        inside = (ph > level + max_shift).all(axis=1)
        band = ~inside & (ph > level - max_shift).any(axis=1)
    return inside, band


def mesh_volume(mesh, dtype=np.float64):
    x = np.asarray(mesh.xg, np.float64).reshape(-1, 3).astype(dtype)[np.asarray(mesh.ien).reshape(-1, 4)]
    return float((np.abs(rm._det4(x[:, 0], x[:, 1], x[:, 2], x[:, 3])) / dtype(6)).astype(LD).sum())


def candidates(a, b, Va, Vb, target):
    """the K candidates of a pass over [a, b]: the K - 1 section points and the trial, ascending"""
    w = (b - a) / float(K)
    trial = a + (b - a) * ((Va - target) / (Va - Vb)) if Va > Vb else a + 0.5 * (b - a)
    if not trial >= a:
        trial = a
    if trial > b:
        trial = b
    out, placed = [], False
    for k in range(1, K):
        u = a + float(k) * w
        if not placed and trial <= u:
            out.append(trial)
            placed = True
        out.append(u)
    if not placed:
        out.append(trial)
    return out


def correct(mesh, phi, level, max_shift, tol, target=np.nan, passes=PASSES):
    """DflMeshVolumeCorrect: dict of the statistics (status, passes, band_tets, shift, target, volume_before, volume_after,
    volume_mesh) and phi, the new field"""
    phi = np.asarray(phi, np.float64)
    ien = np.asarray(mesh.ien).reshape(-1, 4)
    lo, hi = level - max_shift, level + max_shift
    inside, band = classify(mesh, phi, level, max_shift)
    full = rm.tet_volumes(mesh.xg, ien, phi, level)[1]
    V_in = float(full[inside].astype(LD).sum())
    V_mesh = float(full.astype(LD).sum())
    ien_band = ien[band]

    def V(c):
        if not len(ien_band):
            return V_in + 0.0
        return V_in + float(rm.tet_volumes(mesh.xg, ien_band, phi, c)[0].astype(LD).sum())

    at_level, at_lo, at_hi = (level, V(level)), (lo, V(lo)), (hi, V(hi))
    if np.isnan(target):
        target = at_level[1]
    tolV = tol * V_mesh
    res = dict(status=3, passes=0, band_tets=int(band.sum()), shift=0.0, target=float(target), volume_before=at_level[1],
               volume_after=at_level[1], volume_mesh=V_mesh, phi=phi.copy())
    if abs(at_level[1] - target) <= tolV:
        res["status"] = 1
        return res
    if not (target <= at_lo[1] and target >= at_hi[1]):
        res["status"] = 2
        return res
    a, b = (at_lo, at_level) if target > at_level[1] else (at_level, at_hi)
    best = a if abs(a[1] - target) <= abs(b[1] - target) else b
    while abs(best[1] - target) > tolV and res["passes"] < passes:
        p = [a] + [(c, V(c)) for c in candidates(a[0], b[0], a[1], b[1], target)] + [b]
        res["passes"] += 1
        for q in p[1:-1]:
            if abs(q[1] - target) < abs(best[1] - target):
                best = q
        j = 0
        while j < K and not p[j + 1][1] <= target:
            j += 1
        a, b = p[j], p[j + 1]
    if abs(best[1] - target) <= tolV:
        res["status"] = 0
    res["shift"] = level - best[0]
    res["volume_after"] = best[1]
    if res["shift"] != 0.0:
        with np.errstate(invalid="ignore"):
            res["phi"] = np.where(np.isnan(phi), phi, phi + res["shift"])
    return res


def slope(mesh, phi, c, eta):
    """|dV/dc| at c by a central difference of width 2 eta"""
    return abs(float(rm.volume(mesh.xg, mesh.ien, phi, c + eta)) - float(rm.volume(mesh.xg, mesh.ien, phi, c - eta))) / (2.0 * eta)
