"""CPU tests of the polydisperse particle model (tests/poly_model.py; include/dedflow.h, "polydisperse particles"): with equal
radii it is the monodisperse models, the inflow radius and hash formula, closed forms, and the random packing of meshgen."""
import math

import numpy as np
import pytest

import flow_model as flm
import friction_model as fm
import poly_model as pm
import walls_model as wm
from dedflow_amd.meshgen import dem_lattice, dem_particles, dem_particles_poly, kuhn_box

KN, GN = 1.0e4, 1.0


def _l_walls():
    M = 6
    return wm.Walls(kuhn_box(M, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (2 * i >= M and 2 * j >= M)))


def test_default_mass_reference_particle():
    R, M = 0.1, 1.0
    assert pm.default_mass(np.array([R]), R, M)[0] == M  # q = 1 gives M exactly
    assert np.isclose(pm.default_mass(np.array([0.5 * R]), R, M)[0], M / 8.0, rtol=0, atol=1e-15)
    r = np.array([0.03, 0.05, 0.08])
    rho = pm.default_mass(r, R, M) / (4.0 / 3.0 * np.pi * r ** 3)
    assert np.allclose(rho, M / (4.0 / 3.0 * np.pi * R ** 3), rtol=1e-14)


@pytest.mark.parametrize("mesh", [False, True])
def test_equal_radii_frictionless_is_monodisperse(mesh):
    x, v, R = dem_particles(600, 0.03)
    x, v = x.reshape(-1, 3), v.reshape(-1, 3)
    W = _l_walls() if mesh else None
    P = len(x)
    model = pm.Model(x, v, np.full(P, R), np.full(P, 2.0), kn=KN, gn=GN, W=W)
    acc, _ = model.forces()
    if mesh:
        ref, _ = wm.forces(W, x, v, R, mass=2.0, kn=KN, gn=GN)
    else:
        act = np.ones(P, bool)
        ref = (wm.pair_forces(x, v, R, KN, GN, act) + wm.unit_box_wall_forces(x, v, R, KN, GN)) / 2.0
    scale = np.abs(ref).max()
    assert scale > 0
    assert np.abs(acc - ref).max() <= 1e-13 * scale


@pytest.mark.parametrize("mesh", [False, True])
def test_equal_radii_friction_is_monodisperse(mesh):
    R = 0.04
    x = dem_lattice((0.1, 0.1, 0.0), (0.5, 0.5, 0.4), R, jitter=0.1)
    rng = np.random.default_rng(3)
    v, w = rng.normal(0, 0.05, x.shape), rng.normal(0, 2.0, x.shape)
    W = _l_walls() if mesh else None
    P = len(x)
    a = pm.Model(x, v, np.full(P, R), np.full(P, 1.0), kn=KN, gn=GN, mu=0.5, W=W, w=w, gravity=(0, 0, -9.81))
    b = fm.Model(x, v, R, mass=1.0, kn=KN, gn=GN, mu=0.5, W=W, w=w, gravity=(0, 0, -9.81))
    for _ in range(5):
        aa, al = a.step()
        ba, bl = b.step()
        assert np.abs(aa - ba).max() <= 1e-12 * np.abs(ba).max()
        assert np.abs(al - bl).max() <= 1e-12 * max(np.abs(bl).max(), 1e-300)
    assert np.allclose(a.x, b.x, rtol=0, atol=1e-15) and np.allclose(a.w, b.w, rtol=1e-12, atol=1e-12)


def test_slot_radius_formula():
    seed, call = 7, 3
    r_lo, r_hi = 0.01, 0.02
    for k in range(50):
        h = flm.splitmix64(flm.splitmix64(flm.splitmix64(seed) ^ call) ^ (4 * k + 3))
        u = float(h >> 11) * 2.0 ** -53
        r = pm.slot_radius(seed, call, k, r_lo, r_hi)
        assert r == r_lo + (r_hi - r_lo) * u
        assert r_lo <= r < r_hi
        assert pm.slot_radius(seed, call, k, 0.015, 0.015) == 0.015  # r_lo == r_hi gives exactly that radius


def test_equal_radii_inflow_blocking_is_monodisperse():
    R = 0.02
    inlet = flm.Inlet((0.1, 0.1, 0.5), (0.8, 0, 0), (0, 0.8, 0), R, jitter=0.5, seed=9)
    y = np.random.default_rng(4).uniform(0.1, 0.9, size=(400, 3))
    y[:, 2] = 0.5 + np.random.default_rng(5).uniform(-0.05, 0.05, size=400)
    for call in range(3):
        mono = inlet.blocked(call, y)
        poly = pm.blocked(inlet, call, y, np.full(len(y), R), R, R)
        assert mono.any() and np.array_equal(mono, poly)


def test_inflow_model_unequal_radii_no_overlap():
    r_lo, r_hi = 0.01, 0.02
    inlet = flm.Inlet((0.1, 0.1, 0.5), (0.8, 0, 0), (0, 0.8, 0), r_hi, jitter=1.0, seed=2)
    im = pm.InflowModel(inlet, per_call=40, max_particles=10 ** 6, r_lo=r_lo, r_hi=r_hi, R=0.015, M=1.0)
    x, v, t = np.empty((0, 3)), np.empty((0, 3)), np.empty(0, np.int64)
    r, m = np.empty(0), np.empty(0)
    for _ in range(4):
        x, v, t, r, m, n = im.add_sized(x, v, t, len(t), r, m)
        x = x.copy()
        x[:, 2] -= 0.013  # the stream moves off the inlet, not enough to clear every slot
    assert len(x) > 40
    assert np.all((r >= r_lo) & (r < r_hi))
    assert np.allclose(m, pm.default_mass(r, 0.015, 1.0), rtol=0, atol=0)
    d = np.linalg.norm(x[:, None] - x[None], axis=2) + np.eye(len(x)) * 10
    assert np.all(d >= (r[:, None] + r[None, :]) * (1 - 1e-12))


def test_closed_form_head_on():
    r1, r2, m1, m2 = 0.05, 0.03, 2.0, 0.5
    dt, kn = 1.0e-5, KN
    x = np.array([[0.4, 0.5, 0.5], [0.4 + r1 + r2 + 0.0005, 0.5, 0.5]])
    v = np.array([[0.3, 0, 0], [-0.1, 0, 0]])
    model = pm.Model(x, v, [r1, r2], [m1, m2], kn=kn, gn=0.0, dt=dt)
    tc, u1, u2 = pm.head_on(m1, m2, 0.3, -0.1, kn)
    steps = 0
    in_contact = 0
    while steps < 20000:
        acc, _ = model.step()
        steps += 1
        if np.any(acc != 0.0):
            in_contact += 1
        elif in_contact:
            break
    assert abs(in_contact * dt - tc) <= 2 * dt
    assert np.isclose(model.v[0, 0], u1, rtol=2e-3) and np.isclose(model.v[1, 0], u2, rtol=2e-3)
    p0 = m1 * 0.3 + m2 * -0.1
    assert np.isclose(model.momentum()[0], p0, rtol=1e-12)


def test_closed_form_rolling_two_sizes():
    """a sliding sphere on the floor rolls at v = w r = 5/7 v0, whatever its size"""
    for r, m in ((0.05, 1.0), (0.02, 0.064)):
        g = 9.81
        kn = 1.0e6  # stiff: the lever r - delta stays within 1e-3 of r
        x = np.array([[0.5, 0.5, r - m * g / kn]])
        model = pm.Model(x, [[0.2, 0, 0]], [r], [m], kn=kn, gn=2.0 * math.sqrt(kn * m), mu=0.3, dt=1e-5, gravity=(0, 0, -g))
        for _ in range(8000):
            model.step()
        assert np.isclose(model.v[0, 0], 5.0 / 7.0 * 0.2, rtol=5e-3)
        assert np.isclose(model.w[0, 1] * r, model.v[0, 0], rtol=5e-3)


def test_closed_form_resting_stack():
    g = 9.81
    r1, r2, m1, m2 = 0.08, 0.03, 1.0, 0.05
    d1, d2 = pm.stack_overlaps(m1, m2, g, KN)
    x = np.array([[0.5, 0.5, r1 - d1], [0.5, 0.5, 2 * r1 - d1 + r2 - d2]])
    gn = 2.0 * math.sqrt(KN * m2)
    model = pm.Model(x, np.zeros((2, 3)), [r1, r2], [m1, m2], kn=KN, gn=gn, dt=1e-5, gravity=(0, 0, -g))
    for _ in range(3000):
        model.step()
    assert np.isclose(r1 - model.x[0, 2], d1, rtol=1e-6)
    assert np.isclose((r1 + r2) - (model.x[1, 2] - model.x[0, 2]), d2, rtol=1e-6)


def test_dem_particles_poly_packing():
    x, r = dem_particles_poly(2000, 0.01, 0.03, seed=5)
    assert x.shape == (2000, 3) and np.all((r >= 0.01) & (r <= 0.03))
    assert np.all(x - r[:, None] >= 0) and np.all(x + r[:, None] <= 1)
    from scipy.spatial import cKDTree
    for i, j in cKDTree(x).query_pairs(0.06):
        assert np.linalg.norm(x[i] - x[j]) >= r[i] + r[j]
