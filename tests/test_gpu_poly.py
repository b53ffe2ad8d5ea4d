"""GPU tests of polydisperse DEM particles (ParticleContextSetSizes / SetInflowSizes; the POLY instantiations of the force
kernels in csrc/k_dem.hip, csrc/k_walls.hip and csrc/k_couple.hip, the sizes sort and the sized inflow kernels of
csrc/k_flow.hip).  Pinned to the monodisperse kernels (equal radii, bit for bit), to tests/poly_model.py and to closed
forms."""
import math
import os

import numpy as np
import pytest

import coupling_model as cm
import flow_model as flm
import poly_model as pm
import walls_model as wm
from dedflow_amd.meshgen import dem_lattice, dem_particles, dem_particles_poly, kuhn_box, kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu
KN, GN = 1.0e4, 1.0
G = 9.81


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _l_shape(M=6):
    return kuhn_box(M, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (2 * i >= M and 2 * j >= M))


def _state(pc, api, friction=False):
    api.sync()
    x, v, a = (q.reshape(-1, 3) for q in pc.arrays())
    s = {"x": x, "v": v, "a": a}
    if friction:
        s["w"], s["alpha"] = pc.omega(), pc.alpha()
        s["hk"], s["hx"], s["hc"] = pc.friction_history()
    t = pc.tags()
    if t is not None:
        s["tag"] = t
    return s


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. equal radii are the monodisperse kernels, bit for bit -------------------------------------------------------
def _run(api, poly, walls, friction, coupled, steps=20):
    R, M = 0.03, 1.5
    x = dem_lattice((0.1, 0.1, 0.05), (0.55, 0.55, 0.5), R, jitter=0.2)
    v = np.random.default_rng(2).normal(0, 0.2, x.shape)
    m = kuhn_cube(4)
    prob = api.Problem(m) if (walls or coupled) else None
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, mass=M, kn=KN, gamma_n=GN, dt=1e-4)
    try:
        if poly:
            pc.set_sizes(np.full(pc.P, R))
            assert pc.max_radius == R and np.array_equal(pc.masses(), np.full(pc.P, M))
        if walls:
            pc.set_walls(prob)
        if friction:
            pc.set_friction(0.5)
            pc.set_omega(np.random.default_rng(3).normal(0, 3.0, x.shape))
        pc.set_gravity((0.0, 0.0, -G))
        if coupled:
            wg, _ = synthetic_fields(m)
            pc.couple(prob, rho_f=1.0, mu_f=1e-3, gravity=(0.0, 0.0, -G))
            w_d = api.DeviceArray.from_numpy(wg)
        for _ in range(steps):
            if coupled:
                pc.fluid_step(w_d)
            else:
                pc.update()
        s = _state(pc, api, friction)
        if friction:
            assert pc.friction_overflow_count() == 0
        return s
    finally:
        pc.close()
        if prob is not None:
            prob.close()


@pytest.mark.parametrize("coupled", [False, True])
@pytest.mark.parametrize("friction", [False, True])
@pytest.mark.parametrize("walls", [False, True])
def test_equal_radii_are_monodisperse_bit_for_bit(api, walls, friction, coupled):
    a = _run(api, False, walls, friction, coupled)
    b = _run(api, True, walls, friction, coupled)
    assert np.abs(a["a"]).max() > 0
    _equal(a, b)


def _channel(api, steps, poly):
    """tests/test_gpu_flow.py's coupled channel through DflTimeStep: inflow, outflow, mesh walls"""
    m = kuhn_box(4, (0, 0, 0), (1, 1, 1))
    N = m.num_node
    wg, _ = synthetic_fields(m)
    wg[:4 * N] = 0.0
    R, dt = 0.03, 1e-3
    x = dem_lattice((0.3, 0.3, 0.3), (0.5, 0.7, 0.7), R, spacing=2.5 * R)
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R, mass=2000.0 * 4.0 / 3.0 * np.pi * R ** 3, kn=1e5, gamma_n=5.0, dt=dt)
    counts = []
    try:
        if poly:
            pc.set_sizes(np.full(pc.P, R))
            pc.set_inflow_sizes(R, R)
        pc.set_walls(P, (2, 3, 4, 5))
        pc.couple(P, gravity=(30.0, 0.0, 0.0), two_way=True)
        pc.set_inflow((0.1, 0.2, 0.2), (0.0, 0.6, 0.0), (0.0, 0.0, 0.6), vel=(1.0, 0.0, 0.0), per_call=7.5, jitter=0.5, seed=77)
        pc.set_outflow([(1.0, 0.0, 0.0, 0.6)])
        st = [api.DeviceArray.from_numpy(a) for a in (wg, np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        for _ in range(steps):
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            counts.append(pc.P)
        s = _state(pc, api)
        s["w"] = st[0].numpy()
        s["tet"] = pc.tet()
        return s, counts, pc.flow_stats(), pc.radii()
    finally:
        pc.close()
        P.close()


def test_equal_radii_flow_through_time_step_bit_for_bit(api):
    a, ca, sa, _ = _channel(api, 12, False)
    b, cb, sb, rb = _channel(api, 12, True)
    assert sa["inserted"] > 20 and sa["removed"] > 0, sa
    assert ca == cb and sa == sb
    _equal(a, b)
    assert np.array_equal(rb, np.full(len(rb), 0.03))


# ---- 2. distinct radii match the model ------------------------------------------------------------------------------
def _poly_lattice(R):
    x = dem_lattice((0.1, 0.1, 0.0), (0.5, 0.5, 0.35), R, spacing=1.9 * R, jitter=0.1)
    r = np.random.default_rng(8).uniform(0.7 * R, R, len(x))
    return x, r


@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("friction", [False, True])
def test_distinct_radii_match_the_model(api, walls, friction):
    R = 0.04
    x, r = _poly_lattice(R)
    x[:, 2] += 0.3 * R  # some pairs touch, some do not; the floor holds the lowest layer
    rng = np.random.default_rng(4)
    v, w = rng.normal(0, 0.1, x.shape), rng.normal(0, 3.0, x.shape)
    m = 1.3 * (r / R) ** 3
    prob = api.Problem(_l_shape()) if walls else None
    W = wm.Walls(_l_shape()) if walls else None
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN)
    try:
        pc.set_sizes(r, m)
        if walls:
            pc.set_walls(prob)
        if friction:
            pc.set_friction(0.4)
            pc.set_omega(w)
        pc.set_gravity((0.0, 0.0, -G))
        model = pm.Model(x, v, r, m, kn=KN, gn=GN, mu=0.4 if friction else None, W=W, w=w if friction else None,
                         gravity=(0.0, 0.0, -G), rmax=pc.max_radius)
        for _ in range(6):
            ma, mal = model.step()
            pc.update()
            s = _state(pc, api, friction)
            scale = np.abs(ma).max()
            assert scale > 0 and np.abs(s["a"] - ma).max() <= 1e-12 * scale
            if friction:
                assert np.abs(s["alpha"] - mal).max() <= 1e-12 * np.abs(mal).max()
        assert np.abs(s["x"] - model.x).max() <= 1e-12 and np.abs(s["v"] - model.v).max() <= 1e-12 * np.abs(model.v).max()
        if friction:
            assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
        if prob is not None:
            prob.close()


# ---- 3. an unequal pair with friction -------------------------------------------------------------------------------
def test_unequal_pair_antisymmetric_and_conserving(api):
    r = np.array([0.06, 0.035])
    m = np.array([2.0, 0.4])
    x = np.array([[0.45, 0.5, 0.5], [0.45 + 0.09, 0.52, 0.49]])
    v = np.array([[1.0, 0.2, 0.0], [-0.5, 0.0, 0.1]])
    w = np.array([[3.0, -1.0, 20.0], [0.0, 5.0, -2.0]])
    for mu in (0.5, 0.05):
        pc = api.Particles(x.reshape(-1), v.reshape(-1), 0.05, kn=KN, gamma_n=GN)
        try:
            pc.set_sizes(r, m)
            pc.set_friction(mu)
            pc.set_omega(w)
            I = pm.inertia(m, r)
            p0 = (m[:, None] * v).sum(axis=0)
            L0 = (m[:, None] * np.cross(x, v)).sum(axis=0) + (I[:, None] * w).sum(axis=0)
            touched = 0
            for _ in range(300):
                pc.update()
                k, xi, c = pc.friction_history()
                if c[0] and c[1]:
                    touched += 1
                    assert np.array_equal(xi[1, 0], -xi[0, 0])
            assert touched > 10
            s = _state(pc, api, True)
            p1 = (m[:, None] * s["v"]).sum(axis=0)
            L1 = (m[:, None] * np.cross(s["x"], s["v"])).sum(axis=0) + (I[:, None] * s["w"]).sum(axis=0)
            assert np.abs(p1 - p0).max() <= 1e-12 * np.abs(p0).max()
            assert np.abs(L1 - L0).max() <= 1e-9 * np.abs(L0).max()
        finally:
            pc.close()


# ---- 4. closed forms ------------------------------------------------------------------------------------------------
def test_head_on_unequal(api):
    r1, r2, m1, m2, dt = 0.05, 0.03, 2.0, 0.5, 1e-5
    x = np.array([[0.4, 0.5, 0.5], [0.4 + r1 + r2 + 0.0005, 0.5, 0.5]])
    v = np.array([[0.3, 0, 0], [-0.1, 0, 0]])
    pc = api.Particles(x.reshape(-1), v.reshape(-1), 0.05, kn=KN, gamma_n=0.0, dt=dt)
    try:
        pc.set_sizes([r1, r2], [m1, m2])
        tc, u1, u2 = pm.head_on(m1, m2, 0.3, -0.1, KN)
        contact = 0
        steps = 0
        while steps < 20000:
            pc.update()
            steps += 1
            a = pc.arrays()[2]
            if np.any(a != 0.0):
                contact += 1
            elif contact:
                break
        assert abs(contact * dt - tc) <= 2 * dt
        s = _state(pc, api)
        assert np.isclose(s["v"][0, 0], u1, rtol=2e-3) and np.isclose(s["v"][1, 0], u2, rtol=2e-3)
    finally:
        pc.close()


def test_small_on_big_on_the_floor(api):
    r1, r2, m1, m2 = 0.08, 0.03, 1.0, 0.05
    d1, d2 = pm.stack_overlaps(m1, m2, G, KN)
    x = np.array([[0.5, 0.5, r1 - d1], [0.5, 0.5, 2 * r1 - d1 + r2 - d2]])
    pc = api.Particles(x.reshape(-1), np.zeros(6), 0.08, kn=KN, gamma_n=2.0 * math.sqrt(KN * m2), dt=1e-5)
    try:
        pc.set_sizes([r1, r2], [m1, m2])
        pc.set_gravity((0, 0, -G))
        for _ in range(3000):
            pc.update()
        s = _state(pc, api)
        assert np.isclose(r1 - s["x"][0, 2], d1, rtol=1e-6)
        assert np.isclose((r1 + r2) - (s["x"][1, 2] - s["x"][0, 2]), d2, rtol=1e-6)
    finally:
        pc.close()


def test_two_sizes_roll_at_five_sevenths(api):
    kn = 1.0e6
    r = np.array([0.05, 0.02])
    m = np.array([1.0, 0.064])
    x = np.array([[0.3, 0.3, r[0] - m[0] * G / kn], [0.3, 0.7, r[1] - m[1] * G / kn]])
    v = np.array([[0.2, 0, 0], [0.2, 0, 0]])
    pc = api.Particles(x.reshape(-1), v.reshape(-1), 0.05, kn=kn, gamma_n=2.0 * math.sqrt(kn * m[1]), dt=1e-5)
    try:
        pc.set_sizes(r, m)
        pc.set_friction(0.3)
        pc.set_gravity((0, 0, -G))
        for _ in range(8000):
            pc.update()
        s = _state(pc, api, True)
        for i in range(2):
            assert np.isclose(s["v"][i, 0], 5.0 / 7.0 * 0.2, rtol=5e-3)
            assert np.isclose(s["w"][i, 1] * r[i], s["v"][i, 0], rtol=5e-3)
    finally:
        pc.close()


def test_coupled_settling_of_two_sizes(api):
    m = kuhn_cube(4)
    N = m.num_node
    prob = api.Problem(m)
    r = np.array([0.02, 0.01])
    rho_p = 2500.0
    mass = rho_p * 4.0 / 3.0 * np.pi * r ** 3
    x = np.array([[0.3, 0.5, 0.9], [0.7, 0.5, 0.9]])
    pc = api.Particles(x.reshape(-1), np.zeros(6), 0.02, kn=KN, gamma_n=GN, dt=1e-3)
    try:
        pc.set_sizes(r, mass)
        pc.couple(prob, rho_f=1000.0, mu_f=10.0 / 3.0, gravity=(0.0, 0.0, -G))
        w_d = api.DeviceArray.from_numpy(np.zeros(6 * N))
        for _ in range(2000):  # 30 response times of the bigger one
            pc.fluid_step(w_d)
        s = _state(pc, api)
        vts = [cm.terminal_velocity(mass[i], r[i], (0.0, 0.0, -G), rho_f=1000.0, mu_f=10.0 / 3.0) for i in range(2)]
        assert abs(vts[0][2]) > 1.5 * abs(vts[1][2])
        for i in range(2):
            assert np.allclose(s["v"][i], vts[i], rtol=1e-5, atol=1e-9), (s["v"][i], vts[i])
    finally:
        pc.close()
        prob.close()


# ---- 5. search range ------------------------------------------------------------------------------------------------
def test_small_neighbour_of_a_big_particle_is_found(api):
    rb, rs = 0.05, 0.01
    x = np.array([[0.5, 0.5, 0.5], [0.5 + 0.055, 0.5, 0.5]])  # within rb + rs, farther than 2 rs
    for first_small in (False, True):
        xx, rr = (x[::-1], np.array([rs, rb])) if first_small else (x, np.array([rb, rs]))
        pc = api.Particles(xx.reshape(-1), np.zeros(6), 0.1, kn=KN, gamma_n=GN)
        try:
            pc.set_sizes(rr, [1.0, 1.0])
            pc.compute_forces()
            a = _state(pc, api)["a"]
            f = KN * (rb + rs - 0.055)
            ib = 1 if first_small else 0
            assert np.isclose(a[ib, 0], -f, rtol=1e-12) and np.isclose(a[1 - ib, 0], f, rtol=1e-12)
        finally:
            pc.close()


# ---- 6. inflow sizes ------------------------------------------------------------------------------------------------
def test_inflow_sizes_match_the_model(api):
    R, M = 0.03, 1.0
    r_lo, r_hi = 0.015, 0.03
    origin, u, v = (0.1, 0.1, 0.9), (0.8, 0.0, 0.0), (0.0, 0.8, 0.0)
    inlet = flm.Inlet(origin, u, v, r_hi, jitter=0.6, seed=99)
    model = pm.InflowModel(inlet, 25.5, 10 ** 6, r_lo, r_hi, R, M, vel=(0.0, 0.0, -0.5))
    x, r0 = dem_particles_poly(200, 0.01, 0.03, seed=3)
    x[:, 2] *= 0.5
    x[:4] = inlet.centres(0)[[3, 40, 41, 100]]
    r0[:4] = 0.01
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R, mass=M, kn=KN, gamma_n=GN)
    try:
        m0 = pm.default_mass(r0, R, M)
        pc.set_sizes(r0)
        pc.set_inflow_sizes(r_lo, r_hi)
        assert pc.max_radius == r_hi
        pc.set_inflow(origin, u, v, vel=(0.0, 0.0, -0.5), per_call=25.5, jitter=0.6, seed=99)
        coord, vel, tags, rad, mass = x.copy(), np.zeros_like(x), np.arange(200, dtype=np.int64), r0.copy(), m0.copy()
        for call in range(5):
            coord, vel, tags, rad, mass, n = model.add_sized(coord, vel, tags, len(coord), rad, mass)
            pc.add()
            s = _state(pc, api)
            assert pc.P == len(coord)
            assert np.array_equal(s["x"], coord) and np.array_equal(s["tag"], tags), call
            assert np.array_equal(pc.radii(), rad) and np.array_equal(pc.masses(), mass), call
        new = rad[200:]
        assert len(new) > 50 and np.all((new >= r_lo) & (new < r_hi))
        d = np.linalg.norm(coord[200:, None] - coord[None], axis=2)
        d[np.arange(len(new)), 200 + np.arange(len(new))] = np.inf
        assert np.all(d >= (new[:, None] + rad[None, :]) * (1 - 1e-12))
    finally:
        pc.close()


# ---- 7. outflow -----------------------------------------------------------------------------------------------------
def test_sizes_follow_their_tags_through_remove_and_growth(api):
    R = 0.02
    x, r = dem_particles_poly(500, 0.01, 0.02, seed=6)
    m = np.random.default_rng(1).uniform(0.5, 2.0, len(r))
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R, kn=KN, gamma_n=GN)
    try:
        pc.set_sizes(r, m)
        pc.set_friction(0.3)
        pc.set_outflow([(1.0, 0.0, 0.0, 0.5)])
        pc.remove()
        t = pc.tags()
        assert pc.P == int((x[:, 0] <= 0.5).sum())
        assert np.array_equal(pc.radii(), r[t]) and np.array_equal(pc.masses(), m[t])
        pc.set_inflow_sizes(0.005, 0.01)
        pc.set_inflow((0.55, 0.05, 0.05), (0.0, 0.9, 0.0), (0.0, 0.0, 0.9), per_call=2000, seed=5)
        P0 = pc.P
        pc.add()  # grows the capacity
        assert pc.P > 1.5 * P0
        rr, mm, tt = pc.radii(), pc.masses(), pc.tags()
        assert np.array_equal(rr[:P0], r[t]) and np.array_equal(mm[:P0], m[t]) and np.array_equal(tt[:P0], t)
        assert np.all((rr[P0:] >= 0.005) & (rr[P0:] < 0.01))
        assert np.array_equal(mm[P0:], pm.default_mass(rr[P0:], R, 1.0))
        pc.set_outflow([(0.0, 1.0, 0.0, 0.5)])
        pc.remove()
        t2 = pc.tags()
        keep = np.searchsorted(tt, t2)
        assert np.array_equal(pc.radii(), rr[keep]) and np.array_equal(pc.masses(), mm[keep])
        pc.update()
        assert np.isfinite(_state(pc, api, True)["a"]).all()
    finally:
        pc.close()


# ---- 8. off ---------------------------------------------------------------------------------------------------------
def test_set_sizes_none_is_monodisperse_again(api):
    x, v, R = dem_particles(3000, 0.02)
    a = api.Particles(x, v, R, kn=KN, gamma_n=GN)
    b = api.Particles(x, v, R, kn=KN, gamma_n=GN)
    try:
        b.set_sizes(np.random.default_rng(0).uniform(0.5 * R, R, b.P))
        b.compute_forces()
        assert b.radii() is not None
        b.set_sizes(None)
        assert b.radii() is None and b.masses() is None and b.max_radius == R
        for pc in (a, b):
            pc.set_friction(0.5)
            for _ in range(5):
                pc.update()
        _equal(_state(a, api, True), _state(b, api, True))
        with pytest.raises(ValueError):
            b.set_sizes(np.full(b.P, -1.0))
        assert b.radii() is None
    finally:
        a.close()
        b.close()


# ---- 9. HDF5 --------------------------------------------------------------------------------------------------------
def test_h5_round_trip_keeps_sizes(api, tmp_path):
    from dedflow_amd import h5
    if not os.path.exists(os.path.join(os.path.dirname(h5.__file__), "libdedflow_h5.so")):
        pytest.skip("libdedflow_h5.so not built (no HDF5)")
    x, r = dem_particles_poly(300, 0.01, 0.03, seed=2)
    m = np.random.default_rng(2).uniform(0.5, 2.0, 300)
    a = api.Particles(x.reshape(-1), np.zeros(x.size), 0.03)
    b = api.Particles(np.zeros(x.size), np.zeros(x.size), 0.03)
    c = api.Particles(np.zeros(x.size), np.zeros(x.size), 0.03)
    try:
        a.set_sizes(r, m)
        p = str(tmp_path / "poly.h5")
        h5.save_particles(p, a)
        h5.load_particles(p, b)
        assert np.array_equal(b.radii(), r) and np.array_equal(b.masses(), m) and b.max_radius == r.max()
        assert np.array_equal(b.arrays()[0], x.reshape(-1))
        assert np.array_equal(h5.read_dataset(p, "particles/radius", np.float64), r)
        h5.save_particles(str(tmp_path / "mono.h5"), c)  # a monodisperse context writes no sizes; loading it keeps c as it is
        h5.load_particles(str(tmp_path / "mono.h5"), c)
        assert c.radii() is None
    finally:
        for pc in (a, b, c):
            pc.close()


def test_copy_carries_sizes(api):
    x, r = dem_particles_poly(200, 0.01, 0.03, seed=4)
    a = api.Particles(x.reshape(-1), np.zeros(x.size), 0.03)
    b = api.Particles(np.zeros(x.size), np.zeros(x.size), 0.03)
    try:
        a.set_sizes(r)
        api.lib().ParticleContextCopy(b.ctx, a.ctx)
        assert np.array_equal(b.radii(), r) and np.array_equal(b.masses(), a.masses()) and b.max_radius == a.max_radius
    finally:
        a.close()
        b.close()


# ---- 10. scale ------------------------------------------------------------------------------------------------------
def test_100k_half_to_full_radius_matches_the_model(api):
    R = 0.005
    x, r = dem_particles_poly(100_000, 0.5 * R, R, seed=21)
    rng = np.random.default_rng(5)
    x = x + rng.uniform(-0.3 * R, 0.3 * R, x.shape)  # overlaps of up to ~0.5 R
    v = rng.normal(0, 0.1, x.shape)
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN)
    try:
        pc.set_sizes(r)
        pc.compute_forces()
        a = _state(pc, api)["a"]
        idx = rng.choice(len(x), 2000, replace=False)
        model = pm.Model(x, v, r, pm.default_mass(r, R, 1.0), kn=KN, gn=GN)
        ma, _ = model.forces(idx)
        assert np.count_nonzero(np.abs(ma).sum(axis=1)) > 40
        assert np.abs(a[idx] - ma).max() <= 1e-12 * np.abs(ma).max()
    finally:
        pc.close()
