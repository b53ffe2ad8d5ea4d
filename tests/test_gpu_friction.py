"""GPU tests of the DEM contact friction and rotation (ParticleContextSetFriction; csrc/dem_friction.hpp and the friction
variants in csrc/k_dem.hip and csrc/k_walls.hip).  Build-defined (the reference has no particle physics): pinned to the
frictionless kernels, to tests/friction_model.py and to closed forms."""
import numpy as np
import pytest

import friction_model as fm
import walls_model as wm
from dedflow_amd.meshgen import dem_lattice, dem_particles, kuhn_box, kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu
KN, GN = 1.0e4, 1.0
G = 9.81


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _l_shape(M=8):
    return kuhn_box(M, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (2 * i >= M and 2 * j >= M))


def _state(pc, api):
    api.sync()
    x, v, a = (q.reshape(-1, 3) for q in pc.arrays())
    return x, v, a, pc.omega(), pc.alpha()


def _acc(api, x, v, R, problem=None, friction=False):
    pc = api.Particles(np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(v).reshape(-1), R, kn=KN, gamma_n=GN)
    try:
        if problem is not None:
            pc.set_walls(problem)
        if friction:
            pc.set_friction(0.5)
        pc.compute_forces()
        api.sync()
        return pc.arrays()[2].reshape(-1, 3)
    finally:
        pc.close()


@pytest.mark.parametrize("walls", [False, True])
def test_off_means_off(api, walls):
    x, v, R = dem_particles(3000, 0.03)
    P = api.Problem(kuhn_cube(4)) if walls else None
    pc = api.Particles(x, v, R, kn=KN, gamma_n=GN)
    try:
        fresh = _acc(api, x, v, R, P)
        assert not np.array_equal(_acc(api, x, v, R, P, friction=True), fresh)
        if walls:
            pc.set_walls(P)
        pc.set_friction(0.5, kt=100.0, gamma_t=0.3)
        pc.set_omega(np.random.default_rng(1).normal(size=(pc.P, 3)))
        pc.compute_forces()
        pc.compute_forces()
        pc.set_friction(None)
        pc.compute_forces()
        api.sync()
        assert np.array_equal(pc.arrays()[2].reshape(-1, 3), fresh)
        with pytest.raises(RuntimeError):
            pc.omega()
    finally:
        pc.close()
        if P is not None:
            P.close()


def _parity_case(which):
    """(mesh or None, walls_model.Walls or None, x) of a dense lattice state"""
    R = 0.05
    if which == "unit_box":
        return None, None, dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.05, max_particles=700), R
    if which == "cube8":
        m = kuhn_cube(8)
        return m, wm.Walls(m), dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.05, max_particles=700), R
    if which == "l_shape":
        m = _l_shape()
        x = dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.05)
        x = x[(x[:, 0] < 0.5 - 0.1 * R) | (x[:, 1] < 0.5 - 0.1 * R)][:700]
        return m, wm.Walls(m), x, R
    m = kuhn_box(8, (-1, -0.5, 0), (1, 0.5, 0.6))
    return m, wm.Walls(m), dem_lattice((-1, -0.5, 0), (1, 0.5, 0.6), R, kind="fcc", spacing=1.95 * R, jitter=0.05,
                                       max_particles=700), R


@pytest.mark.parametrize("which", ["unit_box", "cube8", "l_shape", "off_box"])
def test_model_parity(api, which):
    m, W, x, R = _parity_case(which)
    rng = np.random.default_rng(21)
    v = rng.normal(scale=0.5, size=x.shape)
    w = rng.normal(scale=10.0, size=x.shape)
    g = (0.0, 0.0, -G)
    law = dict(mu=0.3, kt=2000.0, gamma_t=0.5)
    dt = 1.0e-4
    ref = fm.Model(x, v, R, kn=KN, gn=GN, dt=dt, gravity=g, W=W, w=w, **law)
    P = api.Problem(m) if m is not None else None
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN, dt=dt)
    try:
        if P is not None:
            pc.set_walls(P)
        pc.set_friction(law["mu"], kt=law["kt"], gamma_t=law["gamma_t"])
        pc.set_omega(w)
        pc.set_gravity(g)
        for step in range(5):
            pc.update()
            acc, alpha = ref.step()
            got = _state(pc, api)
            for name, a, b in zip(("x", "v", "acc", "omega", "alpha"), got, (ref.x, ref.v, acc, ref.w, alpha)):
                assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (step, name, np.abs(a - b).max(), np.abs(b).max())
            assert np.abs(alpha).max() > 0.0
        assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
        if P is not None:
            P.close()


def test_pair_forces_are_exactly_opposite(api):
    R = 0.06
    x = np.array([[0.45, 0.5, 0.5], [0.55, 0.52, 0.49]])
    v = np.array([[0.3, -1.0, 0.2], [0.0, 0.4, -0.1]])
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN)
    try:
        pc.set_friction(0.3)
        pc.set_omega([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
        for _ in range(3):
            pc.update()
            _, _, acc, _, alpha = _state(pc, api)
            assert np.array_equal(acc[0], -acc[1]) and np.array_equal(alpha[0], alpha[1])
            assert np.abs(alpha[0]).max() > 0.0
    finally:
        pc.close()


def _run(api, x, v, R, steps, problem=None, mu=0.5, dt=1.0e-4, w=None):
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN, dt=dt)
    try:
        if problem is not None:
            pc.set_walls(problem)
        pc.set_friction(mu)
        if w is not None:
            pc.set_omega(w)
        pc.set_gravity((0.0, 0.0, -G))
        for _ in range(steps):
            pc.update()
        return _state(pc, api), pc.friction_overflow_count()
    finally:
        pc.close()


def test_bitwise_repeatable(api):
    R = 0.02
    x = dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.1, max_particles=10000)
    rng = np.random.default_rng(5)
    v, w = rng.normal(scale=0.3, size=x.shape), rng.normal(scale=5.0, size=x.shape)
    a, na = _run(api, x, v, R, 50, w=w)
    b, nb = _run(api, x, v, R, 50, w=w)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    assert na == nb == 0
    assert np.abs(a[3] - w).max() > 0.0


# ---- a sphere on a floor: closed forms (as tests/test_friction_cpu.py) and the meshed floor ----------------------------
R1, KN1, GN1, GT1, DT1 = 0.05, 1.0e6, 200.0, 50.0, 1.0e-4


def _floor_run(api, g, mu, steps, x0, v0=(0.0, 0.0, 0.0), problem=None, every=500):
    z0 = R1 + g[2] / KN1
    pc = api.Particles(np.array([x0[0], x0[1], z0]), np.asarray(v0, float), R1, kn=KN1, gamma_n=GN1, dt=DT1)
    out = []
    try:
        if problem is not None:
            pc.set_walls(problem)
        pc.set_friction(mu, gamma_t=GT1)
        pc.set_gravity(g)
        for k in range(steps):
            pc.update()
            if (k + 1) % every == 0:
                x, v, _, w, _ = _state(pc, api)
                out.append((x[0].copy(), v[0].copy(), w[0].copy()))
        assert pc.friction_overflow_count() == 0
        return out
    finally:
        pc.close()


def _tilted(theta, phi=0.0):
    return G * np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), -np.cos(theta)])


def test_closed_forms_on_the_device(api):
    th = np.radians(20.0)
    e = np.array([1.0, 0.0, 0.0])
    # rolls
    s = _floor_run(api, _tilted(th), 0.5, 3000, (0.2, 0.5))
    a = (s[5][1] - s[1][1]) @ e / 0.2
    assert abs(a - 5.0 / 7.0 * G * np.sin(th)) <= 0.01 * 5.0 / 7.0 * G * np.sin(th), a
    slip = s[-1][1] + np.cross(s[-1][2], [0.0, 0.0, -R1])
    assert np.linalg.norm(slip) <= 0.01 * np.linalg.norm(s[-1][1])
    # slides
    mu = 0.05
    s = _floor_run(api, _tilted(th), mu, 3000, (0.2, 0.5))
    a = (s[5][1] - s[1][1]) @ e / 0.2
    want = G * (np.sin(th) - mu * np.cos(th))
    assert abs(a - want) <= 0.01 * want, a
    # launched on a level floor
    s = _floor_run(api, _tilted(0.0), 0.3, 5000, (0.2, 0.5), v0=(1.0, 0.0, 0.0))
    assert abs(s[-1][1][0] - 5.0 / 7.0) <= 0.01 * 5.0 / 7.0
    assert abs(s[-1][2][1] * R1 - 5.0 / 7.0) <= 0.01 * 5.0 / 7.0


def test_rolling_on_a_meshed_floor_follows_the_unit_box(api):
    """down a slope diagonal to the mesh lines of kuhn_cube(8)'s floor: the path crosses many triangles and their in-plane
    edges; the plane key keeps one spring, so the trajectory is the unit box's"""
    g = _tilted(np.radians(30.0), np.radians(30.0))
    box = _floor_run(api, g, 0.5, 6000, (0.15, 0.15))
    P = api.Problem(kuhn_cube(8))
    try:
        mesh = _floor_run(api, g, 0.5, 6000, (0.15, 0.15), problem=P)
    finally:
        P.close()
    xs = np.array([s[0] for s in box])
    assert xs[-1][0] - xs[0][0] > 0.4 and xs[-1][1] - xs[0][1] > 0.2    # crosses several mesh lines both ways
    for (xb, vb, wb), (xm, vm, wm_) in zip(box, mesh):
        assert np.abs(xm - xb).max() <= 1e-10 * np.abs(xb).max()
        assert np.abs(vm - vb).max() <= 1e-10 * np.abs(vb).max()
        assert np.abs(wm_ - wb).max() <= 1e-10 * np.abs(wb).max()
    a = (box[-1][1] - box[3][1]) / (0.05 * (len(box) - 4))
    want = 5.0 / 7.0 * np.linalg.norm(g[:2])
    assert abs(np.linalg.norm(a[:2]) - want) <= 0.01 * want


def test_heap(api):
    """a column of 1000 particles released on the unit-box floor: with mu = 0.5 it settles to a pile at least 2R higher
    than the flat bed it spreads into without friction.  Without rolling resistance a heap of spheres on a flat floor
    keeps only a shallow slope, so the particles are large enough (R = 0.035) for the box walls to confine the bed"""
    R = 0.035
    x = dem_lattice((0.1, 0.1, 0.0), (0.9, 0.9, 0.98), R, spacing=2.1 * R, jitter=0.05, max_particles=1000)
    assert len(x) == 1000
    v = np.zeros_like(x)
    top = {}
    for mu in (0.5, 0.0):
        pc = api.Particles(x.reshape(-1), v.reshape(-1), R, mass=1.0, kn=1.0e5, gamma_n=300.0, dt=2.0e-4)
        try:
            pc.set_friction(mu)
            pc.set_gravity((0.0, 0.0, -G))
            for _ in range(7500):
                pc.update()
            xs, vs, _, w, _ = _state(pc, api)
            assert np.isfinite(xs).all() and np.isfinite(w).all() and pc.friction_overflow_count() == 0
            assert (xs >= -R).all() and (xs <= 1.0 + R).all()
            top[mu] = xs[:, 2].max()
            if mu > 0:
                assert 0.5 * (vs ** 2).sum() < 0.1      # settled
        finally:
            pc.close()
    print("heap top", top)
    assert top[0.5] >= top[0.0] + 2 * R, top


def test_fluid_step_with_friction_and_walls(api):
    m = kuhn_box(6, (-1, -1, -1), (1, 1, 1))
    R, dt = 0.05, 5e-3
    rng = np.random.default_rng(4)
    x = rng.uniform((-0.9, -0.9, -0.9), (0.9, 0.9, -0.2), size=(300, 3))
    v = rng.normal(scale=0.5, size=x.shape)
    mass = 2000.0 * 4.0 / 3.0 * np.pi * R ** 3
    P = api.Problem(m)
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, mass=mass, kn=1.0e3, gamma_n=GN, dt=dt)
    w0 = api.DeviceArray.from_numpy(np.zeros(6 * m.num_node))
    try:
        pc.set_walls(P)
        pc.set_friction(0.5)
        pc.couple(P, gravity=(0.0, 0.0, -G))
        for _ in range(400):
            pc.fluid_step(w0)
        xs, vs, acc, w, alpha = _state(pc, api)
        assert np.isfinite(xs).all() and np.isfinite(vs).all() and np.isfinite(w).all() and np.isfinite(alpha).all()
        floor = xs[:, 2] < -1.0 + R
        assert floor.sum() > 10
        assert (np.linalg.norm(w[floor], axis=1) > 0.0).sum() > 0.5 * floor.sum()
        assert pc.lost_count() == 0 and pc.wall_dropped_count() == 0 and pc.friction_overflow_count() == 0
    finally:
        pc.close()
        P.close()


def test_coupled_time_step_with_friction(api):
    m = kuhn_box(6, (-1, -1, -1), (1, 1, 1))
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    R = 0.04
    x = np.random.default_rng(6).uniform(-0.8, 0.8, size=(200, 3))
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R, mass=2000.0 * 4.0 / 3.0 * np.pi * R ** 3, dt=1e-3)
    try:
        pc.set_walls(P)
        pc.set_friction(0.5)
        pc.couple(P, gravity=(0.0, 0.0, -G))
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dw0, 0.1 * dw0)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        for _ in range(2):
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=10)
        xs, _, _, w, _ = _state(pc, api)
        assert np.isfinite(xs).all() and np.isfinite(w).all() and (np.abs(xs) <= 1.0 + R).all()
        assert (pc.tet() >= 0).all() and pc.lost_count() == 0 and pc.wall_dropped_count() == 0
        assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
        P.close()


def test_overflow_is_counted(api):
    R = 0.05
    k = np.arange(20) + 0.5
    th, ph = np.arccos(1 - 2 * k / 20), np.pi * (1 + 5 ** 0.5) * k    # 20 directions spread over the sphere
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    x = np.vstack([[0.5, 0.5, 0.5], 0.5 + 1.5 * R * d])
    v = np.random.default_rng(9).normal(scale=0.1, size=x.shape)
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN)
    try:
        pc.set_friction(0.5)
        pc.compute_forces()
        assert pc.friction_overflow_count() >= 4
        _, _, acc, _, _ = _state(pc, api)
        assert np.isfinite(acc).all()
        pc.set_friction(0.5)      # clears the history and the count
        assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
    xl = dem_lattice((0, 0, 0), (1, 1, 1), R, kind="fcc", jitter=0.05)
    _, n = _run(api, xl, np.zeros_like(xl), R, 3)
    assert n == 0


@pytest.mark.parametrize("walls", [False, True])
def test_scale(api, walls):
    R = 0.0114
    x = dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.05)
    assert len(x) > 95000
    rng = np.random.default_rng(7)
    v, w = rng.normal(scale=0.1, size=x.shape), rng.normal(scale=5.0, size=x.shape)
    P = api.Problem(kuhn_cube(8)) if walls else None
    try:
        a, na = _run(api, x, v, R, 10, problem=P, w=w)
        b, nb = _run(api, x, v, R, 10, problem=P, w=w)
    finally:
        if P is not None:
            P.close()
    for p, q in zip(a, b):
        assert np.isfinite(p).all() and np.array_equal(p, q)
    assert na == nb == 0
    assert np.abs(a[4]).max() > 0.0
