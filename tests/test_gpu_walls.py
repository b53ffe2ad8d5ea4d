"""GPU tests of the DEM walls from a mesh's boundary faces (ParticleContextSetWallMesh; host/walls.c, csrc/k_walls.hip).
Build-defined (the reference has no particle physics): pinned to the unit-box sweep, to tests/walls_model.py and to
closed forms."""
import numpy as np
import pytest

import coupling_model as cm
import walls_model as wm
from dedflow_amd.meshgen import dem_particles, fan_mesh, kuhn_box, kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu
KN, GN = 1.0e4, 1.0


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _l_shape(M=8):
    return kuhn_box(M, (0, 0, 0), (1, 1, 1), keep=lambda i, j, k: not (2 * i >= M and 2 * j >= M))


def _forces(api, x, v, R, problem=None, groups=range(6), mass=1.0, reps=1):
    """acc after `reps` sweeps (all of them returned) and the dropped count"""
    pc = api.Particles(np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(v).reshape(-1), R, mass=mass, kn=KN, gamma_n=GN)
    try:
        if problem is not None:
            pc.set_walls(problem, groups)
        out = []
        for _ in range(reps):
            pc.compute_forces()
            api.sync()
            out.append(pc.arrays()[2].reshape(-1, 3))
        return out, pc.wall_dropped_count()
    finally:
        pc.close()


def _near_box_points(R, seed):
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(0.0, 1.0, size=(200, 3))]
    for k in range(3):   # within R of 1, 2 and 3 faces of the unit cube
        p = rng.uniform(2 * R, 1 - 2 * R, size=(100, 3))
        ax = rng.permuted(np.tile(np.arange(3), (100, 1)), axis=1)[:, :k + 1]
        for col in range(k + 1):
            d = rng.uniform(0.05 * R, 0.95 * R, 100)
            p[np.arange(100), ax[:, col]] = np.where(rng.integers(0, 2, 100) == 0, d, 1.0 - d)
        pts.append(p)
    g = np.array([0.25, 0.375, 0.5625])   # exactly above mesh vertices and mesh edge midpoints of kuhn_cube(8)
    pts.append(np.array([[0.6 * R, a, b] for a in g for b in g] + [[a, 1.0 - 0.3 * R, b] for a in g for b in g]))
    return np.vstack(pts)


def test_unit_box_unchanged(api):
    x, v, R = dem_particles(3000, 0.03)
    fresh, _ = _forces(api, x, v, R)
    pc = api.Particles(x, v, R, kn=KN, gamma_n=GN)
    P = api.Problem(kuhn_cube(4))
    try:
        pc.compute_forces()
        api.sync()
        assert np.array_equal(pc.arrays()[2].reshape(-1, 3), fresh[0])
        pc.set_walls(P)
        pc.compute_forces()
        pc.set_walls(None)
        pc.compute_forces()
        api.sync()
        assert np.array_equal(pc.arrays()[2].reshape(-1, 3), fresh[0])
        assert pc.wall_dropped_count() == 0
    finally:
        pc.close()
        P.close()


def test_cube_parity(api):
    R = 0.05
    x = _near_box_points(R, 1)
    v = np.random.default_rng(2).normal(size=x.shape)
    box, _ = _forces(api, x, v, R)
    P = api.Problem(kuhn_cube(8))
    try:
        walls, dropped = _forces(api, x, v, R, P)
    finally:
        P.close()
    assert dropped == 0
    assert np.abs(walls[0] - box[0]).max() <= 1e-12 * np.abs(box[0]).max()


@pytest.mark.parametrize("which", ["fan", "stretched_box", "l_shape"])
def test_model_parity(api, which):
    m = {"fan": fan_mesh, "stretched_box": lambda: kuhn_box(8, (-1, -0.5, 0), (3, 0.5, 1)), "l_shape": _l_shape}[which]()
    W = wm.Walls(m)
    R = 0.04
    rng = np.random.default_rng(3)
    x = rng.uniform(W.lo - 2 * R, W.hi + 2 * R, size=(1500, 3))     # some outside the padded box
    # and some within R of the walls
    t = rng.integers(0, len(W.v), 500)
    lam = rng.dirichlet(np.ones(3), 500)
    x = np.vstack([x, np.einsum("na,nad->nd", lam, W.v[t]) + W.n[t] * rng.uniform(-0.5 * R, R, (500, 1))])
    v = rng.normal(size=x.shape)
    P = api.Problem(m)
    try:
        acc, dropped = _forces(api, x, v, R, P, reps=2)
    finally:
        P.close()
    ref, dref = wm.forces(W, x, v, R, kn=KN, gn=GN)
    assert dropped == dref == 0
    assert np.count_nonzero(np.abs(ref).sum(axis=1)) > 400
    assert (acc[0][~wm.padded_inside(W, x, R)] == 0.0).all()
    assert np.abs(acc[0] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(acc[0], acc[1])     # bitwise reproducible


@pytest.mark.parametrize("z", ["mesh_edge", "mesh_vertex"])
def test_convex_edge_closed_form(api, z):
    M, R, a = 8, 0.08, 0.03
    nb = -np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    p = np.array([0.5, 0.5, 0.5 + (0.5 / M if z == "mesh_edge" else 0.0)]) + a * nb
    v = np.array([[-0.4, 0.1, 0.25]])
    P = api.Problem(_l_shape(M))
    try:
        acc, dropped = _forces(api, p[None, :], v, R, P)
    finally:
        P.close()
    want = (KN * (R - a) - GN * (v[0] @ nb)) * nb
    assert dropped == 0
    assert np.abs(acc[0][0] - want).max() <= 1e-12 * np.abs(want).max()


def test_open_group(api):
    """z+ left out of the mask: a particle moving up through z+ feels no wall there, leaves the padded box and then gets
    zero contact acceleration and tet -1; with z+ in the mask it bounces back"""
    m = kuhn_box(4, (0, 0, 0), (1, 1, 1))
    R, dt = 0.05, 1e-3
    x0 = np.array([[0.4, 0.6, 1.0 - 0.5 * R]])
    v0 = np.array([[0.0, 0.0, 1.0]])
    P = api.Problem(m)
    try:
        for groups, leaves in ((range(5), True), (range(6), False)):
            pc = api.Particles(x0.reshape(-1), v0.reshape(-1), R, kn=KN, gamma_n=GN, dt=dt)
            try:
                pc.set_walls(P, groups)
                pc.couple(P)
                pc.compute_forces()
                api.sync()
                a = pc.arrays()[2]
                if leaves:
                    assert (a == 0.0).all()
                else:
                    assert a[2] < 0.0 and a[0] == 0.0 and a[1] == 0.0
                for _ in range(200):
                    pc.update()
                pc.compute_forces()
                pc.locate()
                api.sync()
                xs, vs, acc = pc.arrays()
                if leaves:
                    assert xs[2] > 1.0 + R and (acc == 0.0).all() and pc.tet()[0] == -1
                else:
                    assert xs[2] < 1.0 and vs[2] < 0.0 and pc.tet()[0] >= 0
                assert pc.wall_dropped_count() == 0
            finally:
                pc.close()
    finally:
        P.close()


def _surface_distance(W, x):
    return np.array([np.linalg.norm(p - wm.closest_features(W.v, p)[3], axis=1).min() for p in x])


def _drop(api, m, x, R, steps, dt, kn=1.0e3, seed=4):
    """a coupled drop in fluid at rest under gravity (kn dt^2 / m < 0.25: a stable contact step)"""
    rng = np.random.default_rng(seed)
    W = wm.Walls(m)
    P = api.Problem(m)
    v = rng.normal(scale=0.5, size=x.shape)
    mass = 2000.0 * 4.0 / 3.0 * np.pi * R ** 3
    pc = api.Particles(x.reshape(-1), v.reshape(-1), R, mass=mass, kn=kn, gamma_n=GN, dt=dt)
    w = api.DeviceArray.from_numpy(np.zeros(6 * m.num_node))
    ke = []
    try:
        pc.set_walls(P)
        pc.couple(P, gravity=(0.0, 0.0, -9.81))
        for k in range(steps):
            pc.fluid_step(w)
            if k % 50 == 49:
                api.sync()
                ke.append(0.5 * mass * (pc.arrays()[1] ** 2).sum())
        pc.locate()
        api.sync()
        return W, pc.arrays()[0].reshape(-1, 3), pc.tet(), pc.lost_count(), pc.wall_dropped_count(), ke
    finally:
        pc.close()
        P.close()


def test_settling_in_a_closed_box_off_the_unit_cube(api):
    R = 0.05
    x0 = np.random.default_rng(14).uniform((-0.9, -0.9, -0.9), (0.9, 0.9, -0.2), size=(300, 3))
    W, x, tet, lost, dropped, ke = _drop(api, kuhn_box(6, (-1, -1, -1), (1, 1, 1)), x0, R, 600, 5e-3)
    assert np.isfinite(x).all()
    assert (tet >= 0).all() and lost == 0 and dropped == 0
    assert (x >= -1.0 - R).all() and (x <= 1.0 + R).all()
    assert ke[-1] < 0.1 * ke[0], ke
    assert x[:, 2].mean() < -0.5     # settled to the floor


def test_settling_on_the_fan_mesh(api):
    R = 0.03
    rng = np.random.default_rng(15)
    d = rng.normal(size=(300, 3))
    x0 = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.0, 0.5, (300, 1))
    W, x, tet, lost, dropped, ke = _drop(api, fan_mesh(), x0, R, 400, 2e-3)
    assert np.isfinite(x).all() and dropped == 0
    m = fan_mesh()
    inside = cm.locate_brute(m.xg, m.ien, x) >= 0
    assert (_surface_distance(W, x[~inside]) < R).all()


def test_coupled_time_step_with_walls(api):
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
        pc.couple(P, gravity=(0.0, 0.0, -9.81))
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dw0, 0.1 * dw0)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        for _ in range(2):
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=10)
        api.sync()
        xs = pc.arrays()[0].reshape(-1, 3)
        assert np.isfinite(xs).all() and (np.abs(xs) <= 1.0 + R).all()
        assert (pc.tet() >= 0).all() and pc.lost_count() == 0 and pc.wall_dropped_count() == 0
    finally:
        pc.close()
        P.close()


def test_scale_keeps_the_search_local(api):
    P_, R = 100000, 0.004
    m = kuhn_box(16, (-2, -0.5, 0), (2, 0.5, 1))
    W = wm.Walls(m)
    rng = np.random.default_rng(8)
    x = rng.uniform(W.lo, W.hi, size=(P_, 3))
    v = rng.normal(scale=0.1, size=x.shape)
    xu, vu, _ = dem_particles(P_, R)
    prob = api.Problem(m)
    boxed = api.Particles(x.reshape(-1), v.reshape(-1), R, kn=KN, gamma_n=GN)
    cube = api.Particles(xu, vu, R, kn=KN, gamma_n=GN)
    try:
        boxed.set_walls(prob)
        times = {}
        for key, pc in (("walls", boxed), ("cube", cube)):
            for _ in range(5):
                pc.compute_forces()
            ms = []
            for _ in range(20):
                t = api.Timer()
                t.start()
                pc.compute_forces()
                t.stop()
                ms.append(t.ms())
            times[key] = float(np.median(ms))
        api.sync()
        acc = boxed.arrays()[2].reshape(-1, 3)
        near = np.nonzero(np.min(np.minimum(x - W.lo, W.hi - x), axis=1) < R)[0]
        idx = np.r_[rng.choice(P_, 1500, replace=False), near[:1500]]
        ref, dref = wm.forces(W, x, v, R, kn=KN, gn=GN, idx=idx)
        assert np.abs(acc[idx] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert boxed.wall_dropped_count() == 0 and dref == 0
        print("sweep ms", times)
        assert times["walls"] <= 3.0 * times["cube"], times
    finally:
        boxed.close()
        cube.close()
        prob.close()


def test_dropped_contacts_are_counted(api):
    """R larger than the fan ball's radius: a particle near its centre vertex, where all the tets meet, touches far more
    than DFL_WALL_MAX_CONTACTS distinct face planes"""
    m = fan_mesh()
    W = wm.Walls(m)
    R = 0.9
    x = np.array([[0.0, 0.0, 0.0], [0.05, 0.02, -0.03]])
    v = np.array([[0.1, 0.0, 0.0], [0.0, -0.2, 0.1]])
    P = api.Problem(m)
    try:
        acc, dropped = _forces(api, x, v, R, P)
    finally:
        P.close()
    ref, dref = wm.forces(W, x, v, R, kn=KN, gn=GN)
    assert dropped == dref > 0
    assert np.abs(acc[0] - ref).max() <= 1e-12 * np.abs(ref).max()
